// api/step_core.h -- the core of the step dispatched to the solver families over plane ranges, the dissipative stage behind it, and
// the CFL scan of a state as kernels of its own.  See api/ctx.h, api/step.h.
#pragma once
namespace {
// what != 0 (RGPU_CORE_FLUXES / RGPU_CORE_UPDATE) splits the 3D MHD step, the only one whose update is a kernel of its own;
// for every other solver FLUXES is a no-op and UPDATE the whole piece, so a driver may use the split schedule blindly
int step_core_planes(rgpu_ctx* c, int nStep, double dt, double totalTime, int a, int b, int what = 0, int a2 = 0, int b2 = 0) {
  const bool splittable = c->g.three_d && c->p.mhdEnabled;
  int hydro_piece = 0;   // the flags of a 3D hydro piece whose scan accumulates
  if ((what & ~RGPU_CORE_SCAN) != 0 && !splittable) {
    if ((what & ~RGPU_CORE_SCAN) == RGPU_CORE_FLUXES) {   // nothing to compute; with SCAN: reset the slot for the pieces that follow
      c->rec.disarm();
      return ScanPlan(c, hydro3d_sweep_scan(c), false, what, (nStep + 1) % 2).begin();   // (3D hydro only: the sweep covers nothing else)
    }
    if ((what & RGPU_CORE_SCAN) && c->g.three_d && !c->p.mhdEnabled) hydro_piece = RGPU_CORE_UPDATE | RGPU_CORE_SCAN;
    what = 0;
  }
  c->rec.drop_scan();   // the output array is about to change (the kernel that writes it records what it carries along)
  c->rec.drop_ghosts();
  // static gravity of this step (g.grav_on, fill_dev_params): (0.5 * dt) * g, the reference's "HALF_F * dt * h_gravity"
  c->g.hdt = 0.5 * dt;
  c->g.hgx = 0.5 * dt * c->p.gravity_x;
  c->g.hgy = 0.5 * dt * c->p.gravity_y;
  c->g.hgz = 0.5 * dt * c->p.gravity_z;
  const double* in = c->U[nStep % 2];
  double* out = c->U[(nStep + 1) % 2];
  if (!c->g.three_d) {  // 2D: no planes
    if (!c->p.mhdEnabled) return hydro_core<2, 4>(c, in, out, dt, 0, 1);
    return mhd2d_core(c, in, out, dt);
  }
  a = std::max(a, 0); b = std::min(b, c->g.ksize);
  a2 = std::max(a2, 0); b2 = std::min(b2, c->g.ksize);
  if (b <= a) { a = a2; b = b2; a2 = b2 = 0; }
  if (b <= a) return 0;
  if (!c->p.mhdEnabled) {   // the sweep is the whole step: both ranges in one launch of the tiled sweep, else range by range
    if (b2 > a2 && rgpu_tiled::hydro3d_sweep_covers(c->g) && c->g.grav_on != 2) return hydro_core<3, 5>(c, in, out, dt, a, b, hydro_piece, a2, b2);
    const int rc = hydro_core<3, 5>(c, in, out, dt, a, b, hydro_piece);
    if (rc || b2 <= a2) return rc;
    return hydro_core<3, 5>(c, in, out, dt, a2, b2, hydro_piece);
  }
  if (what == 0 && b2 > a2) return mhd3d_core(c, in, out, dt, totalTime, a, b, 0) || mhd3d_core(c, in, out, dt, totalTime, a2, b2, 0);
  return mhd3d_core(c, in, out, dt, totalTime, a, b, what, a2, b2);
}

// Dissipative stage ([hydro] nu, [MHD] eta) on the state the step has just written: refill its ghosts (plain or
// shearing-box fill, as the call sites do), resistive emf + CT (+ energy flux unless isothermal), then viscous fluxes.
// Scratch: fluxes in F, the resistive emf in T (both dead at this point of the step).
template <int ND>
int dissipative_nd(rgpu_ctx* c, double* U, double dt, double nu, double eta) {
  const DevParams& g = c->g;
  const unsigned n = c->n32;
  if (eta > 0) {
    K_resist_emf<ND> ke = {g, U, c->T, eta};
    K_resist_ct<ND> kc = {g, U, c->T, dt / g.dx, dt / g.dy, dt / g.dz};
    if (rg_launch<kBlock>(c->stream, n, ke) || rg_launch<kBlock>(c->stream, n, kc)) return -1;
    if (g.cIso <= 0) {
      K_resist_eflux<ND> kf = {g, U, c->F, eta, dt};
      K_flux_update<ND> ku = {g, U, c->F, IP, IP + 1};
      if (rg_launch<kBlock>(c->stream, n, kf) || rg_launch<kBlock>(c->stream, n, ku)) return -1;
    }
  }
  if (nu > 0) {
    K_visc_flux<ND> kv = {g, U, c->F, nu, dt};
    K_flux_update<ND> ku = {g, U, c->F, 0, ND + 2};
    if (rg_launch<kBlock>(c->stream, n, kv) || rg_launch<kBlock>(c->stream, n, ku)) return -1;
  }
  return 0;
}

int step_dissipative(rgpu_ctx* c, int nStep, double dt, double totalTime, bool fill_ghosts = true) {
  const double nu = c->p.nu, eta = c->p.mhdEnabled ? c->p.eta : 0.0;
  if (!(nu > 0 || eta > 0)) return 0;
  c->rec.forget();
  Phase ph(c, RGPU_T_DISSIPATIVE);
  double* U = c->U[(nStep + 1) % 2];
  // (!fill_ghosts: the slab driver has filled the ghosts itself -- in-plane fills + z exchange)
  if (fill_ghosts && fill_all_ghosts(c, U, totalTime, dt)) return -1;
  return c->g.three_d ? dissipative_nd<3>(c, U, dt, nu, eta) : dissipative_nd<2>(c, U, dt, nu, eta);
}

int step_core(rgpu_ctx* c, int nStep, double dt, double totalTime) {
  return step_core_planes(c, nStep, dt, totalTime, 0, c->g.ksize);
}

// max of the per-cell 1/dt over the flat index range [idx0, idx0+n) into the device slot (reset or accumulate)
int inv_dt_scan(rgpu_ctx* c, int parity, unsigned idx0, unsigned n, bool reset) {
  c->rec.drop_scan();   // the slots are rewritten
  c->rec.disarm();
  Phase ph(c, RGPU_T_DT);
  const double* U = c->U[parity & 1];
  // a fresh scan owns ALL slots: the maximum goes to slot 0, slots 1 .. RG_DT_SLOTS-1 (which a fused scan of an earlier step may
  // have filled) are zeroed, so that whoever folds all of them -- the slab driver after its fixed-size all-reduce, whatever state
  // each rank is in -- reads this scan and nothing older
  if (reset && rg_memset_async(c->d_red, 0, RG_DT_SLOTS * sizeof(unsigned long long), c->stream)) return -1;
  auto scan = [&](const auto& k) { return rg_reduce_max(c->stream, n, k, c->d_red, idx0, false); };   // (accumulates: the memset was the reset)
  if (c->p.mhdEnabled) {
    const int spec = c->g.three_d ? pick_spec(c->g) : 0;
    if (spec == 1) return scan(K_mhd_invdt<kSpecMri>{c->g, U});
    if (spec == 2) return scan(K_mhd_invdt<kSpecPlain>{c->g, U});
    return scan(K_mhd_invdt<>{c->g, U});
  }
  return c->g.three_d ? scan(K_hydro_invdt<5>{c->g, U}) : scan(K_hydro_invdt<4>{c->g, U});
}

int inv_dt_fetch(rgpu_ctx* c, double* invDt, int nslots = 1) {
  if (rg_copy_d2h(c->h_red, c->d_red, (size_t)nslots * sizeof(unsigned long long), c->stream) || rg_stream_sync(c->stream)) return -1;
  double v = 0.0;
  for (int s = 0; s < nslots; ++s) {
    double x;
    std::memcpy(&x, c->h_red + s, sizeof(double));
    v = std::fmax(v, x);
  }
  // seeds and jet term of the CPU paths (HydroRunBase.cpp:382,420-422 ; MHDRunBase.cpp:144,184-186,228-231)
  const rgpu_params& p = c->p;
  if (p.mhdEnabled) v = std::fmax(v, p.smallc / std::fmin(p.dx, p.dy));
  if (p.enableJet) v = std::fmax(v, (p.ujet + p.cjet) / p.dx);
  *invDt = v;
  return 0;
}

int inv_dt(rgpu_ctx* c, int parity, double* invDt) {
  if (const int n = c->rec.slots(parity)) return inv_dt_fetch(c, invDt, n);   // the kernel that wrote this state scanned it
  return inv_dt_scan(c, parity, 0, c->n32, true) || inv_dt_fetch(c, invDt);
}

}  // namespace

