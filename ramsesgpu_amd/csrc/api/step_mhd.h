// api/step_mhd.h -- the MHD cores: the 2D step (LDS-tiled fused kernel, else the flat chain), and the 3D step over plane ranges as a
// value (Mhd3dStep: what one call launches, stage by stage) plus two schedules over it (serial; chunked on two streams, flat kernels
// only).  See api/ctx.h, api/step.h.
#pragma once
namespace {
// shearing-box / rotating-frame coefficients of the momentum update (MHDRunGodunov.cpp:2039-2053)
RotCoef rot_coef(const rgpu_ctx* c, double dt) {
  RotCoef rc = {0.0, 1.0, 1.0, 0.0};
  if (c->g.rot) {
    double lambda = c->p.Omega0 * dt;
    lambda = 0.25 * lambda * lambda;
    rc.lambda = lambda;
    rc.ratio = (1.0 - lambda) / (1.0 + lambda);
    rc.alpha1 = 1.0 / (1.0 + lambda);
    rc.alpha2 = c->p.Omega0 * dt / (1.0 + lambda);
  }
  return rc;
}

// Launch-time specialisations of the 3D MHD kernels (launchers.h): the isothermal rotating box (MRI) and the adiabatic
// inertial one, both with the HLLD pair, slope type 2 and no gravity; everything else runs the generic kernels.
const int kSpecMri = SPEC_HLLD | SPEC_ISOTHERMAL | SPEC_ROTATING | SPEC_NO_GRAVITY | SPEC_SLOPE2;
const int kSpecPlain = SPEC_HLLD | SPEC_ADIABATIC | SPEC_INERTIAL | SPEC_NO_GRAVITY | SPEC_SLOPE2;
inline int pick_spec(const DevParams& g) {
  return !rgpu::options().spec ? 0 : spec_matches(kSpecMri, g) ? 1 : spec_matches(kSpecPlain, g) ? 2 : 0;
}

int mhd2d_core(rgpu_ctx* c, const double* in, double* out, double dt_arg) {
  const DevParams& g = c->g;
  const StepTime st = step_time(c, dt_arg, 0.0);
  if (st.skip) return 0;
  const double dt = st.dt;
  const double dtdx = dt / g.dx, dtdy = dt / g.dy;
  const RotCoef rc = rot_coef(c, dt);
  const int out_par = (out == c->U[0]) ? 0 : 1;
  ScanPlan scan(c, mhd2d_scan(c), true, 0, out_par);
  // LDS-tiled fused step (hip/tiled_mhd2d.h): U -> Unew in one kernel, the CFL term of the new state included as in the flat
  // update kernel below.  Not with a Dirichlet face (its ghost fill leaves B alone, so the output's ghost cells must be copies of
  // the input's: the flat update copies them, the fused kernel writes its own cells only).
  bool faces_ok = true;
  for (int f = 0; f < 4; ++f) faces_ok = faces_ok && (c->p.bc[f] == RGPU_BC_PERIODIC || c->p.bc[f] == RGPU_BC_NEUMANN);
  if (faces_ok && rgpu_tiled::mhd2d_step_covers(g)) {
    if (st.clk && !scan.slots()) return -1;
    if (scan.begin()) return -1;
    Phase ph(c, RGPU_T_SWEEP);
    const bool images = mhd2d_images(c);
    const int rct = rgpu_tiled::mhd2d_step<kSpecPlain>(c->stream, g, rc, pick_spec(g) == 2, in, out, dt, scan.slots(), images ? 1 : 0, st.clk);
    if (rct < 0) return -1;
    if (rct == 0) {
      scan.done();
      if (images) c->rec.ghosts_written(out_par);
      return 0;
    }
  }
  if (st.clk) return -1;   // the flat kernels take dt by value
  { Phase ph(c, RGPU_T_PRIM); K_mhd_prim<> k = {g, in, c->Q, dt}; if (rg_launch<kBlock>(c->stream, c->n32, k)) return -1; }
  { Phase ph(c, RGPU_T_TRACE); K_mhd_trace2d k = {g, in, c->Q, c->T, dtdx, dtdy}; if (rg_launch<kBlock>(c->stream, c->n32, k)) return -1; }
  const bool gf = g.grav_on == 2;
  {
    Phase ph(c, RGPU_T_FLUX);
    K_mhd_flux2d<false> k = {g, c->T, c->F};
    K_mhd_flux2d<true> kg = {g, c->T, c->F};
    if (gf ? rg_launch<kBlockHeavy>(c->stream, c->n32, kg) : rg_launch<kBlockHeavy>(c->stream, c->n32, k)) return -1;
  }
  if (scan.begin()) return -1;   // (again when the fused kernel was tried and answered "not covered")
  Phase ph(c, RGPU_T_UPDATE);
  K_mhd_update2d<false> k = {g, rc, in, out, c->F, dt, dtdx, dtdy, scan.slots()};
  K_mhd_update2d<true> kg = {g, rc, in, out, c->F, dt, dtdx, dtdy, scan.slots()};
  if (gf ? rg_launch<kBlock>(c->stream, c->n32, kg) : rg_launch<kBlock>(c->stream, c->n32, k)) return -1;
  scan.done();
  return 0;
}

template <template <int> class K, int BLOCK, class... A>
int launch_spec(int spec, rg_stream_t s, const DevParams& g, PlaneRange r, A... a) {
  if (spec == 1) { K<kSpecMri> k = {g, a...}; return launch_planes<BLOCK, 1>(s, g, r, k); }
  if (spec == 2) { K<kSpecPlain> k = {g, a...}; return launch_planes<BLOCK, 1>(s, g, r, k); }
  K<SPEC_NONE> k = {g, a...};
  return launch_planes<BLOCK, 1>(s, g, r, k);
}
template <int S> using K_riemann_t = K_mhd_flux3d<DO_ALL, false, S>;

// the planes the LDS-tiled sweep solves Riemann problems on: a plane range clamped to them
inline PlaneRange sweep_planes(const DevParams& g, PlaneRange r) {
  const int top = g.ksize - g.gw + 1;
  return PlaneRange{r.lo < g.gw ? g.gw : r.lo, r.hi > top ? top : r.hi};
}

// shearing box: offsets of the flux / emf remap at totalTime + dt/2 (MHDRunGodunov.cpp:3213-3216)
ShearRemap shear_remap_at(const rgpu_params& p, double totalTime, double dt) {
  const double deltay = std::fmod(1.5 * p.Omega0 * (p.dx * p.nx) * (totalTime + dt / 2), (p.dy * p.ny));
  const double epsi = std::fmod(deltay, p.dy);
  return ShearRemap{(int)(deltay / p.dy), 1.0 - epsi / p.dy, epsi / p.dy};   // jplus, eps_min, eps_max
}

// One call of the 3D MHD core as a value: everything its launches take, and one member function per stage over a range of z planes
// on a stream.  The schedules below decide which stage runs over which planes, on which stream, behind which event.
struct Mhd3dStep {
  rgpu_ctx* c; const DevParams& g;
  const double* in; double* out;
  StepTime st; double dtdx, dtdy, dtdz;
  RotCoef rc; ShearRemap sr;
  // gf: per-cell gravity field, its own instantiations (see half_dt_gravity); spec: pick_spec, 0 with a gravity field; use_sweep: trace +
  // Riemann fused in the LDS-tiled sweep (hip/tiled_mhd.h) instead of the flat prim / elec / trace / Riemann kernels; shear: shearing box
  bool gf; int spec; bool use_sweep, shear;
  // periodic faces whose fluxes / EMFs are bit-identical copies of the opposite layer (see K_copy_periodic_layer): y (2) when both
  // y faces are periodic; x (1) when both x faces are periodic and the frame does not rotate (the rotating-frame terms carry xPos)
  int reuse;
  unsigned long long* slots;   // where the update leaves the CFL maxima of the new state (ScanPlan::slots; 0: it does not scan)

  int prim(rg_stream_t s, PlaneRange r) const { return launch_spec<K_mhd_prim, kBlock>(spec, s, g, r, in, c->Q, st.dt); }
  int elec(rg_stream_t s, PlaneRange r) const { return launch_spec<K_mhd_elec, kBlock>(spec, s, g, r, in, c->Q, c->E); }
  int trace(rg_stream_t s, PlaneRange r) const { return launch_spec<K_mhd_trace3d, kBlock>(spec, s, g, r, in, c->Q, c->E, c->T, dtdx, dtdy, dtdz); }
  // (one launch for the three face (HLLD) and the three edge (2D HLLD) Riemann problems of a cell: they read the same
  // traced states T, and T is 60 % of the step's HBM traffic.  Two launches -- 128 VGPRs / 4 waves per SIMD for the
  // faces, 205 / 2 for the edges -- were faster while the solvers were purely VALU bound; after the shared-reciprocal
  // rewrite and the XCD-aware order the second read of T costs more: 64.4 -> 60.9 ms/step at 512^3.)
  int riemann(rg_stream_t s, PlaneRange r) const {
    if (gf) { K_mhd_flux3d<DO_ALL, true> k = {g, c->T, c->F, c->emf}; return launch_planes<kBlockHeavy, 1>(s, g, r, k); }
    return launch_spec<K_riemann_t, kBlockHeavy>(spec, s, g, r, c->T, c->F, c->emf);
  }
  // LDS-tiled fused trace + Riemann sweep over the Riemann planes r (hip/tiled_mhd.h); 1 = not covered
  // r2: a second range in the same launch (split calls on the two boundary ranges of a slab) -- taken when both ranges clip to the
  // same number of planes; returns 2 when it was not (the caller launches range by range)
  int sweep(rg_stream_t s, PlaneRange r, PlaneRange r2 = PlaneRange{0, 0}) const {
    r = sweep_planes(g, r);
    if (r2.hi > r2.lo) {
      r2 = sweep_planes(g, r2);
      if (r.hi <= r.lo || r2.hi - r2.lo != r.hi - r.lo || r2.lo < r.hi) return 2;
    } else r2.lo = 0;
    // shearing box: the launch that copies the periodic y layer also saves the emfY border columns of these planes for the remap
    return rgpu_tiled::mhd3d_sweep<kSpecMri, kSpecPlain>(s, g, spec, in, c->F, c->emf, st.dt, dtdx, dtdy, dtdz, r.lo, r.hi, reuse, st.clk, shear ? c->shear_save : 0, r2.lo);
  }
  // shearing box: the two 2D (j,k) kernels -- save the emfY border columns, remap -- restricted to planes r (and r2)
  int shear_remap(rg_stream_t s, PlaneRange r, PlaneRange r2 = PlaneRange{0, 0}) const {
    if (!shear || r.hi <= r.lo) return 0;
    // (the host emulation resolves the record by value, st.clk == 0 -- except here: inside a batch the remap takes its offsets from the
    // record as on the device, so that the CPU tests run step_clock_form's offsets and not only the restatement in shear_remap_at)
    K_shear_remap k = {g, sr, c->F, c->emf, c->shear_save, c->shear_remap, dtdx, RG_SYNC_LAUNCH ? c->clk_cur : st.clk};
    if (!use_sweep) {
      K_shear_save_emf k_save = {g, c->emf, c->shear_save};
      const unsigned j0 = (unsigned)r.lo * g.jsize, jn = (unsigned)(r.hi - r.lo) * g.jsize;
      return rg_launch_range<kBlock>(s, j0, jn, k_save) || rg_launch_range<kBlock>(s, j0, jn, k);
    }
    r = sweep_planes(g, r);   // the sweep's closing launch saved the emfY columns of its planes: the remap of exactly those
    if (r.hi <= r.lo) return 0;
    if (r2.hi > r2.lo) {   // both boundary ranges in one launch (after a two-range sweep)
      r2 = sweep_planes(g, r2);
      const unsigned n1 = (unsigned)(r.hi - r.lo) * g.jsize, n2 = (unsigned)(r2.hi - r2.lo) * g.jsize;
      K_two_ranges<K_shear_remap> k2 = {k, (unsigned)r.lo * g.jsize, n1, (unsigned)r2.lo * g.jsize};
      return rg_launch<kBlock>(s, n1 + n2, k2);
    }
    return rg_launch_range<kBlock>(s, (unsigned)r.lo * g.jsize, (unsigned)(r.hi - r.lo) * g.jsize, k);
  }
  // the update is a pure stream over F, emf and U: one thread per column and short z segment, linear workgroup order, the plane
  // k+1 entries carried in registers (mhd_update3d_column; 512^3: 8.07 -> 7.42 ms against one thread per cell)
  // r2: a second range in the same launch
  int update(rg_stream_t s, PlaneRange r, PlaneRange r2 = PlaneRange{0, 0}) const {
    if (r.hi <= r.lo) { r = r2; r2 = PlaneRange{0, 0}; }
    if (r.hi <= r.lo) return 0;
    return g.rot ? update_rot<true>(s, r, r2) : update_rot<false>(s, r, r2);
  }
  // the eight instantiations of the update: frame x { gravity field, MRI, plain, generic }
  template <bool ROT>
  int update_rot(rg_stream_t s, PlaneRange r, PlaneRange r2) const {
    if (gf) return update_as<ROT, true, SPEC_NONE>(s, r, r2);
    if (spec == 1) return update_as<ROT, false, kSpecMri>(s, r, r2);
    if (spec == 2) return update_as<ROT, false, kSpecPlain>(s, r, r2);
    return update_as<ROT, false, SPEC_NONE>(s, r, r2);
  }
  template <bool ROT, bool GF, int S>
  int update_as(rg_stream_t s, PlaneRange r, PlaneRange r2) const {
    const int seg_len = 3;   // planes per thread of the update's z march (512^3: 2 / 3 / 4 / 8 / 32 planes 7.49 / 7.42 / 7.50 / 7.65 / 9.0 ms)
    const unsigned n1 = g.sk * (unsigned)((r.hi - r.lo + seg_len - 1) / seg_len);
    const bool two = r2.hi > r2.lo;
    const unsigned nt = n1 + (two ? g.sk * (unsigned)((r2.hi - r2.lo + seg_len - 1) / seg_len) : 0u);
    const unsigned split = two ? n1 : 0xffffffffu;
    K_mhd_update3d<ROT, GF, S> k = {g, rc, in, out, c->F, c->emf, c->shear_remap, st.dt, dtdx, dtdy, dtdz, slots, r.lo, r.hi, seg_len, split, r2.lo, r2.hi, st.clk};
    return rg_launch_range<kBlock>(s, 0u, nt, k);
  }
};

Mhd3dStep mhd3d_step(rgpu_ctx* c, const double* in, double* out, const StepTime& st) {
  const DevParams& g = c->g;
  const rgpu_params& p = c->p;
  const bool gf = g.grav_on == 2, shear = g.rot && g.shearbox;
  const int reuse = (p.bc[2] == RGPU_BC_PERIODIC && p.bc[3] == RGPU_BC_PERIODIC ? 2 : 0) | (p.bc[0] == RGPU_BC_PERIODIC && p.bc[1] == RGPU_BC_PERIODIC && !g.rot ? 1 : 0);
  return Mhd3dStep{c, g, in, out, st, st.dt / g.dx, st.dt / g.dy, st.dt / g.dz, rot_coef(c, st.dt),
                   shear ? shear_remap_at(p, st.t, st.dt) : ShearRemap{0, 0.0, 0.0}, gf, gf ? 0 : pick_spec(g),
                   !gf && rgpu_tiled::mhd3d_sweep_covers(g), shear, reuse, 0};
}

// everything the update of planes [lo,hi) reads -- F, emf, the shear remap buffers -- on one stream
int mhd3d_fluxes(const Mhd3dStep& m, rg_stream_t s, int lo, int hi) {
  rgpu_ctx* c = m.c;
  const int ks = m.g.ksize;
  const PlaneRange rf = clip(lo, hi + 1, ks);
  if (m.use_sweep) {   // the sweep computes primitives, electric field and traced states itself (in LDS)
    Phase ph(c, RGPU_T_SWEEP);
    if (m.sweep(s, rf)) return -1;
  } else {
    { Phase ph(c, RGPU_T_PRIM); if (m.prim(s, clip(lo - 2, hi + 2, ks))) return -1; }
    { Phase ph(c, RGPU_T_ELEC); if (m.elec(s, clip(lo - 1, hi + 2, ks))) return -1; }
    { Phase ph(c, RGPU_T_TRACE); if (m.trace(s, clip(lo - 1, hi + 1, ks))) return -1; }
    { Phase ph(c, RGPU_T_FLUX); if (m.riemann(s, rf)) return -1; }
  }
  Phase ph(c, RGPU_T_SHEAR);
  return m.shear_remap(s, rf) ? -1 : 0;
}

// Serial schedule: everything on the context's stream, stage after stage.  what: 0 = the whole update of planes [a,b);
// RGPU_CORE_FLUXES = only F, emf (+ the shear remap buffers) that update needs; RGPU_CORE_UPDATE = only the update, from F, emf
// computed by an earlier RGPU_CORE_FLUXES call covering [a,b).
// (a2, b2): a second plane range handled in the same call -- split calls only (the two boundary ranges of a slab): one launch of the
// sweep, of the remap and of the update kernel for both
int mhd3d_serial(const Mhd3dStep& m, int what, int a, int b, int a2, int b2) {
  rgpu_ctx* c = m.c;
  const int ks = m.g.ksize;
  rg_stream_t s = c->stream;
  const bool pair = what != 0 && b2 > a2;
  bool fluxes_done = what == RGPU_CORE_UPDATE;
  if (!fluxes_done && pair && m.use_sweep) {   // both boundary ranges: one launch of the sweep, one of the remap
    int rcs;
    { Phase ph(c, RGPU_T_SWEEP); rcs = m.sweep(s, clip(a, b + 1, ks), clip(a2, b2 + 1, ks)); }
    if (rcs < 0 || rcs == 1) return -1;
    fluxes_done = rcs == 0;   // (2: the ranges do not pair up, range by range below)
    if (fluxes_done) { Phase ph(c, RGPU_T_SHEAR); if (m.shear_remap(s, clip(a, b + 1, ks), clip(a2, b2 + 1, ks))) return -1; }
  }
  if (!fluxes_done && (mhd3d_fluxes(m, s, a, b) || (pair && mhd3d_fluxes(m, s, a2, b2)))) return -1;
  if (what == RGPU_CORE_FLUXES) return 0;
  Phase ph(c, RGPU_T_UPDATE);
  return m.update(s, clip(a, b, ks), pair ? clip(a2, b2, ks) : PlaneRange{0, 0}) ? -1 : 0;
}

// Chunked two-stream schedule, for the flat kernels (!m.use_sweep) and a whole update of planes [a,b): the range is swept in chunks
// of ~8 planes; the HBM-bound stages (prim, elec, trace, update) go to the context's stream, the fp64-VALU-bound Riemann stage (and
// the shear remap) to a second stream, ordering-only events in between, so that trace of chunk i+1 runs next to the Riemann stage of
// chunk i.  Stage s has completed planes [.., d_s); per chunk each stage advances to what the update of planes < kb needs.
int mhd3d_chunked(const Mhd3dStep& m, int a, int b) {
  rgpu_ctx* c = m.c;
  const int ks = m.g.ksize;
  rg_stream_t sm = c->stream, sa = c->stream2;
  const int span = b - a;
  const int C = std::max(1, std::min((span + 7) / 8, c->nchunks));
  if (rg_event_record(c->ev_fork, sm) || rg_stream_wait_event(sa, c->ev_fork)) return -1;
  int d_prim = a - 2, d_elec = a - 1, d_trace = a - 1, d_flux = a, d_upd = a;
  for (int ci = 0; ci <= C; ++ci) {
    if (ci < C) {
      const int kb = (ci + 1 == C) ? b : a + (int)(((long long)span * (ci + 1)) / C);
      if (m.prim(sm, clip(d_prim, kb + 2, ks)) || m.elec(sm, clip(d_elec, kb + 2, ks)) || m.trace(sm, clip(d_trace, kb + 1, ks))) return -1;
      d_prim = d_elec = kb + 2;
      d_trace = kb + 1;
      if (rg_event_record(c->ev_trace[ci], sm) || rg_stream_wait_event(sa, c->ev_trace[ci])) return -1;
      const PlaneRange rf = clip(d_flux, kb + 1, ks);
      if (m.riemann(sa, rf) || m.shear_remap(sa, rf)) return -1;
      d_flux = kb + 1;
      if (rg_event_record(c->ev_flux[ci], sa)) return -1;
    }
    if (ci >= 1) {  // update lags one chunk so that the next chunk's prim/elec/trace are queued ahead of it
      const int kb_prev = (ci == C) ? b : a + (int)(((long long)span * ci) / C);
      if (rg_stream_wait_event(sm, c->ev_flux[ci - 1]) || m.update(sm, clip(d_upd, kb_prev, ks))) return -1;
      d_upd = kb_prev;
    }
  }
  return 0;
}

// 3D MHD: complete the update of planes [a,b) -- or, flags RGPU_CORE_FLUXES / RGPU_CORE_UPDATE (| RGPU_CORE_SCAN), one half of it
// (mhd3d_serial), then also for a second plane range (a2, b2).
int mhd3d_core(rgpu_ctx* c, const double* in, double* out, double dt_arg, double t_arg, int a, int b, int flags = 0, int a2 = 0, int b2 = 0) {
  const StepTime st = step_time(c, dt_arg, t_arg);
  if (st.skip) return 0;
  Mhd3dStep m = mhd3d_step(c, in, out, st);
  if (st.clk && !m.use_sweep) return -1;   // the flat prim / elec / trace / Riemann kernels take dt by value
  // The CFL scan of the new state rides in the update kernel when the whole domain is updated in one call; slab pieces
  // (RGPU_CORE_SCAN with the split calls) accumulate it over the update launches of a step -- the slots are reset by the FLUXES call.
  const int what = flags & ~RGPU_CORE_SCAN;
  ScanPlan scan(c, what == 0 ? mhd3d_scan(c) : mhd3d_pieces_scan(c), a <= 0 && b >= c->g.ksize, flags, (out == c->U[0]) ? 0 : 1);
  if (scan.begin()) return -1;
  m.slots = scan.slots();
  // The chunked schedule is for whole updates by the flat kernels, outside a device-clock batch and with the phase timers off (they
  // time the context's stream).  Never with the fused sweep: it marches along z inside one launch, cutting the range into chunks only
  // adds prologues (measured 60.4 against 55.3 ms/step at 512^3).
  const bool chunked = what == 0 && !m.use_sweep && !c->timers_on && !c->clk_cur && c->nchunks > 1 && (b - a) >= 16;
  const int rc = chunked ? mhd3d_chunked(m, a, b) : mhd3d_serial(m, what, a, b, a2, b2);
  if (rc == 0) scan.done();
  return rc;
}

}  // namespace
