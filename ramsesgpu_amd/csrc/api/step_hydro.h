// api/step_hydro.h -- the hydro core over plane ranges: the LDS-tiled 3D sweep, the LDS-tiled fused 2D step, the flat prim / trace /
// flux / update chain, tried in that order.  See api/ctx.h, api/step.h.
#pragma once
namespace {
// One call of the core -- complete the update of planes [a,b) of `out` -- and the three ways to do it.  Each answers 0 = done,
// < 0 = failed, 1 = not covered, go on; a device-clock step (st.clk) that a tiled kernel does not cover fails: the flat kernels take
// dt by value.
struct HydroStep {
  rgpu_ctx* c; const DevParams& g;
  const double* in; double* out;
  StepTime st; double dtdx, dtdy, dtdz;
  int a, b; bool whole; int out_par;

  // 3D, LDS-tiled z-marching sweep: the whole step in one kernel (hip/tiled_hydro.h).  Slab pieces (flags: RGPU_CORE_UPDATE |
  // RGPU_CORE_SCAN after a reset by the FLUXES call) accumulate the scan into the same slot.
  // (a2, b2): a second plane range in the same launch (the two boundary ranges of a slab)
  int sweep3d(int flags, int a2, int b2) const {
    Phase ph(c, RGPU_T_SWEEP);
    ScanPlan scan(c, hydro3d_sweep_scan(c), whole, flags, out_par);
    if (scan.begin()) return -1;
    const int rc = rgpu_tiled::hydro3d_sweep(c->stream, g, in, out, dtdx, dtdy, dtdz, a, b, scan.slots(), st.clk, a2, b2);
    if (rc == 0) scan.done();
    if (rc <= 0) return rc;
    ph.drop();               // not covered: no sweep ran, the phase timers must not say one did
    if (st.clk) return -1;
    scan.not_covered();
    return 1;
  }
  // 2D, LDS-tiled fused step: one kernel (hip/tiled_hydro2d.h)
  int fused2d(ScanPlan& scan) const {
    Phase ph(c, RGPU_T_SWEEP);
    const bool folding = c->clk_cur && c->fold_mode && c->fold_pending;   // 2D batch: the clock is part of this step's kernel (ClockFold)
    const int images = hydro2d_images(c);
    const int rc = rgpu_tiled::hydro2d_step(c->stream, g, in, out, dtdx, dtdy, scan.slots(), images, folding ? 0 : st.clk, folding ? &c->fold : 0);
    if (rc == 0 && folding) c->fold_pending = false;
    if (rc == 0) scan.done();
    if (rc == 0 && images) c->rec.ghosts_written(out_par);
    if (rc <= 0) return rc;
    ph.drop();               // not covered: the flat kernels are the step
    return st.clk ? -1 : 1;
  }
  // trace and flux, specialised at launch time on the Riemann solver and the slope type (launchers.h: the no-gravity instantiations
  // only) or generic (SPEC_NONE; GF: per-cell gravity field, separate instantiations, see half_dt_gravity)
  template <int ND, int NV, int SPEC, bool GF = false>
  int trace_flux() const {
    { Phase ph(c, RGPU_T_TRACE); K_hydro_trace<ND, NV, SPEC> k = {g, c->Q, c->T, dtdx, dtdy, dtdz}; if (launch_planes<kBlock, 1>(c->stream, g, clip(a - 1, b + 1, g.ksize), k)) return -1; }
    { Phase ph(c, RGPU_T_FLUX); K_hydro_flux<ND, NV, GF, SPEC> k = {g, c->T, c->F}; if (launch_planes<kBlockHeavy, 1>(c->stream, g, clip(a, b + 1, g.ksize), k)) return -1; }
    return 0;
  }
  // the flat kernels: prim, trace, flux, update over plane ranges; the update carries the scan
  template <int ND, int NV>
  int flat(ScanPlan& scan) const {
    const int ks = g.ksize;
    { Phase ph(c, RGPU_T_PRIM); K_hydro_prim<NV> k = {g, in, c->Q}; if (launch_planes<kBlock, 1>(c->stream, g, clip(a - 2, b + 2, ks), k)) return -1; }
    const bool gf = g.grav_on == 2;
    int rc = 1;   // 1 = not handled by a specialisation
    // launchers.h: the six no-gravity entries (mutually exclusive, so their order is free; grav_on != 0 picks none)
    if (const int sp = hydro_pick_spec<false>(g))
      rc = hydro_spec_dispatch<false>(sp, [&](auto tag) { return trace_flux<ND, NV, decltype(tag)::value>(); });
    if (rc == 1) rc = gf ? trace_flux<ND, NV, SPEC_NONE, true>() : trace_flux<ND, NV, SPEC_NONE>();
    if (rc) return -1;
    Phase ph(c, RGPU_T_UPDATE);
    K_hydro_update<ND, NV, false> k = {g, in, out, c->F, dtdx, dtdy, dtdz, scan.slots()};
    K_hydro_update<ND, NV, true> kg = {g, in, out, c->F, dtdx, dtdy, dtdz, scan.slots()};
    if (gf ? launch_planes<kBlock, 1>(c->stream, g, clip(a, b, ks), kg) : launch_planes<kBlock, 1>(c->stream, g, clip(a, b, ks), k)) return -1;
    scan.done();
    return 0;
  }
};

// flags: the RGPU_CORE_* flags of a 3D slab piece (the tiled sweep accumulates its scan), 0 otherwise
// (a2, b2): 3D, tiled sweep only -- a second plane range in the same launch
template <int ND, int NV>
int hydro_core(rgpu_ctx* c, const double* in, double* out, double dt_arg, int a, int b, int flags = 0, int a2 = 0, int b2 = 0) {
  const DevParams& g = c->g;
  const StepTime st = step_time(c, dt_arg, 0.0);
  if (st.skip) return 0;
  const HydroStep h = {c, g, in, out, st, st.dt / g.dx, st.dt / g.dy, st.dt / g.dz, a, b, a <= 0 && b >= g.ksize, (out == c->U[0]) ? 0 : 1};
  int rc = 1;
  if (ND == 3 && (rc = h.sweep3d(flags, a2, b2)) <= 0) return rc;
  // 2D (fused step or flat update) and the flat 3D update: the scan of a whole-domain step
  ScanPlan scan(c, hydro_flat_scan(c), h.whole, 0, h.out_par);
  if (st.clk && !(ND == 2 && scan.slots())) return -1;   // a device-clock step is a fused kernel with the CFL term or nothing
  if (scan.begin()) return -1;
  if (ND == 2 && (rc = h.fused2d(scan)) <= 0) return rc;
  return h.template flat<ND, NV>(scan);
}

}  // namespace
