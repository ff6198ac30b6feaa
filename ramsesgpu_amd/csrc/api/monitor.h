// api/monitor.h -- the monitor of a 2D state on the host side: scratch extent, launches, the butterfly (rgpu_state_monitor).  See api/ctx.h.
#pragma once
namespace {
// ---- the monitor of a 2D state (kernels_monitor.h; rgpu_state_monitor) ----------------------------------------------
// Scratch in F like the history sums: the segment sums part[MON_NQ][nseg][nx], then the lane values [lanes][MON_NQ].  Steps 1 - 3 of
// the summation order on the device, the butterfly over the lane values on the host (the same additions, mon_combine).  Reads the
// state only: no ghost fill, nothing of c->rec or the CFL slots.
static_assert(MON_NQ == RGPU_MON_NQ && MON_ROWS == RGPU_MON_ROWS && MON_LANES == RGPU_MON_LANES, "include/rgpu.h states the summation order");
size_t monitor_scratch_doubles(const DevParams& g) {
  const size_t R = (size_t)mon_nseg(g.ny) * g.nx;
  return MON_NQ * (R + (size_t)(g.nx < MON_LANES ? g.nx : MON_LANES));
}
int state_monitor(rgpu_ctx* c, int parity, double* out) {
  const size_t R = (size_t)mon_nseg(c->g.ny) * c->g.nx;
  const int nl = c->g.nx < MON_LANES ? c->g.nx : MON_LANES;
  double* part = c->F;
  double* lanes = c->F + (size_t)MON_NQ * R;
  K_mon_rows kr = {c->g, c->U[parity & 1], part};
  K_mon_lanes kl = {c->g, part, lanes};
  double h[MON_LANES * MON_NQ];
  for (int l = 0; l < MON_LANES; ++l) mon_init(h + l * MON_NQ);   // (a lane without a column: the neutral elements)
  if (rg_launch<kBlock>(c->stream, (unsigned)R, kr) || rg_launch<kBlock>(c->stream, (unsigned)nl, kl) ||
      rg_copy_d2h(h, lanes, sizeof(double) * nl * MON_NQ, c->stream) || rg_stream_sync(c->stream)) return -1;
  mon_butterfly(h, out);
  return 0;
}

}  // namespace
