// api/monitor.h -- the monitors on the host side: scratch extent and launches of the 2D monitor and its butterfly (rgpu_state_monitor), of
// the 3D monitor (rgpu_state_monitor3d) and of a sample queued inside a device-clock batch (rgpu_run_steps_monitored).  See api/ctx.h.
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

// ---- the monitor of a 3D state (kernels_monitor.h: mon_vol_*; rgpu_state_monitor3d) and the samples of a batch ------------------------
// Everything on the device, the sum over the planes included, so that the same launches serve a sample queued inside a batch of
// device-clock steps: the gfx950 kernels of hip/monitor3d.h where the backend has them, else the flat functors (the butterfly as one
// launch per stage).  Scratch in F, then the ten doubles of a sample taken outside a batch.  F is dead between two steps (see
// history_batch_queue, api/history.h; the 3D hydro steps keep nothing in it either).
size_t monitor3d_scratch_doubles(const DevParams& g) {
#ifdef RGPU_TILED_MONITOR3D
  return rgpu_tiled::monitor_vol_scratch_doubles(g);
#else
  return (size_t)MON_NQ * ((size_t)g.nz * g.nx + 2 * (size_t)g.nz * MON_LANES);
#endif
}
bool monitor3d_scratch_fits(rgpu_ctx* c) { return c->F && monitor3d_scratch_doubles(c->g) + MON_NQ <= (size_t)c->g.fN * plan_for(c->p).f; }
// queues the sample of U into dst[MON_NQ] (device); clk != 0: the record that decides, on the device, whether it is taken
int monitor3d_queue(rgpu_ctx* c, const double* U, const StepClock* clk, double* dst) {
#ifdef RGPU_TILED_MONITOR3D
  return rgpu_tiled::launch_monitor_vol(c->stream, c->g, U, clk, c->F, dst);
#else
  const int nz = c->g.nz;
  const unsigned nl = (unsigned)nz * MON_LANES;
  double* cols = c->F;
  double* src = cols + (size_t)MON_NQ * nz * c->g.nx;
  double* nxt = src + (size_t)MON_NQ * nl;
  K_mon_vol_cols k1 = {c->g, U, cols, clk};
  K_mon_vol_lanes k2 = {c->g, cols, src, clk};
  if (rg_launch<kBlock>(c->stream, (unsigned)nz * (unsigned)c->g.nx, k1) || rg_launch<kBlock>(c->stream, nl, k2)) return -1;
  for (int off = MON_LANES / 2; off > 0; off >>= 1) {
    K_mon_vol_fly kf = {nz, off, src, nxt, clk};
    if (rg_launch<kBlock>(c->stream, nl, kf)) return -1;
    double* x = src; src = nxt; nxt = x;
  }
  K_mon_vol_finish k4 = {nz, src, dst, clk};
  return rg_launch<64>(c->stream, (unsigned)MON_NQ, k4);
#endif
}
int state_monitor3d(rgpu_ctx* c, int parity, double* out) {
  double* dst = c->F + monitor3d_scratch_doubles(c->g);
  double h[MON_NQ];
  if (monitor3d_queue(c, c->U[parity & 1], 0, dst) || rg_copy_d2h(h, dst, sizeof(h), c->stream) || rg_stream_sync(c->stream)) return -1;
  for (int q = 0; q < MON_NQ; ++q) out[q] = h[q];
  return 0;
}

// Can the samples of this context be taken inside its device-clock batches?  3D: always.  2D: through the ensemble's monitor kernels
// with one member, where the backend has them.
bool monitor_batch_ok(rgpu_ctx* c) {
  if (c->g.three_d) return monitor3d_scratch_fits(c);
#ifdef RGPU_TILED_MONITOR3D
  return c->F && monitor_scratch_doubles(c->g) <= (size_t)c->g.fN * plan_for(c->p).f;
#else
  return false;
#endif
}
int monitor_batch_alloc(rgpu_ctx* c) {
  if (c->d_mon) return 0;
  const size_t log_bytes = (size_t)rgpu_ctx::kClockBatch * MON_NQ * sizeof(double), bytes = log_bytes + sizeof(double);   // (+ the bookkeeping of the 2D path)
  if (rg_malloc((void**)&c->d_mon, bytes) || rg_host_alloc((void**)&c->h_mon, log_bytes) || rg_memset_async(c->d_mon, 0, bytes, c->stream)) {
    if (c->d_mon) { rg_free(c->d_mon); c->d_mon = 0; }
    if (c->h_mon) { rg_host_free(c->h_mon); c->h_mon = 0; }
    return -1;
  }
  return 0;
}
// Queues, behind the last kernel of the step whose record is c->clk_cur (the `slot`-th of the open batch), the sample of U[parity],
// the state that step leaves: into d_mon[slot] if the record says that the step ran.
int monitor_batch_queue(rgpu_ctx* c, int parity, int slot) {
  double* dst = c->d_mon + (size_t)slot * MON_NQ;
  int rc = -1;
  if (c->g.three_d) {
    rc = monitor3d_queue(c, c->U[parity & 1], c->clk_cur, dst);
  } else {
#ifdef RGPU_TILED_MONITOR3D
    // one member whose array is U[parity] itself; the zeroed bookkeeping with every = 1 leaves the record as the only condition
    static_assert(sizeof(rgpu_tiled::MonitorSpan) <= sizeof(double), "the zeroed double behind the log slots holds the bookkeeping");
    const rgpu_tiled::MonitorSpan* span = reinterpret_cast<const rgpu_tiled::MonitorSpan*>(c->d_mon + (size_t)rgpu_ctx::kClockBatch * MON_NQ);
    rc = rgpu_tiled::launch_ensemble_monitor(c->stream, 1, c->g, 0, c->U[parity & 1], 0u, span, c->clk_cur, 0, 1, 0, c->F, c->d_mon, (unsigned)slot);
#endif
  }
  if (rc == 0) ++c->mon_samples;
  return rc;
}

}  // namespace
