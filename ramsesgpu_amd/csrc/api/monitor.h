// api/monitor.h -- the monitor of a lone context on the host side (kernels_monitor.h): scratch extent and launches of one sample, for
// rgpu_state_monitor (2D), rgpu_state_monitor3d and a sample queued inside a device-clock batch (rgpu_run_steps_monitored).  See api/ctx.h.
#pragma once
namespace {
// One route for either dimension, a 2D state being a volume of one plane.  Everything on the device, the sum over the planes included,
// so that the same launches serve a sample queued inside a batch of device-clock steps: the gfx950 kernels of hip/monitor3d.h where the
// backend has them, else the flat functors.  Scratch in F, then the ten doubles of a sample taken outside a batch.  F is dead between
// two steps (see history_batch_queue, api/history.h; the hydro steps keep nothing in it either).  Reads the state only: no ghost fill,
// nothing of c->rec or the CFL slots.
static_assert(MON_NQ == RGPU_MON_NQ && MON_ROWS == RGPU_MON_ROWS && MON_LANES == RGPU_MON_LANES, "include/rgpu.h states the summation order");
// (also: whether the samples of this context can be taken inside its device-clock batches)
bool monitor_scratch_fits(rgpu_ctx* c) { return c->F && mon_scratch_doubles(c->g) + MON_NQ <= (size_t)c->g.fN * plan_for(c->p).f; }
// queues the sample of U into dst[MON_NQ] (device); clk != 0: the record that decides, on the device, whether it is taken
int monitor_queue(rgpu_ctx* c, const double* U, const StepClock* clk, double* dst) {
#ifdef RGPU_TILED_MONITOR3D
  return rgpu_tiled::launch_monitor_vol(c->stream, c->g, U, clk, c->F, dst);
#else
  // one plane: its V[0] is the result bit for bit (kernels_monitor.h, below the summation order) -- written to dst, no finish launch
  const int nz = mon_nplanes(c->g);
  double* cols = c->F;
  double* V = nz == 1 ? dst : cols + (size_t)MON_NQ * nz * c->g.nx;
  const unsigned ncols = (unsigned)nz * (unsigned)c->g.nx;
  K_mon_vol_cols<true> k3d = {c->g, U, cols, clk};
  K_mon_vol_cols<false> k2d = {c->g, U, cols, clk};
  K_mon_vol_fold k2 = {c->g.nx, nz, cols, V, clk};
  if ((c->g.three_d ? rg_launch<kBlock>(c->stream, ncols, k3d) : rg_launch<kBlock>(c->stream, ncols, k2d)) || rg_launch<64>(c->stream, (unsigned)nz, k2)) return -1;
  if (nz == 1) return 0;
  K_mon_vol_finish k3 = {nz, V, dst, clk};
  return rg_launch<64>(c->stream, (unsigned)MON_NQ, k3);
#endif
}
// rgpu_state_monitor (want3d == 0) and rgpu_state_monitor3d: the same sample, each entry refusing the other's contexts in its own words
int state_monitor(rgpu_ctx* c, bool want3d, int parity, double* out) {
  RG_CHECK_CTX(c);
  const std::string who = want3d ? "state_monitor3d" : "state_monitor";
  if (!out || !c->U[0]) return fail(c, RGPU_EINVAL, who + ": null pointer / context without state");
  if ((c->g.three_d != 0) != want3d)
    return fail(c, RGPU_EUNSUPPORTED, who + (want3d ? ": 3D contexts only (2D contexts have rgpu_state_monitor)" : ": 2D contexts only (3D contexts have rgpu_state_monitor3d)"));
  if (want3d && c->p.slab_count > 1) return fail(c, RGPU_EINVAL, who + ": single-domain contexts only (a slab holds a part of the box)");
  if (!monitor_scratch_fits(c)) return fail(c, RGPU_EINVAL, who + (want3d ? ": no scratch for the partial sums" : ": no scratch for the segment sums"));
  double* dst = c->F + mon_scratch_doubles(c->g);
  double h[MON_NQ];
  if (monitor_queue(c, c->U[parity & 1], 0, dst) || rg_copy_d2h(h, dst, sizeof(h), c->stream) || rg_stream_sync(c->stream)) return RG_HIPFAIL(c, who);
  for (int q = 0; q < MON_NQ; ++q) out[q] = h[q];
  return RGPU_OK;
}

// ---- the samples of a batch -------------------------------------------------------------------------------------------------------
int monitor_batch_alloc(rgpu_ctx* c) {
  const size_t n = (size_t)rgpu_ctx::kClockBatch * MON_NQ;
  if (c->mon.allocated() || (c->mon.alloc(n) == 0 && rg_memset_async(c->mon.d, 0, n * sizeof(double), c->stream) == 0)) return 0;
  c->mon.release();   // zeroed, or not there
  return -1;
}
// Queues, behind the last kernel of the step whose record is c->clk_cur (the `slot`-th of the open batch), the sample of U[parity],
// the state that step leaves: into slot `slot` of the log if the record says that the step ran.
int monitor_batch_queue(rgpu_ctx* c, int parity, int slot) {
  const int rc = monitor_queue(c, c->U[parity & 1], c->clk_cur, c->mon.d + (size_t)slot * MON_NQ);
  if (rc == 0) ++c->mon_samples;
  return rc;
}

}  // namespace
