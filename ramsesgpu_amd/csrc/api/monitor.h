// api/monitor.h -- the monitor of a lone context on the host side (kernels_monitor.h): scratch extent and launches of one sample, for
// rgpu_state_monitor (2D), rgpu_state_monitor3d and a sample queued inside a device-clock batch (rgpu_run_steps_monitored); the same for
// the plane monitor (kernels_monitor_planes.h: rgpu_state_monitor_planes, rgpu_run_steps_monitored_planes).  See api/ctx.h.
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

// ---- the plane monitor (kernels_monitor_planes.h): the same consumer with another sample, nz rows of MONP_NQ doubles ---------------
static_assert(MONP_NQ == RGPU_MONP_NQ, "include/rgpu.h states the width of a plane row");
// (also: whether the samples of this context can be taken inside its device-clock batches)
bool monitor_planes_scratch_fits(rgpu_ctx* c) {
  return c->F && c->g.three_d && monp_scratch_doubles(c->g) + monp_sample_doubles(c->g) <= (size_t)c->g.fN * plan_for(c->p).f;
}
// queues the rows of U into dst[nz][MONP_NQ] (device); clk != 0: the record that decides, on the device, whether they are taken
int monitor_planes_queue(rgpu_ctx* c, const double* U, const StepClock* clk, double* dst) {
#ifdef RGPU_TILED_MONITOR_PROFILE
  return rgpu_tiled::launch_monitor_profile(c->stream, c->g, U, clk, c->F, dst);
#else
  K_mon_prof_cols k1 = {c->g, U, c->F, clk};
  K_mon_prof_fold k2 = {c->g.nx, c->g.nz, c->F, dst, clk};
  return (rg_launch<kBlock>(c->stream, (unsigned)c->g.nz * (unsigned)c->g.nx, k1) || rg_launch<64>(c->stream, (unsigned)c->g.nz, k2)) ? -1 : 0;
#endif
}
int state_monitor_planes(rgpu_ctx* c, int parity, double* out) {
  RG_CHECK_CTX(c);
  const std::string who = "state_monitor_planes";
  if (!out || !c->U[0]) return fail(c, RGPU_EINVAL, who + ": null pointer / context without state");
  if (!c->g.three_d) return fail(c, RGPU_EUNSUPPORTED, who + ": 3D contexts only (the rows are the interior planes of a volume)");
  if (c->p.slab_count > 1) return fail(c, RGPU_EINVAL, who + ": single-domain contexts only (a slab holds a part of the box)");
  if (!monitor_planes_scratch_fits(c)) return fail(c, RGPU_EINVAL, who + ": no scratch for the partial sums");
  double* dst = c->F + monp_scratch_doubles(c->g);
  if (monitor_planes_queue(c, c->U[parity & 1], 0, dst) || rg_copy_d2h(out, dst, monp_sample_doubles(c->g) * sizeof(double), c->stream) || rg_stream_sync(c->stream))
    return RG_HIPFAIL(c, who);
  return RGPU_OK;
}

// ---- the samples of a batch: of the monitor, or (planes) of the plane monitor ------------------------------------------------------
size_t monitor_sample_doubles(const rgpu_ctx* c, bool planes) { return planes ? monp_sample_doubles(c->g) : (size_t)MON_NQ; }
bool monitor_sample_fits(rgpu_ctx* c, bool planes) { return planes ? monitor_planes_scratch_fits(c) : monitor_scratch_fits(c); }
DeviceMirror<double>& monitor_batch_log(rgpu_ctx* c, bool planes) { return planes ? c->monp : c->mon; }
// The log of a call that samples every `every` steps.  The monitor's: a slot per step of a batch.  The plane monitor's: a slot per
// sample that can fall into one batch, grown (between two batches: nothing is in flight) if this call needs more than the last did
int monitor_batch_alloc(rgpu_ctx* c, bool planes, int every) {
  DeviceMirror<double>& log = monitor_batch_log(c, planes);
  const size_t slots = planes ? (size_t)rgpu_ctx::kClockBatch / (size_t)every + 1 : (size_t)rgpu_ctx::kClockBatch;
  if (planes && log.allocated() && c->monp_slots < slots) log.release();
  if (log.allocated()) return 0;
  const size_t n = slots * monitor_sample_doubles(c, planes);
  if (log.alloc(n) == 0 && rg_memset_async(log.d, 0, n * sizeof(double), c->stream) == 0) {
    if (planes) c->monp_slots = slots;
    return 0;
  }
  log.release();   // zeroed, or not there
  return -1;
}
// Queues, behind the last kernel of the step whose record is c->clk_cur, the sample of U[parity], the state that step leaves: into
// slot k of the log -- k samples were queued in the open batch before it -- if the record says that the step ran.
int monitor_batch_queue(rgpu_ctx* c, bool planes, int parity, int k) {
  double* dst = monitor_batch_log(c, planes).d + (size_t)k * monitor_sample_doubles(c, planes);
  const int rc = planes ? monitor_planes_queue(c, c->U[parity & 1], c->clk_cur, dst) : monitor_queue(c, c->U[parity & 1], c->clk_cur, dst);
  if (rc == 0) ++(planes ? c->monp_samples : c->mon_samples);
  return rc;
}

}  // namespace
