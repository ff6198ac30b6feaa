// api/ensemble_fused.h -- the fused half of an ensemble (included by api/entry_ensemble.h where the backend has the ensemble kernels,
// hip/ensemble2d.h; its device buffers: EnsembleFused there): whether the running members can take a batch, queueing one -- per round ONE clock launch and
// ONE step launch for all members, plus the monitor pair on sampled rounds -- and harvesting it with one read-back of the records.
#pragma once

namespace {
// Can the running members R take a fused batch now?  The step of every one is one fused kernel that reads the device record and
// leaves CFL maxima and ghost images, every one is clock-ready (the state at hand came out of such a kernel), all with the same step
// parity (*par) and the same one of their three slot arrays holding the maxima (*phase: a lone folded run rotates them).  *transient:
// the only obstacle is a member that is not clock-ready (its first step of a run, a state written from outside) -- one plain step cures it
bool fused_batch_possible(const EnsembleRun& run, const std::vector<int>& R, bool* transient, int* par, int* phase) {
  *transient = false; *par = -1; *phase = -1;
  for (int m : R) {
    rgpu_ctx* c = run.e->ctx[(size_t)m];
    if (c->g.three_d || !clock_config_ok(c)) return false;
    if (!(c->p.mhdEnabled ? mhd2d_images(c) && rgpu_tiled::mhd2d_step_covers(c->g) : hydro2d_images(c) != 0 && rgpu_tiled::hydro2d_step_covers(c->g))) return false;
  }
  bool alike = true;
  for (int m : R) {
    rgpu_ctx* c = run.e->ctx[(size_t)m];
    if (!clock_ready(c, run.nStep[m] % 2)) { *transient = true; continue; }
    const int ph = (int)((c->d_red - c->d_red_base) / RG_DT_SLOTS);
    if (*par < 0) { *par = run.nStep[m] % 2; *phase = ph; }
    else if (*par != run.nStep[m] % 2 || *phase != ph) alike = false;
  }
  return alike && !*transient;
}

// Constants by value (one member's, for everybody: *tab = 0) or per member from the table on the device (*tab): a scan whose sets
// differ, or any ensemble under the diagnostic option member_params.  The table holds ALL members, running or not, and is filled and
// copied once for good by the first caller that needs it.  Returns RGPU_OK or a code with the message in e->err
int ensemble_table(rgpu_ensemble* e, const char* who, const rgpu_tiled::MemberConst** tab) {
  EnsembleFused& f = e->fused;
  const bool by_value = !rgpu::options().member_params && !(e->scan && !e->uniform);
  *tab = by_value ? 0 : f.tab.d;
  if (by_value || f.tab_filled) return RGPU_OK;
  const size_t M = (size_t)e->members;
  if (!f.tab.allocated() && f.tab.alloc(M)) return efail(e, RGPU_ENOMEM, std::string(who) + ": allocation of the table of member constants failed");
  for (size_t m = 0; m < M; ++m) {
    rgpu_ctx* c = e->ctx[m];
    rgpu_tiled::MemberConst& mc = f.tab.h[m];
    std::memset(&mc, 0, sizeof(mc));
    mc.g = c->g;
    mc.g.hdt = 0.0; mc.g.hgx = 0.0; mc.g.hgy = 0.0; mc.g.hgz = 0.0;
    mc.k = clock_const(c);
    mc.rc = rot_coef(c, 0.0);
  }
  if (f.tab.upload(M, kStream)) return efail(e, RGPU_EHIP, std::string(who) + ": copy of the table of member constants: " + rg_last_error_string());
  f.tab_filled = true;
  *tab = f.tab.d;
  return RGPU_OK;
}

size_t monitor_part_doubles(const rgpu_params& p) { return (size_t)MON_NQ * (size_t)mon_nseg(p.ny) * (size_t)p.nx; }
// the buffers of the device monitor (see EnsembleFused): all of them or none
int ensemble_monitor_buffers(rgpu_ensemble* e, const char* who) {
  EnsembleFused& f = e->fused;
  if (f.mlog.allocated()) return RGPU_OK;
  const size_t M = (size_t)e->members;
  if (f.mspan.alloc(M) || f.mpart.alloc(M * monitor_part_doubles(e->ctx[0]->p), false) || f.mlog.alloc((size_t)rgpu_ctx::kClockBatch * M * MON_NQ)) {
    f.mspan.release(); f.mpart.release(); f.mlog.release();
    return efail(e, RGPU_ENOMEM, std::string(who) + ": allocation of the monitor buffers failed");
  }
  return RGPU_OK;
}

// what queueing a batch leaves for its harvest
struct FusedBatch {
  int queued = 0;                     // rounds queued completely (tick and step)
  int nlaunch = 0;                    // monitor launches queued: log slots 0 .. nlaunch - 1
  std::vector<int> launch_of_round;   // the log slot of the monitor launch queued behind round r, -1: none
  bool failed = false; std::string launch_err;   // a launch failed behind the `queued` rounds, with this message
};

// Queues up to nb rounds for the members R (input parity par, slot phase `phase`): tick, then step, for all members, and behind the
// step the monitor of the state it wrote when some running member's step number after it is a multiple of every (which members
// really took the step is in the records: the kernels look there, the host when it walks them)
void fused_batch_queue(EnsembleRun& run, const std::vector<int>& R, int par, int phase, int nb, const rgpu_tiled::MemberConst* tab, FusedBatch* b) {
  rgpu_ensemble* e = run.e;
  EnsembleFused& f = e->fused;
  const int M = e->members;
  rgpu_ctx* c0 = e->ctx[(size_t)R[0]];
  DevParams g = c0->g;
  g.hdt = 0.0; g.hgx = 0.0; g.hgy = 0.0; g.hgz = 0.0;   // (no gravity on this path)
  const ClockConst kc = clock_const(c0);
  const RotCoef rotc = rot_coef(c0, 0.0);
  const bool mhd = c0->p.mhdEnabled != 0;
  const int images = mhd ? 1 : hydro2d_images(c0);
  // one instantiation for all members, chosen from g; with a table what it assumes is shared by the sets of a scan (scan_validate) --
  // were a member's constants ever not to satisfy it, the generic instantiation assumes nothing
  bool mhd_plain = pick_spec(g) == 2;
  int hydro_spec = mhd ? 0 : hydro_pick_spec<false>(g);
  for (int m = 0; tab && m < M; ++m) {
    if (!spec_matches(kSpecPlain, e->ctx[(size_t)m]->g)) mhd_plain = false;
    if (!spec_matches(hydro_spec, e->ctx[(size_t)m]->g)) hydro_spec = 0;
  }
  unsigned long long* slots = e->slots + (size_t)phase * RG_DT_SLOTS;
  const size_t pool = (size_t)M * e->stride;
  const unsigned stride = (unsigned)e->stride;
  b->launch_of_round.assign((size_t)nb, -1);
  for (; b->queued < nb; ++b->queued) {
    const int r = b->queued;
    StepClock* rec = f.clk.d + (size_t)r * M;
    if (rgpu_tiled::launch_ensemble_clock(kStream, M, slots, kc, tab, f.span.d, r ? rec - M : 0, rec)) { b->failed = true; break; }
    const int pin = (par + r) % 2, pout = 1 - pin;
    for (int m : R) { e->ctx[(size_t)m]->rec.drop_scan(); e->ctx[(size_t)m]->rec.drop_ghosts(); }   // the output arrays are about to change
    const double* in = e->U + (size_t)pin * pool;
    double* out = e->U + (size_t)pout * pool;
    if (mhd ? rgpu_tiled::mhd2d_ensemble_step<kSpecPlain>(kStream, M, g, rotc, mhd_plain, tab, in, out, stride, slots, images, rec)
            : rgpu_tiled::hydro2d_ensemble_step(kStream, M, g, hydro_spec, tab, in, out, stride, slots, images, rec)) { b->failed = true; break; }
    for (int m : R) { e->ctx[(size_t)m]->rec.scanned(pout, RG_DT_SLOTS); e->ctx[(size_t)m]->rec.ghosts_written(pout); }
    bool sample = false;
    for (int m : R) sample = sample || (run.mon && (run.nStep[m] + r + 1) % run.mon->every == 0);
    if (!sample) continue;
    if (rgpu_tiled::launch_ensemble_monitor(kStream, M, g, tab, e->U, stride, f.mspan.d, rec, r + 1, run.mon->every, pout, f.mpart.d, f.mlog.d, (unsigned)b->nlaunch)) {
      b->failed = true; ++b->queued;   // (the round itself is queued and counts; its samples are lost with the error)
      break;
    }
    b->launch_of_round[(size_t)r] = b->nlaunch++;
  }
  if (b->failed) b->launch_err = rg_last_error_string();
}

// Reads the records (and the monitor log) of the rounds that were queued and advances every member of R for the steps it took, as
// rgpu_run_steps_log would have: after a launch that failed behind b.queued complete rounds those still run, so they are read and
// counted before the failure is reported.  Returns RGPU_OK or the code that ends the call
int fused_batch_harvest(EnsembleRun& run, const std::vector<int>& R, const FusedBatch& b) {
  rgpu_ensemble* e = run.e;
  EnsembleFused& f = e->fused;
  const size_t M = (size_t)e->members;
  if (b.queued > 0 && (f.clk.download((size_t)b.queued * M, kStream) || (b.nlaunch > 0 && f.mlog.download((size_t)b.nlaunch * M * MON_NQ, kStream)) || rg_stream_sync(kStream))) {
    for (int m : R) e->ctx[(size_t)m]->rec.forget();
    return efail(e, RGPU_EHIP, std::string("ensemble_run_steps: read-back of the records: ") + rg_last_error_string());
  }
  int advanced = 0;
  for (int m : R) {
    rgpu_ctx* c = e->ctx[(size_t)m];
    const StepClock* rec = f.clk.h + m;   // of round r: rec[r * M]
    const int n0 = run.nStep[m];
    int r = 0;
    for (; r < b.queued && rec[(size_t)r * M].stop == 0; ++r) {   // t accumulated in the order of the reference's loop
      const double d = rec[(size_t)r * M].dt;
      run.dt[m] = d;
      run.t[m] += d;
      if (run.dt_log) run.dt_log[(size_t)m * run.nsteps + run.done[m] + r] = d;
      const int slot = b.launch_of_round[(size_t)r];
      if (run.mon && slot >= 0 && (n0 + r + 1) % run.mon->every == 0)   // exactly the slots the kernels filled: this step ran and qualifies
        run.put(m, n0 + r + 1, run.t[m], f.mlog.h + ((size_t)slot * M + m) * MON_NQ);
    }
    run.nStep[m] += r;
    c->cur = run.nStep[m] & 1;
    run.done[m] += r;
    if (r > advanced) advanced = r;
    if (r < b.queued) {   // its later steps were no-ops: the state of step n0 + r is the last one written, slots and ghost cells are still its
      run.code[m] = rec[(size_t)r * M].stop;
      c->rec.stopped_at((n0 + r) % 2, true);
      if (run.code[m] >= 2) c->err = stop_message(run.code[m]);
    }
  }
  run.fused += advanced;
  if (b.failed) {
    for (int m : R) e->ctx[(size_t)m]->rec.forget();
    return efail(e, RGPU_EHIP, "ensemble_run_steps: queueing a fused round: " + b.launch_err);
  }
  return RGPU_OK;
}

// One batch of fused rounds, at most `left` of them, for the members R that fused_batch_possible accepted: *queued (0 on entry) of them were queued
// (and count as rounds of the call, whatever is returned).  First what the batch reads besides the states, on the device before its
// first launch: every member's span (a member that is not in R gets tEnd = -inf: its first record says stop), the table where one is
// used, with sampling every member's step number at the start, for the kernels' "is this step of member m a multiple of every"
int fused_batch(EnsembleRun& run, const std::vector<int>& R, int par, int phase, int left, int* queued) {
  rgpu_ensemble* e = run.e;
  EnsembleFused& f = e->fused;
  const size_t M = (size_t)e->members;
  if (!f.clk.allocated() && (f.clk.alloc((size_t)rgpu_ctx::kClockBatch * M) || f.span.alloc(M))) {
    f.clk.release();
    return efail(e, RGPU_ENOMEM, "ensemble_run_steps: allocation of the clock records failed");
  }
  for (size_t m = 0; m < M; ++m) { f.span.h[m].t0 = 0.0; f.span.h[m].tEnd = -HUGE_VAL; }
  for (int m : R) { f.span.h[m].t0 = run.t[m]; f.span.h[m].tEnd = run.end_of(m); }
  if (f.span.upload(M, kStream)) return efail(e, RGPU_EHIP, std::string("ensemble_run_steps: ") + rg_last_error_string());
  const rgpu_tiled::MemberConst* tab = 0;
  if (const int rc = ensemble_table(e, "ensemble_run_steps", &tab)) return rc;
  if (run.mon) {
    if (const int rc = ensemble_monitor_buffers(e, "ensemble_run_steps")) return rc;
    for (size_t m = 0; m < M; ++m) { f.mspan.h[m].nStep0 = run.nStep[m]; f.mspan.h[m].parity = -1; }
    if (f.mspan.upload(M, kStream)) return efail(e, RGPU_EHIP, std::string("ensemble_run_steps: ") + rg_last_error_string());
  }
  FusedBatch b;
  fused_batch_queue(run, R, par, phase, left < (int)rgpu_ctx::kClockBatch ? left : (int)rgpu_ctx::kClockBatch, tab, &b);
  *queued = b.queued;
  return fused_batch_harvest(run, R, b);
}

// rgpu_ensemble_monitor: one kernel pair for all members (hip/ensemble_monitor.h, outside a batch: no records, each member's own
// parity), one read-back
int ensemble_monitor_all(rgpu_ensemble* e, double* out) {
  EnsembleFused& f = e->fused;
  const size_t M = (size_t)e->members;
  if (const int rc = ensemble_monitor_buffers(e, "ensemble_monitor")) return rc;
  const rgpu_tiled::MemberConst* tab = 0;
  if (const int rc = ensemble_table(e, "ensemble_monitor", &tab)) return rc;
  for (size_t m = 0; m < M; ++m) { f.mspan.h[m].nStep0 = 0; f.mspan.h[m].parity = e->ctx[m]->cur; }
  if (f.mspan.upload(M, kStream) || rgpu_tiled::launch_ensemble_monitor(kStream, (int)M, e->ctx[0]->g, tab, e->U, (unsigned)e->stride, f.mspan.d, 0, 0, 1, -1, f.mpart.d, f.mlog.d, 0u) ||
      f.mlog.download(M * MON_NQ, kStream) || rg_stream_sync(kStream))
    return efail(e, RGPU_EHIP, std::string("ensemble_monitor: ") + rg_last_error_string());
  std::memcpy(out, f.mlog.h, M * MON_NQ * sizeof(double));
  return RGPU_OK;
}

// device bytes per member: the clock records and spans of the fused rounds; the table of a scan; the monitor buffers (pinned mirrors not counted)
size_t fused_bytes_per_member() { return (size_t)rgpu_ctx::kClockBatch * sizeof(StepClock) + sizeof(rgpu_tiled::EnsembleSpan); }
size_t fused_table_bytes_per_member() { return sizeof(rgpu_tiled::MemberConst); }
size_t fused_monitor_bytes_per_member(const rgpu_params& p) {
  return sizeof(rgpu_tiled::MonitorSpan) + (monitor_part_doubles(p) + (size_t)rgpu_ctx::kClockBatch * MON_NQ) * sizeof(double);
}
}  // namespace
