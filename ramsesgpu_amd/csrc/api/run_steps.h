// api/run_steps.h -- entry points: the time loop of a lone context (rgpu_run_steps, _log, _history, _monitored, _monitored_planes, _mapped, _pdfs, _spectra, _helm_spectra; every member-alone round
// of an ensemble comes through here too).  One LoneRun per call; per turn either the reference's loop body (literal_turn) or a batch
// of device-clock steps (api/entry_clock.h), queued by batch_queue and read back once by batch_harvest.  The two optional consumers
// of a step -- the history row in front of it, the monitor sample behind it -- each write the caller's arrays in one place, put().
#pragma once

namespace {
// what rgpu_run_steps_history adds to the loop: the history cadence and where the samples go (see include/rgpu.h)
struct HistRun {
  double dtHist; double* tHist;
  int* n; int* step; double* t; double* dt; double* v;   // *n samples so far; step[k], t[k], dt[k], v[k][RGPU_HIST_NQ]
  bool batch;                                            // option "history_batch": sample on the device inside the device-clock batches
  void put(int step_no, double ts, double dts, const double* row) const {
    const int k = (*n)++;
    step[k] = step_no; t[k] = ts; dt[k] = dts;
    std::memcpy(v + (size_t)k * RGPU_HIST_NQ, row, RGPU_HIST_NQ * sizeof(double));
  }
};
static_assert((int)HIST_BATCH_NQ == RGPU_HIST_NQ, "include/rgpu.h states the width of a history row");

// what rgpu_run_steps_monitored, rgpu_run_steps_monitored_planes, rgpu_run_steps_mapped and rgpu_run_steps_pdfs add to the loop: the
// cadence in steps, which of the four samples is taken -- the monitor's RGPU_MON_NQ doubles, the plane monitor's nz x RGPU_MONP_NQ,
// the maps of `what.specs`, or the tables of counts of `what.pdf` -- and where the samples go (see include/rgpu.h).  One consumer, four
// samples: api/monitor.h chooses the launches, the log and its slots by `what`.  The words of a sample are 8 bytes wide, doubles or
// counts, and only ever copied here: the caller's array of counts stands in `v` as the others do
struct MonRun {
  int every; MonSample what; size_t width;   // width: the 8-byte words of a sample
  int* n; int* step; double* t; double* v;   // *n samples so far; step[k], t[k], v[k][width]
  const char* who;                           // the entry point, for messages
  bool due(int step_no) const { return step_no % every == 0; }   // the state step number step_no names is sampled
  double* slot() const { return v + (size_t)*n * width; }        // where the values of the next sample go
  void put(int step_no, double ts) const {                        // the values are in slot()
    const int k = (*n)++;
    step[k] = step_no; t[k] = ts;
  }
};

// One call of rgpu_run_steps*: the caller's arrays and what the pieces of the loop share
struct LoneRun {
  rgpu_ctx* c;
  int nsteps; double tEnd;
  int* nStep; double* t; double* dt; double* dt_log;   // dt_log may be 0
  const HistRun* hist;   // 0, or rgpu_run_steps_history
  const MonRun* mon;     // 0, or rgpu_run_steps_monitored
  bool forced = false;   // forcing_clock_ok(c), asked once per call: the batches of this call carry the forcing stages (api/forcing.h)
  int done = 0;          // steps of this call so far
  int why = 0;           // 0, or the stop code of the record that ended the run (1: tEnd, 2: dt is not a number, 3: 1/dt is not finite --
                         // the last two are also reported as RGPU_EHIP)
};

// the reference's loop body, with the head of MHDRunGodunov.cpp:3975-3984 in front of the step, literally, and the monitor of the
// state the step left, U[*nStep % 2], behind it (one synchronisation per sample on this path)
int literal_turn(LoneRun& run) {
  rgpu_ctx* c = run.c;
  const HistRun* H = run.hist;
  if (H && hist_batch_due(*run.t, *run.dt, *H->tHist, H->dtHist)) {
    double row[RGPU_HIST_NQ];
    if (const int rc = rgpu_history_mri(c, *run.nStep % 2, row)) return rc;
    H->put(*run.nStep, *run.t, *run.dt, row);
    *H->tHist += H->dtHist;
  }
  if (const int rc = rgpu_one_step_integration(c, run.nStep, run.t, run.dt)) return rc;
  if (run.dt_log) run.dt_log[run.done] = *run.dt;
  ++run.done;
  if (run.mon && run.mon->due(*run.nStep)) {
    const MonRun* M = run.mon;
    const int par = *run.nStep & 1;
    if (const int rc = M->what.what == MON_HELM ? helm_take(c, M->who, par, *M->what.helm, M->slot())
                     : M->what.what == MON_SPECTRA ? spectra_take(c, M->who, par, *M->what.spec, M->slot())
                     : M->what.what == MON_PDFS ? pdfs_take(c, M->who, par, *M->what.pdf, M->slot())
                     : M->what.what == MON_MAPS ? state_maps(c, par, M->what.nmaps, M->what.specs, M->slot())
                     : M->what.what == MON_PLANES ? state_monitor_planes(c, par, M->slot()) : state_monitor(c, c->g.three_d != 0, par, M->slot())) return rc;
    M->put(*run.nStep, *run.t);
  }
  return RGPU_OK;
}

// what queueing a batch leaves for its harvest
struct LoneBatch {
  int queued = 0;                                // steps queued completely (their records are read back)
  int samples = 0;                               // monitor samples queued behind them: slots [0, samples) of the log, in step order
  bool failed = false; std::string launch_err;   // a launch failed behind the `queued` steps, with this message
  bool forced = false; ForcingBatch fb;          // the steps carry forcing stages (api/forcing.h): what their open leaves for their close
};

// Opens a batch and queues up to m steps: per step the tick, the history head of U[n % 2] (taken on the device if the record and the
// log say so, kernels_history.h), the pieces of the step == rgpu_godunov_unsplit for this configuration, every dt / t dependence read
// from the record on the device, and the monitor of U[(n + 1) % 2] behind the step's last kernel (taken if the record says that the
// step ran).  A forced context (forcing_clock_ok): its forcing stages behind the core, where rgpu_godunov_unsplit has them.
// != 0: the batch could not be opened, nothing was queued
int batch_queue(LoneRun& run, int m, LoneBatch* b) {
  rgpu_ctx* c = run.c;
  const HistRun* H = run.hist;
  const MonRun* M = run.mon;
  // the logs of a batch: allocated by the first call that needs them
  if (M && monitor_batch_alloc(c, M->what, M->every)) return RG_HIPFAIL(c, std::string(M->who) + ": log of the batch");
  if (H && !c->hist.allocated() && c->hist.alloc(rgpu_ctx::kClockBatch)) return RG_HIPFAIL(c, "run_steps_history: log of the batch");
  if (const int rc = clock_open(c, *run.t, run.tEnd, true)) return rc;
  b->forced = run.forced;
  if (b->forced && forcing_batch_open(c, m, &b->fb)) { c->clk_n = -1; return RG_HIPFAIL(c, "run_steps: tables of the forcing stages"); }
  const int n0 = *run.nStep;
  const double dt0 = *run.dt;   // the loop's *dt at the head of the batch's first step
  int rc = 0;
  for (; b->queued < m; ++b->queued) {
    if ((rc = rgpu_clock_tick(c)) != 0) break;
    if (stop_now(c)) { ++b->queued; break; }   // (host emulation: the record is already there and says the loop has ended)
    const int slot = b->queued, n = n0 + slot;
    if (!clock_ready(c, n % 2)) rc = RGPU_EHIP;   // (cannot happen: the step before left its CFL maxima and, in 2D, its ghost cells)
    if (rc == 0 && H && history_batch_queue(c, n, slot, dt0, *H->tHist, H->dtHist)) rc = RGPU_EHIP;
    if (rc == 0) rc = (step_pre(c, n) || step_core(c, n, 0.0, 0.0) || (b->forced && forcing_batch_step(c, n, slot)) || step_post_a(c, n, 0.0, 0.0) || step_post_b(c, n)) ? RGPU_EHIP : 0;
    if (rc == 0 && !c->rec.slots((n + 1) % 2)) rc = RGPU_EHIP;   // (cannot happen: same configuration, same kernels)
    if (rc == 0 && M && M->due(n + 1)) {
      if (monitor_batch_queue(c, M->what, (n + 1) & 1, b->samples)) rc = RGPU_EHIP;
      else ++b->samples;
    }
    if (rc) { c->clk_n = slot; break; }   // the record of the step that failed to queue is not read back
  }
  if (rc) { b->failed = true; b->launch_err = c->err + " " + rg_last_error_string(); }
  return RGPU_OK;
}

// Reads back what the batch left and advances the run for the steps that ran.  A launch that failed after b.queued complete steps were
// queued: those steps still run on the device -- their records are read and nStep / t / dt advanced for them before the failure is
// reported, so that the caller's step count and parity describe the device state.  != 0: the code that ends the call
int batch_harvest(LoneRun& run, const LoneBatch& b) {
  rgpu_ctx* c = run.c;
  const HistRun* H = run.hist;
  const MonRun* M = run.mon;
  const int queued = b.queued, n0 = *run.nStep;
  // the logs travel with the clock records: queued behind them here, complete after the one synchronisation of rgpu_clock_close.  A
  // history record behind the last head queued, a monitor slot whose step did not run: copied unwritten, not read
  const bool log_ok = !H || queued == 0 || c->hist.download((size_t)queued, c->stream) == 0;
  const bool mon_ok = !M || b.samples == 0 || monitor_batch_log(c, M->what).download((size_t)b.samples * M->width, c->stream) == 0;
  const bool frc_ok = !b.forced || forcing_batch_download(c) == 0;   // (the force of the Ornstein-Uhlenbeck process, likewise)
  const double t_open = *run.t;
  int ran = 0, stop = 0;
  if (const int rc = rgpu_clock_close(c, n0, &ran, run.t, run.dt, run.dt_log ? run.dt_log + run.done : 0, &stop)) {
    if (b.forced) forcing_batch_abandon(c, b.fb);
    return rc;
  }
  *run.nStep += ran;
  run.done += ran;
  if (b.forced) {
    if (!frc_ok) { forcing_batch_abandon(c, b.fb); c->rec.forget(); return fail(c, RGPU_EHIP, "run_steps: read-back of the forcing process"); }
    forcing_batch_close(c, b.fb, ran);
  }
  if (M && ran > 0) {   // the host knows the step numbers; that step n0 + r ran is what the records said
    if (!mon_ok) { c->rec.forget(); return fail(c, RGPU_EHIP, std::string(M->who) + ": read-back of the log"); }
    const double* log = monitor_batch_log(c, M->what).h;
    double ta = t_open;
    for (int r = 0, k = 0; r < ran; ++r) {
      ta += c->clk.h[r].dt;   // (*t as rgpu_clock_close accumulated it)
      if (!M->due(n0 + r + 1)) continue;
      std::memcpy(M->slot(), log + (size_t)k++ * M->width, M->width * sizeof(double));   // the k-th sample queued: the qualifying steps in order
      M->put(n0 + r + 1, ta);
    }
  }
  if (H && ran > 0) {   // a step that ran had its head queued in front of it: records [0, ran) are written
    if (!log_ok) { c->rec.forget(); return fail(c, RGPU_EHIP, "run_steps_history: read-back of the log"); }
    for (int r = 0; r < ran; ++r) {
      const HistBatchRec& hr = c->hist.h[r];
      if (hr.sampled) H->put(hr.step, hr.t, hr.dt, hr.v);
    }
    *H->tHist = c->hist.h[ran - 1].tHist;
  }
  if (b.failed) { c->rec.forget(); return fail(c, RGPU_EHIP, "run_steps: queueing a device-clock step: " + b.launch_err); }
  if (ran < queued) {
    run.why = stop;
    if (stop >= 2) return fail(c, RGPU_EHIP, stop_message(stop));
  }
  return RGPU_OK;
}

// the loop: per turn the literal body (the first step of a run always; a state without device maxima; consumers that cannot sample on
// the device) or one batch.  A forced context that is batched (forcing_clock_ok) is primed instead: a state without device maxima gets its
// scan queued, with no fetch, and the batch opens -- the first step of a run and the state a literal step left are batched too.
// Returns the steps done, or the code that ended the call -- *nStep, *t, *dt and the samples describe the steps that ran either way
int run_steps_impl(LoneRun& run) {
  rgpu_ctx* c = run.c;
  struct Current { rgpu_ctx* c; const int* n; ~Current() { c->cur = *n & 1; } } current = {c, run.nStep};   // however the loop is left: U[*nStep % 2] is the state
  (void)current;
  run.forced = forcing_clock_ok(c);
  const bool primed = run.forced && !run.hist;   // (rgpu_run_steps_history: the turbulence history is not the row a batch samples)
  while (run.done < run.nsteps && *run.t < run.tEnd && !run.why) {
    const int par = *run.nStep % 2;
    if (primed && !clock_ready(c, par) && !(run.mon && !monitor_sample_fits(c, run.mon->what))) {
      if (inv_dt_scan(c, par, 0, c->n32, true)) return RG_HIPFAIL(c, "run_steps: scan of a forced state");
      c->rec.scanned(par, 1);
    }
    if (!clock_ready(c, *run.nStep % 2) || (run.hist && run.forced) || (run.hist && !run.hist->batch) || (run.mon && !monitor_sample_fits(c, run.mon->what))) {
      if (const int rc = literal_turn(run)) return rc;
      continue;
    }
    const int left = run.nsteps - run.done;
    int m = left < (int)rgpu_ctx::kClockBatch ? left : (int)rgpu_ctx::kClockBatch;
    if (run.mon) m = monitor_batch_steps(c, run.mon->what, run.mon->every, *run.nStep, m);   // no more samples than the log has slots
    LoneBatch b;
    if (const int rc = batch_queue(run, m, &b)) return rc;
    if (const int rc = batch_harvest(run, b)) return rc;
  }
  return run.done;
}
}  // namespace

extern "C" {

int rgpu_run_steps_log(rgpu_ctx* c, int nsteps, double tEnd, int* nStep, double* t, double* dt, double* dt_log) {
  RG_CHECK_CTX(c);
  if (!nStep || !t || !dt) return fail(c, RGPU_EINVAL, "run_steps: null pointer");
  LoneRun run = {c, nsteps, tEnd, nStep, t, dt, dt_log, 0, 0};
  return run_steps_impl(run);
}

int rgpu_run_steps(rgpu_ctx* c, int nsteps, double tEnd, int* nStep, double* t, double* dt) {
  return rgpu_run_steps_log(c, nsteps, tEnd, nStep, t, dt, 0);
}

long rgpu_history_batch_heads(rgpu_ctx* c) { return c ? c->hist_heads : 0; }
long rgpu_forcing_batch_steps(rgpu_ctx* c) { return c ? c->forcing_steps : 0; }

int rgpu_run_steps_history(rgpu_ctx* c, int nsteps, double tEnd, int* nStep, double* t, double* dt, double* dt_log, double dtHist, double* tHist,
                           int* hist_n, int* hist_step, double* hist_t, double* hist_dt, double* hist) {
  RG_CHECK_CTX(c);
  if (!nStep || !t || !dt || !tHist || !hist_n || !hist_step || !hist_t || !hist_dt || !hist) return fail(c, RGPU_EINVAL, "run_steps_history: null pointer");
  *hist_n = 0;
  if (!c->U[0]) return fail(c, RGPU_EINVAL, "run_steps_history: context without state");
  if (!c->p.mhdEnabled) return fail(c, RGPU_EUNSUPPORTED, "run_steps_history: history diagnostics are defined for MHD runs");
  if (c->p.slab_count > 1) return fail(c, RGPU_EINVAL, "run_steps_history: slab contexts take their history through the slab driver");
  if (nsteps < 0) return fail(c, RGPU_EINVAL, "run_steps_history: nsteps is negative");
  const HistRun H = {dtHist, tHist, hist_n, hist_step, hist_t, hist_dt, hist, rgpu::options().history_batch != 0};
  LoneRun run = {c, nsteps, tEnd, nStep, t, dt, dt_log, &H, 0};
  return run_steps_impl(run);
}

long rgpu_monitor_batch_samples(rgpu_ctx* c) { return c ? c->mon_samples : 0; }

int rgpu_run_steps_monitored(rgpu_ctx* c, int nsteps, double tEnd, int* nStep, double* t, double* dt, double* dt_log, int every,
                             int* mon_n, int* mon_step, double* mon_t, double* mon) {
  RG_CHECK_CTX(c);
  if (!nStep || !t || !dt || !mon_n || !mon_step || !mon_t || !mon) return fail(c, RGPU_EINVAL, "run_steps_monitored: null pointer");
  *mon_n = 0;
  if (!c->U[0]) return fail(c, RGPU_EINVAL, "run_steps_monitored: context without state");
  if (c->p.slab_count > 1) return fail(c, RGPU_EINVAL, "run_steps_monitored: single-domain contexts only (a slab holds a part of the box)");
  if (nsteps < 0) return fail(c, RGPU_EINVAL, "run_steps_monitored: nsteps is negative");
  if (every < 1) return fail(c, RGPU_EINVAL, "run_steps_monitored: every must be at least 1");
  const MonRun M = {every, {MON_MONITOR, 0, 0, 0, 0}, (size_t)RGPU_MON_NQ, mon_n, mon_step, mon_t, mon, "run_steps_monitored"};
  LoneRun run = {c, nsteps, tEnd, nStep, t, dt, dt_log, 0, &M};
  return run_steps_impl(run);
}

long rgpu_monitor_planes_batch_samples(rgpu_ctx* c) { return c ? c->monp_samples : 0; }

int rgpu_run_steps_monitored_planes(rgpu_ctx* c, int nsteps, double tEnd, int* nStep, double* t, double* dt, double* dt_log, int every,
                                    int* mon_n, int* mon_step, double* mon_t, double* mon) {
  RG_CHECK_CTX(c);
  if (!nStep || !t || !dt || !mon_n || !mon_step || !mon_t || !mon) return fail(c, RGPU_EINVAL, "run_steps_monitored_planes: null pointer");
  *mon_n = 0;
  if (!c->U[0]) return fail(c, RGPU_EINVAL, "run_steps_monitored_planes: context without state");
  if (!c->g.three_d) return fail(c, RGPU_EUNSUPPORTED, "run_steps_monitored_planes: 3D contexts only (the rows are the interior planes of a volume)");
  if (c->p.slab_count > 1) return fail(c, RGPU_EINVAL, "run_steps_monitored_planes: single-domain contexts only (a slab holds a part of the box)");
  if (nsteps < 0) return fail(c, RGPU_EINVAL, "run_steps_monitored_planes: nsteps is negative");
  if (every < 1) return fail(c, RGPU_EINVAL, "run_steps_monitored_planes: every must be at least 1");
  if (!monitor_planes_scratch_fits(c)) return fail(c, RGPU_EINVAL, "run_steps_monitored_planes: no scratch for the partial sums");
  const MonRun M = {every, {MON_PLANES, 0, 0, 0, 0}, monp_sample_doubles(c->g), mon_n, mon_step, mon_t, mon, "run_steps_monitored_planes"};
  LoneRun run = {c, nsteps, tEnd, nStep, t, dt, dt_log, 0, &M};
  return run_steps_impl(run);
}

long rgpu_map_batch_samples(rgpu_ctx* c) { return c ? c->monm_samples : 0; }

int rgpu_run_steps_mapped(rgpu_ctx* c, int nsteps, double tEnd, int* nStep, double* t, double* dt, double* dt_log, int every,
                          int nmaps, const rgpu_map_spec* specs, int* mon_n, int* mon_step, double* mon_t, double* maps) {
  RG_CHECK_CTX(c);
  if (mon_n) *mon_n = 0;
  if (!nStep || !t || !dt || !specs || !mon_n || !mon_step || !mon_t || !maps) return fail(c, RGPU_EINVAL, "run_steps_mapped: null pointer");
  if (const int rc = maps_refusal(c, "run_steps_mapped", nmaps, specs)) return rc;
  if (nsteps < 0) return fail(c, RGPU_EINVAL, "run_steps_mapped: nsteps is negative");
  if (every < 1) return fail(c, RGPU_EINVAL, "run_steps_mapped: every must be at least 1");
  const MonSample S = {MON_MAPS, nmaps, specs, 0, 0};
  const MonRun M = {every, S, monitor_sample_doubles(c, S), mon_n, mon_step, mon_t, maps, "run_steps_mapped"};
  LoneRun run = {c, nsteps, tEnd, nStep, t, dt, dt_log, 0, &M};
  return run_steps_impl(run);
}

long rgpu_pdf_batch_samples(rgpu_ctx* c) { return c ? c->monh_samples : 0; }

int rgpu_run_steps_pdfs(rgpu_ctx* c, int nsteps, double tEnd, int* nStep, double* t, double* dt, double* dt_log, int every,
                        int npdfs, const rgpu_pdf_spec* specs, int* mon_n, int* mon_step, double* mon_t, unsigned long long* pdfs) {
  RG_CHECK_CTX(c);
  if (mon_n) *mon_n = 0;
  if (!nStep || !t || !dt || !specs || !mon_n || !mon_step || !mon_t || !pdfs) return fail(c, RGPU_EINVAL, "run_steps_pdfs: null pointer");
  PdfSet set;
  if (const int rc = pdfs_refusal(c, "run_steps_pdfs", npdfs, specs, &set)) return rc;
  if (nsteps < 0) return fail(c, RGPU_EINVAL, "run_steps_pdfs: nsteps is negative");
  if (every < 1) return fail(c, RGPU_EINVAL, "run_steps_pdfs: every must be at least 1");
  const MonSample S = {MON_PDFS, 0, 0, &set, 0};
  const MonRun M = {every, S, (size_t)set.words, mon_n, mon_step, mon_t, reinterpret_cast<double*>(pdfs), "run_steps_pdfs"};
  LoneRun run = {c, nsteps, tEnd, nStep, t, dt, dt_log, 0, &M};
  return run_steps_impl(run);
}

long rgpu_spectrum_batch_samples(rgpu_ctx* c) { return c ? c->mons_samples : 0; }

int rgpu_run_steps_spectra(rgpu_ctx* c, int nsteps, double tEnd, int* nStep, double* t, double* dt, double* dt_log, int every,
                           int nspec, const rgpu_spectrum_spec* specs, int* mon_n, int* mon_step, double* mon_t, double* spectra) {
  RG_CHECK_CTX(c);
  if (mon_n) *mon_n = 0;
  if (!nStep || !t || !dt || !specs || !mon_n || !mon_step || !mon_t || !spectra) return fail(c, RGPU_EINVAL, "run_steps_spectra: null pointer");
  SpecSet set;
  if (const int rc = spectra_refusal(c, "run_steps_spectra", nspec, specs, &set)) return rc;
  if (nsteps < 0) return fail(c, RGPU_EINVAL, "run_steps_spectra: nsteps is negative");
  if (every < 1) return fail(c, RGPU_EINVAL, "run_steps_spectra: every must be at least 1");
  const MonSample S = {MON_SPECTRA, 0, 0, 0, &set};
  const MonRun M = {every, S, (size_t)set.doubles, mon_n, mon_step, mon_t, spectra, "run_steps_spectra"};
  LoneRun run = {c, nsteps, tEnd, nStep, t, dt, dt_log, 0, &M};
  return run_steps_impl(run);
}

long rgpu_helm_batch_samples(rgpu_ctx* c) { return c ? c->monv_samples : 0; }

int rgpu_run_steps_helm_spectra(rgpu_ctx* c, int nsteps, double tEnd, int* nStep, double* t, double* dt, double* dt_log, int every,
                                int nspec, const rgpu_helm_spec* specs, int* mon_n, int* mon_step, double* mon_t, double* spectra) {
  RG_CHECK_CTX(c);
  if (mon_n) *mon_n = 0;
  if (!nStep || !t || !dt || !specs || !mon_n || !mon_step || !mon_t || !spectra) return fail(c, RGPU_EINVAL, "run_steps_helm_spectra: null pointer");
  HelmSet set;
  if (const int rc = helm_refusal(c, "run_steps_helm_spectra", nspec, specs, &set)) return rc;
  if (nsteps < 0) return fail(c, RGPU_EINVAL, "run_steps_helm_spectra: nsteps is negative");
  if (every < 1) return fail(c, RGPU_EINVAL, "run_steps_helm_spectra: every must be at least 1");
  const MonSample S = {MON_HELM, 0, 0, 0, 0, &set};
  const MonRun M = {every, S, (size_t)set.doubles, mon_n, mon_step, mon_t, spectra, "run_steps_helm_spectra"};
  LoneRun run = {c, nsteps, tEnd, nStep, t, dt, dt_log, 0, &M};
  return run_steps_impl(run);
}

}  // extern "C"
