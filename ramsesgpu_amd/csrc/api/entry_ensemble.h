// api/entry_ensemble.h -- entry points: an ensemble of 2D boxes (rgpu_ensemble_*): members of one shape and one solver configuration,
// each an ordinary rgpu_ctx over a slice of the ensemble's storage, advanced together -- where the step is one fused kernel with the
// time step on the device (entry_clock.h: clock_ready), by ONE step launch and ONE clock launch per step for all of them
// (hip/ensemble2d.h); everywhere else member by member through the single-context loop.  Either way every member gets exactly what
// rgpu_run_steps_log gives a lone context holding its state.
#pragma once

struct rgpu_ensemble {
  int members, device;
  std::vector<rgpu_ctx*> ctx;
  double* U;                     // state of member m, parity q: U + (q * members + m) * stride
  size_t stride;                 // doubles between the states of two members (ncell * nbVar rounded up to whole 128-byte lines)
  unsigned long long* slots;     // members x 3 x RG_DT_SLOTS: the members' d_red_base
#ifdef RGPU_TILED_ENSEMBLE2D
  StepClock *d_clk, *h_clk;      // records of a batch, tick-major: tick n of member m at [n * members + m]
  rgpu_tiled::EnsembleSpan *d_span, *h_span;
#endif
  std::string err;
};

namespace {
int efail(rgpu_ensemble* e, int code, const std::string& msg) {
  if (e) e->err = msg;
  return code;
}
size_t ensemble_stride(const rgpu_params& p) {
  const size_t n = (size_t)(p.nx + 2 * p.ghostWidth) * (size_t)(p.ny + 2 * p.ghostWidth) * (size_t)p.nbVar;
  return (n + 15) & ~(size_t)15;
}
// what rgpu_ensemble_create accepts (besides what rgpu_create accepts)
int ensemble_validate(const rgpu_params* p, int members, std::string* why) {
  if (members < 1 || members > RGPU_ENSEMBLE_MAX_MEMBERS) { *why = "ensemble: members must be 1 .. " + std::to_string(RGPU_ENSEMBLE_MAX_MEMBERS); return RGPU_EINVAL; }
  if (const int vr = validate(p, why)) return vr;
  if (p->nz_global != 1) { *why = "ensemble: 2D boxes only (nz_global must be 1); 3D boxes fill the device alone"; return RGPU_EUNSUPPORTED; }
  if ((double)ensemble_stride(*p) >= 4294967295.0) { *why = "ensemble: more than 2^32 doubles per member"; return RGPU_EUNSUPPORTED; }
  if (p->slab_count != 1) { *why = "ensemble: a slab of a larger box (slab_count > 1) cannot be a member"; return RGPU_EUNSUPPORTED; }
  return RGPU_OK;
}
#ifdef RGPU_TILED_ENSEMBLE2D
// the step of this member is one fused kernel that reads the device record and leaves CFL maxima and ghost images (whatever its state
// is at the moment: clock_ready says whether the state at hand came out of such a kernel)
bool ensemble_member_fusable(rgpu_ctx* c) {
  if (c->g.three_d || !clock_config_ok(c)) return false;
  if (c->p.mhdEnabled) return mhd2d_images(c) && rgpu_tiled::mhd2d_step_covers(c->g);
  return hydro2d_images(c) != 0 && rgpu_tiled::hydro2d_step_covers(c->g);
}
#endif
}  // namespace

extern "C" {

int rgpu_ensemble_create(const rgpu_params* p, int members, rgpu_ensemble** out) {
  if (!out) return RGPU_EINVAL;
  *out = 0;
  rgpu_ensemble* e = new (std::nothrow) rgpu_ensemble();
  if (!e) return RGPU_ENOMEM;
  *out = e;   // returned even on failure so that rgpu_ensemble_last_error can be read; the caller destroys it
  e->members = 0; e->device = -1; e->U = 0; e->stride = 0; e->slots = 0;
#ifdef RGPU_TILED_ENSEMBLE2D
  e->d_clk = e->h_clk = 0; e->d_span = e->h_span = 0;
#endif
  std::string why;
  if (const int vr = ensemble_validate(p, members, &why)) return efail(e, vr, why);
  if (rg_device_count() < 1) return efail(e, RGPU_ENODEVICE, "no HIP device: this library has no CPU fallback (backend " RG_BACKEND_NAME ")");
  e->device = rg_current_device();
  e->stride = ensemble_stride(*p);
  const size_t M = (size_t)members, state_bytes = 2 * M * e->stride * sizeof(double);
  const rg_stream_t s = (rg_stream_t)0;   // the ensemble's one stream: the one rgpu_create gives a lone context
  if (rg_malloc((void**)&e->U, state_bytes) || rg_malloc((void**)&e->slots, M * 3 * RG_DT_SLOTS * sizeof(unsigned long long)) || rg_memset_async(e->U, 0, state_bytes, s))
    return efail(e, RGPU_ENOMEM, "ensemble: device allocation of the state arrays failed");
  e->ctx.reserve(M);
  for (size_t m = 0; m < M; ++m) {
    rgpu_ctx* c = 0;
    const int rc = create_common(p, e->U + m * e->stride, e->U + (M + m) * e->stride, 0, true, &c, e->slots + m * 3 * RG_DT_SLOTS);
    if (c) { c->borrowed = true; e->ctx.push_back(c); }
    if (rc) return efail(e, rc, "ensemble: member " + std::to_string(m) + ": " + (c ? c->err : std::string("allocation failed")));
  }
  e->members = members;
  return RGPU_OK;
}

void rgpu_ensemble_destroy(rgpu_ensemble* e) {
  if (!e) return;
  if (e->device >= 0) rg_set_device(e->device);
  for (rgpu_ctx* c : e->ctx) {
    c->borrowed = false;
    c->d_red_base = 0; c->d_red = 0;   // a slice of e->slots
    rgpu_destroy(c);
  }
  rg_free(e->U); rg_free(e->slots);
#ifdef RGPU_TILED_ENSEMBLE2D
  rg_free(e->d_clk); rg_free(e->d_span);
  if (e->h_clk) rg_host_free(e->h_clk);
  if (e->h_span) rg_host_free(e->h_span);
#endif
  delete e;
}

int rgpu_ensemble_members(rgpu_ensemble* e) { return e ? e->members : 0; }
rgpu_ctx* rgpu_ensemble_member(rgpu_ensemble* e, int m) { return (e && m >= 0 && m < e->members) ? e->ctx[(size_t)m] : 0; }
const char* rgpu_ensemble_last_error(rgpu_ensemble* e) { return e ? e->err.c_str() : "null ensemble"; }

size_t rgpu_ensemble_device_bytes(const rgpu_params* p, int members) {
  std::string why;
  if (ensemble_validate(p, members, &why)) return 0;
  const size_t n = (size_t)(p->nx + 2 * p->ghostWidth) * (size_t)(p->ny + 2 * p->ghostWidth) * (size_t)p->nbVar;
  size_t per_member = rgpu_device_bytes(p) + 2 * (ensemble_stride(*p) - n) * sizeof(double) + 3 * RG_DT_SLOTS * sizeof(unsigned long long);
#ifdef RGPU_TILED_ENSEMBLE2D
  // the clock records and batch spans of the fused rounds, allocated by the first rgpu_ensemble_run_steps that takes one (as many again
  // in pinned host memory)
  per_member += (size_t)rgpu_ctx::kClockBatch * sizeof(StepClock) + sizeof(rgpu_tiled::EnsembleSpan);
#endif
  return (size_t)members * per_member;
}

int rgpu_ensemble_run_steps(rgpu_ensemble* e, int nsteps, const double* tEnd, int* nStep, double* t, double* dt, double* dt_log, int* done, int* stop, int* fused_steps) {
  if (!e) return RGPU_EINVAL;
  if (e->members < 1) return efail(e, RGPU_EINVAL, "ensemble_run_steps: the ensemble was not created");
  if (!nStep || !t || !dt || !done) return efail(e, RGPU_EINVAL, "ensemble_run_steps: null pointer");
  rg_set_device(e->device);
  const int M = e->members;
  std::vector<int> code((size_t)M, 0);      // why member m left the loop before its nsteps were done: 0 = it did not, or 1 / 2 / 3 of its record
  std::vector<char> halted((size_t)M, 0);
  for (int m = 0; m < M; ++m) done[m] = 0;
  int fused = 0;
  auto end_of = [&](int m) { return tEnd ? tEnd[m] : HUGE_VAL; };
  auto running = [&](int m) { return !halted[m] && done[m] < nsteps && t[m] < end_of(m); };
  auto finish = [&](int rc) {
    if (stop) for (int m = 0; m < M; ++m) stop[m] = code[m] >= 2 ? code[m] : (t[m] < end_of(m) ? 0 : 1);
    if (fused_steps) *fused_steps = fused;
    return rc;
  };
  // up to k steps of member m alone: the single-context loop, device clock and all
  auto alone = [&](int m, int k) -> int {
    rgpu_ctx* c = e->ctx[(size_t)m];
    const int n0 = nStep[m];
    int why = 0;
    const int r = run_steps_impl(c, k, end_of(m), nStep + m, t + m, dt + m, dt_log ? dt_log + (size_t)m * nsteps + done[m] : 0, &why);
    done[m] += nStep[m] - n0;
    if (r == RGPU_EHIP && !why) {
      // a plain step of the single-context loop failed: was it a time step that is not a number (nothing was launched then and the
      // scan can be asked again)?  That is this member's business (stop code 2); anything else ends the call.  Asked here and not in
      // the loop that lone contexts share, which reports such a failure as it always did
      double inv = 0.0;
      if (rgpu_compute_inv_dt(c, nStep[m] % 2, &inv) == RGPU_OK && !(c->p.cfl / inv == c->p.cfl / inv)) {
        why = 2;
        c->err = "run_steps: the time step is not a number";
      }
    }
    if (why) { code[m] = why; halted[m] = 1; }
    if (r < 0 && why < 2) return efail(e, r, "ensemble_run_steps: member " + std::to_string(m) + ": " + c->err);
    return 0;
  };
  std::vector<int> R;
  R.reserve((size_t)M);
  for (int round = 0;;) {   // every member that still runs has done `round` steps of this call
    R.clear();
    for (int m = 0; m < M; ++m) if (running(m)) R.push_back(m);
    if (R.empty()) break;
    const int left = nsteps - round;
    bool fusable = false, transient = false;
    int par = -1, phase = -1;
    (void)par; (void)phase;
#ifdef RGPU_TILED_ENSEMBLE2D
    fusable = true;
    for (int m : R) fusable = fusable && ensemble_member_fusable(e->ctx[(size_t)m]);
    if (fusable) {
      for (int m : R) {
        rgpu_ctx* c = e->ctx[(size_t)m];
        if (!clock_ready(c, nStep[m] % 2)) { transient = true; continue; }   // (its first step of a run, a state written from outside)
        const int ph = (int)((c->d_red - c->d_red_base) / RG_DT_SLOTS);      // which of its three slot arrays holds the maxima (a lone folded run rotates them)
        if (par < 0) { par = nStep[m] % 2; phase = ph; }
        else if (par != nStep[m] % 2 || phase != ph) fusable = false;
      }
      if (transient) fusable = false;
    }
#endif
    if (!fusable) {
      // a member that is not clock-ready becomes so by one plain step: one round member by member, then look again.  Anything else
      // (a configuration the fused path does not cover, members of mixed step parity) does not change: each member runs on alone
      const int k = transient ? 1 : left;
      for (int m : R) if (const int rc = alone(m, k)) return finish(rc);
      round += k;
      continue;
    }
#ifdef RGPU_TILED_ENSEMBLE2D
    // ---- one batch of fused rounds: tick, then step, for all members; one read-back of the records (as rgpu_run_steps_log) ----
    const int kBatch = (int)rgpu_ctx::kClockBatch;
    const rg_stream_t s = (rg_stream_t)0;
    if (!e->d_clk) {
      const size_t nrec = (size_t)kBatch * M;
      if (rg_malloc((void**)&e->d_clk, nrec * sizeof(StepClock)) || rg_host_alloc((void**)&e->h_clk, nrec * sizeof(StepClock)) ||
          rg_malloc((void**)&e->d_span, (size_t)M * sizeof(rgpu_tiled::EnsembleSpan)) || rg_host_alloc((void**)&e->h_span, (size_t)M * sizeof(rgpu_tiled::EnsembleSpan)))
        return finish(efail(e, RGPU_ENOMEM, "ensemble_run_steps: allocation of the clock records failed"));
    }
    for (int m = 0; m < M; ++m) { e->h_span[m].t0 = 0.0; e->h_span[m].tEnd = -HUGE_VAL; }   // not in this batch: its first record says stop
    for (int m : R) { e->h_span[m].t0 = t[m]; e->h_span[m].tEnd = end_of(m); }
    if (rg_copy_h2d(e->d_span, e->h_span, (size_t)M * sizeof(rgpu_tiled::EnsembleSpan), s)) return finish(efail(e, RGPU_EHIP, std::string("ensemble_run_steps: ") + rg_last_error_string()));
    rgpu_ctx* c0 = e->ctx[(size_t)R[0]];
    DevParams g = c0->g;
    g.hdt = 0.0; g.hgx = 0.0; g.hgy = 0.0; g.hgz = 0.0;   // (no gravity on this path)
    const ClockConst kc = clock_const(c0);
    const RotCoef rotc = rot_coef(c0, 0.0);
    const int images = c0->p.mhdEnabled ? 1 : hydro2d_images(c0);
    unsigned long long* slots = e->slots + (size_t)phase * RG_DT_SLOTS;
    const size_t pool = (size_t)M * e->stride;
    const unsigned stride = (unsigned)e->stride;
    const int nb = left < kBatch ? left : kBatch;
    int queued = 0, rc = 0;
    for (; queued < nb; ++queued) {
      StepClock* rec = e->d_clk + (size_t)queued * M;
      if (rgpu_tiled::launch_ensemble_clock(s, M, slots, kc, e->d_span, queued ? rec - M : 0, rec)) { rc = -1; break; }
      const int pin = (par + queued) % 2, pout = 1 - pin;
      for (int m : R) { e->ctx[(size_t)m]->rec.drop_scan(); e->ctx[(size_t)m]->rec.drop_ghosts(); }   // the output arrays are about to change
      const double* in = e->U + (size_t)pin * pool;
      double* out = e->U + (size_t)pout * pool;
      const int rs = c0->p.mhdEnabled ? rgpu_tiled::mhd2d_ensemble_step<kSpecPlain>(s, M, g, rotc, pick_spec(g) == 2, in, out, stride, slots, images, rec)
                                      : rgpu_tiled::hydro2d_ensemble_step(s, M, g, in, out, stride, slots, images, rec);
      if (rs) { rc = -1; break; }
      for (int m : R) { e->ctx[(size_t)m]->rec.scanned(pout, RG_DT_SLOTS); e->ctx[(size_t)m]->rec.ghosts_written(pout); }
    }
    // a launch that failed after `queued` complete rounds were queued: those still run -- read their records and advance the members
    // for them before reporting (as rgpu_run_steps_log)
    const std::string launch_err = rc ? std::string(rg_last_error_string()) : std::string();
    if (queued > 0 && (rg_copy_d2h(e->h_clk, e->d_clk, (size_t)queued * M * sizeof(StepClock), s) || rg_stream_sync(s))) {
      for (int m : R) e->ctx[(size_t)m]->rec.forget();
      return finish(efail(e, RGPU_EHIP, std::string("ensemble_run_steps: read-back of the records: ") + rg_last_error_string()));
    }
    int advanced = 0;
    for (int m : R) {
      rgpu_ctx* c = e->ctx[(size_t)m];
      const int n0 = nStep[m];
      int r = 0;
      for (; r < queued && e->h_clk[(size_t)r * M + m].stop == 0; ++r) {   // t accumulated in the order of the reference's loop
        const double d = e->h_clk[(size_t)r * M + m].dt;
        dt[m] = d;
        t[m] += d;
        if (dt_log) dt_log[(size_t)m * nsteps + done[m] + r] = d;
      }
      nStep[m] += r;
      done[m] += r;
      if (r > advanced) advanced = r;
      if (r < queued) {   // its later steps were no-ops: the state of step n0 + r is the last one written, slots and ghost cells are still its
        code[m] = e->h_clk[(size_t)r * M + m].stop;
        halted[m] = 1;
        c->rec.stopped_at((n0 + r) % 2, true);
        if (code[m] >= 2) c->err = code[m] == 2 ? "run_steps: the time step is not a number" : "run_steps: 1/dt is not finite";
      }
    }
    fused += advanced;
    round += queued;
    if (rc) {
      for (int m : R) e->ctx[(size_t)m]->rec.forget();
      return finish(efail(e, RGPU_EHIP, "ensemble_run_steps: queueing a fused round: " + launch_err));
    }
#endif
  }
  return finish(RGPU_OK);
}

}  // extern "C"
