// api/entry_ensemble.h -- entry points: an ensemble of 2D boxes (rgpu_ensemble_*): members of one shape and one solver configuration,
// each an ordinary rgpu_ctx over a slice of the ensemble's storage, advanced together -- where the step is one fused kernel with the
// time step on the device (entry_clock.h: clock_ready), by ONE step launch and ONE clock launch per step for all of them
// (hip/ensemble2d.h); everywhere else member by member through the single-context loop.  Either way every member gets exactly what
// rgpu_run_steps_log gives a lone context holding its state.
// A parameter scan (rgpu_ensemble_create_scan) is the same object with one parameter set per member: the sets share what selects code
// or shape (scan_validate), each member context is created from its own set, and the fused rounds read every member's constants from
// a table on the device (hip/ensemble_scan.h) instead of handing one member's to the kernels by value.
// Monitors (kernels_monitor.h): rgpu_ensemble_run_steps_monitored is the same loop with per-member samples of the ten monitor
// quantities -- on the fused rounds taken by a kernel pair queued inside the batch (hip/ensemble_monitor.h) and read back with the
// clock records, on the member-by-member rounds by the flat monitor of the member's context.
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
  // the constants of member m at [m] (by member, never by position in a batch), filled and copied once (ensemble_table) by the first
  // caller that reads them -- a fused round, or rgpu_ensemble_monitor outside any round, on the ensemble's stream before the kernels
  // that read it -- and never written again: the kernels read them through scalar loads (hip/ensemble_scan.h).  0: not yet
  rgpu_tiled::MemberConst *d_tab, *h_tab;
  // monitors, allocated by the first call that samples on the device: per member and batch its step number at the start (and, outside
  // a batch, the parity of its state); the segment sums of one launch; the log of a batch, slot (launch, m) -- the log as many again
  // in pinned host memory
  rgpu_tiled::MonitorSpan *d_mspan, *h_mspan;
  double *d_mpart, *d_mlog, *h_mlog;
#endif
  bool scan;                     // created by rgpu_ensemble_create_scan ...
  bool uniform;                  // ... all of whose sets are bytewise equal (always true for rgpu_ensemble_create)
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
// what rgpu_ensemble_create_scan accepts: every set what rgpu_ensemble_create accepts, and the sets alike in everything that selects
// code or shape -- the integers, slope_type, the sign classes of cIso, Omega0, nu and eta (what spec_matches, clock_config_ok,
// hydro2d_images and mhd2d_images look at).  Every other double may differ from member to member
int scan_validate(const rgpu_params* sets, int members, std::string* why) {
  if (members < 1 || members > RGPU_ENSEMBLE_MAX_MEMBERS) { *why = "ensemble: members must be 1 .. " + std::to_string(RGPU_ENSEMBLE_MAX_MEMBERS); return RGPU_EINVAL; }
  if (!sets) { *why = "ensemble: the array of parameter sets is NULL"; return RGPU_EINVAL; }
  const rgpu_params& a = sets[0];
  for (int m = 0; m < members; ++m) {
    const rgpu_params& b = sets[m];
    std::string w;
    if (const int vr = ensemble_validate(&b, members, &w)) { *why = "ensemble: member " + std::to_string(m) + ": " + w; return vr; }
    const char* field = 0;
#define RG_SHARED(F) if (!field && a.F != b.F) field = #F;
    RG_SHARED(abi_version) RG_SHARED(nx) RG_SHARED(ny) RG_SHARED(nz) RG_SHARED(ghostWidth) RG_SHARED(nbVar) RG_SHARED(mhdEnabled)
    RG_SHARED(bc[0]) RG_SHARED(bc[1]) RG_SHARED(bc[2]) RG_SHARED(bc[3]) RG_SHARED(bc[4]) RG_SHARED(bc[5])
    RG_SHARED(slope_type) RG_SHARED(niter_riemann) RG_SHARED(iorder) RG_SHARED(riemannSolver) RG_SHARED(magRiemannSolver)
    RG_SHARED(implementationVersion) RG_SHARED(unsplitVersion) RG_SHARED(shearingBoxEnabled) RG_SHARED(enableJet) RG_SHARED(ijet) RG_SHARED(offsetJet)
    RG_SHARED(slab_rank) RG_SHARED(slab_count) RG_SHARED(nz_global) RG_SHARED(gravityEnabled) RG_SHARED(zStratifiedFloor)
    RG_SHARED(randomForcingEnabled) RG_SHARED(ouForcingEnabled) RG_SHARED(ouInitRandom)
#undef RG_SHARED
    if (field) { *why = std::string("ensemble scan: ") + field + " of member " + std::to_string(m) + " differs from member 0's: the members of a scan share every integer field and slope_type"; return RGPU_EINVAL; }
#define RG_SIGN(F) if (!field && (a.F > 0) != (b.F > 0)) field = #F;
    RG_SIGN(cIso) RG_SIGN(Omega0) RG_SIGN(nu) RG_SIGN(eta)
#undef RG_SIGN
    if (field) { *why = std::string("ensemble scan: ") + field + " of member " + std::to_string(m) + " is > 0 where member 0's is not, or the other way round: that selects other code"; return RGPU_EINVAL; }
  }
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

// The table of member constants (hip/ensemble_scan.h) on the device: ALL members, running or not, filled and copied once for good by
// the first caller that needs it.  Returns RGPU_OK or a code with the message in e->err
int ensemble_table(rgpu_ensemble* e, rg_stream_t s, const char* who) {
  if (e->d_tab) return RGPU_OK;
  const int M = e->members;
  if (rg_malloc((void**)&e->d_tab, (size_t)M * sizeof(rgpu_tiled::MemberConst)) || (!e->h_tab && rg_host_alloc((void**)&e->h_tab, (size_t)M * sizeof(rgpu_tiled::MemberConst)))) {
    rg_free(e->d_tab); e->d_tab = 0;   // (d_tab != 0 means "filled and copied")
    return efail(e, RGPU_ENOMEM, std::string(who) + ": allocation of the table of member constants failed");
  }
  for (int m = 0; m < M; ++m) {
    rgpu_ctx* c = e->ctx[(size_t)m];
    rgpu_tiled::MemberConst& mc = e->h_tab[m];
    std::memset(&mc, 0, sizeof(mc));
    mc.g = c->g;
    mc.g.hdt = 0.0; mc.g.hgx = 0.0; mc.g.hgy = 0.0; mc.g.hgz = 0.0;
    mc.k = clock_const(c);
    mc.rc = rot_coef(c, 0.0);
  }
  if (rg_copy_h2d(e->d_tab, e->h_tab, (size_t)M * sizeof(rgpu_tiled::MemberConst), s)) {
    const std::string why = rg_last_error_string();
    rg_free(e->d_tab); e->d_tab = 0;
    return efail(e, RGPU_EHIP, std::string(who) + ": copy of the table of member constants: " + why);
  }
  return RGPU_OK;
}
bool ensemble_uses_table(const rgpu_ensemble* e) { return rgpu::options().member_params != 0 || (e->scan && !e->uniform); }
size_t monitor_part_doubles(const rgpu_params& p) { return (size_t)MON_NQ * (size_t)mon_nseg(p.ny) * (size_t)p.nx; }
// the buffers of the device monitor (see struct rgpu_ensemble)
int ensemble_monitor_buffers(rgpu_ensemble* e, const char* who) {
  if (e->d_mlog) return RGPU_OK;
  const size_t M = (size_t)e->members, nlog = (size_t)rgpu_ctx::kClockBatch * M * MON_NQ;
  if (rg_malloc((void**)&e->d_mspan, M * sizeof(rgpu_tiled::MonitorSpan)) || rg_host_alloc((void**)&e->h_mspan, M * sizeof(rgpu_tiled::MonitorSpan)) ||
      rg_malloc((void**)&e->d_mpart, M * monitor_part_doubles(e->ctx[0]->p) * sizeof(double)) || rg_host_alloc((void**)&e->h_mlog, nlog * sizeof(double)) ||
      rg_malloc((void**)&e->d_mlog, nlog * sizeof(double))) {
    rg_free(e->d_mlog); e->d_mlog = 0;   // (d_mlog != 0 means "all five are there"; the others are freed by rgpu_ensemble_destroy or reused)
    rg_free(e->d_mspan); e->d_mspan = 0; rg_free(e->d_mpart); e->d_mpart = 0;
    if (e->h_mspan) { rg_host_free(e->h_mspan); e->h_mspan = 0; }
    if (e->h_mlog) { rg_host_free(e->h_mlog); e->h_mlog = 0; }
    return efail(e, RGPU_ENOMEM, std::string(who) + ": allocation of the monitor buffers failed");
  }
  return RGPU_OK;
}
#endif

// sets: one parameter set (!scan: every member is created from it) or `members` of them (scan)
int ensemble_create_impl(const rgpu_params* sets, int members, bool scan, rgpu_ensemble** out) {
  if (!out) return RGPU_EINVAL;
  const rgpu_params* p = sets;   // member 0's: the shape, shared
  *out = 0;
  rgpu_ensemble* e = new (std::nothrow) rgpu_ensemble();
  if (!e) return RGPU_ENOMEM;
  *out = e;   // returned even on failure so that rgpu_ensemble_last_error can be read; the caller destroys it
  e->members = 0; e->device = -1; e->U = 0; e->stride = 0; e->slots = 0;
#ifdef RGPU_TILED_ENSEMBLE2D
  e->d_clk = e->h_clk = 0; e->d_span = e->h_span = 0; e->d_tab = e->h_tab = 0;
  e->d_mspan = e->h_mspan = 0; e->d_mpart = e->d_mlog = e->h_mlog = 0;
#endif
  e->scan = scan; e->uniform = true;
  std::string why;
  if (const int vr = scan ? scan_validate(sets, members, &why) : ensemble_validate(p, members, &why)) return efail(e, vr, why);
  for (int m = 1; scan && m < members; ++m) e->uniform = e->uniform && !std::memcmp(&sets[0], &sets[m], sizeof(rgpu_params));
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
    const int rc = create_common(scan ? &sets[m] : p, e->U + m * e->stride, e->U + (M + m) * e->stride, 0, true, &c, e->slots + m * 3 * RG_DT_SLOTS);
    if (c) { c->borrowed = true; e->ctx.push_back(c); }
    if (rc) return efail(e, rc, "ensemble: member " + std::to_string(m) + ": " + (c ? c->err : std::string("allocation failed")));
  }
  e->members = members;
  return RGPU_OK;
}
}  // namespace

extern "C" {

int rgpu_ensemble_create(const rgpu_params* p, int members, rgpu_ensemble** out) { return ensemble_create_impl(p, members, false, out); }
int rgpu_ensemble_create_scan(const rgpu_params* sets, int members, rgpu_ensemble** out) { return ensemble_create_impl(sets, members, true, out); }

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
  rg_free(e->d_clk); rg_free(e->d_span); rg_free(e->d_tab);
  if (e->h_clk) rg_host_free(e->h_clk);
  if (e->h_span) rg_host_free(e->h_span);
  if (e->h_tab) rg_host_free(e->h_tab);
  rg_free(e->d_mspan); rg_free(e->d_mpart); rg_free(e->d_mlog);
  if (e->h_mspan) rg_host_free(e->h_mspan);
  if (e->h_mlog) rg_host_free(e->h_mlog);
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

size_t rgpu_ensemble_scan_device_bytes(const rgpu_params* sets, int members) {
  std::string why;
  if (scan_validate(sets, members, &why)) return 0;
  size_t n = rgpu_ensemble_device_bytes(&sets[0], members);   // (what a member allocates follows from the shared integers)
#ifdef RGPU_TILED_ENSEMBLE2D
  n += (size_t)members * sizeof(rgpu_tiled::MemberConst);      // the table of the fused rounds (as many again in pinned host memory)
#endif
  return n;
}

}  // extern "C"

namespace {
// where rgpu_ensemble_run_steps_monitored leaves its samples (0: rgpu_ensemble_run_steps, no sampling)
struct EnsembleMon { int every, cap; int* n; int* step; double* t; double* values; };

// rgpu_ensemble_run_steps (mon == 0: exactly its launches) and rgpu_ensemble_run_steps_monitored
int ensemble_run_impl(rgpu_ensemble* e, int nsteps, const double* tEnd, int* nStep, double* t, double* dt, double* dt_log, int* done, int* stop, int* fused_steps,
                      const EnsembleMon* mon) {
  rg_set_device(e->device);
  const int M = e->members;
  // sample k of member m: its step number, its t after that step, the ten values
  auto put = [&](int m, int step, double tm, const double* v) {
    const int k = mon->n[m];
    if (k >= mon->cap) return;   // (cannot happen: at most nsteps / every + 1 multiples of every in nsteps consecutive step numbers)
    mon->step[(size_t)m * mon->cap + k] = step;
    mon->t[(size_t)m * mon->cap + k] = tm;
    std::memcpy(mon->values + ((size_t)m * mon->cap + k) * MON_NQ, v, MON_NQ * sizeof(double));
    mon->n[m] = k + 1;
  };
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
  auto alone_plain = [&](int m, int k) -> int {
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
  // ... sampled: cut at the member's next sampling step, the sample taken by the flat monitor of its context (one synchronisation
  // per sample on this path)
  auto alone = [&](int m, int k) -> int {
    if (!mon) return alone_plain(m, k);
    while (k > 0 && running(m)) {
      const int to_next = mon->every - nStep[m] % mon->every, kk = k < to_next ? k : to_next, n0 = nStep[m];
      if (const int rc = alone_plain(m, kk)) return rc;
      if (nStep[m] > n0 && nStep[m] % mon->every == 0 && code[m] < 2) {
        double v[MON_NQ];
        rgpu_ctx* c = e->ctx[(size_t)m];
        if (const int rc = rgpu_state_monitor(c, nStep[m] & 1, v)) return efail(e, rc, "ensemble_run_steps: member " + std::to_string(m) + ": " + c->err);
        put(m, nStep[m], t[m], v);
      }
      k -= kk;
    }
    return 0;
  };
  std::vector<int> R, launch_of_round;
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
    // Constants by value (member R[0]'s, for everybody) or per member from the table: a scan whose sets differ, or any ensemble under
    // the diagnostic option member_params.  The table holds ALL members, running or not, and is written here once for good
    const bool use_tab = ensemble_uses_table(e);
    if (const int rt = use_tab ? ensemble_table(e, s, "ensemble_run_steps") : RGPU_OK) return finish(rt);
    // sampling: every member's step number at the start of the batch, for the kernels' "is this step of member m a multiple of every"
    if (mon) {
      if (const int rt = ensemble_monitor_buffers(e, "ensemble_run_steps")) return finish(rt);
      for (int m = 0; m < M; ++m) { e->h_mspan[m].nStep0 = nStep[m]; e->h_mspan[m].parity = -1; }
      if (rg_copy_h2d(e->d_mspan, e->h_mspan, (size_t)M * sizeof(rgpu_tiled::MonitorSpan), s)) return finish(efail(e, RGPU_EHIP, std::string("ensemble_run_steps: ") + rg_last_error_string()));
    }
    rgpu_ctx* c0 = e->ctx[(size_t)R[0]];
    DevParams g = c0->g;
    g.hdt = 0.0; g.hgx = 0.0; g.hgy = 0.0; g.hgz = 0.0;   // (no gravity on this path)
    const ClockConst kc = clock_const(c0);
    const RotCoef rotc = rot_coef(c0, 0.0);
    const int images = c0->p.mhdEnabled ? 1 : hydro2d_images(c0);
    // table path: one instantiation for all members, chosen as the by-value path chooses it; what it assumes is shared by the sets
    // of a scan (scan_validate) -- were a member's constants ever not to satisfy it, the generic instantiation assumes nothing
    bool mhd_plain = pick_spec(g) == 2;
    int hydro_spec = use_tab && !c0->p.mhdEnabled ? rgpu_tiled::hydro2d_scan_spec(g) : 0;
    for (int m = 0; use_tab && m < M; ++m) {
      if (!spec_matches(kSpecPlain, e->ctx[(size_t)m]->g)) mhd_plain = false;
      if (!spec_matches(hydro_spec, e->ctx[(size_t)m]->g)) hydro_spec = 0;
    }
    unsigned long long* slots = e->slots + (size_t)phase * RG_DT_SLOTS;
    const size_t pool = (size_t)M * e->stride;
    const unsigned stride = (unsigned)e->stride;
    const int nb = left < kBatch ? left : kBatch;
    int queued = 0, rc = 0, nlaunch = 0;
    launch_of_round.assign((size_t)nb, -1);   // the log slot of the monitor launch queued behind round r, -1: none
    for (; queued < nb; ++queued) {
      StepClock* rec = e->d_clk + (size_t)queued * M;
      if (use_tab ? rgpu_tiled::launch_scan_clock(s, M, slots, e->d_tab, e->d_span, queued ? rec - M : 0, rec)
                  : rgpu_tiled::launch_ensemble_clock(s, M, slots, kc, e->d_span, queued ? rec - M : 0, rec)) { rc = -1; break; }
      const int pin = (par + queued) % 2, pout = 1 - pin;
      for (int m : R) { e->ctx[(size_t)m]->rec.drop_scan(); e->ctx[(size_t)m]->rec.drop_ghosts(); }   // the output arrays are about to change
      const double* in = e->U + (size_t)pin * pool;
      double* out = e->U + (size_t)pout * pool;
      int rs;
      if (use_tab)
        rs = c0->p.mhdEnabled ? rgpu_tiled::mhd2d_scan_step<kSpecPlain>(s, M, g, mhd_plain, e->d_tab, in, out, stride, slots, images, rec)
                              : rgpu_tiled::hydro2d_scan_step(s, M, g, hydro_spec, e->d_tab, in, out, stride, slots, images, rec);
      else
        rs = c0->p.mhdEnabled ? rgpu_tiled::mhd2d_ensemble_step<kSpecPlain>(s, M, g, rotc, pick_spec(g) == 2, in, out, stride, slots, images, rec)
                              : rgpu_tiled::hydro2d_ensemble_step(s, M, g, in, out, stride, slots, images, rec);
      if (rs) { rc = -1; break; }
      for (int m : R) { e->ctx[(size_t)m]->rec.scanned(pout, RG_DT_SLOTS); e->ctx[(size_t)m]->rec.ghosts_written(pout); }
      if (mon) {
        // the monitor of the state this round wrote, when some running member's step number after it is a multiple of every; which
        // members really took the step is in the records: the kernels look there, the host when it walks them below
        bool any = false;
        for (int m : R) any = any || (nStep[m] + queued + 1) % mon->every == 0;
        if (any) {
          if (rgpu_tiled::launch_ensemble_monitor(s, M, g, use_tab ? e->d_tab : 0, e->U, stride, e->d_mspan, rec, queued + 1, mon->every, pout, e->d_mpart, e->d_mlog, (unsigned)nlaunch)) {
            rc = -1; ++queued;   // (the round itself is queued and counts; its samples are lost with the error)
            break;
          }
          launch_of_round[(size_t)queued] = nlaunch++;
        }
      }
    }
    // a launch that failed after `queued` complete rounds were queued: those still run -- read their records and advance the members
    // for them before reporting (as rgpu_run_steps_log)
    const std::string launch_err = rc ? std::string(rg_last_error_string()) : std::string();
    if (queued > 0 && (rg_copy_d2h(e->h_clk, e->d_clk, (size_t)queued * M * sizeof(StepClock), s) ||
                       (nlaunch > 0 && rg_copy_d2h(e->h_mlog, e->d_mlog, (size_t)nlaunch * M * MON_NQ * sizeof(double), s)) || rg_stream_sync(s))) {
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
        if (mon && launch_of_round[(size_t)r] >= 0 && (n0 + r + 1) % mon->every == 0)   // exactly the slots the kernels filled: this step ran and qualifies
          put(m, n0 + r + 1, t[m], e->h_mlog + ((size_t)launch_of_round[(size_t)r] * M + m) * MON_NQ);
      }
      nStep[m] += r;
      c->cur = nStep[m] & 1;
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
}  // namespace

extern "C" {

int rgpu_ensemble_run_steps(rgpu_ensemble* e, int nsteps, const double* tEnd, int* nStep, double* t, double* dt, double* dt_log, int* done, int* stop, int* fused_steps) {
  if (!e) return RGPU_EINVAL;
  if (e->members < 1) return efail(e, RGPU_EINVAL, "ensemble_run_steps: the ensemble was not created");
  if (!nStep || !t || !dt || !done) return efail(e, RGPU_EINVAL, "ensemble_run_steps: null pointer");
  return ensemble_run_impl(e, nsteps, tEnd, nStep, t, dt, dt_log, done, stop, fused_steps, 0);
}

int rgpu_ensemble_run_steps_monitored(rgpu_ensemble* e, int nsteps, const double* tEnd, int* nStep, double* t, double* dt, double* dt_log, int* done, int* stop,
                                      int* fused_steps, int every, int* mon_n, int* mon_step, double* mon_t, double* mon) {
  if (!e) return RGPU_EINVAL;
  if (e->members < 1) return efail(e, RGPU_EINVAL, "ensemble_run_steps_monitored: the ensemble was not created");
  if (!nStep || !t || !dt || !done || !mon_n || !mon_step || !mon_t || !mon) return efail(e, RGPU_EINVAL, "ensemble_run_steps_monitored: null pointer");
  if (every < 1) return efail(e, RGPU_EINVAL, "ensemble_run_steps_monitored: every must be >= 1");
  for (int m = 0; m < e->members; ++m) mon_n[m] = 0;
  const EnsembleMon em = {every, (nsteps > 0 ? nsteps : 0) / every + 1, mon_n, mon_step, mon_t, mon};
  return ensemble_run_impl(e, nsteps, tEnd, nStep, t, dt, dt_log, done, stop, fused_steps, &em);
}

int rgpu_ensemble_monitor(rgpu_ensemble* e, double* out) {
  if (!e) return RGPU_EINVAL;
  if (e->members < 1) return efail(e, RGPU_EINVAL, "ensemble_monitor: the ensemble was not created");
  if (!out) return efail(e, RGPU_EINVAL, "ensemble_monitor: null pointer");
  rg_set_device(e->device);
  const int M = e->members;
#ifdef RGPU_TILED_ENSEMBLE2D
  // one kernel pair for all members (hip/ensemble_monitor.h, outside a batch: no records, each member's own parity), one read-back
  const rg_stream_t s = (rg_stream_t)0;
  if (const int rt = ensemble_monitor_buffers(e, "ensemble_monitor")) return rt;
  const bool use_tab = ensemble_uses_table(e);
  if (const int rt = use_tab ? ensemble_table(e, s, "ensemble_monitor") : RGPU_OK) return rt;
  for (int m = 0; m < M; ++m) { e->h_mspan[m].nStep0 = 0; e->h_mspan[m].parity = e->ctx[(size_t)m]->cur; }
  if (rg_copy_h2d(e->d_mspan, e->h_mspan, (size_t)M * sizeof(rgpu_tiled::MonitorSpan), s) ||
      rgpu_tiled::launch_ensemble_monitor(s, M, e->ctx[0]->g, use_tab ? e->d_tab : 0, e->U, (unsigned)e->stride, e->d_mspan, 0, 0, 1, -1, e->d_mpart, e->d_mlog, 0u) ||
      rg_copy_d2h(e->h_mlog, e->d_mlog, (size_t)M * MON_NQ * sizeof(double), s) || rg_stream_sync(s))
    return efail(e, RGPU_EHIP, std::string("ensemble_monitor: ") + rg_last_error_string());
  std::memcpy(out, e->h_mlog, (size_t)M * MON_NQ * sizeof(double));
#else
  for (int m = 0; m < M; ++m) {   // no ensemble kernels in this build: member by member through the flat monitor
    rgpu_ctx* c = e->ctx[(size_t)m];
    if (const int rc = rgpu_state_monitor(c, c->cur, out + (size_t)m * MON_NQ)) return efail(e, rc, "ensemble_monitor: member " + std::to_string(m) + ": " + c->err);
  }
#endif
  return RGPU_OK;
}

size_t rgpu_ensemble_monitor_device_bytes(const rgpu_params* p, int members) {
  std::string why;
  if (ensemble_validate(p, members, &why)) return 0;
#ifdef RGPU_TILED_ENSEMBLE2D
  return (size_t)members * (sizeof(rgpu_tiled::MonitorSpan) + (monitor_part_doubles(*p) + (size_t)rgpu_ctx::kClockBatch * MON_NQ) * sizeof(double));
#else
  return 0;
#endif
}

}  // extern "C"
