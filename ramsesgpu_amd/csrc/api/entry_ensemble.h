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
// clock records, on the member-by-member rounds by the monitor of the member's context.
// Here: the object, what it accepts, the loop over rounds and the member-alone path.  The fused half (device buffers, the decision,
// queueing and harvesting a batch, the device monitor, byte counts) is api/ensemble_fused.h, behind the functions the stand-in below names.
#pragma once

namespace {
const rg_stream_t kStream = (rg_stream_t)0;   // the ensemble's one stream: the one rgpu_create gives a lone context
}  // namespace

#ifdef RGPU_TILED_ENSEMBLE2D
// What the fused rounds (api/ensemble_fused.h) keep on the device (DeviceMirror: api/ctx.h): each allocated by the first caller that needs it, freed with the ensemble
struct EnsembleFused {
  DeviceMirror<StepClock> clk;                  // records of a batch, tick-major: tick n of member m at [n * members + m]
  DeviceMirror<rgpu_tiled::EnsembleSpan> span;
  // the constants of member m at [m] (by member, never by position in a batch), filled and copied once (ensemble_table) by the first
  // caller that reads them -- a fused round, or rgpu_ensemble_monitor outside any round, on the ensemble's stream before the kernels
  // that read it -- and never written again: the kernels read them through scalar loads (hip/ensemble_scan.h)
  DeviceMirror<rgpu_tiled::MemberConst> tab;
  bool tab_filled = false;
  // monitors: per member and batch its step number at the start (and, outside a batch, the parity of its state); the log of a batch,
  // slot (launch, m); the segment sums of one launch (device only)
  DeviceMirror<rgpu_tiled::MonitorSpan> mspan;
  DeviceMirror<double> mlog, mpart;
};
#else
struct EnsembleFused {};
#endif

struct rgpu_ensemble {
  int members = 0, device = -1;
  std::vector<rgpu_ctx*> ctx;
  double* U = 0;                 // state of member m, parity q: U + (q * members + m) * stride
  size_t stride = 0;             // doubles between the states of two members (ensemble_member_doubles rounded up to whole 128-byte lines)
  unsigned long long* slots = 0; // members x 3 x RG_DT_SLOTS: the members' d_red_base
  EnsembleFused fused;
  bool scan = false;             // created by rgpu_ensemble_create_scan ...
  bool uniform = true;           // ... all of whose sets are bytewise equal (always true for rgpu_ensemble_create)
  std::string err;
};

namespace {
int efail(rgpu_ensemble* e, int code, const std::string& msg) {
  if (e) e->err = msg;
  return code;
}
size_t ensemble_member_doubles(const rgpu_params& p) { return (size_t)(p.nx + 2 * p.ghostWidth) * (size_t)(p.ny + 2 * p.ghostWidth) * (size_t)p.nbVar; }
size_t ensemble_stride(const rgpu_params& p) { return (ensemble_member_doubles(p) + 15) & ~(size_t)15; }
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
// where rgpu_ensemble_run_steps_monitored leaves its samples
struct EnsembleMon { int every, cap; int* n; int* step; double* t; double* values; };

// One call of rgpu_ensemble_run_steps(_monitored): the caller's arrays and what the pieces of the loop share
struct EnsembleRun {
  rgpu_ensemble* e;
  int nsteps;
  const double* tEnd;
  int* nStep; double* t; double* dt; double* dt_log; int* done;
  const EnsembleMon* mon;      // 0: rgpu_ensemble_run_steps, no sampling and exactly its launches
  std::vector<int> code;       // why member m left the loop before its nsteps were done: 0 = it did not, or 1 / 2 / 3 of its record
  int fused;                   // fused rounds so far

  double end_of(int m) const { return tEnd ? tEnd[m] : HUGE_VAL; }
  bool running(int m) const { return !code[m] && done[m] < nsteps && t[m] < end_of(m); }
  // sample k of member m: its step number, its t after that step, the ten values
  void put(int m, int step_no, double tm, const double* v) const {
    const int k = mon->n[m];
    if (k >= mon->cap) return;   // (cannot happen: at most nsteps / every + 1 multiples of every in nsteps consecutive step numbers)
    mon->step[(size_t)m * mon->cap + k] = step_no;
    mon->t[(size_t)m * mon->cap + k] = tm;
    std::memcpy(mon->values + ((size_t)m * mon->cap + k) * MON_NQ, v, MON_NQ * sizeof(double));
    mon->n[m] = k + 1;
  }
};
}  // namespace

#ifdef RGPU_TILED_ENSEMBLE2D
#include "ensemble_fused.h"
#else
// no ensemble kernels in this build (the test-only host emulation): never a fused batch, every round member by member
namespace {
bool fused_batch_possible(const EnsembleRun&, const std::vector<int>&, bool* transient, int*, int*) { *transient = false; return false; }
int fused_batch(EnsembleRun&, const std::vector<int>&, int, int, int, int*) { return RGPU_EUNSUPPORTED; }   // (never called)
int ensemble_monitor_all(rgpu_ensemble* e, double* out) {   // member by member through the monitor of a lone context
  for (int m = 0; m < e->members; ++m) {
    rgpu_ctx* c = e->ctx[(size_t)m];
    if (const int rc = rgpu_state_monitor(c, c->cur, out + (size_t)m * MON_NQ)) return efail(e, rc, "ensemble_monitor: member " + std::to_string(m) + ": " + c->err);
  }
  return RGPU_OK;
}
size_t fused_bytes_per_member() { return 0; }
size_t fused_table_bytes_per_member() { return 0; }
size_t fused_monitor_bytes_per_member(const rgpu_params&) { return 0; }
}  // namespace
#endif

namespace {
// sets: one parameter set (!scan: every member is created from it) or `members` of them (scan)
int ensemble_create_impl(const rgpu_params* sets, int members, bool scan, rgpu_ensemble** out) {
  if (!out) return RGPU_EINVAL;
  const rgpu_params* p = sets;   // member 0's: the shape, shared
  *out = 0;
  rgpu_ensemble* e = new (std::nothrow) rgpu_ensemble();
  if (!e) return RGPU_ENOMEM;
  *out = e;   // returned even on failure so that rgpu_ensemble_last_error can be read; the caller destroys it
  e->scan = scan;
  std::string why;
  if (const int vr = scan ? scan_validate(sets, members, &why) : ensemble_validate(p, members, &why)) return efail(e, vr, why);
  for (int m = 1; scan && m < members; ++m) e->uniform = e->uniform && !std::memcmp(&sets[0], &sets[m], sizeof(rgpu_params));
  if (rg_device_count() < 1) return efail(e, RGPU_ENODEVICE, "no HIP device: this library has no CPU fallback (backend " RG_BACKEND_NAME ")");
  e->device = rg_current_device();
  e->stride = ensemble_stride(*p);
  const size_t M = (size_t)members, state_bytes = 2 * M * e->stride * sizeof(double);
  if (rg_malloc((void**)&e->U, state_bytes) || rg_malloc((void**)&e->slots, M * 3 * RG_DT_SLOTS * sizeof(unsigned long long)) || rg_memset_async(e->U, 0, state_bytes, kStream))
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
  delete e;
}

int rgpu_ensemble_members(rgpu_ensemble* e) { return e ? e->members : 0; }
rgpu_ctx* rgpu_ensemble_member(rgpu_ensemble* e, int m) { return (e && m >= 0 && m < e->members) ? e->ctx[(size_t)m] : 0; }
const char* rgpu_ensemble_last_error(rgpu_ensemble* e) { return e ? e->err.c_str() : "null ensemble"; }

size_t rgpu_ensemble_device_bytes(const rgpu_params* p, int members) {
  std::string why;
  if (ensemble_validate(p, members, &why)) return 0;
  // a member's own context, the padding of its two states to the stride, its slots, the clock records and spans of the fused rounds
  const size_t per_member = rgpu_device_bytes(p) + 2 * (ensemble_stride(*p) - ensemble_member_doubles(*p)) * sizeof(double) + 3 * RG_DT_SLOTS * sizeof(unsigned long long) +
                            fused_bytes_per_member();
  return (size_t)members * per_member;
}

size_t rgpu_ensemble_scan_device_bytes(const rgpu_params* sets, int members) {
  std::string why;
  if (scan_validate(sets, members, &why)) return 0;
  // (what a member allocates follows from the shared integers) + the table of the fused rounds
  return rgpu_ensemble_device_bytes(&sets[0], members) + (size_t)members * fused_table_bytes_per_member();
}

}  // extern "C"

namespace {
// up to k steps of member m alone: the single-context loop, device clock and all
int run_member_alone_plain(EnsembleRun& run, int m, int k) {
  rgpu_ctx* c = run.e->ctx[(size_t)m];
  const int n0 = run.nStep[m];
  LoneRun lone = {c, k, run.end_of(m), run.nStep + m, run.t + m, run.dt + m, run.dt_log ? run.dt_log + (size_t)m * run.nsteps + run.done[m] : 0, 0, 0};
  const int r = run_steps_impl(lone);
  int why = lone.why;
  run.done[m] += run.nStep[m] - n0;
  if (r == RGPU_EHIP && !why) {
    // a plain step of the single-context loop failed: was it a time step that is not a number (nothing was launched then and the
    // scan can be asked again)?  That is this member's business (stop code 2); anything else ends the call.  Asked here and not in
    // the loop that lone contexts share, which reports such a failure as it always did
    double inv = 0.0;
    if (rgpu_compute_inv_dt(c, run.nStep[m] % 2, &inv) == RGPU_OK && !(c->p.cfl / inv == c->p.cfl / inv)) {
      why = 2;
      c->err = stop_message(why);
    }
  }
  if (why) run.code[m] = why;
  if (r < 0 && why < 2) return efail(run.e, r, "ensemble_run_steps: member " + std::to_string(m) + ": " + c->err);
  return 0;
}
// ... sampled: cut at the member's next sampling step, the sample taken by the monitor of its context (one synchronisation
// per sample on this path)
int run_member_alone(EnsembleRun& run, int m, int k) {
  if (!run.mon) return run_member_alone_plain(run, m, k);
  while (k > 0 && run.running(m)) {
    const int to_next = run.mon->every - run.nStep[m] % run.mon->every, kk = k < to_next ? k : to_next, n0 = run.nStep[m];
    if (const int rc = run_member_alone_plain(run, m, kk)) return rc;
    if (run.nStep[m] > n0 && run.nStep[m] % run.mon->every == 0 && run.code[m] < 2) {
      double v[MON_NQ];
      rgpu_ctx* c = run.e->ctx[(size_t)m];
      if (const int rc = rgpu_state_monitor(c, run.nStep[m] & 1, v)) return efail(run.e, rc, "ensemble_run_steps: member " + std::to_string(m) + ": " + c->err);
      run.put(m, run.nStep[m], run.t[m], v);
    }
    k -= kk;
  }
  return 0;
}

// the loop over rounds: member by member, or in fused batches wherever the running members can take one
int ensemble_rounds(EnsembleRun& run) {
  const int M = run.e->members;
  std::vector<int> R;
  R.reserve((size_t)M);
  for (int round = 0;;) {   // every member that still runs has done `round` steps of this call
    R.clear();
    for (int m = 0; m < M; ++m) if (run.running(m)) R.push_back(m);
    if (R.empty()) return RGPU_OK;
    const int left = run.nsteps - round;
    bool transient = false;
    int par = -1, phase = -1, queued = 0;
    if (fused_batch_possible(run, R, &transient, &par, &phase)) {
      // one batch of fused rounds: tick, then step, for all members; one read-back of the records (as rgpu_run_steps_log)
      if (const int rc = fused_batch(run, R, par, phase, left, &queued)) return rc;
      round += queued;
      continue;
    }
    // a member that is not clock-ready becomes so by one plain step: one round member by member, then look again.  Anything else
    // (a configuration the fused path does not cover, members of mixed step parity) does not change: each member runs on alone
    const int k = transient ? 1 : left;
    for (int m : R) if (const int rc = run_member_alone(run, m, k)) return rc;
    round += k;
  }
}

// rgpu_ensemble_run_steps (mon == 0: exactly its launches) and rgpu_ensemble_run_steps_monitored
int ensemble_run_impl(rgpu_ensemble* e, int nsteps, const double* tEnd, int* nStep, double* t, double* dt, double* dt_log, int* done, int* stop, int* fused_steps,
                      const EnsembleMon* mon) {
  rg_set_device(e->device);
  const int M = e->members;
  EnsembleRun run = {e, nsteps, tEnd, nStep, t, dt, dt_log, done, mon, std::vector<int>((size_t)M, 0), 0};
  for (int m = 0; m < M; ++m) done[m] = 0;
  const int rc = ensemble_rounds(run);   // however it ended: the stop codes and the count of fused rounds
  if (stop) for (int m = 0; m < M; ++m) stop[m] = run.code[m] >= 2 ? run.code[m] : (t[m] < run.end_of(m) ? 0 : 1);
  if (fused_steps) *fused_steps = run.fused;
  return rc;
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
  return ensemble_monitor_all(e, out);
}

size_t rgpu_ensemble_monitor_device_bytes(const rgpu_params* p, int members) {
  std::string why;
  if (ensemble_validate(p, members, &why)) return 0;
  return (size_t)members * fused_monitor_bytes_per_member(*p);
}

}  // extern "C"
