// kernels_history.h -- the device side of the MHD history diagnostics: per-thread bodies of the row / column sums, their flat functors
// (rgpu_history_mri, rgpu_history_turbulence: api/history.h, api/entry_core.h), and the MRI row sampled INSIDE a batch of device-clock
// steps (rgpu_run_steps_history, api/run_steps.h).  Flat rg_launch functors throughout: any backend, the test-only host emulation
// included.  The arithmetic behind the column sums is history_row.h, shared with the host and the slab driver.
#pragma once
#include "dev_numerics.h"
#include "history_row.h"
#include "step_clock_rec.h"

namespace rgpu_dev {

enum { HIST_NQ = rgpu_hist::NCOL, HIST_TURB_NQ = 18 };

// history diagnostics of the MHD runs (MHDRunBase::history_mri / history_default, MHDRunBase.cpp:3311-3407,
// 3476-3619).  The reference copies the whole state to the host and loops over it; here the y sums are done on the
// device, one thread per (i,k) row in increasing j (coalesced along i), a second kernel adds the rows of a column in
// increasing k, and the host adds the isize column values: a fixed summation order, reproducible run to run (it is
// not the reference's k,j,i order, so sums agree to round-off, not bit for bit).
//   q = 0 rho, 1 vx = mx/rho, 2 vy = my/rho            (all i, ghosts included: the y-z means of history_mri)
//       3 magp terms, 4 maxwell term, 5 Bx, 6 By, 7 Bz, 8 divB   (interior i only)
RG_DEVFN void hist_row_cell(const DevParams& g, const double* __restrict__ U, double* __restrict__ rows, unsigned idx) {
  const int nk = g.three_d ? g.nz : 1;
  const int i = (int)(idx % (unsigned)g.isize), kk = (int)(idx / (unsigned)g.isize);
  if (kk >= nk) return;
  const int k = g.three_d ? kk + g.gw : 0;
  const size_t N = g.ncell;
  const unsigned sj = g.sj, sk = g.three_d ? g.sk : 0u;
  const bool inner = i >= g.gw && i < g.isize - g.gw;
  double acc[HIST_NQ];
#pragma unroll
  for (int q = 0; q < HIST_NQ; ++q) acc[q] = 0.0;
  for (int j = g.gw; j < g.jsize - g.gw; ++j) {
    const unsigned o = (unsigned)i + sj * (unsigned)j + g.sk * (unsigned)k;
    const double rho = U[o + ID * N];
    acc[0] += rho;
    acc[1] += U[o + IU * N] / rho;
    acc[2] += U[o + IV * N] / rho;
    if (inner) {
      const double bx = U[o + IA * N], by = U[o + IB * N], bz = U[o + IC * N];
      const double sx = bx + U[o + 1 + IA * N], sy = by + U[o + sj + IB * N];
      acc[3] += 0.25 * (sx * sx);
      acc[3] += 0.25 * (sy * sy);
      double dv = (U[o + 1 + IA * N] - bx) / g.dx + (U[o + sj + IB * N] - by) / g.dy;
      if (g.three_d) {
        const double sz = bz + U[o + sk + IC * N];
        acc[3] += 0.25 * (sz * sz);
        dv = dv + (U[o + sk + IC * N] - bz) / g.dz;
      }
      acc[4] -= 0.25 * sx * sy;
      acc[5] += bx; acc[6] += by; acc[7] += bz;
      acc[8] += dv;
    }
  }
  const size_t R = (size_t)g.isize * nk;
#pragma unroll
  for (int q = 0; q < HIST_NQ; ++q) rows[(size_t)q * R + idx] = acc[q];
}

// history_turbulence (MHDRunBase.cpp:3626-3810): row sums over the interior y of the 19 quantities of its two loops, interior
// i only.  q = 0 mass, 1 eKin, 2 mean_v2, 3 eMag, 4 helicity, 5-7 mean_B, 8-10 mean_rhov, 11-16 the high-k DFT coefficients of
// Bx (x re/im, y re/im, z re/im; phases from the ghost-inclusive integer indices like the reference), 17 divB, 18 unused
RG_DEVFN void hist_turb_row_cell(const DevParams& g, const double* __restrict__ U, double* __restrict__ rows, unsigned idx) {
  const int nk = g.nz;
  const int i = (int)(idx % (unsigned)g.isize), kk = (int)(idx / (unsigned)g.isize);
  if (kk >= nk) return;
  const int k = kk + g.gw;
  const size_t N = g.ncell;
  const unsigned sj = g.sj, sk = g.sk;
  double acc[HIST_TURB_NQ];
#pragma unroll
  for (int q = 0; q < HIST_TURB_NQ; ++q) acc[q] = 0.0;
  if (i >= g.gw && i < g.isize - g.gw) {
    const double pi = 2 * asin(1.0);
    const int kfft = g.nx - 3;
    for (int j = g.gw; j < g.jsize - g.gw; ++j) {
      const unsigned o = (unsigned)i + sj * (unsigned)j + sk * (unsigned)k;
      const double rho = U[o + ID * N];
      const double mu = U[o + IU * N], mv = U[o + IV * N], mw = U[o + IW * N];
      const double bx = U[o + IA * N], by = U[o + IB * N], bz = U[o + IC * N];
      acc[0] += rho;
      acc[1] += (mu * mu) / rho; acc[1] += (mv * mv) / rho; acc[1] += (mw * mw) / rho;
      acc[2] += (mu / rho) * (mu / rho); acc[2] += (mv / rho) * (mv / rho); acc[2] += (mw / rho) * (mw / rho);
      acc[3] += bx * bx; acc[3] += by * by; acc[3] += bz * bz;
      acc[4] += mu * bx / sqrt(rho); acc[4] += mv * by / sqrt(rho); acc[4] += mw * bz / sqrt(rho);
      acc[5] += bx; acc[6] += by; acc[7] += bz;
      acc[8] += mu; acc[9] += mv; acc[10] += mw;
      acc[11] += bx * cos(2 * pi * kfft * i / g.nx); acc[12] += bx * sin(2 * pi * kfft * i / g.nx);
      acc[13] += bx * cos(2 * pi * kfft * j / g.ny); acc[14] += bx * sin(2 * pi * kfft * j / g.ny);
      acc[15] += bx * cos(2 * pi * kfft * k / g.nz); acc[16] += bx * sin(2 * pi * kfft * k / g.nz);
      acc[17] += (U[o + 1 + IA * N] - bx) / g.dx + (U[o + sj + IB * N] - by) / g.dy + (U[o + sk + IC * N] - bz) / g.dz;
    }
  }
  const size_t R = (size_t)g.isize * nk;
#pragma unroll
  for (int q = 0; q < HIST_TURB_NQ; ++q) rows[(size_t)q * R + idx] = acc[q];
}

// column sums: thread (i,q) adds rows[q][k][i] over k
RG_DEVFN void hist_col_cell(const DevParams& g, const double* __restrict__ rows, double* __restrict__ cols, int nq, unsigned idx) {
  const int nk = g.three_d ? g.nz : 1;
  const int i = (int)(idx % (unsigned)g.isize), q = (int)(idx / (unsigned)g.isize);
  if (q >= nq) return;
  const size_t R = (size_t)g.isize * nk;
  double a = 0.0;
  for (int kk = 0; kk < nk; ++kk) a += rows[(size_t)q * R + (size_t)kk * g.isize + i];
  cols[(size_t)q * g.isize + i] = a;
}

// Reynolds stress rows: sum_j rho * dTau * (vx - <vx>(i)) * (vy - <vy>(i)) for interior i (MHDRunBase.cpp:3589-3595)
RG_DEVFN void hist_reynolds_cell(const DevParams& g, const double* __restrict__ U, const double* __restrict__ mean_vx,
                                 const double* __restrict__ mean_vy, double dTau, double* __restrict__ rows, unsigned idx) {
  const int nk = g.three_d ? g.nz : 1;
  const int i = (int)(idx % (unsigned)g.isize), kk = (int)(idx / (unsigned)g.isize);
  if (kk >= nk) return;
  const int k = g.three_d ? kk + g.gw : 0;
  const size_t N = g.ncell;
  double a = 0.0;
  if (i >= g.gw && i < g.isize - g.gw) {
    const double m1 = mean_vx[i], m2 = mean_vy[i];
    for (int j = g.gw; j < g.jsize - g.gw; ++j) {
      const unsigned o = (unsigned)i + g.sj * (unsigned)j + g.sk * (unsigned)k;
      const double rho = U[o + ID * N];
      a += rho * dTau * (U[o + IU * N] / rho - m1) * (U[o + IV * N] / rho - m2);
    }
  }
  rows[idx] = a;
}

struct K_hist_rows {
  DevParams g; const double* U; double* rows;
  RG_DEVFN void operator()(unsigned idx) const { hist_row_cell(g, U, rows, idx); }
};
struct K_hist_turb_rows {
  DevParams g; const double* U; double* rows;
  RG_DEVFN void operator()(unsigned idx) const { hist_turb_row_cell(g, U, rows, idx); }
};
struct K_hist_cols {
  DevParams g; const double* rows; double* cols; int nq;
  RG_DEVFN void operator()(unsigned idx) const { hist_col_cell(g, rows, cols, nq, idx); }
};
struct K_hist_reynolds {
  DevParams g; const double* U; const double* mean_vx; const double* mean_vy; double dTau; double* rows;
  RG_DEVFN void operator()(unsigned idx) const { hist_reynolds_cell(g, U, mean_vx, mean_vy, dTau, rows, idx); }
};

// ---- the MRI row inside a batch of device-clock steps ---------------------------------------------------------------------------
// The sampling decision of the reference's loop (MHDRunGodunov.cpp:3975-3984) and the small host arithmetic of rgpu_history_mri moved
// to the device, so that a batch with a history cadence needs no host turn either.
//
// Behind the tick of step n five launches are queued (history_batch_queue, api/history.h):
//   rows        K_hist_rows          } the kernels of rgpu_history_mri, unchanged, behind a gate
//   columns     K_hist_cols (9)      } + the two mean-velocity columns  mean = col / (ny nz)  by the thread that formed the column
//   Reynolds    K_hist_reynolds      } reading those means
//   its columns K_hist_cols (1)      } into column 1, whose vx sums have served (the host version reuses column 0 after copying it out)
//   finish      eight threads: out[q] of the row each (rgpu_hist::mri_row_value)
// The gate (HistBatchGate::due) is the loop's condition, evaluated by every thread from launch-uniform addresses -- the step's
// StepClock record, the previous record's dt, the previous step's HistBatchRec -- before anything else: a step that does not sample
// costs five launches of threads that load four scalars and return; the pass over U happens for sampling steps only.
// Nothing is updated in place: the finish of step n writes HistBatchRec n (tHist after its head, the sample if one was taken), which
// the gates of step n + 1 read; the first step of a batch takes tHist and dt by value.  The host reads the records of a batch back
// together with the clock records, copies out the ones marked `sampled` and counts them itself.

enum { HIST_BATCH_NQ = rgpu_hist::NROW };   // the out[8] of rgpu_history_mri

struct HistBatchRec {
  double tHist;                 // the loop's tHist after the head of this step
  double t, dt;                 // of the sample: *t and *dt at the head of the step
  double v[HIST_BATCH_NQ];
  int step, sampled;            // step number of this head; 1: t, dt, v hold a sample
};

// the loop's "tHist == 0 || (t - dt <= tHist + dtHist && t > tHist + dtHist)", in doubles, with those expressions in that order
// (host and device: the literal loop of rgpu_run_steps_history evaluates the same function)
RG_HIST_FN bool hist_batch_due(double t, double dt, double tHist, double dtHist) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return tHist == 0 || ((t - dt <= tHist + dtHist) && (t > tHist + dtHist));
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
struct K_hist_batch_gated {
  HistBatchGate gate; K k;
  RG_DEVFN void operator()(unsigned idx) const { if (!gate.due()) return; k(idx); }
};

// the nine column sums, and by the threads of columns 1 and 2 the y-z means of vx, vy
struct K_hist_batch_cols {
  HistBatchGate gate; K_hist_cols k; double* mean; int nyz;
  RG_DEVFN void operator()(unsigned idx) const {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (!gate.due()) return;
    k(idx);
    const unsigned is = (unsigned)k.g.isize, q = idx / is, i = idx - q * is;
    if (q == 1u || q == 2u) mean[(size_t)(q - 1u) * is + i] = rgpu_hist::yz_mean(k.cols[(size_t)q * is + i], nyz);
  }
};

// thread q < 8 forms out[q] of rgpu_history_mri; thread 0 also writes the bookkeeping of the record -- for every step, sampled or
// not (the next step's gates read tHist from it)
struct K_hist_batch_finish {
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
    if (due) out->v[q] = rgpu_hist::mri_row_value((int)q, cols, rcol, isize, gw, dTau);
  }
};

}  // namespace rgpu_dev
