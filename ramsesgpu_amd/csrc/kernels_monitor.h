// kernels_monitor.h -- the monitor of a 2D state (rgpu_state_monitor, rgpu_ensemble_monitor, rgpu_ensemble_run_steps_monitored;
// include/rgpu.h, "monitors"): RGPU_MON_NQ = 10 raw quantities over the interior cells of U[parity] -- seven sums (mass, the
// three momenta, total / kinetic / magnetic energy) and three extrema (min density, min internal energy, max |div B|).
//
// ONE definition of the per-cell terms (mon_cell_terms) and of the summation order (mon_segment, mon_lane, mon_butterfly), shared
// by the flat functor kernels below (any backend, the test-only host emulation included) and by the ensemble kernels with the
// member in blockIdx.y (hip/ensemble_monitor.h).  Every floating-point operation sits under "fp contract(off)" -- inside the
// function bodies, so that nothing else in the translation unit changes -- with the products pinned besides (mon_mul: the pragma does
// not bind the backend of the contracted build), and uses IEEE + - * / only: the ten doubles of a given
// state are the same in librgpu.so and librgpu_fast.so, and tests/monitor_checks.py reproduces them bit for bit in numpy.
//
// Operation order of the terms of cell (i, j); U = the state, N = component stride, o = flat index of the cell:
//   rho = U[ID], E = U[IP], mx = U[IU], my = U[IV], mz = U[IW] (nvar == 4: +0.0)
//   ekin = (0.5 * ((mx * mx + my * my) + mz * mz)) / rho
//   MHD:   bxc = 0.5 * (Bx(i,j) + Bx(i+1,j)), byc = 0.5 * (By(i,j) + By(i,j+1)), bzc = U[IC]
//          emag = 0.5 * ((bxc * bxc + byc * byc) + bzc * bzc)
//          divb = | (Bx(i+1,j) - Bx(i,j)) / dx + (By(i,j+1) - By(i,j)) / dy |
//   hydro: emag = +0.0, divb = +0.0
//   eint = (E - ekin) - emag
//   t[0..9] = rho, mx, my, mz, E, ekin, emag | rho, eint | divb
// The high faces of the last interior row / column are in the first ghost layer and carry their constrained-transport value
// after every step and after a ghost fill (hist_row_cell, kernels_history.h, reads the same faces): no ghost fill is needed.
//
// Summation order of a sum over the nx x ny interior cells, ii = i - gw in [0, nx), jj = j - gw in [0, ny); every accumulator
// starts at +0.0 and takes "a = a + x" in the order given:
//   1. segments of RGPU_MON_ROWS rows: P[s][ii] = sum over jj = s * ROWS .. min(ny, (s + 1) * ROWS) - 1, ascending, of the term
//   2. columns:                        C[ii]    = sum over s = 0 .. nseg - 1, ascending, of P[s][ii]      (nseg = ceil(ny / ROWS))
//   3. lanes, l in [0, RGPU_MON_LANES): L[l]    = sum over ii = l, l + LANES, l + 2 LANES, .. < nx, ascending, of C[ii]
//   4. butterfly: for off = LANES / 2, LANES / 4, .., 1:  L[l] <- L[l] + L[l ^ off] for all l at once; the sum is L[0]
// The extrema take the same route with fmin (from +inf) / fmax (from +0.0) in place of the addition: order-free; fmin / fmax
// return their other operand when one is NaN, so a NaN cell drops out of the extrema (it propagates into the sums).
#pragma once
#include "dev_numerics.h"
#include "step_clock_rec.h"

namespace rgpu_dev {

enum { MON_NQ = 10, MON_NSUM = 7, MON_ROWS = 32, MON_LANES = 64 };

// (mon_init / mon_combine also run on the host: step 4 of the flat path)
#if defined(__HIPCC__)
#define RG_MON_FN __host__ __device__ __forceinline__
#else
#define RG_MON_FN inline
#endif

RG_MON_FN int mon_nseg(int ny) { return (ny + MON_ROWS - 1) / MON_ROWS; }

RG_MON_FN void mon_init(double* a) {
#pragma unroll
  for (int q = 0; q < MON_NSUM; ++q) a[q] = 0.0;
  a[7] = __builtin_huge_val(); a[8] = __builtin_huge_val(); a[9] = 0.0;
}
// a <- a (+) x: the sums add, the extrema take fmin / fmax
RG_MON_FN void mon_combine(double* a, const double* x) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
#pragma unroll
  for (int q = 0; q < MON_NSUM; ++q) a[q] = a[q] + x[q];
  a[7] = fmin(a[7], x[7]); a[8] = fmin(a[8], x[8]); a[9] = fmax(a[9], x[9]);
}

// A product that stays a product.  librgpu_fast.so is compiled with -ffp-contract=fast, under which the backend fuses a multiplication
// into the addition that follows it whatever the pragma in the function says (seen in its assembly: v_fmac_f64 in these very terms);
// the empty asm -- the form of rg_in_vector, hip/ensemble2d.h -- makes the rounded product a value of its own.  Every multiplication
// whose result is added or subtracted goes through it; the host emulation has no FMA to contract into.  Being volatile it also keeps
// the compiler from moving code across it: accepted for a streaming reduction whose time is its loads.
RG_DEVFN double mon_mul(double a, double b) {
  double x = a * b;
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("" : "+v"(x));
#endif
  return x;
}

// the ten terms of the cell at flat index o (shape, strides and the MHD switch from g; dx, dy given: a member's own)
RG_DEVFN void mon_cell_terms(const DevParams& g, double dx, double dy, const double* __restrict__ U, unsigned o, double* t) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const size_t N = g.ncell;
  const double rho = U[o + ID * N], E = U[o + IP * N], mx = U[o + IU * N], my = U[o + IV * N];
  const double mz = g.nvar > 4 ? U[o + IW * N] : 0.0;
  const double ekin = (0.5 * ((mon_mul(mx, mx) + mon_mul(my, my)) + mon_mul(mz, mz))) / rho;
  double emag = 0.0, divb = 0.0;
  if (g.mhd) {
    const double bx = U[o + IA * N], bx1 = U[o + 1 + IA * N], by = U[o + IB * N], by1 = U[o + g.sj + IB * N], bzc = U[o + IC * N];
    const double bxc = 0.5 * (bx + bx1), byc = 0.5 * (by + by1);
    emag = mon_mul(0.5, (mon_mul(bxc, bxc) + mon_mul(byc, byc)) + mon_mul(bzc, bzc));
    divb = fabs((bx1 - bx) / dx + (by1 - by) / dy);
  }
  t[0] = rho; t[1] = mx; t[2] = my; t[3] = mz; t[4] = E; t[5] = ekin; t[6] = emag;
  t[7] = rho; t[8] = (E - ekin) - emag; t[9] = divb;
}

// step 1: P[s][ii], the rows of segment s of interior column ii, ascending
RG_DEVFN void mon_segment(const DevParams& g, double dx, double dy, const double* __restrict__ U, int s, int ii, double* a) {
  mon_init(a);
  const int j0 = s * MON_ROWS, j1 = j0 + MON_ROWS < g.ny ? j0 + MON_ROWS : g.ny;
  for (int jj = j0; jj < j1; ++jj) {
    double t[MON_NQ];
    mon_cell_terms(g, dx, dy, U, (unsigned)(ii + g.gw) + g.sj * (unsigned)(jj + g.gw), t);
    mon_combine(a, t);
  }
}

// steps 2 and 3: L[l] from part[q * R + s * nx + ii], R = nseg * nx
RG_DEVFN void mon_lane(int nx, int nseg, const double* __restrict__ part, int l, double* a) {
  const size_t R = (size_t)nseg * nx;
  mon_init(a);
  for (int ii = l; ii < nx; ii += MON_LANES) {
    double c[MON_NQ];
    mon_init(c);
    for (int s = 0; s < nseg; ++s) {
      double x[MON_NQ];
#pragma unroll
      for (int q = 0; q < MON_NQ; ++q) x[q] = part[(size_t)q * R + (size_t)s * nx + ii];
      mon_combine(c, x);
    }
    mon_combine(a, c);
  }
}

// step 4 on an array of lane values, lanes[l * MON_NQ + q] (the flat path: on the host after the read-back; the ensemble kernel does
// the same additions across the lanes of a wave): out[q] = L[0]
inline void mon_butterfly(double* lanes, double* out) {
  for (int off = MON_LANES / 2; off > 0; off >>= 1) {
    double next[MON_LANES * MON_NQ];
    for (int l = 0; l < MON_LANES; ++l) {
#pragma unroll
      for (int q = 0; q < MON_NQ; ++q) next[l * MON_NQ + q] = lanes[l * MON_NQ + q];
      mon_combine(next + l * MON_NQ, lanes + (l ^ off) * MON_NQ);
    }
    for (int n = 0; n < MON_LANES * MON_NQ; ++n) lanes[n] = next[n];
  }
  for (int q = 0; q < MON_NQ; ++q) out[q] = lanes[q];
}

// ---- the flat kernels (rg_launch) --------------------------------------------------------------------------------
// thread idx = s * nx + ii (coalesced in ii) -> part[q][idx]
struct K_mon_rows {
  DevParams g; const double* U; double* part;
  RG_DEVFN void operator()(unsigned idx) const {
    const int nseg = mon_nseg(g.ny);
    const int s = (int)(idx / (unsigned)g.nx), ii = (int)(idx % (unsigned)g.nx);
    if (s >= nseg) return;
    double a[MON_NQ];
    mon_segment(g, g.dx, g.dy, U, s, ii, a);
    const size_t R = (size_t)nseg * g.nx;
#pragma unroll
    for (int q = 0; q < MON_NQ; ++q) part[(size_t)q * R + idx] = a[q];
  }
};
// thread l < min(MON_LANES, nx) -> lanes[l][q] (a lane without a column keeps the neutral elements: the host fills them in)
struct K_mon_lanes {
  DevParams g; const double* part; double* lanes;
  RG_DEVFN void operator()(unsigned l) const {
    if (l >= (unsigned)MON_LANES || l >= (unsigned)g.nx) return;
    double a[MON_NQ];
    mon_lane(g.nx, mon_nseg(g.ny), part, (int)l, a);
#pragma unroll
    for (int q = 0; q < MON_NQ; ++q) lanes[l * MON_NQ + q] = a[q];
  }
};

// ---- the monitor of a 3D state (rgpu_state_monitor3d, rgpu_run_steps_monitored) ------------------------------------------------
// The same ten quantities over the nx x ny x nz interior cells.  Terms of cell (i, j, k), o its flat index:
//   rho, E, mx, my as above, mz = U[IW] (3D hydro has five variables), ekin as above
//   MHD:   bxc, byc as above, bzc = 0.5 * (Bz(i,j,k) + Bz(i,j,k+1)), emag = 0.5 * ((bxc * bxc + byc * byc) + bzc * bzc)
//          divb = | ((Bx(i+1,j,k) - Bx(i,j,k)) / dx + (By(i,j+1,k) - By(i,j,k)) / dy) + (Bz(i,j,k+1) - Bz(i,j,k)) / dz |
//   hydro: emag = +0.0, divb = +0.0;   eint = (E - ekin) - emag
// The high faces of the last interior row / column / plane come from the first ghost layer (hist_row_cell reads the same faces).
// Summation order: V[kk], kk = k - gw, is steps 1 - 4 above applied to the nx x ny cells of interior plane kk; the result is
// V[0] + V[1] + .. ascending in kk from +0.0 (fmin from +inf / fmax from +0.0 for the extrema).
RG_DEVFN void mon_vol_cell_terms(const DevParams& g, const double* __restrict__ U, unsigned o, double* t) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const size_t N = g.ncell;
  const double rho = U[o + ID * N], E = U[o + IP * N], mx = U[o + IU * N], my = U[o + IV * N], mz = U[o + IW * N];
  const double ekin = (0.5 * ((mon_mul(mx, mx) + mon_mul(my, my)) + mon_mul(mz, mz))) / rho;
  double emag = 0.0, divb = 0.0;
  if (g.mhd) {
    const double bx = U[o + IA * N], bx1 = U[o + 1 + IA * N], by = U[o + IB * N], by1 = U[o + g.sj + IB * N];
    const double bz = U[o + IC * N], bz1 = U[o + g.sk + IC * N];
    const double bxc = 0.5 * (bx + bx1), byc = 0.5 * (by + by1), bzc = 0.5 * (bz + bz1);
    emag = mon_mul(0.5, (mon_mul(bxc, bxc) + mon_mul(byc, byc)) + mon_mul(bzc, bzc));
    divb = fabs(((bx1 - bx) / g.dx + (by1 - by) / g.dy) + (bz1 - bz) / g.dz);
  }
  t[0] = rho; t[1] = mx; t[2] = my; t[3] = mz; t[4] = E; t[5] = ekin; t[6] = emag;
  t[7] = rho; t[8] = (E - ekin) - emag; t[9] = divb;
}

// step 1 of interior plane kk: P[s][ii]
RG_DEVFN void mon_vol_segment(const DevParams& g, const double* __restrict__ U, int kk, int s, int ii, double* a) {
  mon_init(a);
  const int j0 = s * MON_ROWS, j1 = j0 + MON_ROWS < g.ny ? j0 + MON_ROWS : g.ny;
  const unsigned o0 = (unsigned)(ii + g.gw) + g.sk * (unsigned)(kk + g.gw);
  for (int jj = j0; jj < j1; ++jj) {
    double t[MON_NQ];
    mon_vol_cell_terms(g, U, o0 + g.sj * (unsigned)(jj + g.gw), t);
    mon_combine(a, t);
  }
}
// steps 1 and 2 of interior plane kk by one thread: C[ii], an accumulator per segment, the segments added in ascending order -- the
// additions of mon_lane's inner loop over P[s][ii], hence its bits
RG_DEVFN void mon_vol_column(const DevParams& g, const double* __restrict__ U, int kk, int ii, double* c) {
  mon_init(c);
  const int nseg = mon_nseg(g.ny);
  for (int s = 0; s < nseg; ++s) {
    double a[MON_NQ];
    mon_vol_segment(g, U, kk, s, ii, a);
    mon_combine(c, a);
  }
}
// one quantity of mon_combine
RG_MON_FN double mon_op(int q, double a, double x) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return q < MON_NSUM ? a + x : (q < 9 ? fmin(a, x) : fmax(a, x));
}
// the sum over the planes: quantity q of V[kk] at V[kk * stride + q], ascending in kk
RG_DEVFN double mon_vol_planes(int nz, const double* __restrict__ V, size_t stride, int q) {
  double a = q < MON_NSUM ? 0.0 : (q < 9 ? __builtin_huge_val() : 0.0);
  for (int kk = 0; kk < nz; ++kk) a = mon_op(q, a, V[(size_t)kk * stride + q]);
  return a;
}

// A sample taken inside a batch of device-clock steps (rgpu_run_steps_monitored): every kernel of it is queued behind the last
// kernel of the step and returns at once when the step's record says that the step did not run (clk == 0: outside a batch)
RG_DEVFN bool mon_gate_open(const StepClock* clk) { return !clk || clk->stop == 0; }

// ---- the flat kernels of the 3D monitor (rg_launch): the host emulation and any backend without kernels of its own ----------------
// Scratch: cols[kk][q][ii] (mon_lane's layout of one segment per plane), then two arrays of lane values [kk][l][q] the butterfly
// alternates between (one launch per stage: "for all l at once").
// thread idx = kk * nx + ii (coalesced in ii)
struct K_mon_vol_cols {
  DevParams g; const double* U; double* cols; const StepClock* clk;
  RG_DEVFN void operator()(unsigned idx) const {
    if (!mon_gate_open(clk)) return;
    const int kk = (int)(idx / (unsigned)g.nx), ii = (int)(idx % (unsigned)g.nx);
    if (kk >= g.nz) return;
    double c[MON_NQ];
    mon_vol_column(g, U, kk, ii, c);
#pragma unroll
    for (int q = 0; q < MON_NQ; ++q) cols[((size_t)kk * MON_NQ + q) * g.nx + ii] = c[q];
  }
};
// thread idx = kk * MON_LANES + l (a lane without a column: the neutral elements)
struct K_mon_vol_lanes {
  DevParams g; const double* cols; double* lanes; const StepClock* clk;
  RG_DEVFN void operator()(unsigned idx) const {
    if (!mon_gate_open(clk)) return;
    const int kk = (int)(idx / (unsigned)MON_LANES), l = (int)(idx % (unsigned)MON_LANES);
    if (kk >= g.nz) return;
    double a[MON_NQ];
    mon_lane(g.nx, 1, cols + (size_t)kk * MON_NQ * g.nx, l, a);
#pragma unroll
    for (int q = 0; q < MON_NQ; ++q) lanes[(size_t)idx * MON_NQ + q] = a[q];
  }
};
// one stage of the butterfly of every plane: dst[l] = src[l] (+) src[l ^ off]
struct K_mon_vol_fly {
  int nz, off; const double* src; double* dst; const StepClock* clk;
  RG_DEVFN void operator()(unsigned idx) const {
    if (!mon_gate_open(clk) || idx >= (unsigned)nz * MON_LANES) return;
    double a[MON_NQ];
#pragma unroll
    for (int q = 0; q < MON_NQ; ++q) a[q] = src[(size_t)idx * MON_NQ + q];
    mon_combine(a, src + (size_t)(idx ^ (unsigned)off) * MON_NQ);
#pragma unroll
    for (int q = 0; q < MON_NQ; ++q) dst[(size_t)idx * MON_NQ + q] = a[q];
  }
};
// thread q: out[q] = V[0][q] + V[1][q] + ..; V[kk] is lane 0 of plane kk
struct K_mon_vol_finish {
  int nz; const double* lanes; double* out; const StepClock* clk;
  RG_DEVFN void operator()(unsigned q) const {
    if (!mon_gate_open(clk) || q >= (unsigned)MON_NQ) return;
    out[q] = mon_vol_planes(nz, lanes, (size_t)MON_LANES * MON_NQ, (int)q);
  }
};

}  // namespace rgpu_dev
