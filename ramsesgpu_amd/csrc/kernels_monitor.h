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

}  // namespace rgpu_dev
