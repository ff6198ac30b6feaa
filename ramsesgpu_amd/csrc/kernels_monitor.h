// kernels_monitor.h -- the monitors (rgpu_state_monitor, rgpu_state_monitor3d, rgpu_run_steps_monitored, rgpu_ensemble_monitor,
// rgpu_ensemble_run_steps_monitored; include/rgpu.h, "monitors"): RGPU_MON_NQ = 10 raw quantities over the interior cells of U[parity]
// -- seven sums (mass, the three momenta, total / kinetic / magnetic energy) and three extrema (min density, min internal energy,
// max |div B|).
//
// ONE definition of the per-cell terms (mon_cell_terms) and of the summation order (mon_segment, mon_lane, the butterfly, the sum over
// the planes), shared by the flat functors below (the test-only host emulation and any backend without kernels of its own), by the
// gfx950 kernels of a lone context (hip/monitor3d.h) and by the ensemble kernels with the member in blockIdx.y
// (hip/ensemble_monitor.h).  A 2D state is a volume of one plane: the only differences are the three places where a cell looks along z
// (VOL below).  Every floating-point operation sits under "fp contract(off)" -- inside the function bodies, so that nothing else in
// the translation unit changes -- with the products pinned besides (mon_mul: the pragma does not bind the backend of the contracted
// build), and uses IEEE + - * / only: the ten doubles of a given state are the same in librgpu.so and librgpu_fast.so, and
// tests/monitor_checks.py / tests/monitor3d_checks.py reproduce them bit for bit in numpy.
//
// Operation order of the terms of cell (i, j, k); U = the state, N = component stride, o = flat index of the cell:
//   rho = U[ID], E = U[IP], mx = U[IU], my = U[IV], mz = U[IW] (2D with nvar == 4: +0.0; 3D hydro has five variables)
//   ekin = (0.5 * ((mx * mx + my * my) + mz * mz)) / rho
//   MHD:   bxc = 0.5 * (Bx(i,j,k) + Bx(i+1,j,k)), byc = 0.5 * (By(i,j,k) + By(i,j+1,k))
//          bzc = U[IC] (2D) | 0.5 * (Bz(i,j,k) + Bz(i,j,k+1)) (3D)
//          emag = 0.5 * ((bxc * bxc + byc * byc) + bzc * bzc)
//          d2 = (Bx(i+1,j,k) - Bx(i,j,k)) / dx + (By(i,j+1,k) - By(i,j,k)) / dy
//          divb = | d2 | (2D) | | d2 + (Bz(i,j,k+1) - Bz(i,j,k)) / dz | (3D)
//   hydro: emag = +0.0, divb = +0.0
//   eint = (E - ekin) - emag
//   t[0..9] = rho, mx, my, mz, E, ekin, emag | rho, eint | divb
// The high faces of the last interior row / column / plane are in the first ghost layer and carry their constrained-transport value
// after every step and after a ghost fill (hist_row_cell, kernels_history.h, reads the same faces): no ghost fill is needed.
//
// Summation order of a sum over the nx x ny x nz interior cells (2D: nz = 1), ii = i - gw in [0, nx), jj = j - gw in [0, ny),
// kk = k - gw in [0, nz); every accumulator starts at +0.0 and takes "a = a + x" in the order given.  Per interior plane kk:
//   1. segments of RGPU_MON_ROWS rows: P[s][ii] = sum over jj = s * ROWS .. min(ny, (s + 1) * ROWS) - 1, ascending, of the term
//   2. columns:                        C[ii]    = sum over s = 0 .. nseg - 1, ascending, of P[s][ii]      (nseg = ceil(ny / ROWS))
//   3. lanes, l in [0, RGPU_MON_LANES): L[l]    = sum over ii = l, l + LANES, l + 2 LANES, .. < nx, ascending, of C[ii]
//   4. butterfly: for off = LANES / 2, LANES / 4, .., 1:  L[l] <- L[l] + L[l ^ off] for all l at once; V[kk] = L[0]
// and then
//   5. planes: V[0] + V[1] + .. ascending in kk from +0.0
// The extrema take the same route with fmin (from +inf) / fmax (from +0.0) in place of the addition: order-free; fmin / fmax
// return their other operand when one is NaN, so a NaN cell drops out of the extrema (it propagates into the sums).
// With one plane, step 5 returns V[0] bit for bit and is left out: a sum accumulated from +0.0 is never -0.0, so +0.0 + V == V (NaN
// included); fmin(+inf, x) == x for the minima, which are never NaN; fmax(+0.0, divb) == divb, divb being a fabs or +0.0.
#pragma once
#include "dev_numerics.h"
#include "step_clock_rec.h"

namespace rgpu_dev {

enum { MON_NQ = 10, MON_NSUM = 7, MON_ROWS = 32, MON_LANES = 64 };

#if defined(__HIPCC__)
#define RG_MON_FN __host__ __device__ __forceinline__
#else
#define RG_MON_FN inline
#endif

RG_MON_FN int mon_nseg(int ny) { return (ny + MON_ROWS - 1) / MON_ROWS; }
// the planes of a lone context's state: a 2D state is a volume of one
RG_MON_FN int mon_nplanes(const DevParams& g) { return g.three_d ? g.nz : 1; }

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

// the ten terms of the cell at flat index o (shape, strides and the MHD switch from g; dx, dy, dz given: a member's own).  VOL: the
// cell has neighbours along z (a 3D state).  A template argument and not a flag tested per cell: each instantiation is straight-line
// code, the loads of a row issued together, and the 3D one is the code the 3D monitor had before the 2D one joined it
template <bool VOL>
RG_DEVFN void mon_cell_terms(const DevParams& g, double dx, double dy, double dz, const double* __restrict__ U, unsigned o, double* t) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const size_t N = g.ncell;
  const double rho = U[o + ID * N], E = U[o + IP * N], mx = U[o + IU * N], my = U[o + IV * N];
  const double mz = (VOL || g.nvar > 4) ? U[o + IW * N] : 0.0;
  const double ekin = (0.5 * ((mon_mul(mx, mx) + mon_mul(my, my)) + mon_mul(mz, mz))) / rho;
  double emag = 0.0, divb = 0.0;
  if (g.mhd) {
    const double bx = U[o + IA * N], bx1 = U[o + 1 + IA * N], by = U[o + IB * N], by1 = U[o + g.sj + IB * N], bz = U[o + IC * N];
    const double bxc = 0.5 * (bx + bx1), byc = 0.5 * (by + by1);
    double bzc = bz;
    divb = (bx1 - bx) / dx + (by1 - by) / dy;
    if (VOL) {
      const double bz1 = U[o + g.sk + IC * N];
      bzc = 0.5 * (bz + bz1);
      divb = divb + (bz1 - bz) / dz;
    }
    emag = mon_mul(0.5, (mon_mul(bxc, bxc) + mon_mul(byc, byc)) + mon_mul(bzc, bzc));
    divb = fabs(divb);
  }
  t[0] = rho; t[1] = mx; t[2] = my; t[3] = mz; t[4] = E; t[5] = ekin; t[6] = emag;
  t[7] = rho; t[8] = (E - ekin) - emag; t[9] = divb;
}

// step 1: P[s][ii] of interior plane kk (!VOL: the one plane there is), the rows of segment s of interior column ii, ascending
template <bool VOL>
RG_DEVFN void mon_segment(const DevParams& g, double dx, double dy, double dz, const double* __restrict__ U, int kk, int s, int ii, double* a) {
  mon_init(a);
  const int j0 = s * MON_ROWS, j1 = j0 + MON_ROWS < g.ny ? j0 + MON_ROWS : g.ny;
  const unsigned o0 = (unsigned)(ii + g.gw) + (VOL ? g.sk * (unsigned)(kk + g.gw) : 0u);
  for (int jj = j0; jj < j1; ++jj) {
    double t[MON_NQ];
    mon_cell_terms<VOL>(g, dx, dy, dz, U, o0 + g.sj * (unsigned)(jj + g.gw), t);
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

// steps 1 and 2 of interior plane kk by one thread: C[ii], an accumulator per segment, the segments added in ascending order -- the
// additions of mon_lane's inner loop over P[s][ii], hence its bits
template <bool VOL>
RG_DEVFN void mon_vol_column(const DevParams& g, const double* __restrict__ U, int kk, int ii, double* c) {
  mon_init(c);
  const int nseg = mon_nseg(g.ny);
  for (int s = 0; s < nseg; ++s) {
    double a[MON_NQ];
    mon_segment<VOL>(g, g.dx, g.dy, g.dz, U, kk, s, ii, a);
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
// step 5: quantity q of V[kk] at V[kk * MON_NQ + q], ascending in kk
RG_DEVFN double mon_vol_planes(int nz, const double* __restrict__ V, int q) {
  double a = q < MON_NSUM ? 0.0 : (q < 9 ? __builtin_huge_val() : 0.0);
  for (int kk = 0; kk < nz; ++kk) a = mon_op(q, a, V[(size_t)kk * MON_NQ + q]);
  return a;
}

// A sample taken inside a batch of device-clock steps (rgpu_run_steps_monitored): every kernel of it is queued behind the last
// kernel of the step and returns at once when the step's record says that the step did not run (clk == 0: outside a batch)
RG_DEVFN bool mon_gate_open(const StepClock* clk) { return !clk || clk->stop == 0; }

// Scratch of one sample of a lone context, in doubles: the segment sums part[kk][q][s * nx + ii] of the gfx950 kernels, then V[kk][q]
// (the flat functors keep cols[kk][q][ii] in the same place: never more)
RG_MON_FN size_t mon_scratch_doubles(const DevParams& g) { return (size_t)MON_NQ * mon_nplanes(g) * ((size_t)mon_nseg(g.ny) * g.nx + 1); }

// ---- the flat kernels (rg_launch): the host emulation and any backend without kernels of its own -----------------------------------
// thread idx = kk * nx + ii (coalesced in ii) -> cols[kk][q][ii], mon_lane's layout of one segment per plane.  VOL: chosen at launch
template <bool VOL>
struct K_mon_vol_cols {
  DevParams g; const double* U; double* cols; const StepClock* clk;
  RG_DEVFN void operator()(unsigned idx) const {
    if (!mon_gate_open(clk)) return;
    const int kk = (int)(idx / (unsigned)g.nx), ii = (int)(idx % (unsigned)g.nx);
    if (kk >= mon_nplanes(g)) return;
    double c[MON_NQ];
    mon_vol_column<VOL>(g, U, kk, ii, c);
#pragma unroll
    for (int q = 0; q < MON_NQ; ++q) cols[((size_t)kk * MON_NQ + q) * g.nx + ii] = c[q];
  }
};
// thread kk: steps 3 and 4 of plane kk -> V[kk].  The lanes one after another (a lane without a column: the neutral elements), then the
// butterfly on them: only L[0] is wanted, and what reaches it from stage `off` are the lanes below off, for which l ^ off == l + off
struct K_mon_vol_fold {
  int nx, nz; const double* cols; double* V; const StepClock* clk;
  RG_DEVFN void operator()(unsigned kk) const {
    if (!mon_gate_open(clk) || kk >= (unsigned)nz) return;
    double L[MON_LANES * MON_NQ];
    for (int l = 0; l < MON_LANES; ++l) mon_lane(nx, 1, cols + (size_t)kk * MON_NQ * nx, l, L + l * MON_NQ);
    for (int off = MON_LANES / 2; off > 0; off >>= 1)
      for (int l = 0; l < off; ++l) mon_combine(L + l * MON_NQ, L + (l + off) * MON_NQ);
    for (int q = 0; q < MON_NQ; ++q) V[(size_t)kk * MON_NQ + q] = L[q];
  }
};
// thread q: step 5, out[q] = V[0][q] + V[1][q] + ..
struct K_mon_vol_finish {
  int nz; const double* V; double* out; const StepClock* clk;
  RG_DEVFN void operator()(unsigned q) const {
    if (!mon_gate_open(clk) || q >= (unsigned)MON_NQ) return;
    out[q] = mon_vol_planes(nz, V, (int)q);
  }
};

}  // namespace rgpu_dev
