// kernels_monitor_planes.h -- the plane monitor (rgpu_state_monitor_planes, rgpu_run_steps_monitored_planes; include/rgpu.h, "plane
// monitors"): MONP_NQ = 16 raw quantities of EVERY interior plane kk of a 3D state U[parity] -- the ten of the monitor
// (kernels_monitor.h) and six more sums, the cell-centred field, bx by, rho vx vy and rho^2 -- that is the z profiles a butterfly
// diagram, a stress profile or a mixing-layer width is drawn from.
//
// Nothing of the monitor's definition is restated here.  The first ten terms of a cell are mon_cell_terms<true>'s; the summation order
// of a row is steps 1 - 4 of kernels_monitor.h (segments of MON_ROWS rows, columns, MON_LANES lanes, butterfly) applied to the plane;
// the 16-wide monp_init / monp_combine call the 10-wide ones and add the six sums behind them.  There is no step 5: row kk is V[kk] of
// the monitor in its first ten columns, so folding the rows ascending in kk with mon_op gives rgpu_state_monitor3d bit for bit.
//
// The six terms of cell (i, j, k), IEEE + - * / in this order, every product that is later added pinned (mon_mul):
//   MHD:   bx = bxc = 0.5 * (Bx(i,j,k) + Bx(i+1,j,k)), by = byc = 0.5 * (By(i,j,k) + By(i,j+1,k)), bz = bzc = 0.5 * (Bz(i,j,k) + Bz(i,j,k+1))
//          bxby = bxc * byc
//   hydro: bx = by = bz = bxby = +0.0
//   rvxvy = (mx * my) / rho,   rho2 = rho * rho
// bxc, byc, bzc are formed again from the faces mon_cell_terms read (the same operations on the same doubles: the same bits).
//
// Shared by the flat functors below (the test-only host emulation and any backend without kernels of its own) and by the gfx950
// kernels of hip/monitor_profile.h.
#pragma once
#include "kernels_monitor.h"

namespace rgpu_dev {

enum { MONP_NQ = 16 };   // MON_NQ, then six sums

RG_MON_FN void monp_init(double* a) {
  mon_init(a);
#pragma unroll
  for (int q = MON_NQ; q < MONP_NQ; ++q) a[q] = 0.0;
}
// a <- a (+) x: the monitor's ten, then the six sums
RG_MON_FN void monp_combine(double* a, const double* x) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  mon_combine(a, x);
#pragma unroll
  for (int q = MON_NQ; q < MONP_NQ; ++q) a[q] = a[q] + x[q];
}

// the sixteen terms of the cell at flat index o of a 3D state
RG_DEVFN void monp_cell_terms(const DevParams& g, const double* __restrict__ U, unsigned o, double* t) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  mon_cell_terms<true>(g, g.dx, g.dy, g.dz, U, o, t);
  const size_t N = g.ncell;
  const double rho = U[o + ID * N], mx = U[o + IU * N], my = U[o + IV * N];
  double bxc = 0.0, byc = 0.0, bzc = 0.0, bxby = 0.0;
  if (g.mhd) {
    bxc = mon_mul(0.5, U[o + IA * N] + U[o + 1 + IA * N]);
    byc = mon_mul(0.5, U[o + IB * N] + U[o + g.sj + IB * N]);
    bzc = mon_mul(0.5, U[o + IC * N] + U[o + g.sk + IC * N]);
    bxby = mon_mul(bxc, byc);
  }
  t[10] = bxc; t[11] = byc; t[12] = bzc; t[13] = bxby;
  t[14] = mon_mul(mx, my) / rho;
  t[15] = mon_mul(rho, rho);
}

// step 1: P[s][ii] of interior plane kk, the rows of segment s of interior column ii, ascending (mon_segment, sixteen wide)
RG_DEVFN void monp_segment(const DevParams& g, const double* __restrict__ U, int kk, int s, int ii, double* a) {
  monp_init(a);
  const int j0 = s * MON_ROWS, j1 = j0 + MON_ROWS < g.ny ? j0 + MON_ROWS : g.ny;
  const unsigned o0 = (unsigned)(ii + g.gw) + g.sk * (unsigned)(kk + g.gw);
  for (int jj = j0; jj < j1; ++jj) {
    double t[MONP_NQ];
    monp_cell_terms(g, U, o0 + g.sj * (unsigned)(jj + g.gw), t);
    monp_combine(a, t);
  }
}

// steps 2 and 3: L[l] from part[q * R + s * nx + ii], R = nseg * nx (mon_lane, sixteen wide)
RG_DEVFN void monp_lane(int nx, int nseg, const double* __restrict__ part, int l, double* a) {
  const size_t R = (size_t)nseg * nx;
  monp_init(a);
  for (int ii = l; ii < nx; ii += MON_LANES) {
    double c[MONP_NQ];
    monp_init(c);
    for (int s = 0; s < nseg; ++s) {
      double x[MONP_NQ];
#pragma unroll
      for (int q = 0; q < MONP_NQ; ++q) x[q] = part[(size_t)q * R + (size_t)s * nx + ii];
      monp_combine(c, x);
    }
    monp_combine(a, c);
  }
}

// Scratch of one sample, in doubles: the segment sums part[kk][q][s * nx + ii] of the gfx950 kernels (the flat functors keep
// cols[kk][q][ii] in the same place: never more).  The rows themselves go straight to their destination
RG_MON_FN size_t monp_scratch_doubles(const DevParams& g) { return (size_t)MONP_NQ * g.nz * ((size_t)mon_nseg(g.ny) * g.nx); }
RG_MON_FN size_t monp_sample_doubles(const DevParams& g) { return (size_t)MONP_NQ * g.nz; }

// ---- the flat kernels (rg_launch): the host emulation and any backend without kernels of its own -----------------------------------
// thread idx = kk * nx + ii (coalesced in ii): steps 1 and 2, an accumulator per segment, the segments added in ascending order
// -> cols[kk][q][ii], monp_lane's layout of one segment per plane
struct K_mon_prof_cols {
  DevParams g; const double* U; double* cols; const StepClock* clk;
  RG_DEVFN void operator()(unsigned idx) const {
    if (!mon_gate_open(clk)) return;
    const int kk = (int)(idx / (unsigned)g.nx), ii = (int)(idx % (unsigned)g.nx);
    if (kk >= g.nz) return;
    double c[MONP_NQ];
    monp_init(c);
    const int nseg = mon_nseg(g.ny);
    for (int s = 0; s < nseg; ++s) {
      double a[MONP_NQ];
      monp_segment(g, U, kk, s, ii, a);
      monp_combine(c, a);
    }
#pragma unroll
    for (int q = 0; q < MONP_NQ; ++q) cols[((size_t)kk * MONP_NQ + q) * g.nx + ii] = c[q];
  }
};
// thread kk: steps 3 and 4 of plane kk -> out[kk][MONP_NQ], the row at its destination.  The lanes one after another, then the
// butterfly on them as K_mon_vol_fold runs it: what reaches L[0] from stage `off` are the lanes below off, for which l ^ off == l + off
struct K_mon_prof_fold {
  int nx, nz; const double* cols; double* out; const StepClock* clk;
  RG_DEVFN void operator()(unsigned kk) const {
    if (!mon_gate_open(clk) || kk >= (unsigned)nz) return;
    double L[MON_LANES * MONP_NQ];
    for (int l = 0; l < MON_LANES; ++l) monp_lane(nx, 1, cols + (size_t)kk * MONP_NQ * nx, l, L + l * MONP_NQ);
    for (int off = MON_LANES / 2; off > 0; off >>= 1)
      for (int l = 0; l < off; ++l) monp_combine(L + l * MONP_NQ, L + (l + off) * MONP_NQ);
    for (int q = 0; q < MONP_NQ; ++q) out[(size_t)kk * MONP_NQ + q] = L[q];
  }
};

}  // namespace rgpu_dev
