// tiled_hydro2d.h (HIP / gfx950 only) -- the whole 2D hydro unsplit step (primitives, slopes + trace, two Riemann problems per cell,
// conservative update, CFL term of the new state) as ONE LDS-tiled kernel: U -> Unew.
//
// Flat pipeline (kernels_hydro.h): K_hydro_prim, K_hydro_trace, K_hydro_flux, K_hydro_update -- four launches that pass Q (4),
// T (12) and F (8 doubles per cell) through L2 / HBM: 0.063 ms per step at 512^2 (a chain of 7-16 us kernels), 1.81 ms at
// 4096^2 (HBM-bound at ~400 B per cell).  Reference idiom: the one-kernel 2D step with a shared-memory tile and a ghost overlap,
// godunov_unsplit.cuh (kernel_godunov_unsplit_2d_v1), HydroRunGodunov.cpp:779-1005.
//
// One thread per cell of a TX x TY tile (tiles overlap by one cell per side: the inner (TX-2) x (TY-2) threads finish a cell):
//   phase 0  U of the cell -> primitives -> LDS (the one-cell ring around the tile by the first 2 TX + 2 TY threads)
//   phase 1  slopes + trace of the cell; the states at its HIGH x / y faces -> LDS, the LOW ones stay in registers
//   phase 2  Riemann problems at its LOW x / y faces -> fluxes to LDS
//   phase 3  update (both update orders), uniform-gravity source, CFL term of the new cell into the device slots
// Three barriers, 43 KB of LDS.  The arithmetic of phases 1-3 is the cell functions of kernels_hydro.h (hydro_half_slope,
// hydro_trace_advance, hydro_face_grid, hydro_face_flux, hydro_apply_flux, hydro_gravity_source, hydro_cfl_term) that the flat
// kernels call too: the same bits.  Tile geometry and LDS layout: tiled_hydro.h (HydroTile, tile_ring_cell, tile_owns, tile_inner).
#pragma once
#include "step_clock.h"

namespace rgpu_tiled {

// The ghost cells an interior cell is the source of, along one direction (bc_face_cell: dirichlet = mirror image with the normal
// momentum negated, neumann = copies of the first / last interior cell, periodic = the image one period away).  x = the cell's index,
// n = interior cells, gw = ghost width (n >= gw), bc = the face types (RGPU_BC_DIRICHLET 1, NEUMANN 2, PERIODIC 3).
struct ImgDim {
  int x, nlo, lo0, nhi, hi0;
  bool fliplo, fliphi;
  RG_DEVFN int count() const { return 1 + nlo + nhi; }
  RG_DEVFN int coord(int e) const { return e == 0 ? x : (e <= nlo ? lo0 + (e - 1) : hi0 + (e - 1 - nlo)); }
  RG_DEVFN bool flip(int e) const { return e == 0 ? false : (e <= nlo ? fliplo : fliphi); }
};
RG_DEVFN ImgDim images_of(int x, int n, int gw, int bc_lo, int bc_hi) {
  ImgDim d = {x, 0, 0, 0, 0, bc_lo == 1, bc_hi == 1};
  // low ghosts [0, gw)
  if (bc_lo == 1) { if (x < 2 * gw) { d.nlo = 1; d.lo0 = 2 * gw - 1 - x; } }
  else if (bc_lo == 2) { if (x == gw) { d.nlo = gw; d.lo0 = 0; } }
  else { if (x >= n) { d.nlo = 1; d.lo0 = x - n; } }
  // high ghosts [n + gw, n + 2 gw)
  if (bc_hi == 1) { if (x >= n) { d.nhi = 1; d.hi0 = 2 * n + 2 * gw - 1 - x; } }
  else if (bc_hi == 2) { if (x == n + gw - 1) { d.nhi = gw; d.hi0 = n + gw; } }
  else { if (x < 2 * gw) { d.nhi = 1; d.hi0 = x + n; } }
  return d;
}

// images != 0 (bit 12 set, the four face types in bits 2f .. 2f+1; caller: whole-domain step, every face dirichlet / neumann /
// periodic, no jet, nothing modifies the new state after this kernel): the interior cells also write the ghost cells the next
// step's ghost fill (X, then Y over the full extent: corners are images of images) would copy them into -- the same doubles -- and
// the ghost cells' own threads do not store: one writer per location, and that fill is not launched (StateRecord::ghosts_written).
// The body is a device function of its own: the single-box kernel below and the ensemble kernel (ensemble2d.h: many boxes of one
// shape in one launch, the member in blockIdx.y) call it -- one copy of the numerics, the tile of a workgroup from blockIdx.x alone,
// the time step by value (where it comes from -- arguments, a device record, the folded clock -- is the calling kernel's business).
template <int TX, int TY, int SPEC>
__device__ __forceinline__ void hydro2d_step_body(const DevParams& g, int nbx, const double* __restrict__ Uin, double* __restrict__ Uout,
                                                  double dtdx, double dtdy, unsigned long long* dt_slots, int images) {
  constexpr int NV = 4;
  constexpr int RING = 2 * TX + 2 * TY;
  static_assert(RING <= TX * TY, "ring cells are handled by the first RING threads");
  __shared__ HydroTile<TX, TY, NV> L;

  const int t = (int)threadIdx.x;
  const int by = (int)blockIdx.x / nbx, bx = (int)blockIdx.x - by * nbx;
  const int ti = t % TX, tj = t / TX;
  const int i = bx * (TX - 2) + ti, j = by * (TY - 2) + tj;
  const bool ina = i < g.isize && j < g.jsize;
  const size_t N = g.ncell;
  const unsigned idx2 = ina ? (unsigned)i + (unsigned)j * g.sj : 0u;
  const int gw = g.gw;
  const bool own = tile_owns<TX, TY>(ina, ti, tj, i, j);
  const bool inner = tile_inner(g, i, j);

  // ---- phase 0: primitives of the tile and of its ring (corners excluded: no stencil reads them) ----
  double u[NV], q[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v) { u[v] = 1.0; q[v] = 1.0; }
  if (ina) {
#pragma unroll
    for (int v = 0; v < NV; ++v) u[v] = Uin[idx2 + v * N];
  }
  {
    int rti, rtj;
    tile_ring_cell<TX, TY>(t, rti, rtj);
    const int ri = bx * (TX - 2) + rti, rj = by * (TY - 2) + rtj;
    const bool ring = t < RING && ri >= 0 && ri < g.isize && rj >= 0 && rj < g.jsize;
    double ur[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) ur[v] = 1.0;
    if (ring) {
#pragma unroll
      for (int v = 0; v < NV; ++v) ur[v] = Uin[(unsigned)ri + (unsigned)rj * g.sj + v * N];
    }
    if (ina) hydro_prim<NV>(g, u, q);
#pragma unroll
    for (int v = 0; v < NV; ++v) L.q[v][tj + 1][ti + 1] = q[v];
    if (t < RING) {
      double rq[NV] = {1.0, 1.0, 1.0, 1.0};
      if (ring) hydro_prim<NV>(g, ur, rq);
#pragma unroll
      for (int v = 0; v < NV; ++v) L.q[v][rtj + 1][rti + 1] = rq[v];
    }
  }
  __syncthreads();

  // ---- phase 1: slopes and trace of the cell; its high x / y face states -> LDS ----
  double qp[2][NV];   // states at the low x / y face
  {
    const double st = g.slope_type;
    double h[2][NV], tq[NV], qm[2][NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const double nb[2][2] = {{L.q[v][tj + 1][ti], L.q[v][tj + 1][ti + 2]}, {L.q[v][tj][ti + 1], L.q[v][tj + 2][ti + 1]}};
#pragma unroll
      for (int d = 0; d < 2; ++d) h[d][v] = hydro_half_slope<2>(st, nb[d][0], q[v], nb[d][1]);
    }
    hydro_trace_advance<2, NV>(g, q, h, dtdx, dtdy, 0.0, tq);
#pragma unroll
    for (int d = 0; d < 2; ++d) {
      hydro_face_grid<+1, NV>(g, tq, h[d], g.grav_on, g.hgx, g.hgy, 0.0, qm[d]);
      hydro_face_grid<-1, NV>(g, tq, h[d], g.grav_on, g.hgx, g.hgy, 0.0, qp[d]);
    }
#pragma unroll
    for (int n = 0; n < NV; ++n) { L.qm[0][n][tj][ti] = qm[0][n]; L.qm[1][n][tj][ti] = qm[1][n]; }
  }
  __syncthreads();

  // ---- phase 2: Riemann problems at the two low faces of the cell ----
  double fx[NV], fy[NV];
  {
    const int tim = ti > 0 ? ti - 1 : 0, tjm = tj > 0 ? tj - 1 : 0;
    double ql[NV];
#pragma unroll
    for (int n = 0; n < NV; ++n) ql[n] = L.qm[0][n][tj][tim];
    hydro_face_flux<0, NV>(g, ql, qp[0], fx);
#pragma unroll
    for (int n = 0; n < NV; ++n) ql[n] = L.qm[1][n][tjm][ti];
    hydro_face_flux<1, NV>(g, ql, qp[1], fy);
#pragma unroll
    for (int n = 0; n < NV; ++n) { L.f[0][n][tj][ti] = fx[n]; L.f[1][n][tj][ti] = fy[n]; }
  }
  __syncthreads();

  // ---- phase 3: update, CFL term of the new state ----
  double inv = 0.0;
  if (own) {
    const double rho_old = u[ID];
    if (inner) {
      const int tip = ti + 1 < TX ? ti + 1 : ti, tjp = tj + 1 < TY ? tj + 1 : tj;
      double fxh[NV], fyh[NV];   // fluxes through the high x / y faces: the neighbours' low faces
#pragma unroll
      for (int n = 0; n < NV; ++n) { fxh[n] = L.f[0][n][tj][tip]; fyh[n] = L.f[1][n][tjp][ti]; }
      if (!g.dirwise_update) {   // unsplitVersion 1: low faces, then high faces
        hydro_apply_flux<0, +1, NV>(u, fx, dtdx); hydro_apply_flux<1, +1, NV>(u, fy, dtdy);
        hydro_apply_flux<0, -1, NV>(u, fxh, dtdx); hydro_apply_flux<1, -1, NV>(u, fyh, dtdy);
      } else {                   // unsplitVersion 2: direction by direction
        hydro_apply_flux<0, +1, NV>(u, fx, dtdx); hydro_apply_flux<0, -1, NV>(u, fxh, dtdx);
        hydro_apply_flux<1, +1, NV>(u, fy, dtdy); hydro_apply_flux<1, -1, NV>(u, fyh, dtdy);
      }
      if (g.grav_on) hydro_gravity_source<NV>(u, rho_old, g.hgx, g.hgy, 0.0);
      if (dt_slots) inv = hydro_cfl_term<NV>(g, u);
    }
    if (!images) {
#pragma unroll
      for (int v = 0; v < NV; ++v) Uout[idx2 + v * N] = u[v];
    } else if (inner && i >= 2 * gw && i < g.nx && j >= 2 * gw && j < g.ny) {   // no ghost cell is an image of this cell
#pragma unroll
      for (int v = 0; v < NV; ++v) Uout[idx2 + v * N] = u[v];
    } else if (inner) {
      const ImgDim ix = images_of(i, g.nx, gw, images & 3, (images >> 2) & 3), iy = images_of(j, g.ny, gw, (images >> 4) & 3, (images >> 6) & 3);
      const int nxi = ix.count(), nyi = iy.count();
      for (int b = 0; b < nyi; ++b)
        for (int a = 0; a < nxi; ++a) {
          double* o = Uout + (size_t)ix.coord(a) + (size_t)iy.coord(b) * g.sj;
          o[ID * N] = u[ID];
          o[IP * N] = u[IP];
          o[IU * N] = ix.flip(a) ? u[IU] * -1.0 : u[IU];
          o[IV * N] = iy.flip(b) ? u[IV] * -1.0 : u[IV];
        }
    }
  }
  if (dt_slots) rgpu::rg_slot_max_wave(dt_slots + (((unsigned)blockIdx.x * (unsigned)(TX * TY / 64) + (unsigned)(t >> 6)) & (rgpu::RG_DT_SLOTS - 1)), inv);
}

template <int TX, int TY, int SPEC>
__global__ void __launch_bounds__(TX * TY) hydro2d_step_kernel(DevParams g, int nbx, const double* __restrict__ Uin, double* __restrict__ Uout,
                                                               double dtdx, double dtdy, unsigned long long* dt_slots, int images, const StepClock* clk, ClockFold fold) {
  spec_assume<SPEC>(g);
  if (fold.out) {   // the clock of this step is part of the kernel (step_clock.h: clock_fold)
    __shared__ double Lred[TX * TY / 64];
    const StepClock r = clock_fold<TX * TY>(fold, Lred);
    if (r.stop) return;
    dtdx = rg_uniform(r.dtdx); dtdy = rg_uniform(r.dtdy);
  } else if (clk) {   // the time step lives on the device (hip/step_clock.h)
    if (clk->stop) return;
    dtdx = clk->dtdx; dtdy = clk->dtdy;
  }
  hydro2d_step_body<TX, TY, SPEC>(g, nbx, Uin, Uout, dtdx, dtdy, dt_slots, images);
}

// The tile and the grid of a fused 2D hydro launch, single box or ensemble: H2_TX x H2_TY threads finish (H2_TX-2) x (H2_TY-2) cells,
// owners cover i in [1, nbx*(H2_TX-2)] plus column 0.  Returns the tiles of a box (the workgroups of the single-box step), *nbx: those along x.
constexpr int H2_TX = 16, H2_TY = 16;
inline int hydro2d_tiles(const DevParams& g, int* nbx) {
  *nbx = (g.isize - 1 + (H2_TX - 2) - 1) / (H2_TX - 2);
  return *nbx * ((g.jsize - 1 + (H2_TY - 2) - 1) / (H2_TY - 2));
}

// configurations the fused 2D hydro step covers (the per-cell gravity field runs the flat kernels' own instantiations)
inline bool hydro2d_step_covers(const DevParams& g) { return tiled_enabled() && !g.three_d && !g.mhd && g.nvar == 4 && g.grav_on != 2; }

// The whole 2D hydro step U -> Unew.  dt_slots: RG_DT_SLOTS device slots for the CFL maximum of the new state (reset by the caller),
// or 0; images: see the kernel.  The instantiation: launchers.h (hydro_pick_spec, the list with the uniform-gravity entries).
// Returns 0 = done, 1 = not covered (the caller runs the flat kernels), < 0 = launch error.
inline int hydro2d_step(rg_stream_t s, const DevParams& g, const double* in, double* out, double dtdx, double dtdy, unsigned long long* dt_slots, int images, const StepClock* clk = 0,
                        const ClockFold* fold_in = 0) {
  if (!hydro2d_step_covers(g)) return 1;
  ClockFold fold;
  if (fold_in) fold = *fold_in; else { fold.prev = 0; fold.out = 0; fold.in = 0; fold.zero = 0; fold.t0 = 0.0; fold.tEnd = 0.0; }
  int nbx;
  const dim3 grid((unsigned)hydro2d_tiles(g, &nbx));
  return hydro_spec_dispatch<true>(hydro_pick_spec<true>(g), [&](auto tag) {
    hipLaunchKernelGGL((hydro2d_step_kernel<H2_TX, H2_TY, decltype(tag)::value>), grid, dim3(H2_TX * H2_TY), 0, s, g, nbx, in, out, dtdx, dtdy, dt_slots, images, clk, fold);
    return hipGetLastError() == hipSuccess ? 0 : -1;
  });
}

}  // namespace rgpu_tiled
