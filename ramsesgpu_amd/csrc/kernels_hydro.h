// kernels_hydro.h -- the hydro unsplit step ("unsplitVersion 1" and, through the order of the update, "unsplitVersion 2"),
// 2D (NV=4) and 3D (NV=5): the cell numerics as functions of register values, and the per-cell bodies of the flat kernels.
//   hydro_prim_cell    U         -> Q  (NV)          convertToPrimitives   HydroRunGodunov.cpp:4133-4262
//   hydro_trace_cell   Q         -> TH (NV*(1+ND))   slopes + trace        HydroRunGodunov.cpp:2454-2509, 2666-2748
//   hydro_flux_cell    TH        -> FH (NV*ND)       Riemann at low faces  HydroRunGodunov.cpp:2525-2565, 2757-2822
//   hydro_update_cell  Uold,FH   -> Unew             gather form of the scatter update :2574-2607, :2831-2895
//   hydro_invdt_cell   U         -> CFL term of the cell
// TH is the compact traced state: the time-advanced cell state and the limited half slopes; the face states
// qm/qp = state +/- half slope (+ floors) are rebuilt in the flux kernel (trace.h:384-412, 610-659).
#pragma once
#include "kernels_mhd3d.h"

namespace rgpu_dev {

template <int NV>
RG_DEVFN void hydro_prim_cell(const DevParams& g, const double* __restrict__ U, double* __restrict__ Q, unsigned idx) {
  const size_t N = g.ncell;
  double u[NV], q[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v) u[v] = U[idx + v * N];
  hydro_prim<NV>(g, u, q);
#pragma unroll
  for (int v = 0; v < NV; ++v) Q[idx + v * N] = q[v];
}

// ---- the cell numerics, written once: values in registers, no memory access.  The flat kernels below, the fused 2D step
// (hip/tiled_hydro2d.h) and the 3D sweep (hip/tiled_hydro.h) call these, so the emulation build of the flat kernels pins the very
// functions the tiled kernels inline.  Operand order: the reference's, expression by expression (dev_numerics.h). ----

// limited HALF slope of one variable along one direction: the reference's slope x 0.5 (trace.h:350-360), formed as a half slope
// (dev_numerics.h: tvd_half_slope); slope_unsplit_3d type 1 is the minmod of slope.h:351-384
template <int ND>
RG_DEVFN double hydro_half_slope(double st, double qm, double q, double qp) {
  if (st == 0) return 0.0;
  if (ND == 3 && st == 1) return minmod_half_slope(qm, q, qp);
  return tvd_half_slope(st, qm, q, qp);
}

// primitives q and half slopes h[d][v] of a cell -> its state advanced by half a time step, tq (trace.h:362-382, 560-608)
template <int ND, int NV>
RG_DEVFN void hydro_trace_advance(const DevParams& g, const double* q, const double (*h)[NV], double dtdx, double dtdy, double dtdz,
                                  double* tq) {
  const double r = q[ID], p = q[IP], u = q[IU], v = q[IV], w = (NV == 5) ? q[IW] : 0.0;
  const double gamma = g.gamma0;
  const double drx = h[0][ID], dpx = h[0][IP], dux = h[0][IU], dvx = h[0][IV];
  const double dry = h[1][ID], dpy = h[1][IP], duy = h[1][IU], dvy = h[1][IV];
  double sr0, su0, sv0, sw0 = 0.0, sp0;
  const rg_recip_t inv_r = rg_recip(r);
  if (ND == 2) {
    sr0 = (-u * drx - dux * r) * dtdx + (-v * dry - dvy * r) * dtdy;
    su0 = (-u * dux - rg_div(dpx, inv_r)) * dtdx + (-v * duy) * dtdy;
    sv0 = (-u * dvx) * dtdx + (-v * dvy - rg_div(dpy, inv_r)) * dtdy;
    sp0 = (-u * dpx - dux * gamma * p) * dtdx + (-v * dpy - dvy * gamma * p) * dtdy;
  } else {
    const double dwx = h[0][NV - 1], dwy = h[1][NV - 1];
    const double drz = h[ND - 1][ID], dpz = h[ND - 1][IP], duz = h[ND - 1][IU], dvz = h[ND - 1][IV], dwz = h[ND - 1][NV - 1];
    sr0 = (-u * drx - dux * r) * dtdx + (-v * dry - dvy * r) * dtdy + (-w * drz - dwz * r) * dtdz;
    su0 = (-u * dux - rg_div(dpx, inv_r)) * dtdx + (-v * duy) * dtdy + (-w * duz) * dtdz;
    sv0 = (-u * dvx) * dtdx + (-v * dvy - rg_div(dpy, inv_r)) * dtdy + (-w * dvz) * dtdz;
    sw0 = (-u * dwx) * dtdx + (-v * dwy) * dtdy + (-w * dwz - rg_div(dpz, inv_r)) * dtdz;
    sp0 = (-u * dpx - dux * gamma * p) * dtdx + (-v * dpy - dvy * gamma * p) * dtdy + (-w * dpz - dwz * gamma * p) * dtdz;
  }
  tq[ID] = r + sr0; tq[IP] = p + sp0; tq[IU] = u + su0; tq[IV] = v + sv0;
  if (NV == 5) tq[NV - 1] = w + sw0;
}

// state at the high (SIDE=+1, the reference's qm) / low (SIDE=-1, qp) face of a cell along the direction of the half slopes hd, grid
// frame: the floors of trace.h:388-389, then the gravity predictor on the traced state (HydroRunGodunov.cpp:2485-2497, 2705-2734)
// with (0.5 dt) g = (gx, gy, gz) when grav is set
template <int SIDE, int NV>
RG_DEVFN void hydro_face_grid(const DevParams& g, const double* tq, const double* hd, bool grav, double gx, double gy, double gz,
                              double* o) {
#pragma unroll
  for (int n = 0; n < NV; ++n) o[n] = (SIDE > 0) ? tq[n] + hd[n] : tq[n] - hd[n];
  o[ID] = fmax(g.smallr, o[ID]);
  o[IP] = fmax(g.smallp * o[ID], o[IP]);
  if (grav) {
    o[IU] += gx;
    o[IV] += gy;
    if (NV == 5) o[NV - 1] += gz;
  }
}

// grid frame <-> face-normal frame of direction D: IU trades places with the normal velocity (the map is its own inverse)
template <int D, int NV>
RG_DEVFN void hydro_to_normal(const double* a, double* o) {
  constexpr int swp = (D == 0) ? IU : (D == 1) ? IV : IW;
#pragma unroll
  for (int n = 0; n < NV; ++n) o[n] = a[(n == IU) ? swp : (n == swp) ? IU : n];
}

// Riemann problem at a face normal to D between the grid-frame states ql (high face of the cell below) and qr (low face of the
// cell above); the flux f is in the face-normal frame
template <int D, int NV>
RG_DEVFN void hydro_face_flux(const DevParams& g, const double* ql, const double* qr, double* f) {
  double l[NV], r[NV];
  hydro_to_normal<D, NV>(ql, l);
  hydro_to_normal<D, NV>(qr, r);
#pragma unroll
  for (int n = 0; n < NV; ++n) f[n] = 0.0;
  hydro_riemann<NV>(g, l, r, f);
}

// u += (SIGN=+1: the cell's low face) or -= (SIGN=-1: its high face) dtd * f, f a flux through a face normal to D in the face-normal
// frame.  The caller sequences the faces: low faces then high faces in x,y,z order (unsplitVersion 1), or +x, -x, +y, -y, +z, -z
// (unsplitVersion 2, g.dirwise_update: the direction-wise sweeps of the reference, HydroRunGodunov.cpp:2955-3849).
template <int D, int SIGN, int NV>
RG_DEVFN void hydro_apply_flux(double* u, const double* f, double dtd) {
  double fg[NV];
  hydro_to_normal<D, NV>(f, fg);
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    if (SIGN > 0) u[v] += fg[v] * dtd; else u[v] -= fg[v] * dtd;
  }
}

// momentum source of static gravity, (0.5 dt) g = (gx, gy, gz), with the old plus the new density (compute_gravity_source_term,
// HydroRunBase.cpp:1925-1985); energy untouched
template <int NV>
RG_DEVFN void hydro_gravity_source(double* u, double rho_old, double gx, double gy, double gz) {
  const double rho_sum = rho_old + u[ID];
  u[IU] += gx * rho_sum;
  u[IV] += gy * rho_sum;
  if (NV == 5) u[NV - 1] += gz * rho_sum;
}

// CFL term of a cell with conservative state u: sum over the directions of (c + |v_d|) / delta_d
template <int NV>
RG_DEVFN double hydro_cfl_term(const DevParams& g, const double* u) {
  double q[NV];
  const double cs = hydro_prim<NV>(g, u, q);
  if (NV == 5) return (cs + fabs(q[IU])) / g.dx + (cs + fabs(q[IV])) / g.dy + (cs + fabs(q[IW])) / g.dz;
  return (cs + fabs(q[IU])) / g.dx + (cs + fabs(q[IV])) / g.dy;
}

// ---- the flat kernels' cells: load from global memory, call the functions above, store ----

template <int ND, int NV>
RG_DEVFN void hydro_trace_cell(const DevParams& g, const double* __restrict__ Q, double* __restrict__ T, double dtdx,
                               double dtdy, double dtdz, unsigned idx) {
  const IJK c = unflatten(g, idx);
  if (c.i < 1 || c.i >= g.isize - 1 || c.j < 1 || c.j >= g.jsize - 1) return;
  if (ND == 3 && (c.k < 1 || c.k >= g.ksize - 1)) return;
  const size_t N = g.ncell;
  const unsigned strd[3] = {1u, g.sj, g.sk};
  const double st = g.slope_type;
  double q[NV], h[ND][NV], tq[NV];  // h = HALF slopes
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    const double* Qc = Q + v * N;
    q[v] = Qc[idx];
#pragma unroll
    for (int d = 0; d < ND; ++d) h[d][v] = hydro_half_slope<ND>(st, Qc[idx - strd[d]], q[v], Qc[idx + strd[d]]);
  }
  hydro_trace_advance<ND, NV>(g, q, h, dtdx, dtdy, dtdz, tq);
  double* t = T + idx;
#pragma unroll
  for (int n = 0; n < NV; ++n) t[(size_t)n * N] = tq[n];
#pragma unroll
  for (int d = 0; d < ND; ++d)
#pragma unroll
    for (int n = 0; n < NV; ++n) t[(size_t)(NV * (1 + d) + n) * N] = h[d][n];
}

// qm[D] (SIDE=+1) / qp[D] (SIDE=-1) of cell m, rebuilt from the compact traced state (grid frame)
template <int D, int SIDE, int NV, bool GF>
RG_DEVFN void hydro_face_state(const DevParams& g, const double* __restrict__ T, unsigned m, double* o) {
  const size_t N = g.ncell;
  const double* t = T + m;
  double tq[NV], hd[NV];
#pragma unroll
  for (int n = 0; n < NV; ++n) { tq[n] = t[(size_t)n * N]; hd[n] = t[(size_t)(NV * (1 + D) + n) * N]; }
  const bool grav = GF || g.grav_on;
  double gx = 0.0, gy = 0.0, gz = 0.0;
  if (grav) half_dt_gravity<GF>(g, m, gx, gy, gz);
  hydro_face_grid<SIDE, NV>(g, tq, hd, grav, gx, gy, gz, o);
}

// flux through the low face of cell idx along D (strd = the flat stride of D)
template <int D, int NV, bool GF>
RG_DEVFN void hydro_flux_dir(const DevParams& g, const double* __restrict__ T, double* __restrict__ F, unsigned idx, unsigned strd) {
  double ql[NV], qr[NV], fl[NV];
  hydro_face_state<D, +1, NV, GF>(g, T, idx - strd, ql);
  hydro_face_state<D, -1, NV, GF>(g, T, idx, qr);
  hydro_face_flux<D, NV>(g, ql, qr, fl);
#pragma unroll
  for (int n = 0; n < NV; ++n) F[idx + (size_t)(D * NV + n) * g.ncell] = fl[n];
}

template <int ND, int NV, bool GF>
RG_DEVFN void hydro_flux_cell(const DevParams& g, const double* __restrict__ T, double* __restrict__ F, unsigned idx) {
  const IJK c = unflatten(g, idx);
  if (c.i < g.gw || c.i > g.isize - g.gw || c.j < g.gw || c.j > g.jsize - g.gw) return;
  if (ND == 3 && (c.k < g.gw || c.k > g.ksize - g.gw)) return;
  hydro_flux_dir<0, NV, GF>(g, T, F, idx, 1u);
  hydro_flux_dir<1, NV, GF>(g, T, F, idx, g.sj);
  if (ND == 3) hydro_flux_dir<2, NV, GF>(g, T, F, idx, g.sk);
}

// the flux the flux kernel stored for the low face of cell m along D, applied to u
template <int D, int SIGN, int NV>
RG_DEVFN void hydro_apply_stored_flux(const DevParams& g, const double* __restrict__ F, unsigned m, double* u, double dtd) {
  double f[NV];
#pragma unroll
  for (int n = 0; n < NV; ++n) f[n] = F[m + (size_t)(D * NV + n) * g.ncell];
  hydro_apply_flux<D, SIGN, NV>(u, f, dtd);
}

template <int ND, int NV, bool GF>
RG_DEVFN void hydro_update_cell(const DevParams& g, const double* __restrict__ Uold, double* __restrict__ Unew,
                                const double* __restrict__ F, double dtdx, double dtdy, double dtdz, unsigned idx,
                                unsigned long long* dt_slots = 0) {
  const IJK c = unflatten(g, idx);
  const size_t N = g.ncell;
  const int gw = g.gw;
  double u[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v) u[v] = Uold[idx + v * N];
  bool inner = c.i >= gw && c.i < g.isize - gw && c.j >= gw && c.j < g.jsize - gw;
  if (ND == 3) inner = inner && c.k >= gw && c.k < g.ksize - gw;
  if (inner) {
    const double rho_old = u[ID];
    const unsigned hx = idx + 1u, hy = idx + g.sj, hz = idx + g.sk;   // the cells whose low faces are this cell's high faces
    if (!g.dirwise_update) {
      hydro_apply_stored_flux<0, +1, NV>(g, F, idx, u, dtdx);
      hydro_apply_stored_flux<1, +1, NV>(g, F, idx, u, dtdy);
      if (ND == 3) hydro_apply_stored_flux<2, +1, NV>(g, F, idx, u, dtdz);
      hydro_apply_stored_flux<0, -1, NV>(g, F, hx, u, dtdx);
      hydro_apply_stored_flux<1, -1, NV>(g, F, hy, u, dtdy);
      if (ND == 3) hydro_apply_stored_flux<2, -1, NV>(g, F, hz, u, dtdz);
    } else {
      hydro_apply_stored_flux<0, +1, NV>(g, F, idx, u, dtdx);
      hydro_apply_stored_flux<0, -1, NV>(g, F, hx, u, dtdx);
      hydro_apply_stored_flux<1, +1, NV>(g, F, idx, u, dtdy);
      hydro_apply_stored_flux<1, -1, NV>(g, F, hy, u, dtdy);
      if (ND == 3) hydro_apply_stored_flux<2, +1, NV>(g, F, idx, u, dtdz);
      if (ND == 3) hydro_apply_stored_flux<2, -1, NV>(g, F, hz, u, dtdz);
    }
    if (GF || g.grav_on) {
      double gx, gy, gz;
      half_dt_gravity<GF>(g, idx, gx, gy, gz);
      hydro_gravity_source<NV>(u, rho_old, gx, gy, gz);
    }
  }
  if (dt_slots)   // the CFL scan of the new state rides along (hydro_invdt_cell on the cell just updated); all lanes of the wave
    rgpu::rg_slot_max_wave(dt_slots + ((idx >> 6) & (rgpu::RG_DT_SLOTS - 1)), inner ? hydro_cfl_term<NV>(g, u) : 0.0);
#pragma unroll
  for (int v = 0; v < NV; ++v) Unew[idx + v * N] = u[v];
}

// CFL scan: value of one cell, 0 outside the interior (all contributions are >= 0)
template <int NV>
RG_DEVFN double hydro_invdt_cell(const DevParams& g, const double* __restrict__ U, unsigned idx) {
  const IJK c = unflatten(g, idx);
  const int gw = g.gw;
  if (c.i < gw || c.i >= g.isize - gw || c.j < gw || c.j >= g.jsize - gw) return 0.0;
  if (NV == 5 && (c.k < gw || c.k >= g.ksize - gw)) return 0.0;
  double u[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v) u[v] = U[idx + v * g.ncell];
  return hydro_cfl_term<NV>(g, u);
}

}  // namespace rgpu_dev
