// kernels_monitor_maps.h -- the map monitor (rgpu_state_maps, rgpu_run_steps_mapped; include/rgpu.h, "map monitors"): MAP_NQ = 12
// channels per pixel of a 2D picture of a 3D state U[parity] -- a slice, or the sum over a range of cells along one axis: the mid-plane
// density, an x-z cut of By, the column density along each axis.
//
// Nothing of the per-cell arithmetic is restated here.  The channels of a cell are twelve of the sixteen terms of monp_cell_terms
// (kernels_monitor_planes.h), which are the monitor's (kernels_monitor.h): rho mx my mz E ekin emag eint bx by bz rho2 = its columns
// 0 1 2 3 4 5 6 8 10 11 12 15.  A pixel is the sum of the channel over w = lo .. hi - 1 along the map's axis, ascending, from +0.0,
// "a = a + x" at every step: no segments, no butterfly, no floating-point atomics.  A slice is the range of one cell.
//
// The axes: axis 0 = x, 1 = y, 2 = z is the direction summed over (w); the remaining two are (u, v), u fastest in memory:
//   z: u = i, v = j      y: u = i, v = k      x: u = j, v = k          out[q][v][u], q the channel
//
// Shared by the flat functor below (the test-only host emulation and any backend without kernels of its own) and by the gfx950
// kernels of hip/monitor_maps.h.  A header of its own: nothing the other kernels include changes.
#pragma once
#include "kernels_monitor_planes.h"

namespace rgpu_dev {

enum { MAP_NQ = 12 };

// where a map lies in the state: extents of (u, v), strides of (u, v, w) in cells, the offset of the cell u = v = 0, w = lo
struct MapGeom {
  int nu, nv, lo, hi;
  unsigned su, sv, sw, o0;
};
RG_MON_FN MapGeom map_geom(const DevParams& g, int axis, int lo, int hi) {
  MapGeom m;
  const unsigned s[3] = {1u, g.sj, g.sk};
  const int n[3] = {g.nx, g.ny, g.nz};
  const int iu = axis == 0 ? 1 : 0, iv = axis == 2 ? 1 : 2;
  m.nu = n[iu]; m.nv = n[iv]; m.lo = lo; m.hi = hi;
  m.su = s[iu]; m.sv = s[iv]; m.sw = s[axis];
  m.o0 = (unsigned)g.gw * (1u + g.sj + g.sk) + (unsigned)lo * m.sw;
  return m;
}
RG_MON_FN size_t map_pixels(const MapGeom& m) { return (size_t)m.nu * (size_t)m.nv; }

// the twelve channels of the cell at flat index o of a 3D state
RG_DEVFN void map_cell_terms(const DevParams& g, const double* __restrict__ U, unsigned o, double* m) {
  double t[MONP_NQ];
  monp_cell_terms(g, U, o, t);
  m[0] = t[0]; m[1] = t[1]; m[2] = t[2]; m[3] = t[3]; m[4] = t[4]; m[5] = t[5]; m[6] = t[6];
  m[7] = t[8]; m[8] = t[10]; m[9] = t[11]; m[10] = t[12]; m[11] = t[15];
}
// a <- a + x, the twelve channels
RG_MON_FN void map_add(double* a, const double* x) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
#pragma unroll
  for (int q = 0; q < MAP_NQ; ++q) a[q] = a[q] + x[q];
}
// the pixel (u, v): the cells w = lo .. hi - 1 in ascending order
RG_DEVFN void map_pixel(const DevParams& g, const MapGeom& m, const double* __restrict__ U, int u, int v, double* a) {
#pragma unroll
  for (int q = 0; q < MAP_NQ; ++q) a[q] = 0.0;
  unsigned o = m.o0 + (unsigned)u * m.su + (unsigned)v * m.sv;
  for (int w = m.lo; w < m.hi; ++w, o += m.sw) {
    double x[MAP_NQ];
    map_cell_terms(g, U, o, x);
    map_add(a, x);
  }
}

// ---- the flat kernel (rg_launch): the host emulation and any backend without kernels of its own -------------------------------------
// thread idx = v * nu + u (u fastest) -> out[q][v][u]
struct K_mon_map {
  DevParams g; MapGeom m; const double* U; double* out; const StepClock* clk;
  RG_DEVFN void operator()(unsigned idx) const {
    if (!mon_gate_open(clk)) return;
    const size_t P = map_pixels(m);
    if (idx >= P) return;
    double a[MAP_NQ];
    map_pixel(g, m, U, (int)(idx % (unsigned)m.nu), (int)(idx / (unsigned)m.nu), a);
#pragma unroll
    for (int q = 0; q < MAP_NQ; ++q) out[(size_t)q * P + idx] = a[q];
  }
};

}  // namespace rgpu_dev
