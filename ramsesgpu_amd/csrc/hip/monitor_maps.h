// monitor_maps.h (HIP / gfx950 only; included from rg_tiled.h) -- the map monitor of a lone 3D context (kernels_monitor_maps.h) for
// rgpu_state_maps and the samples rgpu_run_steps_mapped takes inside its device-clock batches.
//
//   monitor_map_pixels_kernel    one thread per pixel (u, v), the 64 lanes of a wave along u, twelve accumulators, walking w ascending
//                                (map_pixel).  Axis z and axis y: u = i, every load of a wave is one contiguous run of 64 doubles.  Axis
//                                x, the "direct" variant: u = j, the lanes of a wave sit in 64 different rows of the state and walk along
//                                them -- the scattered access shape; right for a slice or a thin range, wrong for a projection
//   monitor_map_x_tiled_kernel   axis x, the "tiled" variant: a workgroup of four waves owns MAPX_ROWS rows (j, k) of the state and
//                                walks them in tiles of 64 cells along i.  Per tile each wave computes the channels of 64 consecutive
//                                cells of a row, one cell per lane (contiguous loads), and stores them to LDS at [channel][row][i]
//                                with a row pitch of MAPX_PITCH = 65 doubles; then lane (channel, row) of the first MAP_NQ * MAPX_ROWS
//                                threads adds its 64 values ascending in i to the accumulator it carries from tile to tile.  The odd
//                                pitch puts the 32 lanes an LDS read serves at once on 32 different pairs of banks (the address of
//                                lane L at step i is 65 L + i doubles: bank pair (L + i) mod 32), and the stores of a wave are 64
//                                consecutive doubles: neither side conflicts.  The additions of a pixel are those of the direct
//                                variant, in the same order: the same bits.
// LDS of the tiled kernel: MAP_NQ * MAPX_ROWS * MAPX_PITCH doubles = 49,920 bytes, three workgroups per CU of 160 KB.
// Every kernel writes straight to its destination, `out` or the log slot: a map needs no scratch.
// clk != 0 (inside a batch): the StepClock record of the step the sample follows; a record that says stop ends every workgroup in its
// first instructions, and the log slot stays unwritten -- the host reads the same record and does not look at it.
#pragma once
#include "kernels_monitor_maps.h"

namespace rgpu_tiled {

using namespace rgpu_dev;

enum { MAPX_ROWS = 8, MAPX_TILE = 64, MAPX_PITCH = MAPX_TILE + 1, MAPX_WAVES = 4 };
// Thickness hi - lo from which launch_monitor_map sums along x with the tiled variant: the smallest of 1, 2, 4, 8, 16, 64, nx from
// which it was the faster one at both sizes measured (scripts/monitor_maps_bench.py, profiles/monitor_maps_bench.json).
// Direct against tiled, microseconds: 512^3 MRI 4 cells 210 / 241, 8 cells 422 / 244; 256^3 implode3d 4 cells 22 / 28, 8 cells 41 / 28
// (the tiled kernel costs what one 64-cell tile costs however thin the range; the direct one grows with the thickness from the start)
enum { MAPX_TILED_FROM = 8 };

__global__ void __launch_bounds__(256) monitor_map_pixels_kernel(DevParams g, MapGeom m, const double* __restrict__ U, const StepClock* clk, double* __restrict__ out) {
  if (!mon_gate_open(clk)) return;
  const int u = (int)(blockIdx.x * 64u + threadIdx.x), v = (int)(blockIdx.y * 4u + threadIdx.y);
  if (u >= m.nu || v >= m.nv) return;
  double a[MAP_NQ];
  map_pixel(g, m, U, u, v, a);
  const size_t P = map_pixels(m);
  double* po = out + (size_t)v * m.nu + u;
#pragma unroll
  for (int q = 0; q < MAP_NQ; ++q) po[(size_t)q * P] = a[q];
}

__global__ void __launch_bounds__(64 * MAPX_WAVES) monitor_map_x_tiled_kernel(DevParams g, MapGeom m, const double* __restrict__ U, const StepClock* clk, double* __restrict__ out) {
  if (!mon_gate_open(clk)) return;
  __shared__ double tile[MAP_NQ * MAPX_ROWS * MAPX_PITCH];
  const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
  const size_t P = map_pixels(m);                       // rows of the state = pixels: row = v * nu + u = kk * ny + jj
  const size_t row0 = (size_t)blockIdx.x * MAPX_ROWS;
  // the summing lanes: thread L = q * MAPX_ROWS + r carries channel q of row row0 + r
  const bool sums = threadIdx.x < (unsigned)(MAP_NQ * MAPX_ROWS);
  const double* mine = tile + (size_t)threadIdx.x * MAPX_PITCH;
  double acc = 0.0;
  for (int w0 = m.lo; w0 < m.hi; w0 += MAPX_TILE) {
    const int nw = m.hi - w0 < MAPX_TILE ? m.hi - w0 : MAPX_TILE;
#pragma unroll
    for (int r = wave; r < MAPX_ROWS; r += MAPX_WAVES) {
      const size_t row = row0 + (size_t)r;
      if (row < P && lane < nw) {
        const unsigned o = m.o0 + (unsigned)(row % (size_t)m.nu) * m.su + (unsigned)(row / (size_t)m.nu) * m.sv + (unsigned)(w0 - m.lo + lane);
        double x[MAP_NQ];
        map_cell_terms(g, U, o, x);
#pragma unroll
        for (int q = 0; q < MAP_NQ; ++q) tile[(q * MAPX_ROWS + r) * MAPX_PITCH + lane] = x[q];
      }
    }
    __syncthreads();
    if (sums) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
      for (int i = 0; i < nw; ++i) acc = acc + mine[i];
    }
    __syncthreads();
  }
  if (sums) {
    const size_t row = row0 + (threadIdx.x % (unsigned)MAPX_ROWS);
    if (row < P) out[(size_t)(threadIdx.x / (unsigned)MAPX_ROWS) * P + row] = acc;
  }
}

// The launch of one map of U into out[MAP_NQ][nv][nu].  x_tiled: -1 the variant by the thickness, 0 direct, 1 tiled (axis x only)
inline int launch_monitor_map(rg_stream_t s, const DevParams& g, int axis, int lo, int hi, int x_tiled, const double* U, const StepClock* clk, double* out) {
  const MapGeom m = map_geom(g, axis, lo, hi);
  if (axis == 0 && (x_tiled < 0 ? hi - lo >= (int)MAPX_TILED_FROM : x_tiled != 0)) {
    const unsigned nblk = (unsigned)((map_pixels(m) + MAPX_ROWS - 1) / MAPX_ROWS);
    hipLaunchKernelGGL(monitor_map_x_tiled_kernel, dim3(nblk), dim3(64 * MAPX_WAVES), 0, s, g, m, U, clk, out);
  } else {
    const dim3 grid(((unsigned)m.nu + 63u) / 64u, ((unsigned)m.nv + 3u) / 4u);
    hipLaunchKernelGGL(monitor_map_pixels_kernel, grid, dim3(64, 4), 0, s, g, m, U, clk, out);
  }
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace rgpu_tiled
