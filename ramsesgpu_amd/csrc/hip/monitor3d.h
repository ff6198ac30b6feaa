// monitor3d.h (HIP / gfx950 only; included from rg_tiled.h and ensemble_monitor.h) -- the monitor of a lone context's state
// (kernels_monitor.h), 3D or 2D (a volume of one plane), for rgpu_state_monitor, rgpu_state_monitor3d and the samples
// rgpu_run_steps_monitored takes inside its device-clock batches.
//
//   monitor_vol_cols_kernel     the pass over the state (monitor_plane_cols_kernel: the same body for a 2D state, chosen at launch).
//                               Thread ii of segment s (blockIdx.z) of plane kk (blockIdx.y), coalesced in
//                               ii, walks the rows of the segment in ascending j (mon_segment) -> part[kk][q][s * nx + ii].  (A thread
//                               per whole column, forming C[ii] itself, was measured too and lost at every size: DESIGN 3.4.2.)
//   monitor_vol_planes_kernel   one wave64 per plane: lane l does steps 2 and 3 (mon_lane), the butterfly runs across the lanes
//                               (mon_wave_butterfly), lane 0 writes V[kk]
//   monitor_vol_finish_kernel   one wave64: V[0] + V[1] + .. in ascending order.  Lane l loads V[k0 + l] of a block of 64 planes (one
//                               round of loads instead of a chain of nz); every lane then adds the block's planes in order, each
//                               read from its lane (v_readlane); lane 0 writes out[MON_NQ].  Not launched for one plane, whose V[0]
//                               is the result bit for bit (kernels_monitor.h): the planes kernel writes it to `out`.
// All three call the functions the flat functors call.  clk != 0 (inside a batch): the StepClock record of the step the sample
// follows; a record that says stop ends every workgroup in its first instructions (a uniform scalar load), and the log slot stays
// unwritten -- the host reads the same record and does not look at it.
#pragma once
#include "kernels_monitor.h"

namespace rgpu_tiled {

using namespace rgpu_dev;

// step 4 across the lanes of a wave64 holding L[lane] in a: "L[l] + L[l ^ off]" on every lane; every lane ends with the result
__device__ __forceinline__ void mon_wave_butterfly(double* a) {
  static_assert(MON_LANES == 64, "the lanes of the summation order are those of a wave");
#pragma unroll
  for (int off = MON_LANES / 2; off > 0; off >>= 1) {
    double x[MON_NQ];
#pragma unroll
    for (int q = 0; q < MON_NQ; ++q) x[q] = __shfl_xor(a[q], off, 64);
    mon_combine(a, x);
  }
}

template <bool VOL>
__device__ __forceinline__ void monitor_cols_body(const DevParams& g, const double* __restrict__ U, const StepClock* clk, double* __restrict__ part) {
  if (!mon_gate_open(clk)) return;
  const int ii = (int)(blockIdx.x * 256u + threadIdx.x), kk = (int)blockIdx.y, s = (int)blockIdx.z;
  if (ii >= g.nx) return;
  double a[MON_NQ];
  mon_segment<VOL>(g, g.dx, g.dy, g.dz, U, kk, s, ii, a);
  const size_t R = (size_t)mon_nseg(g.ny) * g.nx;
  double* pk = part + (size_t)kk * MON_NQ * R + (size_t)s * g.nx + ii;
#pragma unroll
  for (int q = 0; q < MON_NQ; ++q) pk[(size_t)q * R] = a[q];
}
// the two instantiations, chosen at launch by the dimension of the context (two names: the 3D one keeps the name, the code and the
// compiler-reported numbers it had)
__global__ void __launch_bounds__(256) monitor_vol_cols_kernel(DevParams g, const double* __restrict__ U, const StepClock* clk, double* __restrict__ part) {
  monitor_cols_body<true>(g, U, clk, part);
}
__global__ void __launch_bounds__(256) monitor_plane_cols_kernel(DevParams g, const double* __restrict__ U, const StepClock* clk, double* __restrict__ part) {
  monitor_cols_body<false>(g, U, clk, part);
}

__global__ void __launch_bounds__(MON_LANES) monitor_vol_planes_kernel(int nx, int nseg, const StepClock* clk, const double* __restrict__ part, double* __restrict__ V) {
  if (!mon_gate_open(clk)) return;
  const unsigned kk = blockIdx.x;
  double a[MON_NQ];
  mon_lane(nx, nseg, part + (size_t)kk * MON_NQ * ((size_t)nseg * nx), (int)threadIdx.x, a);
  mon_wave_butterfly(a);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int q = 0; q < MON_NQ; ++q) V[(size_t)kk * MON_NQ + q] = a[q];
  }
}

__global__ void __launch_bounds__(64) monitor_vol_finish_kernel(int nz, const StepClock* clk, const double* __restrict__ V, double* __restrict__ out) {
  if (!mon_gate_open(clk)) return;
  const int lane = (int)threadIdx.x;
  double a[MON_NQ];
  mon_init(a);
  for (int k0 = 0; k0 < nz; k0 += 64) {
    double x[MON_NQ];
    const int kk = k0 + lane < nz ? k0 + lane : nz - 1;   // (a lane past the last plane loads a plane that is not added from it)
#pragma unroll
    for (int q = 0; q < MON_NQ; ++q) x[q] = V[(size_t)kk * MON_NQ + q];
#pragma unroll
    for (int l = 0; l < 64; ++l) {
      if (k0 + l < nz) {   // (uniform)
        double y[MON_NQ];
#pragma unroll
        for (int q = 0; q < MON_NQ; ++q) y[q] = __shfl(x[q], l, 64);
        mon_combine(a, y);
      }
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int q = 0; q < MON_NQ; ++q) out[q] = a[q];
  }
}

// The launches; scratch: mon_scratch_doubles(g) doubles (the segment sums, then V)
inline int launch_monitor_vol(rg_stream_t s, const DevParams& g, const double* U, const StepClock* clk, double* scratch, double* out) {
  const int nseg = mon_nseg(g.ny), nz = mon_nplanes(g);
  double* V = nz == 1 ? out : scratch + (size_t)MON_NQ * nz * nseg * g.nx;
  const dim3 grid(((unsigned)g.nx + 255u) / 256u, (unsigned)nz, (unsigned)nseg);
  if (g.three_d) hipLaunchKernelGGL(monitor_vol_cols_kernel, grid, dim3(256), 0, s, g, U, clk, scratch);
  else hipLaunchKernelGGL(monitor_plane_cols_kernel, grid, dim3(256), 0, s, g, U, clk, scratch);
  if (hipGetLastError() != hipSuccess) return -1;
  hipLaunchKernelGGL(monitor_vol_planes_kernel, dim3((unsigned)nz), dim3(MON_LANES), 0, s, g.nx, nseg, clk, (const double*)scratch, V);
  if (hipGetLastError() != hipSuccess) return -1;
  if (nz == 1) return 0;
  hipLaunchKernelGGL(monitor_vol_finish_kernel, dim3(1), dim3(64), 0, s, nz, clk, (const double*)V, out);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace rgpu_tiled
