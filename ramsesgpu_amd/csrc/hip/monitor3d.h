// monitor3d.h (HIP / gfx950 only; included from rg_tiled.h) -- the monitor of a 3D state (kernels_monitor.h: mon_vol_*) in three
// launches, for rgpu_state_monitor3d and for the samples rgpu_run_steps_monitored takes inside its device-clock batches.
//
//   monitor_vol_cols_kernel     the pass over the state.  Thread ii of segment s (blockIdx.z) of plane kk (blockIdx.y), coalesced in
//                               ii, walks the rows of the segment in ascending j (mon_vol_segment) -> part[kk][q][s * nx + ii], the
//                               layout of the 2D rows kernel per plane.  (A thread per whole column, forming C[ii] itself, was
//                               measured too and lost at every size: DESIGN 3.4.2.)
//   monitor_vol_planes_kernel   one wave64 per plane: lane l does steps 2 and 3 (mon_lane), the butterfly runs across the lanes
//                               (__shfl_xor, as ensemble_monitor_fold_kernel), lane 0 writes V[kk]
//   monitor_vol_finish_kernel   one wave64: V[0] + V[1] + .. in ascending order.  Lane l loads V[k0 + l] of a block of 64 planes (one
//                               round of loads instead of a chain of nz); every lane then adds the block's planes in order, each
//                               read from its lane (v_readlane); lane 0 writes out[MON_NQ]
// All three call the functions the flat functors call.  clk != 0 (inside a batch): the StepClock record of the step the sample
// follows; a record that says stop ends every workgroup in its first instructions (a uniform scalar load), and the log slot stays
// unwritten -- the host reads the same record and does not look at it.
#pragma once
#include "kernels_monitor.h"

namespace rgpu_tiled {

using namespace rgpu_dev;

__global__ void __launch_bounds__(256) monitor_vol_cols_kernel(DevParams g, const double* __restrict__ U, const StepClock* clk, double* __restrict__ part) {
  if (!mon_gate_open(clk)) return;
  const int ii = (int)(blockIdx.x * 256u + threadIdx.x), kk = (int)blockIdx.y, s = (int)blockIdx.z;
  if (ii >= g.nx) return;
  double a[MON_NQ];
  mon_vol_segment(g, U, kk, s, ii, a);
  const size_t R = (size_t)mon_nseg(g.ny) * g.nx;
  double* pk = part + (size_t)kk * MON_NQ * R + (size_t)s * g.nx + ii;
#pragma unroll
  for (int q = 0; q < MON_NQ; ++q) pk[(size_t)q * R] = a[q];
}

__global__ void __launch_bounds__(MON_LANES) monitor_vol_planes_kernel(int nx, int nseg, const StepClock* clk, const double* __restrict__ part, double* __restrict__ V) {
  static_assert(MON_LANES == 64, "one wave per plane");
  if (!mon_gate_open(clk)) return;
  const unsigned kk = blockIdx.x;
  double a[MON_NQ];
  mon_lane(nx, nseg, part + (size_t)kk * MON_NQ * ((size_t)nseg * nx), (int)threadIdx.x, a);
#pragma unroll
  for (int off = MON_LANES / 2; off > 0; off >>= 1) {
    double x[MON_NQ];
#pragma unroll
    for (int q = 0; q < MON_NQ; ++q) x[q] = __shfl_xor(a[q], off, 64);
    mon_combine(a, x);
  }
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

inline size_t monitor_vol_scratch_doubles(const DevParams& g) { return (size_t)MON_NQ * ((size_t)g.nz * mon_nseg(g.ny) * g.nx + (size_t)g.nz); }

// The three launches; scratch: monitor_vol_scratch_doubles(g) doubles (the segment sums, then V)
inline int launch_monitor_vol(rg_stream_t s, const DevParams& g, const double* U, const StepClock* clk, double* scratch, double* out) {
  const int nseg = mon_nseg(g.ny);
  double* V = scratch + (size_t)MON_NQ * g.nz * nseg * g.nx;
  hipLaunchKernelGGL(monitor_vol_cols_kernel, dim3(((unsigned)g.nx + 255u) / 256u, (unsigned)g.nz, (unsigned)nseg), dim3(256), 0, s, g, U, clk, scratch);
  if (hipGetLastError() != hipSuccess) return -1;
  hipLaunchKernelGGL(monitor_vol_planes_kernel, dim3((unsigned)g.nz), dim3(MON_LANES), 0, s, g.nx, nseg, clk, (const double*)scratch, V);
  if (hipGetLastError() != hipSuccess) return -1;
  hipLaunchKernelGGL(monitor_vol_finish_kernel, dim3(1), dim3(64), 0, s, g.nz, clk, (const double*)V, out);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace rgpu_tiled
