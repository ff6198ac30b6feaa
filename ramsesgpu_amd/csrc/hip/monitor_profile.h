// monitor_profile.h (HIP / gfx950 only; included from rg_tiled.h) -- the plane monitor of a lone 3D context (kernels_monitor_planes.h)
// for rgpu_state_monitor_planes and the samples rgpu_run_steps_monitored_planes takes inside its device-clock batches.
//
//   monitor_profile_cols_kernel     the pass over the state, in the split form DESIGN 3.4.2 measured as the faster one for the monitor:
//                                   thread ii of segment s (blockIdx.z) of plane kk (blockIdx.y), coalesced in ii, walks the rows of
//                                   the segment in ascending j with sixteen accumulators (monp_segment) -> part[kk][q][s * nx + ii]
//   monitor_profile_planes_kernel   one wave64 per plane: lane l does steps 2 and 3 (monp_lane), the butterfly runs across the lanes,
//                                   lane 0 writes the row to its destination -- `out` or the log slot -- at kk * MONP_NQ
// Two launches per sample; no sum over the planes, hence no finish kernel.  Both call the functions the flat functors call.
// clk != 0 (inside a batch): the StepClock record of the step the sample follows; a record that says stop ends every workgroup in its
// first instructions (a uniform scalar load), and the log slot stays unwritten -- the host reads the same record and does not look at it.
#pragma once
#include "kernels_monitor_planes.h"

namespace rgpu_tiled {

using namespace rgpu_dev;

// step 4 across the lanes of a wave64 holding L[lane] in a (mon_wave_butterfly, sixteen wide); every lane ends with the result
__device__ __forceinline__ void monp_wave_butterfly(double* a) {
  static_assert(MON_LANES == 64, "the lanes of the summation order are those of a wave");
#pragma unroll
  for (int off = MON_LANES / 2; off > 0; off >>= 1) {
    double x[MONP_NQ];
#pragma unroll
    for (int q = 0; q < MONP_NQ; ++q) x[q] = __shfl_xor(a[q], off, 64);
    monp_combine(a, x);
  }
}

__global__ void __launch_bounds__(256) monitor_profile_cols_kernel(DevParams g, const double* __restrict__ U, const StepClock* clk, double* __restrict__ part) {
  if (!mon_gate_open(clk)) return;
  const int ii = (int)(blockIdx.x * 256u + threadIdx.x), kk = (int)blockIdx.y, s = (int)blockIdx.z;
  if (ii >= g.nx) return;
  double a[MONP_NQ];
  monp_segment(g, U, kk, s, ii, a);
  const size_t R = (size_t)mon_nseg(g.ny) * g.nx;
  double* pk = part + (size_t)kk * MONP_NQ * R + (size_t)s * g.nx + ii;
#pragma unroll
  for (int q = 0; q < MONP_NQ; ++q) pk[(size_t)q * R] = a[q];
}

__global__ void __launch_bounds__(MON_LANES) monitor_profile_planes_kernel(int nx, int nseg, const StepClock* clk, const double* __restrict__ part, double* __restrict__ out) {
  if (!mon_gate_open(clk)) return;
  const unsigned kk = blockIdx.x;
  double a[MONP_NQ];
  monp_lane(nx, nseg, part + (size_t)kk * MONP_NQ * ((size_t)nseg * nx), (int)threadIdx.x, a);
  monp_wave_butterfly(a);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int q = 0; q < MONP_NQ; ++q) out[(size_t)kk * MONP_NQ + q] = a[q];
  }
}

// The launches; scratch: monp_scratch_doubles(g) doubles (the segment sums); out: g.nz rows of MONP_NQ doubles
inline int launch_monitor_profile(rg_stream_t s, const DevParams& g, const double* U, const StepClock* clk, double* scratch, double* out) {
  const int nseg = mon_nseg(g.ny);
  const dim3 grid(((unsigned)g.nx + 255u) / 256u, (unsigned)g.nz, (unsigned)nseg);
  hipLaunchKernelGGL(monitor_profile_cols_kernel, grid, dim3(256), 0, s, g, U, clk, scratch);
  if (hipGetLastError() != hipSuccess) return -1;
  hipLaunchKernelGGL(monitor_profile_planes_kernel, dim3((unsigned)g.nz), dim3(MON_LANES), 0, s, g.nx, nseg, clk, (const double*)scratch, out);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace rgpu_tiled
