// ensemble_monitor.h (HIP / gfx950 only; included from ensemble2d.h) -- the monitor of kernels_monitor.h for every member of an
// ensemble at once, sampled on the device INSIDE a batch of fused rounds (rgpu_ensemble_run_steps_monitored) or on the current
// states (rgpu_ensemble_monitor, api/entry_ensemble.h).
//
// Two launches per sample, the member in blockIdx.y:
//   ensemble_monitor_rows_kernel   thread (s, ii) of member m: step 1 of the summation order (mon_segment: the rows of segment s of
//                                  column ii, coalesced in ii) -> part[m][q][s * nx + ii]
//   ensemble_monitor_fold_kernel   one wave per member: lane l does steps 2 and 3 (mon_lane), the butterfly of step 4 runs across
//                                  the lanes (mon_wave_butterfly, hip/monitor3d.h), lane 0 writes the ten doubles to the log
//                                  slot (launch, m)
// Both call the functions the kernels of a lone context call, hence the bits of rgpu_state_monitor on one holding that state.
// Whether member m is sampled by a launch is decided on the device, in the first instructions of every workgroup, from values that
// are uniform over the workgroup (scalar loads): inside a batch the record of the round's tick must say that the step ran and the
// member's own step number after it, span[m].nStep0 + r1, must be a multiple of `every` -- the host queues the pair only for rounds
// where this can hold for some member and keeps exactly the slots it knows to be valid when it walks the records.
// dx, dy: by value (g) or, with the table of a parameter scan, member m's own (tab[m].g; the table is read, never written).
#pragma once
#include "monitor3d.h"

namespace rgpu_tiled {

// per member and batch: the member's step number before the batch's first round; parity: which of its two arrays holds the state
// (read only where the launch does not name one parity for all, i.e. outside a batch)
struct MonitorSpan { int nStep0, parity; };

// clk: the records of the round's tick, one per member (0: outside a batch -- every member is sampled)
__device__ __forceinline__ bool monitor_samples(const MonitorSpan* __restrict__ span, const StepClock* clk, unsigned m, int r1, int every) {
  if (!clk) return true;
  if (clk[m].stop) return false;
  return (span[m].nStep0 + r1) % every == 0;
}

// U: array 0 of member 0; array q of member m at + (q * members + m) * stride.  parity >= 0: the array every sampled member's state
// is in (the output of the round); < 0: span[m].parity.  part: members x MON_NQ x nseg x nx doubles
__global__ void __launch_bounds__(256) ensemble_monitor_rows_kernel(DevParams g, const MemberConst* __restrict__ tab, const double* __restrict__ U, unsigned stride,
                                                                    unsigned members, const MonitorSpan* __restrict__ span, const StepClock* clk, int r1, int every,
                                                                    int parity, double* __restrict__ part) {
  const unsigned m = blockIdx.y;
  if (!monitor_samples(span, clk, m, r1, every)) return;
  const int nseg = mon_nseg(g.ny);
  const unsigned R = (unsigned)nseg * (unsigned)g.nx;
  const unsigned idx = blockIdx.x * 256u + threadIdx.x;
  if (idx >= R) return;
  const double dx = tab ? tab[m].g.dx : g.dx, dy = tab ? tab[m].g.dy : g.dy;
  const unsigned par = parity >= 0 ? (unsigned)parity : (unsigned)span[m].parity;
  const double* Um = U + ((size_t)par * members + m) * stride;
  double a[MON_NQ];
  mon_segment<false>(g, dx, dy, g.dz, Um, 0, (int)(idx / (unsigned)g.nx), (int)(idx % (unsigned)g.nx), a);
  double* pm = part + (size_t)m * MON_NQ * R;
#pragma unroll
  for (int q = 0; q < MON_NQ; ++q) pm[(size_t)q * R + idx] = a[q];
}

// out: the log, slot (launch, m) at out[(launch * members + m) * MON_NQ]
__global__ void __launch_bounds__(MON_LANES) ensemble_monitor_fold_kernel(int nx, int ny, unsigned members, const MonitorSpan* __restrict__ span, const StepClock* clk, int r1,
                                                                          int every, const double* __restrict__ part, double* __restrict__ out, unsigned launch) {
  const unsigned m = blockIdx.y;
  if (!monitor_samples(span, clk, m, r1, every)) return;
  const int nseg = mon_nseg(ny);
  double a[MON_NQ];
  mon_lane(nx, nseg, part + (size_t)m * MON_NQ * ((size_t)nseg * nx), (int)threadIdx.x, a);
  mon_wave_butterfly(a);
  if (threadIdx.x == 0) {
    double* o = out + ((size_t)launch * members + m) * MON_NQ;
#pragma unroll
    for (int q = 0; q < MON_NQ; ++q) o[q] = a[q];
  }
}

// One sample of every member that qualifies (see above) into log slot `launch`.  g: the shared shape (and dx, dy when tab == 0).
inline int launch_ensemble_monitor(rg_stream_t s, int members, const DevParams& g, const MemberConst* tab, const double* U, unsigned stride, const MonitorSpan* span,
                                   const StepClock* clk, int r1, int every, int parity, double* part, double* out, unsigned launch) {
  const unsigned R = (unsigned)mon_nseg(g.ny) * (unsigned)g.nx;
  hipLaunchKernelGGL(ensemble_monitor_rows_kernel, dim3((R + 255u) / 256u, (unsigned)members), dim3(256), 0, s, g, tab, U, stride, (unsigned)members, span, clk, r1, every, parity, part);
  if (hipGetLastError() != hipSuccess) return -1;
  hipLaunchKernelGGL(ensemble_monitor_fold_kernel, dim3(1u, (unsigned)members), dim3(MON_LANES), 0, s, g.nx, g.ny, (unsigned)members, span, clk, r1, every, part, out, launch);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace rgpu_tiled
