// ensemble2d.h (HIP / gfx950 only) -- many 2D boxes of ONE shape and ONE solver configuration stepped by one launch (rgpu_ensemble_*,
// api/entry_ensemble.h).
//
// A fused 2D step (tiled_hydro2d.h, tiled_mhd2d.h) is one kernel of 20-50 us: a 128^2 hydro box is ~100 workgroups on a device that
// keeps ~768 resident, Orszag-Tang 512^2 is bound by launch latency.  What 2D users run is many such boxes (seeds of a perturbation,
// parameter scans); stepped one after another, M boxes cost M latency-bound steps.  Here the member is the second grid dimension:
//   workgroup (blockIdx.x, blockIdx.y = m) runs the single-box body (hydro2d_step_body / mhd2d_step_body: the same instructions, hence
//   the same doubles) on tile blockIdx.x of member m: it reads U + m * stride, writes Unew + m * stride, accumulates the CFL maxima of
//   the state it writes into member m's own RG_DT_SLOTS slots and takes its time step from member m's own StepClock record;
//   a member whose record says stop (its t reached its tEnd, its dt is not a number) returns in its first instructions.
// ensemble_clock_kernel is step_clock_kernel with one workgroup per member: the same fold, the same step_clock_form, the same
// re-zeroing rule -- one launch per step for all members.  Records are laid out tick-major (record of tick n, member m at
// [n * members + m]) so that the host reads the records of a batch back in one contiguous copy.
// ensemble_scan.h (included at the end): the same three kernels with DevParams / RotCoef / ClockConst per member, read from a table in
// device memory instead of the kernel arguments -- a parameter scan (rgpu_ensemble_create_scan).
// ensemble_monitor.h (after it): the monitor of kernels_monitor.h with the member as the second grid dimension.
#pragma once
#include "tiled_hydro2d.h"
#include "tiled_mhd2d.h"

namespace rgpu_tiled {

// where a batch of member m starts and ends: t0 = its time, tEnd = its end time (a member that does not take part in the batch has
// tEnd = -inf: its first record says stop, its state, ghost cells and slots stay as they are)
struct EnsembleSpan { double t0, tEnd; };
constexpr size_t ENSEMBLE_SLOT_STRIDE = 3 * (size_t)rgpu::RG_DT_SLOTS;   // member to member in the slot arrays (rgpu_ctx::d_red_base: three rotating arrays each)

// slots: member 0's slot array, member m's at + m * ENSEMBLE_SLOT_STRIDE; prev / out: the records of the previous / this tick, one per member
// (prev == 0: the batch starts at span[m].t0)
__global__ void __launch_bounds__(1024) ensemble_clock_kernel(unsigned long long* __restrict__ slots, ClockConst k,
                                                              const EnsembleSpan* __restrict__ span, const StepClock* prev, StepClock* out) {
  __shared__ double red[16];
  __shared__ int runs;
  const int t = (int)threadIdx.x;
  const size_t m = blockIdx.x;
  unsigned long long* mine = slots + m * ENSEMBLE_SLOT_STRIDE;
  static_assert(rgpu::RG_DT_SLOTS == 1024, "one slot per thread");
  double v = __longlong_as_double((long long)mine[t]);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
  if ((t & 63) == 0) red[t >> 6] = v;
  __syncthreads();
  if (t == 0) {
    double mx = red[0];
#pragma unroll
    for (int w = 1; w < 16; ++w) mx = fmax(mx, red[w]);
    StepClock r;
    step_clock_form(k, mx, prev ? prev[m].t_next : span[m].t0, span[m].tEnd, prev ? prev[m].stop : 0, &r);
    out[m] = r;
    runs = r.stop == 0;
  }
  __syncthreads();
  if (runs) mine[t] = 0ull;   // (as step_clock_kernel: a stopped member keeps the maxima of the last state it wrote)
}

// The step kernels.  in / out: member 0's arrays, member m's at + m * stride doubles (stride < 2^32: rgpu_ensemble_create checks);
// dt_slots: member 0's slot array, member m's 3 * RG_DT_SLOTS further (the three rotating arrays of a context, rgpu_ctx::d_red_base);
// clk: the records of this step's tick, one per member.  The record of member m is read here (uniform loads) and handed to the body by
// value, as the single-box kernel hands on its arguments.

// a double kept in vector registers from here on (the opposite of rg_uniform, step_clock.h)
__device__ __forceinline__ double rg_in_vector(double x) { asm volatile("" : "+v"(x)); return x; }

template <int TX, int TY, int SPEC>
__global__ void __launch_bounds__(TX * TY) hydro2d_ensemble_kernel(DevParams g, int nbx, const double* __restrict__ Uin, double* __restrict__ Uout, unsigned stride,
                                                                   unsigned long long* dt_slots, int images, const StepClock* clk) {
  const unsigned m = blockIdx.y;
  const StepClock* rec = clk + m;
  if (rec->stop) return;
  spec_assume<SPEC>(g);
  // NO FUNCTIONAL PURPOSE: 32 bytes of padding.  The single-box kernel carries the scratch of its folded clock (clock_fold: TX * TY / 64
  // doubles), which the ensemble does not need; the store below only keeps the same allocation alive here, so that a workgroup of
  // either kernel takes exactly the same LDS (tests/test_ensemble_resources.py compares the two for equality).  Three workgroups fit
  // a CU with or without it.
  __shared__ double Lfold[TX * TY / 64];
  *(volatile double*)&Lfold[threadIdx.x >> 6] = 0.0;
  hydro2d_step_body<TX, TY, SPEC>(g, nbx, Uin + (size_t)m * stride, Uout + (size_t)m * stride, rec->dtdx, rec->dtdy, dt_slots + m * ENSEMBLE_SLOT_STRIDE, images);
}

template <int SPEC>
__global__ void __launch_bounds__(M2_THREADS, 2) mhd2d_ensemble_kernel(DevParams g, RotCoef rc, int nbx, const double* __restrict__ U, double* __restrict__ Unew, unsigned stride,
                                                                       unsigned long long* dt_slots, int images, const StepClock* clk) {
  const unsigned m = blockIdx.y;
  const StepClock* rec = clk + m;
  if (rec->stop) return;
  spec_assume<SPEC>(g);
  // SPEC_NONE (every solver in one kernel) sits at the limit of the scalar register file: its dt rides in vector registers, of which
  // it has to spare at two workgroups per CU (no scalar register spilled, as in mhd2d_step_kernel<0>)
  const double dt = SPEC == SPEC_NONE ? rg_in_vector(rec->dt) : rec->dt;
  mhd2d_step_body<SPEC>(g, rc, nbx, U + (size_t)m * stride, Unew + (size_t)m * stride, dt, rec->dtdx, rec->dtdy, dt_slots + m * ENSEMBLE_SLOT_STRIDE, images);
}

inline int launch_ensemble_clock(rg_stream_t s, int members, unsigned long long* slots, const ClockConst& k, const EnsembleSpan* span,
                                 const StepClock* prev, StepClock* out) {
  hipLaunchKernelGGL(ensemble_clock_kernel, dim3((unsigned)members), dim3(1024), 0, s, slots, k, span, prev, out);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

template <int TX, int TY, int SPEC>
inline int launch_hydro2d_ensemble(rg_stream_t s, int members, const DevParams& g, const double* in, double* out, unsigned stride, unsigned long long* dt_slots,
                                   int images, const StepClock* clk) {
  const int nbx = (g.isize - 1 + (TX - 2) - 1) / (TX - 2), nby = (g.jsize - 1 + (TY - 2) - 1) / (TY - 2);   // as launch_hydro2d_step
  hipLaunchKernelGGL((hydro2d_ensemble_kernel<TX, TY, SPEC>), dim3((unsigned)(nbx * nby), (unsigned)members), dim3(TX * TY), 0, s, g, nbx, in, out, stride, dt_slots, images, clk);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

// One 2D hydro step of every member: in / out = member 0's arrays, member m's at + m * stride; dt_slots: see the kernels; clk =
// the records of this step's tick (one per member); images != 0 as for hydro2d_step.  The same choice of instantiation as hydro2d_step.
// Returns 0 = done, 1 = not covered, < 0 = launch error.
inline int hydro2d_ensemble_step(rg_stream_t s, int members, const DevParams& g, const double* in, double* out, unsigned stride, unsigned long long* dt_slots,
                                 int images, const StepClock* clk) {
  if (!hydro2d_step_covers(g)) return 1;
  const bool no_spec = !rgpu::options().spec;
  constexpr int TX = 16, TY = 16;
#define RG_TRY(SP) if (spec_matches(SP, g)) return launch_hydro2d_ensemble<TX, TY, SP>(s, members, g, in, out, stride, dt_slots, images, clk);
  if (!no_spec) {   // (no gravity on the device-clock path: the uniform-gravity instantiations of hydro2d_step have no counterpart here)
    const int SL1 = SPEC_SLOPE1 | SPEC_NO_GRAVITY, SL2 = SPEC_SLOPE2 | SPEC_NO_GRAVITY;
    RG_TRY(SPEC_HYDRO_HLLC | SL2) RG_TRY(SPEC_HYDRO_HLLC | SL1)
    RG_TRY(SPEC_HYDRO_APPROX | SL2) RG_TRY(SPEC_HYDRO_APPROX | SL1)
    RG_TRY(SPEC_HYDRO_HLL | SL2) RG_TRY(SPEC_HYDRO_HLL | SL1)
  }
#undef RG_TRY
  return launch_hydro2d_ensemble<TX, TY, SPEC_NONE>(s, members, g, in, out, stride, dt_slots, images, clk);
}

// ... and one 2D MHD step of every member (arguments as above; spec_plain / SPEC_PLAIN as mhd2d_step)
template <int SPEC_PLAIN>
inline int mhd2d_ensemble_step(rg_stream_t s, int members, const DevParams& g, const RotCoef& rc, bool spec_plain, const double* U, double* Unew, unsigned stride,
                               unsigned long long* dt_slots, int images, const StepClock* clk) {
  if (!mhd2d_step_covers(g)) return 1;
  const int nbx = (g.isize - 2 * g.gw + 1 + M2_OX - 1) / M2_OX, nby = (g.jsize - 2 * g.gw + 1 + M2_OY - 1) / M2_OY;   // as mhd2d_step
  const dim3 grid((unsigned)(nbx * nby), (unsigned)members);
  if (spec_plain)
    hipLaunchKernelGGL((mhd2d_ensemble_kernel<SPEC_PLAIN>), grid, dim3(M2_THREADS), 0, s, g, rc, nbx, U, Unew, stride, dt_slots, images, clk);
  else
    hipLaunchKernelGGL((mhd2d_ensemble_kernel<SPEC_NONE>), grid, dim3(M2_THREADS), 0, s, g, rc, nbx, U, Unew, stride, dt_slots, images, clk);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace rgpu_tiled

#include "ensemble_scan.h"   // the same kernels with per-member constants from a device table (parameter scans)
#include "ensemble_monitor.h"   // per-member totals and extrema sampled on the device inside a batch (kernels_monitor.h)
