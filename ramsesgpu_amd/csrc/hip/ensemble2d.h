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
// ensemble_clock_kernel is step_clock_kernel with one workgroup per member: the same clock_tick_body (step_clock.h) -- one launch per
// step for all members.  Records are laid out tick-major (record of tick n, member m at [n * members + m]) so that the host reads the
// records of a batch back in one contiguous copy.
// ensemble_scan.h (included below the kernels): the same three kernels with DevParams / RotCoef / ClockConst per member, read from a
// table in device memory instead of the kernel arguments -- a parameter scan.  The launch functions at the end serve both (`tab`).
// ensemble_monitor.h (after them): the monitor of kernels_monitor.h with the member as the second grid dimension.
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
  const size_t m = blockIdx.x;
  clock_tick_body(slots + m * ENSEMBLE_SLOT_STRIDE, &k, prev ? prev + m : 0, span[m].t0, span[m].tEnd, out + m);
}

// The step kernels.  in / out: member 0's arrays, member m's at + m * stride doubles (stride < 2^32: rgpu_ensemble_create checks);
// dt_slots: member 0's slot array, member m's 3 * RG_DT_SLOTS further (the three rotating arrays of a context, rgpu_ctx::d_red_base);
// clk: the records of this step's tick, one per member.  The record of member m is read here (uniform loads) and handed to the body by
// value, as the single-box kernel hands on its arguments.

// a double kept in vector registers from here on (the opposite of rg_uniform, step_clock.h)
__device__ __forceinline__ double rg_in_vector(double x) { asm volatile("" : "+v"(x)); return x; }

// NO FUNCTIONAL PURPOSE: 32 bytes of LDS padding in the hydro kernels of an ensemble.  The single-box kernel carries the scratch of its
// folded clock (clock_fold: TX * TY / 64 doubles), which the ensemble does not need; the store only keeps the same allocation alive
// here, so that a workgroup of either kernel takes exactly the same LDS (tests/test_ensemble_resources.py compares the two for
// equality).  Three workgroups fit a CU with or without it.
template <int NT> __device__ __forceinline__ void hydro2d_fold_padding() {
  __shared__ double Lfold[NT / 64];
  *(volatile double*)&Lfold[threadIdx.x >> 6] = 0.0;
}

template <int TX, int TY, int SPEC>
__global__ void __launch_bounds__(TX * TY) hydro2d_ensemble_kernel(DevParams g, int nbx, const double* __restrict__ Uin, double* __restrict__ Uout, unsigned stride,
                                                                   unsigned long long* dt_slots, int images, const StepClock* clk) {
  const unsigned m = blockIdx.y;
  const StepClock* rec = clk + m;
  if (rec->stop) return;
  spec_assume<SPEC>(g);
  hydro2d_fold_padding<TX * TY>();
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

}  // namespace rgpu_tiled

#include "ensemble_scan.h"   // MemberConst and the same kernels with per-member constants from a device table (parameter scans)

namespace rgpu_tiled {

// The launches: one entry per operation for all members.  tab == 0: the constants passed here (k; g; g and rc), by value, for
// everybody; otherwise member m's from tab[m] (g still gives the shared shape, and with it the grid).
inline int launch_ensemble_clock(rg_stream_t s, int members, unsigned long long* slots, const ClockConst& k, const MemberConst* tab, const EnsembleSpan* span,
                                 const StepClock* prev, StepClock* out) {
  if (tab) hipLaunchKernelGGL(scan_clock_kernel, dim3((unsigned)members), dim3(1024), 0, s, slots, tab, span, prev, out);
  else hipLaunchKernelGGL(ensemble_clock_kernel, dim3((unsigned)members), dim3(1024), 0, s, slots, k, span, prev, out);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

// One 2D hydro step of every member: in / out = member 0's arrays, member m's at + m * stride; dt_slots: see the kernels; clk =
// the records of this step's tick (one per member); images != 0 as for hydro2d_step.  spec: hydro_pick_spec<false>(g) -- the list of
// hydro2d_step without its uniform-gravity entries (no gravity on the device-clock path) -- which, with a table, the caller has
// checked against every member's set.  Returns 0 = done, 1 = not covered, < 0 = launch error.
inline int hydro2d_ensemble_step(rg_stream_t s, int members, const DevParams& g, int spec, const MemberConst* tab, const double* in, double* out, unsigned stride,
                                 unsigned long long* dt_slots, int images, const StepClock* clk) {
  if (!hydro2d_step_covers(g)) return 1;
  int nbx;
  const dim3 grid((unsigned)hydro2d_tiles(g, &nbx), (unsigned)members), block(H2_TX * H2_TY);
  return hydro_spec_dispatch<false>(spec, [&](auto tag) {
    constexpr int SP = decltype(tag)::value;
    if (tab) hipLaunchKernelGGL((hydro2d_scan_kernel<H2_TX, H2_TY, SP>), grid, block, 0, s, tab, nbx, in, out, stride, dt_slots, images, clk);
    else hipLaunchKernelGGL((hydro2d_ensemble_kernel<H2_TX, H2_TY, SP>), grid, block, 0, s, g, nbx, in, out, stride, dt_slots, images, clk);
    return hipGetLastError() == hipSuccess ? 0 : -1;
  });
}

// ... and one 2D MHD step of every member (arguments as above; spec_plain / SPEC_PLAIN as mhd2d_step)
template <int SPEC_PLAIN>
inline int mhd2d_ensemble_step(rg_stream_t s, int members, const DevParams& g, const RotCoef& rc, bool spec_plain, const MemberConst* tab, const double* U, double* Unew,
                               unsigned stride, unsigned long long* dt_slots, int images, const StepClock* clk) {
  if (!mhd2d_step_covers(g)) return 1;
  int nbx;
  const dim3 grid((unsigned)mhd2d_tiles(g, &nbx), (unsigned)members), block(M2_THREADS);
  if (tab && spec_plain) hipLaunchKernelGGL((mhd2d_scan_kernel<SPEC_PLAIN>), grid, block, 0, s, tab, nbx, U, Unew, stride, dt_slots, images, clk);
  else if (tab) hipLaunchKernelGGL((mhd2d_scan_kernel<SPEC_NONE>), grid, block, 0, s, tab, nbx, U, Unew, stride, dt_slots, images, clk);
  else if (spec_plain) hipLaunchKernelGGL((mhd2d_ensemble_kernel<SPEC_PLAIN>), grid, block, 0, s, g, rc, nbx, U, Unew, stride, dt_slots, images, clk);
  else hipLaunchKernelGGL((mhd2d_ensemble_kernel<SPEC_NONE>), grid, block, 0, s, g, rc, nbx, U, Unew, stride, dt_slots, images, clk);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace rgpu_tiled

#include "ensemble_monitor.h"   // per-member totals and extrema sampled on the device inside a batch (kernels_monitor.h)
