// ensemble_scan.h (HIP / gfx950 only; included from ensemble2d.h) -- the ensemble kernels with PER-MEMBER constants: a parameter scan
// (rgpu_ensemble_create_scan, api/entry_ensemble.h) is an ensemble whose members share everything that selects code or shape -- the
// integers of rgpu_params, slope_type, the sign classes of cIso / Omega0 / nu / eta -- and differ in the doubles: gamma0, cfl, cIso,
// the floors, the box extents and with them dx, dy.
//
// The uniform kernels (ensemble2d.h) get DevParams, RotCoef and ClockConst by value, one set for everybody.  Here they sit in a
// table in device memory, one MemberConst per member, indexed by the member and never by its position in a batch; workgroup
// (blockIdx.x, m = blockIdx.y) loads tab[m] -- m is uniform, so these are scalar loads -- and calls the same hydro2d_step_body /
// mhd2d_step_body / step_clock_form: one copy of the numerics, hence the doubles of a lone context created from member m's set.
// The table is written once, before the first fused round, and is never rewritten while work is queued: the scalar data cache is
// not coherent with later stores, so what a kernel can see there has to be immutable.
// The instantiation (SPEC) is chosen once on the host from member 0's set; it holds for all members because what spec_matches looks
// at is shared (the host checks every set against it before the table is used).  Launched by the functions of ensemble2d.h.
#pragma once

namespace rgpu_tiled {

struct MemberConst {
  DevParams g;      // the member's c->g with hdt = hgx = hgy = hgz = 0 (no gravity on this path)
  ClockConst k;     // clock_const(member)
  RotCoef rc;       // rot_coef(member, 0.0)
};

// ensemble_clock_kernel with member m's ClockConst from the table
__global__ void __launch_bounds__(1024) scan_clock_kernel(unsigned long long* __restrict__ slots, const MemberConst* __restrict__ tab,
                                                          const EnsembleSpan* __restrict__ span, const StepClock* prev, StepClock* out) {
  const size_t m = blockIdx.x;
  clock_tick_body(slots + m * ENSEMBLE_SLOT_STRIDE, &tab[m].k, prev ? prev + m : 0, span[m].t0, span[m].tEnd, out + m);
}

// The step kernels: arguments as the ensemble kernels' (ensemble2d.h), `tab` in place of g (and rc).
template <int TX, int TY, int SPEC>
__global__ void __launch_bounds__(TX * TY) hydro2d_scan_kernel(const MemberConst* __restrict__ tab, int nbx, const double* __restrict__ Uin, double* __restrict__ Uout, unsigned stride,
                                                               unsigned long long* dt_slots, int images, const StepClock* clk) {
  const unsigned m = blockIdx.y;
  const StepClock* rec = clk + m;
  if (rec->stop) return;
  const DevParams g = tab[m].g;
  spec_assume<SPEC>(g);
  hydro2d_fold_padding<TX * TY>();
  hydro2d_step_body<TX, TY, SPEC>(g, nbx, Uin + (size_t)m * stride, Uout + (size_t)m * stride, rec->dtdx, rec->dtdy, dt_slots + m * ENSEMBLE_SLOT_STRIDE, images);
}

template <int SPEC>
__global__ void __launch_bounds__(M2_THREADS, 2) mhd2d_scan_kernel(const MemberConst* __restrict__ tab, int nbx, const double* __restrict__ U, double* __restrict__ Unew, unsigned stride,
                                                                   unsigned long long* dt_slots, int images, const StepClock* clk) {
  const unsigned m = blockIdx.y;
  const StepClock* rec = clk + m;
  if (rec->stop) return;
  const DevParams g = tab[m].g;
  RotCoef rc = tab[m].rc;
  spec_assume<SPEC>(g);
  // SPEC_NONE sits at the limit of the scalar register file (ensemble2d.h): dt rides in vector registers as in mhd2d_ensemble_kernel,
  // and so do the four rotating-frame coefficients -- with the constants fetched from memory instead of the kernel arguments the
  // kernel spilled 5 scalar registers without this (the exact build; none with it)
  if (SPEC == SPEC_NONE) { rc.lambda = rg_in_vector(rc.lambda); rc.ratio = rg_in_vector(rc.ratio); rc.alpha1 = rg_in_vector(rc.alpha1); rc.alpha2 = rg_in_vector(rc.alpha2); }
  const double dt = SPEC == SPEC_NONE ? rg_in_vector(rec->dt) : rec->dt;
  mhd2d_step_body<SPEC>(g, rc, nbx, U + (size_t)m * stride, Unew + (size_t)m * stride, dt, rec->dtdx, rec->dtdy, dt_slots + m * ENSEMBLE_SLOT_STRIDE, images);
}

}  // namespace rgpu_tiled
