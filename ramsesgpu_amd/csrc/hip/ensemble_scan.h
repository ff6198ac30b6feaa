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
// at is shared (the host checks every set against it before the table is used).
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
    const ClockConst k = tab[m].k;
    StepClock r;
    step_clock_form(k, mx, prev ? prev[m].t_next : span[m].t0, span[m].tEnd, prev ? prev[m].stop : 0, &r);
    out[m] = r;
    runs = r.stop == 0;
  }
  __syncthreads();
  if (runs) mine[t] = 0ull;
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
  // NO FUNCTIONAL PURPOSE: the 32 bytes of padding of hydro2d_ensemble_kernel, for the same reason (equal LDS per workgroup)
  __shared__ double Lfold[TX * TY / 64];
  *(volatile double*)&Lfold[threadIdx.x >> 6] = 0.0;
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

inline int launch_scan_clock(rg_stream_t s, int members, unsigned long long* slots, const MemberConst* tab, const EnsembleSpan* span,
                             const StepClock* prev, StepClock* out) {
  hipLaunchKernelGGL(scan_clock_kernel, dim3((unsigned)members), dim3(1024), 0, s, slots, tab, span, prev, out);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

template <int TX, int TY, int SPEC>
inline int launch_hydro2d_scan(rg_stream_t s, int members, const DevParams& g, const MemberConst* tab, const double* in, double* out, unsigned stride,
                               unsigned long long* dt_slots, int images, const StepClock* clk) {
  const int nbx = (g.isize - 1 + (TX - 2) - 1) / (TX - 2), nby = (g.jsize - 1 + (TY - 2) - 1) / (TY - 2);   // the shared shape
  hipLaunchKernelGGL((hydro2d_scan_kernel<TX, TY, SPEC>), dim3((unsigned)(nbx * nby), (unsigned)members), dim3(TX * TY), 0, s, tab, nbx, in, out, stride, dt_slots, images, clk);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

// The instantiation a scan over these sets would run: hydro2d_ensemble_step's list, chosen from g (member 0's); 0 = the generic one
inline int hydro2d_scan_spec(const DevParams& g) {
  if (!rgpu::options().spec) return SPEC_NONE;
  const int SL1 = SPEC_SLOPE1 | SPEC_NO_GRAVITY, SL2 = SPEC_SLOPE2 | SPEC_NO_GRAVITY;
  const int list[6] = {SPEC_HYDRO_HLLC | SL2, SPEC_HYDRO_HLLC | SL1, SPEC_HYDRO_APPROX | SL2, SPEC_HYDRO_APPROX | SL1, SPEC_HYDRO_HLL | SL2, SPEC_HYDRO_HLL | SL1};
  for (int sp : list) if (spec_matches(sp, g)) return sp;
  return SPEC_NONE;
}

// One 2D hydro step of every member with member m's constants from tab[m]; g: member 0's (shape and the choice of instantiation:
// `spec`, from hydro2d_scan_spec(g), which the caller has checked against every member's set).  Returns as hydro2d_ensemble_step.
inline int hydro2d_scan_step(rg_stream_t s, int members, const DevParams& g, int spec, const MemberConst* tab, const double* in, double* out, unsigned stride,
                             unsigned long long* dt_slots, int images, const StepClock* clk) {
  if (!hydro2d_step_covers(g)) return 1;
  constexpr int TX = 16, TY = 16;
#define RG_TRY(SP) if (spec == (SP)) return launch_hydro2d_scan<TX, TY, SP>(s, members, g, tab, in, out, stride, dt_slots, images, clk);
  const int SL1 = SPEC_SLOPE1 | SPEC_NO_GRAVITY, SL2 = SPEC_SLOPE2 | SPEC_NO_GRAVITY;
  RG_TRY(SPEC_HYDRO_HLLC | SL2) RG_TRY(SPEC_HYDRO_HLLC | SL1)
  RG_TRY(SPEC_HYDRO_APPROX | SL2) RG_TRY(SPEC_HYDRO_APPROX | SL1)
  RG_TRY(SPEC_HYDRO_HLL | SL2) RG_TRY(SPEC_HYDRO_HLL | SL1)
#undef RG_TRY
  return launch_hydro2d_scan<TX, TY, SPEC_NONE>(s, members, g, tab, in, out, stride, dt_slots, images, clk);
}

// ... and one 2D MHD step of every member (spec_plain / SPEC_PLAIN as mhd2d_ensemble_step)
template <int SPEC_PLAIN>
inline int mhd2d_scan_step(rg_stream_t s, int members, const DevParams& g, bool spec_plain, const MemberConst* tab, const double* U, double* Unew, unsigned stride,
                           unsigned long long* dt_slots, int images, const StepClock* clk) {
  if (!mhd2d_step_covers(g)) return 1;
  const int nbx = (g.isize - 2 * g.gw + 1 + M2_OX - 1) / M2_OX, nby = (g.jsize - 2 * g.gw + 1 + M2_OY - 1) / M2_OY;   // the shared shape
  const dim3 grid((unsigned)(nbx * nby), (unsigned)members);
  if (spec_plain)
    hipLaunchKernelGGL((mhd2d_scan_kernel<SPEC_PLAIN>), grid, dim3(M2_THREADS), 0, s, tab, nbx, U, Unew, stride, dt_slots, images, clk);
  else
    hipLaunchKernelGGL((mhd2d_scan_kernel<SPEC_NONE>), grid, dim3(M2_THREADS), 0, s, tab, nbx, U, Unew, stride, dt_slots, images, clk);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace rgpu_tiled
