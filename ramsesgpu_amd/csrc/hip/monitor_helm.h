// monitor_helm.h (HIP / gfx950 only; included from rg_tiled.h) -- the Helmholtz spectra of a lone 3D context (kernels_monitor_helm.h)
// for rgpu_state_helm_spectra and the samples rgpu_run_steps_helm_spectra takes inside its device-clock batches.  Per spec nine launches:
//
//   monitor_spectrum_x_kernel, monitor_spectrum_y_kernel   (hip/monitor_spectrum.h, as they are) once per component c of the field, with
//                                 cb = -1: the component with imaginary part zero, transformed along x and y into Z_c.  Six launches.
//   monitor_helm_z_kernel         the y kernel's tile along z (one jj, 2^logw adjacent ii, every kk) of Z0 (blockIdx.y = 0) and of Z1
//                                 (blockIdx.y = 1): loaded, transformed in LDS, written back in place.
//   monitor_helm_bin_kernel       the tile walk of monitor_spectrum_z_kernel over Z2, which is transformed in LDS and not written back.
//                                 Then every thread takes the elements w = tid + 1024 t of the tile, reads u^x and u^y of the same mode
//                                 from Z0 and Z1 (runs of 2^logw complex numbers, as the tile load), forms kappa from the tile's jj,
//                                 x0 + x and p, calls helm_mode and overwrites the slot with (T, L): two doubles in the place of a
//                                 complex number, the LDS does not grow.  After a barrier the owners of monitor_spectrum_z_kernel -- the
//                                 same shells, parts, columns and |kz| order, +kz before -kz -- add .x into their solenoidal and .y into
//                                 their compressive sum and count.  At its end a workgroup stores three partials per owner.
//   monitor_helm_fold_kernel      the fold of monitor_spectrum_fold_kernel with three outputs: sixteen ordered runs over the pieces,
//                                 their sums added ascending, scaled by 1 / N^2, STORED as Psol[s], Pcomp[s] and M[s].
//
// The order of every sum is that of the spectrum monitor, fixed by the box and the spec -- and, where the flux array has no room for the
// partials of all its workgroups, by the fewer the binning pass then runs with (helm_bin_groups); option "spectrum_tile_y" changes which
// lines travel together in the y pass, not what is computed on a line.  LDS of the z and bin kernels: the 147,456 bytes of the spectrum
// monitor's passes, one workgroup of 1024 threads per CU.  clk: as there.
#pragma once
#include "kernels_monitor_helm.h"
#include "monitor_spectrum.h"

namespace rgpu_tiled {

using namespace rgpu_dev;

__global__ void __launch_bounds__(SPEC_BLOCK) monitor_helm_z_kernel(SpecBox b, int logw, unsigned long long stride, const double2* __restrict__ tw, const StepClock* clk, double2* Zs) {
  if (!mon_gate_open(clk)) return;
  __shared__ double2 tile[SPEC_LDS];
  __shared__ double2 tws[SPEC_TW];
  spec_load_twiddles(tws, tw, b.lz);
  double2* Z = Zs + (size_t)blockIdx.y * stride;
  const unsigned per = (unsigned)b.nx >> logw, jj = blockIdx.x / per, x0 = (blockIdx.x % per) << logw;
  spec_tile_load(tile, Z, b, 2, b.lz, logw, jj, x0);
  spec_tile_fft<false>(tile, tws, b.lz, logw);
  for (unsigned w = threadIdx.x; w < (1u << (b.lz + logw)); w += SPEC_BLOCK) Z[spec_tile_elem(b, 2, jj, x0, w >> logw, w & ((1u << logw) - 1u))] = tile[spec_pad(w)];
}

__global__ void __launch_bounds__(SPEC_BLOCK) monitor_helm_bin_kernel(SpecBox b, HelmOne S, int logw, int logp, const double2* __restrict__ tw, const StepClock* clk,
                                                                       const double2* __restrict__ Z0, const double2* __restrict__ Z1, const double2* __restrict__ Z2, double* __restrict__ part) {
  if (!mon_gate_open(clk)) return;
  __shared__ double2 tile[SPEC_LDS];
  __shared__ double2 tws[SPEC_TW];
  spec_load_twiddles(tws, tw, b.lz);
  const unsigned per = (unsigned)b.nx >> logw, tiles = (unsigned)b.ny * per;
  const unsigned t0 = (unsigned)((unsigned long long)blockIdx.x * tiles / gridDim.x), t1 = (unsigned)((blockIdx.x + 1ull) * tiles / gridDim.x);
  // owner k = part * S + s, as in monitor_spectrum_z_kernel
  const unsigned shells = (unsigned)S.shells, owners = shells << logp;
  double* mine = part + (size_t)blockIdx.x * 3 * owners;
  double sol[SPEC_OWN], comp[SPEC_OWN], cnt[SPEC_OWN];
  unsigned own_s[SPEC_OWN], own_x[SPEC_OWN];
#pragma unroll
  for (int u = 0; u < SPEC_OWN; ++u) {
    const unsigned k = threadIdx.x + (unsigned)u * SPEC_BLOCK, p = k < owners ? k / shells : 0u;
    own_s[u] = k - p * shells;
    own_x[u] = p << (logw - logp);
    sol[u] = 0.0;
    comp[u] = 0.0;
    cnt[u] = 0.0;
  }
  const int hz = b.nz / 2;
  for (unsigned t = t0; t < t1; ++t) {
    const unsigned jj = t / per, x0 = (t % per) << logw;
    if (t != t0) __syncthreads();   // the parts of the tile before have been read
    spec_tile_load(tile, Z2, b, 2, b.lz, logw, jj, x0);
    spec_tile_fft<false>(tile, tws, b.lz, logw);
    // the projection, mode by mode: a thread reads and writes only the slots it owns here
    const double ky = (double)(S.wy * helm_signed(jj, (unsigned)b.ny));
    for (unsigned w = threadIdx.x; w < (1u << (b.lz + logw)); w += SPEC_BLOCK) {
      const unsigned x = w & ((1u << logw) - 1u), p = w >> logw;
      const size_t e = spec_tile_elem(b, 2, jj, x0, p, x);
      const double2 zx = Z0[e], zy = Z1[e], zz = tile[spec_pad(w)];
      const double ux[2] = {zx.x, zx.y}, uy[2] = {zy.x, zy.y}, uz[2] = {zz.x, zz.y};
      const double kx = (double)(S.wx * helm_signed(x0 + x, (unsigned)b.nx)), kz = (double)(S.wz * helm_signed(p, (unsigned)b.nz));
      double T, L;
      helm_mode(kx, ky, kz, ux, uy, uz, (kx * kx + ky * ky) + kz * kz, &T, &L);   // (integers below 2^25: the sum is exact)
      tile[spec_pad(w)] = make_double2(T, L);
    }
    __syncthreads();
    const unsigned ay = (unsigned)S.wy * spec_fold(jj, (unsigned)b.ny);
#pragma unroll
    for (int u = 0; u < SPEC_OWN; ++u) {
      if (threadIdx.x + (unsigned)u * SPEC_BLOCK >= owners) continue;
      const unsigned s = own_s[u];
      for (unsigned x = own_x[u]; x < own_x[u] + (1u << (logw - logp)); ++x) {
        const unsigned ax = (unsigned)S.wx * spec_fold(x0 + x, (unsigned)b.nx);
        int lo, hi;
        spec_interval(ax * ax + ay * ay, (unsigned)S.wz, hz, s, &lo, &hi);
        for (int m = lo; m <= hi; ++m) {
          double2 z = tile[spec_pad(((unsigned)m << logw) + x)];
          sol[u] = sol[u] + z.x;
          comp[u] = comp[u] + z.y;
          cnt[u] += 1.0;
          if (m != 0 && m != hz) {
            z = tile[spec_pad(((unsigned)(b.nz - m) << logw) + x)];
            sol[u] = sol[u] + z.x;
            comp[u] = comp[u] + z.y;
            cnt[u] += 1.0;
          }
        }
      }
    }
  }
#pragma unroll
  for (int u = 0; u < SPEC_OWN; ++u) {
    const unsigned k = threadIdx.x + (unsigned)u * SPEC_BLOCK;
    if (k >= owners) continue;
    mine[k] = sol[u];
    mine[owners + k] = comp[u];
    mine[2 * owners + k] = cnt[u];
  }
}

// thread (c, l) as in monitor_spectrum_fold_kernel: shell s = 16 blockIdx.x + l over chunk c of the pieces, ascending, SPEC_FOLD_DEPTH
// loads of each of the three partials in flight; then thread (0, l) adds the sixteen chunk sums in ascending order and stores
__global__ void __launch_bounds__(SPEC_FOLD_BLOCK) monitor_helm_fold_kernel(HelmOne S, unsigned groups, int logp, double scale, const StepClock* clk, const double* __restrict__ part, double* __restrict__ out) {
  if (!mon_gate_open(clk)) return;
  __shared__ double sols[SPEC_FOLD_CHUNKS][SPEC_FOLD_SHELLS], comps[SPEC_FOLD_CHUNKS][SPEC_FOLD_SHELLS], cnts[SPEC_FOLD_CHUNKS][SPEC_FOLD_SHELLS];
  const unsigned l = threadIdx.x % SPEC_FOLD_SHELLS, c = threadIdx.x / SPEC_FOLD_SHELLS;
  const unsigned s = blockIdx.x * SPEC_FOLD_SHELLS + l, shells = (unsigned)S.shells, owners = shells << logp;
  const unsigned pieces = groups << logp;
  const unsigned j_lo = (unsigned)((unsigned long long)c * pieces / SPEC_FOLD_CHUNKS), j_hi = (unsigned)((c + 1ull) * pieces / SPEC_FOLD_CHUNKS);
  double sol = 0.0, comp = 0.0, cnt = 0.0;
  if (s < shells) {
    for (unsigned j0 = j_lo; j0 < j_hi; j0 += SPEC_FOLD_DEPTH) {
      double x[SPEC_FOLD_DEPTH], y[SPEC_FOLD_DEPTH], n[SPEC_FOLD_DEPTH];
#pragma unroll
      for (int u = 0; u < SPEC_FOLD_DEPTH; ++u) {
        const unsigned j = j0 + (unsigned)u;
        const size_t at = (size_t)(j >> logp) * 3 * owners + (size_t)(j & ((1u << logp) - 1u)) * shells + s;
        x[u] = j < j_hi ? part[at] : 0.0;
        y[u] = j < j_hi ? part[at + owners] : 0.0;
        n[u] = j < j_hi ? part[at + 2 * (size_t)owners] : 0.0;
      }
#pragma unroll
      for (int u = 0; u < SPEC_FOLD_DEPTH; ++u) {   // ascending in the workgroup, then in the part; the padding zeros at the end add nothing to a sum >= 0
        sol = sol + x[u];
        comp = comp + y[u];
        cnt = cnt + n[u];
      }
    }
  }
  sols[c][l] = sol;
  comps[c][l] = comp;
  cnts[c][l] = cnt;
  __syncthreads();
  if (c != 0 || s >= shells) return;
  sol = 0.0;
  comp = 0.0;
  cnt = 0.0;
  for (int k = 0; k < SPEC_FOLD_CHUNKS; ++k) {
    sol = sol + sols[k][l];
    comp = comp + comps[k][l];
    cnt = cnt + cnts[k][l];
  }
  out[S.base + s] = sol * scale;
  out[S.base + shells + s] = comp * scale;
  out[S.base + 2 * shells + s] = cnt;
}

// The launches of one sample of U into out[S.doubles]; scratch: helm_scratch_doubles of each spec with its set.groups[m]
inline int launch_monitor_helm(rg_stream_t st, const DevParams& g, const HelmSet& set, int y_logw_option, const double* U, const double* tw, const StepClock* clk,
                               double* scratch, double* out) {
  const SpecBox b = spec_box(g);
  const size_t N = (size_t)b.nx * b.ny * b.nz;
  double2* Z = reinterpret_cast<double2*>(scratch);
  double* part = scratch + 6 * N;
  const double2* tw2 = reinterpret_cast<const double2*>(tw);
  const int xl = spec_tile_logw(spec_tile_log(), b.lx, b.ly + b.lz);
  const int yw = spec_y_logw(b, y_logw_option), zw = spec_tile_logw(spec_tile_log(), b.lz, b.lx);
  const unsigned ztiles = (unsigned)b.ny * ((unsigned)b.nx >> zw);
  const double scale = 1.0 / ((double)N * (double)N);
  for (int m = 0; m < set.n; ++m) {
    const HelmOne& S = set.s[m];
    const int logp = spec_bin_logp(b, (unsigned)S.shells);
    const unsigned groups = set.groups[m];
    for (int c = 0; c < 3; ++c) {
      hipLaunchKernelGGL(monitor_spectrum_x_kernel, dim3((unsigned)(b.ny * b.nz) >> xl), dim3(SPEC_BLOCK), 0, st, g, b, xl, helm_first_channel(S.field) + c, -1, U, tw2, clk, Z + c * N);
      hipLaunchKernelGGL(monitor_spectrum_y_kernel, dim3((unsigned)b.nz * ((unsigned)b.nx >> yw)), dim3(SPEC_BLOCK), 0, st, b, yw, tw2, clk, Z + c * N);
      if (hipGetLastError() != hipSuccess) return -1;
    }
    hipLaunchKernelGGL(monitor_helm_z_kernel, dim3(ztiles, 2), dim3(SPEC_BLOCK), 0, st, b, zw, (unsigned long long)N, tw2, clk, Z);
    hipLaunchKernelGGL(monitor_helm_bin_kernel, dim3(groups), dim3(SPEC_BLOCK), 0, st, b, S, zw, logp, tw2, clk, (const double2*)Z, (const double2*)(Z + N), (const double2*)(Z + 2 * N), part);
    hipLaunchKernelGGL(monitor_helm_fold_kernel, dim3(((unsigned)S.shells + SPEC_FOLD_SHELLS - 1) / SPEC_FOLD_SHELLS), dim3(SPEC_FOLD_BLOCK), 0, st, S, groups, logp, scale, clk, (const double*)part, out);
    if (hipGetLastError() != hipSuccess) return -1;
  }
  return 0;
}

}  // namespace rgpu_tiled
