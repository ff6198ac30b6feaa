// monitor_spectrum.h (HIP / gfx950 only; included from rg_tiled.h) -- the spectrum monitor of a lone 3D context
// (kernels_monitor_spectrum.h) for rgpu_state_spectra and the samples rgpu_run_steps_spectra takes inside its device-clock batches.
// Per transform (two channels, Z = a + i b) three launches, per spec one more:
//
//   monitor_spectrum_x_kernel     a workgroup takes 2^logl consecutive interior rows (j, k) of the state, SPEC_TILE cells: every thread
//                                 forms the two channels of its cells (contiguous loads along i) and stores a + i b into LDS at the
//                                 bit-reversed place of its row; the rows are transformed in LDS and written to Z, contiguous.
//   monitor_spectrum_y_kernel     a tile is one plane kk, 2^logw adjacent ii and every jj: each global access is a run of 2^logw complex
//                                 numbers (16 B each: 8 make a 128-byte line) one row apart, not one element per line stride.  In LDS
//                                 the lines lie innermost, [jj][ii]; transformed in place, written back over Z.
//   monitor_spectrum_z_kernel     the same tile along z (one jj, 2^logw adjacent ii, every kk), not written back: after the transform
//                                 a shell has an owner among the threads -- S shells, the columns of a tile cut into 2^logp parts
//                                 (spec_bin_logp: as many as 1024 threads have owners for), owner part * S + s; more than 1024 shells:
//                                 thread t owns the shells t, t + 1024, ... -- who adds, column after column of its part, the |Z|^2 of
//                                 the range of |kz| that spec_interval gives it, ascending, +kz before -kz.  A workgroup walks a fixed
//                                 run of tiles in ascending order and keeps its sums in registers; at the end it stores them (first
//                                 transform of a spec) or adds them to what it stored for the transform before, as partial sums and
//                                 partial mode counts of its own in scratch, one of each per owner.
//   monitor_spectrum_fold_kernel  the partial sums of shell s in the order workgroup, part: sixteen threads add a sixteenth of them each,
//                                 ascending, SPEC_FOLD_DEPTH loads in flight; one adds the sixteen results, ascending, scales by 1 / N^2
//                                 (a power of two) and STORES P[s] and M[s] to the destination.
//
// The order of every sum is thereby fixed by the box and the spec alone: tiles to workgroups by spec_bin_groups, columns to parts by
// spec_bin_logp, columns ascending, |kz| ascending; then workgroups ascending, parts ascending, in sixteen runs whose sums are added ascending.  The width of the y tile (option "spectrum_tile_y") changes which lines travel together, not
// what is computed on a line: the same doubles.  The z tile has no option, its width is part of the summation order.
//
// LDS: SPEC_TILE complex doubles, one 16-byte slot of padding after every 16 (a power-of-two stride between the lanes of a
// ds_read_b128 group would put them on one bank row: with the padding, elements 16 e apart fall one slot apart), and the n / 2
// twiddle factors of the line length: 139,264 + 8,192 = 147,456 bytes, one workgroup of 1024 threads per CU, four waves per SIMD.  The
// tile is sized by the longest line, 1024 points of 16 bytes, eight of which make a 128-byte line; shorter lines take more of them.
// clk != 0 (inside a batch): the StepClock record of the step the sample follows; a record that says stop ends every workgroup in its
// first instructions, and the log slot stays unwritten -- the host reads the same record and does not look at it.
#pragma once
#include "kernels_monitor_spectrum.h"

namespace rgpu_tiled {

using namespace rgpu_dev;

enum { SPEC_LDS = SPEC_TILE + SPEC_TILE / 16, SPEC_FOLD_DEPTH = 8, SPEC_FOLD_SHELLS = 16, SPEC_FOLD_CHUNKS = 16, SPEC_FOLD_BLOCK = SPEC_FOLD_SHELLS * SPEC_FOLD_CHUNKS, SPEC_OWN = SPEC_MAX_SHELLS / SPEC_BLOCK };

__device__ __forceinline__ unsigned spec_pad(unsigned e) { return e + (e >> 4); }

// the n / 2 factors of a line of 2^logn points out of the table of 1024-point ones
__device__ __forceinline__ void spec_load_twiddles(double2* tws, const double2* __restrict__ tw, int logn) {
  for (unsigned k = threadIdx.x; k < (1u << (logn - 1)); k += SPEC_BLOCK) tws[k] = tw[k << (SPEC_MAX_LOG - logn)];
}

// The 2^logl lines of 2^logn points in `tile`, in bit-reversed order, transformed in place.  ROWS: a line is contiguous, element p of
// line l at (l << logn) + p; else the lines lie innermost, at (p << logl) + l.  One butterfly per thread and turn, a barrier per stage
template <bool ROWS>
__device__ __forceinline__ void spec_tile_fft(double2* tile, const double2* tws, int logn, int logl) {
  const unsigned items = 1u << (logn - 1 + logl);
  for (int st = 0; st < logn; ++st) {
    __syncthreads();
    for (unsigned w = threadIdx.x; w < items; w += SPEC_BLOCK) {
      const unsigned bf = ROWS ? w & ((1u << (logn - 1)) - 1u) : w >> logl;
      const unsigned l = ROWS ? w >> (logn - 1) : w & ((1u << logl) - 1u);
      const unsigned j = bf & ((1u << st) - 1u), p = ((bf >> st) << (st + 1)) + j;
      const unsigned e0 = spec_pad(ROWS ? (l << logn) + p : (p << logl) + l);
      const unsigned e1 = spec_pad(ROWS ? (l << logn) + p + (1u << st) : ((p + (1u << st)) << logl) + l);
      const double2 f = tws[j << (logn - 1 - st)];
      const double2 a = tile[e0], b = tile[e1];
      const double br = b.x * f.x - b.y * f.y, bi = b.x * f.y + b.y * f.x;
      tile[e0] = make_double2(a.x + br, a.y + bi);
      tile[e1] = make_double2(a.x - br, a.y - bi);
    }
  }
  __syncthreads();
}

__global__ void __launch_bounds__(SPEC_BLOCK) monitor_spectrum_x_kernel(DevParams g, SpecBox b, int logl, int ca, int cb, const double* __restrict__ U, const double2* __restrict__ tw,
                                                                         const StepClock* clk, double2* __restrict__ Z) {
  if (!mon_gate_open(clk)) return;
  __shared__ double2 tile[SPEC_LDS];
  __shared__ double2 tws[SPEC_TW];
  spec_load_twiddles(tws, tw, b.lx);
  const unsigned row0 = blockIdx.x << logl, cells = 1u << (b.lx + logl);
  for (unsigned w = threadIdx.x; w < cells; w += SPEC_BLOCK) {
    const unsigned i = w & ((unsigned)b.nx - 1u), l = w >> b.lx;
    double c[SPEC_NQ];
    spec_cell_channels(g, U, spec_row_origin(g, row0 + l) + i, c);
    tile[spec_pad((l << b.lx) + (__brev(i) >> (32 - b.lx)))] = make_double2(spec_pick(c, ca), spec_pick(c, cb));
  }
  spec_tile_fft<true>(tile, tws, b.lx, logl);
  double2* dst = Z + ((size_t)row0 << b.lx);
  for (unsigned w = threadIdx.x; w < cells; w += SPEC_BLOCK) dst[w] = tile[spec_pad(w)];
}

// the element of Z that stands at point p of line x of a y or z tile: axis 1: plane `fix`, row p; axis 2: row `fix` of plane p
__device__ __forceinline__ size_t spec_tile_elem(const SpecBox& b, int axis, unsigned fix, unsigned x0, unsigned p, unsigned x) {
  const size_t row = axis == 1 ? (size_t)fix * (unsigned)b.ny + p : (size_t)p * (unsigned)b.ny + fix;
  return (row << b.lx) + x0 + x;
}
__device__ __forceinline__ void spec_tile_load(double2* tile, const double2* __restrict__ Z, const SpecBox& b, int axis, int logn, int logw, unsigned fix, unsigned x0) {
  for (unsigned w = threadIdx.x; w < (1u << (logn + logw)); w += SPEC_BLOCK) {
    const unsigned x = w & ((1u << logw) - 1u), p = w >> logw;
    tile[spec_pad(((__brev(p) >> (32 - logn)) << logw) + x)] = Z[spec_tile_elem(b, axis, fix, x0, p, x)];
  }
}

__global__ void __launch_bounds__(SPEC_BLOCK) monitor_spectrum_y_kernel(SpecBox b, int logw, const double2* __restrict__ tw, const StepClock* clk, double2* Z) {
  if (!mon_gate_open(clk)) return;
  __shared__ double2 tile[SPEC_LDS];
  __shared__ double2 tws[SPEC_TW];
  spec_load_twiddles(tws, tw, b.ly);
  const unsigned per = (unsigned)b.nx >> logw, kk = blockIdx.x / per, x0 = (blockIdx.x % per) << logw;
  spec_tile_load(tile, Z, b, 1, b.ly, logw, kk, x0);
  spec_tile_fft<false>(tile, tws, b.ly, logw);
  for (unsigned w = threadIdx.x; w < (1u << (b.ly + logw)); w += SPEC_BLOCK) Z[spec_tile_elem(b, 1, kk, x0, w >> logw, w & ((1u << logw) - 1u))] = tile[spec_pad(w)];
}

__global__ void __launch_bounds__(SPEC_BLOCK) monitor_spectrum_z_kernel(SpecBox b, SpecOne S, int logw, int logp, int first, const double2* __restrict__ tw, const StepClock* clk,
                                                                         const double2* __restrict__ Z, double* __restrict__ part) {
  if (!mon_gate_open(clk)) return;
  __shared__ double2 tile[SPEC_LDS];
  __shared__ double2 tws[SPEC_TW];
  spec_load_twiddles(tws, tw, b.lz);
  const unsigned per = (unsigned)b.nx >> logw, tiles = (unsigned)b.ny * per;
  const unsigned t0 = (unsigned)((unsigned long long)blockIdx.x * tiles / gridDim.x), t1 = (unsigned)((blockIdx.x + 1ull) * tiles / gridDim.x);
  // owner k = part * S + s: shell s over the columns [part, part + 1) << (logw - logp) of every tile.  More than one part only where
  // all owners fit one turn (u = 0)
  const unsigned shells = (unsigned)S.shells, owners = shells << logp;
  double* mine = part + (size_t)blockIdx.x * 2 * owners;
  double sum[SPEC_OWN], cnt[SPEC_OWN];
  unsigned own_s[SPEC_OWN], own_x[SPEC_OWN];
#pragma unroll
  for (int u = 0; u < SPEC_OWN; ++u) {
    const unsigned k = threadIdx.x + (unsigned)u * SPEC_BLOCK, p = k < owners ? k / shells : 0u;
    own_s[u] = k - p * shells;
    own_x[u] = p << (logw - logp);
    sum[u] = (!first && k < owners) ? mine[k] : 0.0;
    cnt[u] = 0.0;
  }
  const int hz = b.nz / 2;
  for (unsigned t = t0; t < t1; ++t) {
    const unsigned jj = t / per, x0 = (t % per) << logw;
    if (t != t0) __syncthreads();   // the sums of the tile before have been read
    spec_tile_load(tile, Z, b, 2, b.lz, logw, jj, x0);
    spec_tile_fft<false>(tile, tws, b.lz, logw);
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
          sum[u] = sum[u] + (z.x * z.x + z.y * z.y);
          cnt[u] += 1.0;
          if (m != 0 && m != hz) {
            z = tile[spec_pad(((unsigned)(b.nz - m) << logw) + x)];
            sum[u] = sum[u] + (z.x * z.x + z.y * z.y);
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
    mine[k] = sum[u];
    if (first) mine[owners + k] = cnt[u];
  }
}

// thread (c, l) of a workgroup of SPEC_FOLD_CHUNKS x SPEC_FOLD_SHELLS: shell s = 16 blockIdx.x + l over chunk c of the pieces (piece j: part
// j mod 2^logp of workgroup j >> logp): the pieces [c, c + 1) * pieces / 16, ascending, SPEC_FOLD_DEPTH loads in flight; then thread
// (0, l) adds the sixteen chunk sums in ascending order.  (One thread per shell walking every piece waited for 4096 loads in turn:
// 504 us at 256^3.)
__global__ void __launch_bounds__(SPEC_FOLD_BLOCK) monitor_spectrum_fold_kernel(SpecOne S, unsigned groups, int logp, double scale, const StepClock* clk, const double* __restrict__ part, double* __restrict__ out) {
  if (!mon_gate_open(clk)) return;
  __shared__ double sums[SPEC_FOLD_CHUNKS][SPEC_FOLD_SHELLS], cnts[SPEC_FOLD_CHUNKS][SPEC_FOLD_SHELLS];
  const unsigned l = threadIdx.x % SPEC_FOLD_SHELLS, c = threadIdx.x / SPEC_FOLD_SHELLS;
  const unsigned s = blockIdx.x * SPEC_FOLD_SHELLS + l, shells = (unsigned)S.shells, owners = shells << logp;
  const unsigned pieces = groups << logp;
  const unsigned j_lo = (unsigned)((unsigned long long)c * pieces / SPEC_FOLD_CHUNKS), j_hi = (unsigned)((c + 1ull) * pieces / SPEC_FOLD_CHUNKS);
  double sum = 0.0, cnt = 0.0;
  if (s < shells) {
    for (unsigned j0 = j_lo; j0 < j_hi; j0 += SPEC_FOLD_DEPTH) {
      double x[SPEC_FOLD_DEPTH], n[SPEC_FOLD_DEPTH];
#pragma unroll
      for (int u = 0; u < SPEC_FOLD_DEPTH; ++u) {
        const unsigned j = j0 + (unsigned)u;
        const size_t at = (size_t)(j >> logp) * 2 * owners + (size_t)(j & ((1u << logp) - 1u)) * shells + s;
        x[u] = j < j_hi ? part[at] : 0.0;
        n[u] = j < j_hi ? part[at + owners] : 0.0;
      }
#pragma unroll
      for (int u = 0; u < SPEC_FOLD_DEPTH; ++u) {   // ascending in the workgroup, then in the part; the padding zeros at the end add nothing to a sum >= 0
        sum = sum + x[u];
        cnt = cnt + n[u];
      }
    }
  }
  sums[c][l] = sum;
  cnts[c][l] = cnt;
  __syncthreads();
  if (c != 0 || s >= shells) return;
  sum = 0.0;
  cnt = 0.0;
  for (int k = 0; k < SPEC_FOLD_CHUNKS; ++k) {
    sum = sum + sums[k][l];
    cnt = cnt + cnts[k][l];
  }
  out[S.base + s] = sum * scale;
  out[S.base + shells + s] = cnt;
}

// log2 of the width of the y tile: the option where it is 0 .. SPEC_TILE_MAX_LOGW (clamped to what the box and the tile hold), else
// the widest that fits
inline int spec_y_logw(const SpecBox& b, int option) {
  const int fit = spec_tile_logw(spec_tile_log(), b.ly, b.lx);
  return option >= 0 && option < fit ? option : fit;
}

// The launches of one sample of U into out[S.doubles]; scratch: spec_scratch_doubles
inline int launch_monitor_spectrum(rg_stream_t st, const DevParams& g, const SpecSet& set, int y_logw_option, const double* U, const double* tw, const StepClock* clk,
                                   double* scratch, double* out) {
  const SpecBox b = spec_box(g);
  const size_t N = (size_t)b.nx * b.ny * b.nz;
  double2* Z = reinterpret_cast<double2*>(scratch);
  double* part = scratch + 2 * N;
  const double2* tw2 = reinterpret_cast<const double2*>(tw);
  const int xl = spec_tile_logw(spec_tile_log(), b.lx, b.ly + b.lz);
  const int yw = spec_y_logw(b, y_logw_option), zw = spec_tile_logw(spec_tile_log(), b.lz, b.lx);
  const unsigned groups = spec_bin_groups(b);
  const double scale = 1.0 / ((double)N * (double)N);
  for (int m = 0; m < set.n; ++m) {
    int ca[SPEC_NQ], cb[SPEC_NQ];
    const int nt = spec_pairs(set.s[m].channels, ca, cb);
    for (int t = 0; t < nt; ++t) {
      hipLaunchKernelGGL(monitor_spectrum_x_kernel, dim3((unsigned)(b.ny * b.nz) >> xl), dim3(SPEC_BLOCK), 0, st, g, b, xl, ca[t], cb[t], U, tw2, clk, Z);
      hipLaunchKernelGGL(monitor_spectrum_y_kernel, dim3((unsigned)b.nz * ((unsigned)b.nx >> yw)), dim3(SPEC_BLOCK), 0, st, b, yw, tw2, clk, Z);
      hipLaunchKernelGGL(monitor_spectrum_z_kernel, dim3(groups), dim3(SPEC_BLOCK), 0, st, b, set.s[m], zw, spec_bin_logp(b, (unsigned)set.s[m].shells), t == 0 ? 1 : 0, tw2, clk, (const double2*)Z, part);
      if (hipGetLastError() != hipSuccess) return -1;
    }
    hipLaunchKernelGGL(monitor_spectrum_fold_kernel, dim3(((unsigned)set.s[m].shells + SPEC_FOLD_SHELLS - 1) / SPEC_FOLD_SHELLS), dim3(SPEC_FOLD_BLOCK), 0, st, set.s[m], groups, spec_bin_logp(b, (unsigned)set.s[m].shells), scale,
                                      clk, (const double*)part, out);
    if (hipGetLastError() != hipSuccess) return -1;
  }
  return 0;
}

}  // namespace rgpu_tiled
