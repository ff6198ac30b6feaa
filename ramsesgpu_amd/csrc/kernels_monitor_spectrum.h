// kernels_monitor_spectrum.h -- the spectrum monitor (rgpu_state_spectra, rgpu_run_steps_spectra; include/rgpu.h, "spectrum monitors"):
// shell-binned power spectra of the interior cells of a 3D state U[parity], the box taken as periodic -- E(k) of a turbulent box, the
// magnetic spectrum of an MRI run, the one-dimensional spectra along an axis.
//
// Nothing of the per-cell arithmetic is restated here.  rho, mx my mz and bx by bz of a cell are terms 0, 1 2 3 and 10 11 12 of
// monp_cell_terms (kernels_monitor_planes.h); v = m / rho and w = m / sqrt(rho) are formed from them with rg_recip / rg_div / rg_sqrt.
//
// The shell of a mode is an integer rule (spec_shell): q = (wx kx)^2 + (wy ky)^2 + (wz kz)^2 with the folded integer wave numbers, shell
// s the s >= 0 with s^2 - s + 1 <= q <= s^2 + s, found with an integer square root and two comparisons.  Every kernel bins by the
// inverse of that rule (spec_interval): along z the shell does not decrease with |kz|, so the |kz| of one column (kx, ky) that fall into
// shell s are a range, and an owner of shell s adds them in ascending |kz|, +kz before -kz, column after column.  No sum is ever
// added to by two threads: no atomics, the order is fixed.
//
// The transform: three passes of radix-2 decimation-in-time line transforms, x then y then z, input in bit-reversed order, twiddle
// factors from ONE table of SPEC_TW entries computed on the host (spec_twiddle_table), entry k = exp(-2 pi i k / 1024); a line of n
// points reads every (1024 / n)-th entry.  Two real channels a, b share a transform as Z = a + i b: every shell is symmetric under
// k -> -k, so the shell sums of |Z^|^2 are those of |a^|^2 + |b^|^2.
//
// Shared by the flat functors below (the test-only host emulation and any backend without kernels of its own) and by the gfx950
// kernels of hip/monitor_spectrum.h.  A header of its own: nothing the other kernels include changes.
#pragma once
#include "kernels_monitor_planes.h"

namespace rgpu_dev {

enum { SPEC_NQ = 13, SPEC_MAX = 4, SPEC_MAX_SHELLS = 4096, SPEC_MAX_WEIGHT = 64, SPEC_MIN_LOG = 2, SPEC_MAX_LOG = 10, SPEC_TW = 1 << (SPEC_MAX_LOG - 1) };
// what the gfx950 kernels are sized by (hip/monitor_spectrum.h); here because the scratch they need is worked out on the host:
// complex elements of a tile in LDS, the widest tile in lines, and the workgroups of the binning pass
enum { SPEC_TILE = 8192, SPEC_TILE_MAX_LOGW = 6, SPEC_GROUPS = 1024, SPEC_BLOCK = 1024 };

// one spec as the kernels read it: the caller's rgpu_spectrum_spec, its shells on this box, and where its 2 S doubles begin in a sample
struct SpecOne {
  unsigned channels;
  int wx, wy, wz;
  int shells;
  unsigned base;
};
// the specs of a call (a kernel argument of the launch routines, by value): `doubles` is the sum of 2 S over the specs
struct SpecSet {
  int n;
  unsigned doubles;
  SpecOne s[SPEC_MAX];
};
// the box as the transforms see it: the extents and their logarithms
struct SpecBox {
  int nx, ny, nz, lx, ly, lz;
};

// log2 n for n a power of two in 4 .. 1024, else -1
RG_MON_FN int spec_log2(int n) {
  for (int l = SPEC_MIN_LOG; l <= SPEC_MAX_LOG; ++l)
    if (n == (1 << l)) return l;
  return -1;
}
RG_MON_FN SpecBox spec_box(const DevParams& g) {
  SpecBox b = {g.nx, g.ny, g.nz, spec_log2(g.nx), spec_log2(g.ny), spec_log2(g.nz)};
  return b;
}

// the integer square root, floor(sqrt(x)): bit by bit, no floating point
RG_MON_FN unsigned spec_isqrt(unsigned long long x) {
  unsigned long long r = 0;
  for (unsigned long long b = 1ull << 62; b; b >>= 2) {
    if (x >= r + b) { x -= r + b; r = (r >> 1) + b; }
    else r >>= 1;
  }
  return (unsigned)r;
}
// The rule: the shell of q.  r = floor(sqrt(q)): r^2 <= q < (r + 1)^2, and q belongs to shell r if q <= r^2 + r, else to shell r + 1
// (whose lower edge (r + 1)^2 - (r + 1) + 1 = r^2 + r + 1 follows at once)
RG_MON_FN unsigned spec_shell(unsigned long long q) {
  const unsigned long long r = spec_isqrt(q);
  return (unsigned)(q <= r * r + r ? r : r + 1);
}
// the folded wave number of index i on an axis of n points, as its absolute value: 0 .. n / 2
RG_MON_FN unsigned spec_fold(unsigned i, unsigned n) { return i <= n / 2 ? i : n - i; }
// the shells of weights (wx, wy, wz) on box b: the shell of the corner mode, plus one.  (64-bit: called before the limits are checked)
RG_MON_FN unsigned long long spec_shell_count(const SpecBox& b, int wx, int wy, int wz) {
  const unsigned long long ax = (unsigned long long)wx * (unsigned)(b.nx / 2), ay = (unsigned long long)wy * (unsigned)(b.ny / 2), az = (unsigned long long)wz * (unsigned)(b.nz / 2);
  return (unsigned long long)spec_shell(ax * ax + ay * ay + az * az) + 1;
}
// The inverse of the rule along z: the |kz| = m in 0 .. hz for which qxy + (wz m)^2 lies in shell s are lo .. hi (none: hi < lo).
// With d = s^2 - s + 1 - qxy > 0 the least m has (wz m)^2 >= d, that is wz m > isqrt(d - 1); the greatest has wz m <= isqrt(s^2 + s - qxy).
// q stays below 2^25 (SPEC_MAX_SHELLS shells): 32-bit arithmetic
RG_MON_FN unsigned spec_isqrt32(unsigned x) {
#if defined(__HIP_DEVICE_COMPILE__)
  // the same integer, found from a rounded guess: the two loops leave r^2 <= x < (r + 1)^2 whatever the guess was
  unsigned r = (unsigned)__builtin_sqrtf((float)x);
  while (r * r > x) --r;
  while ((r + 1) * (r + 1) <= x) ++r;
  return r;
#else
  return spec_isqrt(x);
#endif
}
// h / w for h < 2^13 and 1 <= w <= SPEC_MAX_WEIGHT, exactly
RG_MON_FN unsigned spec_div(unsigned h, unsigned w) {
#if defined(__HIP_DEVICE_COMPILE__)
  // the same integer, found from a rounded guess: one step either way puts it right (the integer division costs thirty instructions)
  unsigned q = (unsigned)((float)h * __builtin_amdgcn_rcpf((float)w));
  if (q * w > h) --q;
  else if ((q + 1) * w <= h) ++q;
  return q;
#else
  return h / w;
#endif
}
RG_MON_FN void spec_interval(unsigned qxy, unsigned wz, int hz, unsigned s, int* lo, int* hi) {
  const unsigned top = s * s + s, bot = s ? s * s - s + 1 : 0u;
  *lo = 0;
  *hi = -1;
  if (qxy > top) return;
  if (wz == 0) {
    if (qxy >= bot) *hi = hz;
    return;
  }
  const int h = (int)spec_div(spec_isqrt32(top - qxy), wz);
  *hi = h < hz ? h : hz;
  if (qxy < bot) *lo = (int)spec_div(spec_isqrt32(bot - qxy - 1), wz) + 1;
}

// The pairs of channels that share a transform: the channels of the mask in ascending order, two at a time, an odd last one with -1
// (zero).  Returns the number of transforms
RG_MON_FN int spec_pairs(unsigned channels, int* ca, int* cb) {
  int n = 0, open = 0;
  for (int q = 0; q < SPEC_NQ; ++q) {
    if (!(channels >> q & 1u)) continue;
    if (open) { cb[n++] = q; open = 0; }
    else { ca[n] = q; cb[n] = -1; open = 1; }
  }
  return n + open;
}

// The twiddle table: tw[2 k], tw[2 k + 1] = cos, -sin of 2 pi k / 1024, k < SPEC_TW.  Computed once per context on the host, in long
// double and rounded: the same doubles in both libraries and in the emulation
inline void spec_twiddle_table(double* tw) {
  const long double two_pi = 6.283185307179586476925286766559005768L;
  for (int k = 0; k < SPEC_TW; ++k) {
    const long double a = two_pi * (long double)k / (long double)(2 * SPEC_TW);
    tw[2 * k] = (double)cosl(a);
    tw[2 * k + 1] = (double)-sinl(a);
  }
  tw[0] = 1.0; tw[1] = -0.0;
  tw[SPEC_TW] = 0.0; tw[SPEC_TW + 1] = -1.0;   // k = 256: exactly -i
}

// the thirteen channels of the cell at flat index o of a 3D state: rho mx my mz vx vy vz wx wy wz bx by bz
RG_DEVFN void spec_cell_channels(const DevParams& g, const double* __restrict__ U, unsigned o, double* c) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  double t[MONP_NQ];
  monp_cell_terms(g, U, o, t);
  const rg_recip_t inv_r = rg_recip(t[0]), inv_s = rg_recip(rg_sqrt(t[0]));
  c[0] = t[0]; c[1] = t[1]; c[2] = t[2]; c[3] = t[3];
  c[4] = rg_div(t[1], inv_r); c[5] = rg_div(t[2], inv_r); c[6] = rg_div(t[3], inv_r);
  c[7] = rg_div(t[1], inv_s); c[8] = rg_div(t[2], inv_s); c[9] = rg_div(t[3], inv_s);
  c[10] = t[10]; c[11] = t[11]; c[12] = t[12];
}
// channel ch of c, +0.0 for ch < 0: a chain of selects on a uniform index, so that c stays in registers
RG_DEVFN double spec_pick(const double* c, int ch) {
  static_assert(SPEC_NQ == 13, "the chain names every channel");
  const double c0 = c[0], c1 = c[1], c2 = c[2], c3 = c[3], c4 = c[4], c5 = c[5], c6 = c[6], c7 = c[7], c8 = c[8], c9 = c[9], c10 = c[10], c11 = c[11], c12 = c[12];
  double x = 0.0;
  x = ch == 0 ? c0 : x; x = ch == 1 ? c1 : x; x = ch == 2 ? c2 : x; x = ch == 3 ? c3 : x; x = ch == 4 ? c4 : x;
  x = ch == 5 ? c5 : x; x = ch == 6 ? c6 : x; x = ch == 7 ? c7 : x; x = ch == 8 ? c8 : x;
  x = ch == 9 ? c9 : x; x = ch == 10 ? c10 : x; x = ch == 11 ? c11 : x; x = ch == 12 ? c12 : x;
  return x;
}

// the interior rows (j, k) of the state, row = kk * ny + jj: the flat index of the cell i = 0 of a row.  Z, the complex work array,
// holds the interior only in this order: element (kk, jj, ii) at ((kk * ny + jj) * nx + ii), real part first
RG_MON_FN unsigned spec_row_origin(const DevParams& g, unsigned row) {
  return (unsigned)g.gw + g.sj * (row % (unsigned)g.ny + (unsigned)g.gw) + g.sk * (row / (unsigned)g.ny + (unsigned)g.gw);
}
RG_MON_FN unsigned spec_bitrev(unsigned i, int logn) {
  unsigned r = 0;
  for (int b = 0; b < logn; ++b) r |= (i >> b & 1u) << (logn - 1 - b);
  return r;
}

// ---- the geometry of the gfx950 kernels, which the host needs for the scratch ------------------------------------------------------
// log2 of the lines a tile of `tile` complex elements holds of lines of 2^logn points, where 2^lavail lines lie side by side
RG_MON_FN int spec_tile_logw(int tile_log, int logn, int lavail) {
  int w = tile_log - logn;
  if (w > SPEC_TILE_MAX_LOGW) w = SPEC_TILE_MAX_LOGW;
  if (w > lavail) w = lavail;
  return w < 0 ? 0 : w;
}
RG_MON_FN int spec_tile_log() { return 13; }
static_assert(1 << 13 == SPEC_TILE, "spec_tile_log is the logarithm of SPEC_TILE");
// the workgroups of the binning pass: a tile (one ky, 2^logw adjacent kx, every kz) at least each
RG_MON_FN unsigned spec_bin_groups(const SpecBox& b) {
  const unsigned tiles = (unsigned)b.ny << (b.lx - spec_tile_logw(spec_tile_log(), b.lz, b.lx));
  return tiles < (unsigned)SPEC_GROUPS ? tiles : (unsigned)SPEC_GROUPS;
}
// log2 of the parts the columns of a tile of the binning pass are cut into, each part with an owner per shell: as many as the
// SPEC_BLOCK threads of a workgroup have owners for, at most the columns of the tile.  Fixed by the box and the spec: it is part of the
// summation order
RG_MON_FN int spec_bin_logp(const SpecBox& b, unsigned shells) {
  int p = 0;
  while (p < spec_tile_logw(spec_tile_log(), b.lz, b.lx) && (shells << (p + 1)) <= (unsigned)SPEC_BLOCK) ++p;
  return p;
}
// Scratch of one sample, in doubles: Z, then per workgroup of the binning pass and part S partial sums and S partial counts -- parts
// times S is at most SPEC_BLOCK where there is more than one part (the flat functors need Z only: never more)
RG_MON_FN size_t spec_scratch_doubles(const SpecBox& b, unsigned max_shells) {
  return 2 * ((size_t)b.nx * b.ny * b.nz) + (size_t)spec_bin_groups(b) * 2 * (max_shells > (unsigned)SPEC_BLOCK ? max_shells : (unsigned)SPEC_BLOCK);
}

// ---- the flat kernels (rg_launch): the host emulation and any backend without kernels of its own -----------------------------------
// the in-place transform of the n = 2^logn points Z[base + p * stride], p < n, which stand in bit-reversed order
RG_DEVFN void spec_fft_line(double* Z, size_t base, size_t stride, int logn, const double* __restrict__ tw) {
  const unsigned n = 1u << logn;
  for (int st = 0; st < logn; ++st) {
    const unsigned h = 1u << st;
    for (unsigned bf = 0; bf < n / 2; ++bf) {
      const unsigned j = bf & (h - 1), p = ((bf >> st) << (st + 1)) + j;
      const unsigned k = (j << (logn - 1 - st)) << (SPEC_MAX_LOG - logn);
      const double wr = tw[2 * k], wi = tw[2 * k + 1];
      double* a = Z + 2 * (base + (size_t)p * stride);
      double* b = Z + 2 * (base + (size_t)(p + h) * stride);
      const double br = b[0] * wr - b[1] * wi, bi = b[0] * wi + b[1] * wr;
      const double ar = a[0], ai = a[1];
      a[0] = ar + br; a[1] = ai + bi;
      b[0] = ar - br; b[1] = ai - bi;
    }
  }
}
// thread row = kk * ny + jj: the channels (ca, cb) of the row -> Z, transformed along x
struct K_mon_spectrum_x {
  DevParams g; SpecBox b; int ca, cb; const double* U; const double* tw; double* Z; const StepClock* clk;
  RG_DEVFN void operator()(unsigned row) const {
    if (!mon_gate_open(clk) || row >= (unsigned)b.ny * (unsigned)b.nz) return;
    const unsigned o0 = spec_row_origin(g, row);
    const size_t base = (size_t)row * b.nx;
    for (unsigned i = 0; i < (unsigned)b.nx; ++i) {
      double c[SPEC_NQ];
      spec_cell_channels(g, U, o0 + i, c);
      const size_t e = base + spec_bitrev(i, b.lx);
      Z[2 * e] = spec_pick(c, ca);
      Z[2 * e + 1] = spec_pick(c, cb);
    }
    spec_fft_line(Z, base, 1, b.lx, tw);
  }
};
// thread line: axis 1: line = kk * nx + ii, the points jj; axis 2: line = jj * nx + ii, the points kk.  Brought into bit-reversed
// order by swaps, then transformed
struct K_mon_spectrum_line {
  SpecBox b; int axis; const double* tw; double* Z; const StepClock* clk;
  RG_DEVFN void operator()(unsigned line) const {
    if (!mon_gate_open(clk)) return;
    const unsigned lines = (unsigned)b.nx * (unsigned)(axis == 1 ? b.nz : b.ny);
    if (line >= lines) return;
    const unsigned ii = line % (unsigned)b.nx, other = line / (unsigned)b.nx;
    const int logn = axis == 1 ? b.ly : b.lz;
    const size_t stride = axis == 1 ? (size_t)b.nx : (size_t)b.nx * b.ny;
    const size_t base = axis == 1 ? (size_t)other * b.nx * b.ny + ii : (size_t)other * b.nx + ii;
    for (unsigned p = 0; p < (1u << logn); ++p) {
      const unsigned r = spec_bitrev(p, logn);
      if (r <= p) continue;
      double* x = Z + 2 * (base + p * stride);
      double* y = Z + 2 * (base + r * stride);
      const double xr = x[0], xi = x[1];
      x[0] = y[0]; x[1] = y[1];
      y[0] = xr; y[1] = xi;
    }
    spec_fft_line(Z, base, stride, logn, tw);
  }
};
// thread s: shell s of spec S over the whole of Z^: ky ascending, kx ascending, |kz| ascending, +kz before -kz.  first: the first
// transform of the spec stores the power and the mode count, a later one adds its power.  scale = 1 / N^2, a power of two
struct K_mon_spectrum_bin {
  SpecBox b; SpecOne S; int first; double scale; const double* Z; double* out; const StepClock* clk;
  RG_DEVFN void operator()(unsigned s) const {
    if (!mon_gate_open(clk) || s >= (unsigned)S.shells) return;
    double sum = 0.0, cnt = 0.0;
    const int hz = b.nz / 2;
    const size_t plane = (size_t)b.nx * b.ny;
    for (unsigned jj = 0; jj < (unsigned)b.ny; ++jj) {
      const unsigned ay = (unsigned)S.wy * spec_fold(jj, (unsigned)b.ny);
      for (unsigned ii = 0; ii < (unsigned)b.nx; ++ii) {
        const unsigned ax = (unsigned)S.wx * spec_fold(ii, (unsigned)b.nx);
        int lo, hi;
        spec_interval(ax * ax + ay * ay, (unsigned)S.wz, hz, s, &lo, &hi);
        const size_t col = (size_t)jj * b.nx + ii;
        for (int m = lo; m <= hi; ++m) {
          const double* z = Z + 2 * (col + (size_t)m * plane);
          sum = sum + (z[0] * z[0] + z[1] * z[1]);
          cnt += 1.0;
          if (m != 0 && m != hz) {
            z = Z + 2 * (col + (size_t)(b.nz - m) * plane);
            sum = sum + (z[0] * z[0] + z[1] * z[1]);
            cnt += 1.0;
          }
        }
      }
    }
    const double p = sum * scale;
    out[S.base + s] = first ? p : out[S.base + s] + p;
    if (first) out[S.base + S.shells + s] = cnt;
  }
};

}  // namespace rgpu_dev
