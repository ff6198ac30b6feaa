// kernels_monitor_helm.h -- the Helmholtz spectra (rgpu_state_helm_spectra, rgpu_run_steps_helm_spectra; include/rgpu.h, "Helmholtz
// spectra"): the power of a vector field of a 3D state per wave-number shell, split into its solenoidal (transverse to the wave
// vector) and its compressive (longitudinal) part -- what an OU-forced run with ksi between 0 and 1 is judged by, the sound-wave
// content of w = m / sqrt(rho), the distance of the cell-centred B from a divergence-free field.
//
// Everything but the projection is the spectrum monitor's (kernels_monitor_spectrum.h) and is not restated: the channels
// (spec_cell_channels: the triples 1-3, 4-6, 7-9, 10-12 are m, v, w, b), the shell rule (spec_shell, spec_shell_count) and its inverse
// (spec_interval), the twiddle table, the line transforms and the order of every sum.  The components of a vector never meet in a
// transform packed as a + i b, so each component has a transform of its own with imaginary part zero: three arrays Z0, Z1, Z2, and
// helm_mode combines them mode by mode before the binning.
//
// Shared by the flat functor below (the test-only host emulation and any backend without kernels of its own) and by the gfx950
// kernels of hip/monitor_helm.h.  A header of its own: nothing the other kernels include changes.
#pragma once
#include "kernels_monitor_spectrum.h"

namespace rgpu_dev {

enum { HELM_NF = 4, HELM_MAX = 4 };

// one spec as the kernels read it: the caller's rgpu_helm_spec, its shells on this box, and where its 3 S doubles begin in a sample
struct HelmOne {
  int field;
  int wx, wy, wz;
  int shells;
  unsigned base;
};
// the specs of a call (what the launch routines read): `doubles` is the sum of 3 S over the specs, groups[m] the workgroups of the
// binning pass of spec m (helm_bin_groups)
struct HelmSet {
  int n;
  unsigned doubles;
  HelmOne s[HELM_MAX];
  unsigned groups[HELM_MAX];
};

// the first of the three channels of field f among the SPEC_NQ channels of spec_cell_channels: m 1, v 4, w 7, b 10
RG_MON_FN int helm_first_channel(int field) { return 1 + 3 * field; }
// the signed folded wave number of index i on an axis of n points: 0 .. n / 2 - 1, then -n / 2 .. -1 (the Nyquist index is -n / 2)
RG_MON_FN int helm_signed(unsigned i, unsigned n) { return i < n / 2 ? (int)i : (int)i - (int)n; }

// The one definition of the projection.  kx ky kz: the weighted wave vector kappa (exact integers as doubles); ux uy uz: the transforms
// of the three components, {re, im}; q = kappa^2, the integer of the shell rule.  *T: the power transverse to kappa, |kappa x u^|^2 / q;
// *L: the power along it, |kappa . u^|^2 / q.  Both formed directly, neither as a difference: a nearly pure field keeps its small
// part.  q = 0, the mean: all of it counts as transverse.  Not contracted (the division is the library's own)
RG_DEVFN void helm_mode(double kx, double ky, double kz, const double* ux, const double* uy, const double* uz, double q, double* T, double* L) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (q == 0.0) {
    *L = 0.0;
    *T = ((ux[0] * ux[0] + ux[1] * ux[1]) + (uy[0] * uy[0] + uy[1] * uy[1])) + (uz[0] * uz[0] + uz[1] * uz[1]);
    return;
  }
  const double dr = (kx * ux[0] + ky * uy[0]) + kz * uz[0], di = (kx * ux[1] + ky * uy[1]) + kz * uz[1];
  const double cxr = ky * uz[0] - kz * uy[0], cxi = ky * uz[1] - kz * uy[1];
  const double cyr = kz * ux[0] - kx * uz[0], cyi = kz * ux[1] - kx * uz[1];
  const double czr = kx * uy[0] - ky * ux[0], czi = kx * uy[1] - ky * ux[1];
  const rg_recip_t inv_q = rg_recip(q);
  *L = rg_div(dr * dr + di * di, inv_q);
  *T = rg_div(((cxr * cxr + cxi * cxi) + (cyr * cyr + cyi * cyi)) + (czr * czr + czi * czi), inv_q);
}

// Scratch of one sample, in doubles: Z0, Z1, Z2 (6 N), then per workgroup of the binning pass and owner three partials (solenoidal,
// compressive, count); the specs of a call use it one after another (the flat functor needs the three arrays only: never more)
RG_MON_FN unsigned helm_owners(const SpecBox& b, unsigned shells) { return shells << spec_bin_logp(b, shells); }
RG_MON_FN size_t helm_scratch_doubles(const SpecBox& b, unsigned shells, unsigned groups) {
  return 6 * ((size_t)b.nx * b.ny * b.nz) + (size_t)groups * 3 * helm_owners(b, shells);
}
// The workgroups of the binning pass of a spec of `shells` shells where the scratch holds `capacity` doubles: those of the spectrum
// monitor (spec_bin_groups), or as many fewer as have room for their partials -- a long thin box (4 x 1024 x 4: 1024 tiles) with
// thousands of shells would else ask for more than its flux array holds; each workgroup then walks more tiles.  0: not even one has
// room.  Fixed by the box, the spec and the flux array of the context, whatever other specs share the call: part of the summation order
RG_MON_FN unsigned helm_bin_groups(const SpecBox& b, unsigned shells, size_t capacity) {
  const size_t z = 6 * ((size_t)b.nx * b.ny * b.nz), per = 3 * (size_t)helm_owners(b, shells);
  if (capacity < z + per) return 0;
  const size_t room = (capacity - z) / per;
  return room < (size_t)spec_bin_groups(b) ? (unsigned)room : spec_bin_groups(b);
}

// ---- the flat kernel (rg_launch): the host emulation and any backend without kernels of its own; its transforms are K_mon_spectrum_x
// (cb = -1) and K_mon_spectrum_line, once per component -----------------------------------------------------------------------------
// thread s: shell s of spec S over the whole of the three transforms, in the column and |kz| order of K_mon_spectrum_bin: ky ascending,
// kx ascending, |kz| ascending, +kz before -kz.  Stores Psol[s], Pcomp[s] and M[s].  scale = 1 / N^2, a power of two
struct K_mon_helm_bin {
  SpecBox b; HelmOne S; double scale; const double* Z0; const double* Z1; const double* Z2; double* out; const StepClock* clk;
  RG_DEVFN void mode(unsigned ii, unsigned jj, unsigned kk, double* T, double* L) const {
    const size_t e = ((size_t)kk * b.ny + jj) * b.nx + ii;
    const int kx = S.wx * helm_signed(ii, (unsigned)b.nx), ky = S.wy * helm_signed(jj, (unsigned)b.ny), kz = S.wz * helm_signed(kk, (unsigned)b.nz);
    helm_mode((double)kx, (double)ky, (double)kz, Z0 + 2 * e, Z1 + 2 * e, Z2 + 2 * e, (double)(kx * kx + ky * ky + kz * kz), T, L);
  }
  RG_DEVFN void operator()(unsigned s) const {
    if (!mon_gate_open(clk) || s >= (unsigned)S.shells) return;
    double sol = 0.0, comp = 0.0, cnt = 0.0, T, L;
    const int hz = b.nz / 2;
    for (unsigned jj = 0; jj < (unsigned)b.ny; ++jj) {
      const unsigned ay = (unsigned)S.wy * spec_fold(jj, (unsigned)b.ny);
      for (unsigned ii = 0; ii < (unsigned)b.nx; ++ii) {
        const unsigned ax = (unsigned)S.wx * spec_fold(ii, (unsigned)b.nx);
        int lo, hi;
        spec_interval(ax * ax + ay * ay, (unsigned)S.wz, hz, s, &lo, &hi);
        for (int m = lo; m <= hi; ++m) {
          mode(ii, jj, (unsigned)m, &T, &L);
          sol = sol + T; comp = comp + L;
          cnt += 1.0;
          if (m != 0 && m != hz) {
            mode(ii, jj, (unsigned)(b.nz - m), &T, &L);
            sol = sol + T; comp = comp + L;
            cnt += 1.0;
          }
        }
      }
    }
    out[S.base + s] = sol * scale;
    out[S.base + S.shells + s] = comp * scale;
    out[S.base + 2 * S.shells + s] = cnt;
  }
};

}  // namespace rgpu_dev
