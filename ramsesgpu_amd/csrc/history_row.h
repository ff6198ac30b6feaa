// history_row.h -- the arithmetic of the MHD history rows behind the device's column sums, written ONCE: the volume element, the
// y-z mean of a column entry, the ascending sum over the interior i, and out[q] of the MRI / default row (rgpu_history_mri).
// No HIP and no context type in here: rgpu_history_mri and the turbulence rows (api/entry_core.h) include it as host code, the
// finish functor of a batch (kernels_history.h: K_hist_batch_finish) as device code, and the separately built slab driver
// (comm/rgpu_comm.cpp) by relative path, around its two all-reduces.  The oracle's restatement (oracle/restate/orc_api.cpp) and the
// numpy statements in tests/ are the independent anchor and do not include it.
//
// Same doubles wherever it is compiled: IEEE + - * / only, "fp contract(off)" inside the bodies (nothing else of a translation unit
// changes), the one product that is followed by a division pinned on the device (hb_mul; the form of mon_mul, kernels_monitor.h).
#pragma once
#include <cstddef>

#include "../../include/rgpu.h"

#if defined(__HIPCC__)
#define RG_HIST_FN __host__ __device__ __forceinline__
#else
#define RG_HIST_FN inline
#endif

namespace rgpu_hist {

// columns of the MRI sums (kernels_history.h: hist_row_cell states what they hold) and values of a row (RGPU_HIST_NQ)
enum { NCOL = 9, NROW = 8 };

// The volume element of the history sums, normalised by the whole box (MHDRunBase.cpp:3533-3536; 2D: :3351-3353).  "3D" is
// nz_global != 1, which is what both kinds of caller meant: a context's DevParams::three_d is set from exactly that expression of its
// unmodified copy of the parameters (fill_dev_params, api/ctx.h), and the slab driver tested it literally.
RG_HIST_FN double dtau(const rgpu_params& p) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (p.nz_global != 1) return p.dx * p.dy * p.dz / (p.xMax - p.xMin) / (p.yMax - p.yMin) / (p.zMax - p.zMin);
  return p.dx * p.dy / (p.xMax - p.xMin) / (p.yMax - p.yMin);
}

// the y-z mean of vx or vy at one i, from its column sum (all i, ghosts included); nyz = ny * nz of the whole box
RG_HIST_FN double yz_mean(double colsum, double nyz) {
  return colsum / nyz;
}

// the sum of a column over the interior i, ascending from +0.0
RG_HIST_FN double interior_sum(const double* col, int isize, int gw) {
  double s = 0.0;
  for (int i = gw; i < isize - gw; ++i) s += col[i];
  return s;
}

// a product that stays a product in front of a division (a no-op on the host, which has nothing to fold it into)
RG_HIST_FN double hb_mul(double a, double b) {
  double x = a * b;
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("" : "+v"(x));
#endif
  return x;
}

// out[q] of rgpu_history_mri, q in [0, NROW): cols = the NCOL column sums [NCOL][isize], rcol = the column sums of the Reynolds rows
//   out[0] mass <- column 0, [1] maxwell <- 4, [2] reynolds <- its own column, [3] magp <- 3, [4..6] mean B <- 5..7, [7] divB <- 8
RG_HIST_FN double mri_row_value(int q, const double* cols, const double* rcol, int isize, int gw, double dTau) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const int src = q == 0 ? 0 : q == 1 ? 4 : q == 3 ? 3 : q == 7 ? 8 : q + 1;
  const double s = interior_sum(q == 2 ? rcol : cols + (size_t)src * isize, isize, gw);
  if (q == 2 || q == 7) return s;          // reynolds (dTau is inside the sum, as in the reference), divB
  if (q == 3) return hb_mul(s, dTau) / 2.;   // magp
  return s * dTau;                         // mass, maxwell, mean B
}

}  // namespace rgpu_hist
