// kernels_monitor_pdf.h -- the PDF monitor (rgpu_state_pdfs, rgpu_run_steps_pdfs; include/rgpu.h, "PDF monitors"): histograms of the
// interior cells of a 3D state U[parity] -- tables of 64-bit counts over the classes of one channel (1D) or of a pair of channels (the
// joint PDF, a phase diagram): the density PDF of a turbulent box, the PDF of |div B|, rho against eint.
//
// Nothing of the per-cell arithmetic is restated here.  Channels 0 - 11 of a cell are twelve of the sixteen terms of monp_cell_terms
// (kernels_monitor_planes.h), which are the monitor's (kernels_monitor.h): rho mx my mz E ekin emag eint bx by bz absdivb = its columns
// 0 1 2 3 4 5 6 8 10 11 12 9.  Channel 12, v2 = (ekin + ekin) / rho, is formed from those terms without contraction.
//
// A value x of a channel falls into one of nbins + 3 classes of an axis: the bins 0 .. nbins - 1, then under, over, nan (pdf_class).
// Counts are integers: they do not depend on the order in which the cells arrive, so every kernel, every grid size and a numpy model
// (tests/monitor_pdf_checks.py) give the same words and no summation order needs stating.
//
// Shared by the flat functors below (the test-only host emulation and any backend without kernels of its own) and by the gfx950
// kernels of hip/monitor_pdf.h.  A header of its own: nothing the other kernels include changes.
#pragma once
#include "kernels_monitor_planes.h"

namespace rgpu_dev {

enum { PDF_NQ = 13, PDF_MAX = 8, PDF_MAX_WORDS = 16384 };

// one axis as the kernels read it: the caller's rgpu_pdf_axis, with what the host works out once -- linear: inv = nbins / (hi - lo);
// octave: shift = 52 - sub and key0 = bits(lo) >> shift
struct PdfAxis {
  int channel, scale, nbins, shift;
  double lo, hi, inv;
  unsigned long long key0;
};
// one table: it begins at word `base` of the sample; the word of a cell is ia * pitch + ib (1D: pitch == 1 and ib == 0)
struct PdfTable {
  PdfAxis a, b;
  unsigned base, pitch;
  int joint;
};
// the tables of a call (a kernel argument, passed by value): `words` is the sum over the tables, at most PDF_MAX_WORDS
struct PdfSet {
  int n;
  unsigned words;
  PdfTable t[PDF_MAX];
};

RG_DEVFN unsigned long long pdf_bits(double x) {
  unsigned long long u;
  __builtin_memcpy(&u, &x, sizeof(u));
  return u;
}

// the class of x on axis a: 0 .. nbins - 1 the bins, nbins under, nbins + 1 over, nbins + 2 nan
RG_DEVFN int pdf_class(const PdfAxis& a, double x) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (x != x) return a.nbins + 2;
  if (a.scale == 0) {
    if (x < a.lo) return a.nbins;
    if (x >= a.hi) return a.nbins + 1;
    const double d = x - a.lo;
    const double s = mon_mul(d, a.inv);   // >= 0: its floor is its integer part
    return s >= (double)a.nbins ? a.nbins - 1 : (int)s;
  }
  const double ax = fabs(x);
  if (ax < a.lo) return a.nbins;       // zeros and subnormals too: lo is a normal number
  if (ax >= a.hi) return a.nbins + 1;   // infinity too
  return (int)((pdf_bits(ax) >> a.shift) - a.key0);
}

// the thirteen channels of the cell at flat index o of a 3D state
RG_DEVFN void pdf_cell_terms(const DevParams& g, const double* __restrict__ U, unsigned o, double* c) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  double t[MONP_NQ];
  monp_cell_terms(g, U, o, t);
  c[0] = t[0]; c[1] = t[1]; c[2] = t[2]; c[3] = t[3]; c[4] = t[4]; c[5] = t[5]; c[6] = t[6];
  c[7] = t[8]; c[8] = t[10]; c[9] = t[11]; c[10] = t[12]; c[11] = t[9];
  c[12] = (t[5] + t[5]) / t[0];
}
// channel ch of c: a chain of selects on a uniform index, so that c stays in registers
RG_DEVFN double pdf_pick(const double* c, int ch) {
  static_assert(PDF_NQ == 13, "the chain names every channel");
  // (every channel read first: a select between values, not between addresses)
  const double c0 = c[0], c1 = c[1], c2 = c[2], c3 = c[3], c4 = c[4], c5 = c[5], c6 = c[6], c7 = c[7], c8 = c[8], c9 = c[9], c10 = c[10], c11 = c[11], c12 = c[12];
  double x = c0;
  x = ch == 1 ? c1 : x; x = ch == 2 ? c2 : x; x = ch == 3 ? c3 : x; x = ch == 4 ? c4 : x;
  x = ch == 5 ? c5 : x; x = ch == 6 ? c6 : x; x = ch == 7 ? c7 : x; x = ch == 8 ? c8 : x;
  x = ch == 9 ? c9 : x; x = ch == 10 ? c10 : x; x = ch == 11 ? c11 : x; x = ch == 12 ? c12 : x;
  return x;
}
// the word of the sample that the cell with channels c counts into for table t
RG_DEVFN unsigned pdf_word(const PdfTable& t, const double* c) {
  unsigned w = t.base + (unsigned)pdf_class(t.a, pdf_pick(c, t.a.channel)) * t.pitch;
  if (t.joint) w += (unsigned)pdf_class(t.b, pdf_pick(c, t.b.channel));
  return w;
}

// the interior rows (j, k) of the state, row = kk * ny + jj: their number, and the flat index of the cell i = 0 of a row
RG_MON_FN unsigned pdf_rows(const DevParams& g) { return (unsigned)g.ny * (unsigned)g.nz; }
RG_MON_FN unsigned pdf_row_origin(const DevParams& g, unsigned row) {
  return (unsigned)g.gw + g.sj * (row % (unsigned)g.ny + (unsigned)g.gw) + g.sk * (row / (unsigned)g.ny + (unsigned)g.gw);
}

// ---- the flat kernels (rg_launch): the host emulation and any backend without kernels of its own -----------------------------------
// thread w: word w of the sample at its destination <- 0
struct K_mon_pdf_zero {
  unsigned words; unsigned long long* out; const StepClock* clk;
  RG_DEVFN void operator()(unsigned w) const {
    if (mon_gate_open(clk) && w < words) out[w] = 0ull;
  }
};
// thread idx = row * nx + ii: the cell counts into one word of every table.  The host emulation runs its threads one after another
struct K_mon_pdf {
  DevParams g; PdfSet S; const double* U; unsigned long long* out; const StepClock* clk;
  RG_DEVFN void operator()(unsigned idx) const {
    if (!mon_gate_open(clk)) return;
    const unsigned row = idx / (unsigned)g.nx;
    if (row >= pdf_rows(g)) return;
    double c[PDF_NQ];
    pdf_cell_terms(g, U, pdf_row_origin(g, row) + idx % (unsigned)g.nx, c);
    for (int m = 0; m < S.n; ++m) {
#if !defined(__HIP_DEVICE_COMPILE__)
      out[pdf_word(S.t[m], c)] += 1ull;
#else
      atomicAdd(out + pdf_word(S.t[m], c), 1ull);
#endif
    }
  }
};

}  // namespace rgpu_dev
