// monitor_pdf.h (HIP / gfx950 only; included from rg_tiled.h) -- the PDF monitor of a lone 3D context (kernels_monitor_pdf.h) for
// rgpu_state_pdfs and the samples rgpu_run_steps_pdfs takes inside its device-clock batches.  Two launches per sample, the state read
// once however many tables the call has:
//
//   monitor_pdf_count_kernel   a workgroup of four waves owns a contiguous run of the interior rows (j, k); a wave walks a row with its
//                              64 lanes along i (contiguous loads, the ragged end of a row masked).  Per cell pdf_cell_terms once,
//                              then per table the word of the cell and one LDS add without return value on a table of u32 counts of
//                              all the tables of the call.  `replicas` copies of that table, lane l counting into copy l % replicas: in
//                              a smooth field the lanes of a wave hit the same word, and the adds on one address are served one after
//                              another; the copies lie an odd number of words apart, so that equal words of different copies fall into
//                              different banks.  After the barrier the copies are added and the workgroup stores its counts as a slab
//                              of `words` u32 to scratch (the flux array, dead between two steps).
//                              A count fits a u32: cells are addressed by a 32-bit flat index throughout (DevParams, `unsigned o`),
//                              so a state, let alone the rows of one workgroup, holds fewer than 2^32 of them.
//   monitor_pdf_fold_kernel    one wave per PDF_FOLD_WORDS = 16 consecutive words: lane l adds the slabs l / 16, l / 16 + 4, ... of word
//                              l % 16 into a u64, PDF_FOLD_DEPTH loads in flight (a row of 16 words is one 64-byte piece of a slab;
//                              one thread per word walking all the slabs waited for every load in turn: 117 us for 512 slabs), the
//                              four partial counts of a word meet by two shuffles, and the sum is STORED to the destination, `out`
//                              or the log slot -- no slot is zeroed beforehand, no global atomic, no memset between batches.
// LDS of the count kernel: PDF_MAX_WORDS u32 = 65,536 bytes, two workgroups per CU of 160 KB.
// clk != 0 (inside a batch): the StepClock record of the step the sample follows; a record that says stop ends every workgroup in its
// first instructions, and the log slot stays unwritten -- the host reads the same record and does not look at it.
#pragma once
#include "kernels_monitor_pdf.h"

namespace rgpu_tiled {

using namespace rgpu_dev;

enum { PDF_WAVES = 4, PDF_BLOCK = 64 * PDF_WAVES, PDF_FOLD_WORDS = 16, PDF_FOLD_PHASES = 64 / PDF_FOLD_WORDS, PDF_FOLD_DEPTH = 8 };
// The automatic choices (options "pdf_replicas", "pdf_groups" = -1), from scripts/monitor_pdf_bench.py (profiles/monitor_pdf_bench.json;
// DESIGN 3.4.5), the 512^3 MRI box, count + fold in microseconds.
// PDF_AUTO_GROUPS: 256 / 512 / 1024 / 2048 workgroups: one 1D spec 4845 / 2732 / 2758 / 2802, four 6830 / 4125 / 4129 / 4162, the
// joint one 5429 / 3163 / 3193 / 3250 -- 512 is two workgroups on each of the 256 CUs, all the LDS admits; below it half the waves
// are missing, above it only the fold grows (10.5 us at 512 slabs, 42 at 2048).
// PDF_AUTO_REPLICAS, as many copies as fit up to this: 1 / 2 / 4 / 8 / 16 / 32 / 64 copies: one 1D spec on the constant density of
// step 0, every lane on one word, 2744 / 2718 / 2723 / 2720 / 2721 / 2729 / 2734; four specs after 30 steps 4153 / 4124 / 4118 / 4127 /
// 4127 / 4124 / 4130 -- within 1 % of one another: the LDS adds are not what bounds the kernel.  4 is the fastest or within 0.2 % of it
// in each of the four series, and leaves small tables small to clear and to add up.
enum { PDF_AUTO_GROUPS = 512, PDF_AUTO_REPLICAS = 4 };

// the words from one copy of the table to the next
RG_MON_FN unsigned pdf_replica_pitch(unsigned words) { return words | 1u; }
// the copies the count kernel keeps: the option where it is positive, else PDF_AUTO_REPLICAS; never more than fit or than a wave has lanes
inline int pdf_replicas(unsigned words, int option) {
  int r = option > 0 ? option : (int)PDF_AUTO_REPLICAS;
  const int fit = words >= (unsigned)PDF_MAX_WORDS ? 1 : (int)((unsigned)PDF_MAX_WORDS / pdf_replica_pitch(words));
  if (r > fit) r = fit;
  if (r > 64) r = 64;
  return r < 1 ? 1 : r;
}
// the workgroups of the count kernel: the option where it is positive, else PDF_AUTO_GROUPS; a row at least each, and no more slabs
// than the scratch holds (max_groups >= 1)
inline unsigned pdf_groups(const DevParams& g, int option, size_t max_groups) {
  size_t n = option > 0 ? (size_t)option : (size_t)PDF_AUTO_GROUPS;
  if (n > pdf_rows(g)) n = pdf_rows(g);
  if (n > max_groups) n = max_groups;
  return (unsigned)(n < 1 ? 1 : n);
}

__global__ void __launch_bounds__(PDF_BLOCK) monitor_pdf_count_kernel(DevParams g, PdfSet S, int replicas, const double* __restrict__ U, const StepClock* clk, unsigned* __restrict__ slabs) {
  if (!mon_gate_open(clk)) return;
  __shared__ unsigned tab[PDF_MAX_WORDS];
  const unsigned W = S.words, pitch = replicas > 1 ? pdf_replica_pitch(W) : W;
  for (unsigned w = threadIdx.x; w < pitch * (unsigned)replicas; w += PDF_BLOCK) tab[w] = 0u;
  __syncthreads();
  const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  unsigned* mine = tab + (lane % (unsigned)replicas) * pitch;
  const unsigned long long rows = pdf_rows(g);
  const unsigned r0 = (unsigned)(blockIdx.x * rows / gridDim.x), r1 = (unsigned)((blockIdx.x + 1ull) * rows / gridDim.x);
  for (unsigned r = r0 + wave; r < r1; r += PDF_WAVES) {
    const unsigned o0 = pdf_row_origin(g, r);
    for (unsigned i = lane; i < (unsigned)g.nx; i += 64u) {
      double c[PDF_NQ];
      pdf_cell_terms(g, U, o0 + i, c);
      for (int m = 0; m < S.n; ++m) atomicAdd(mine + pdf_word(S.t[m], c), 1u);   // (the value is not used: an add without return)
    }
  }
  __syncthreads();
  unsigned* slab = slabs + (size_t)blockIdx.x * W;
  for (unsigned w = threadIdx.x; w < W; w += PDF_BLOCK) {
    unsigned n = 0u;
    for (int r = 0; r < replicas; ++r) n += tab[(unsigned)r * pitch + w];
    slab[w] = n;
  }
}

__global__ void __launch_bounds__(64) monitor_pdf_fold_kernel(unsigned words, unsigned groups, const StepClock* clk, const unsigned* __restrict__ slabs, unsigned long long* __restrict__ out) {
  if (!mon_gate_open(clk)) return;
  const unsigned w = blockIdx.x * PDF_FOLD_WORDS + (threadIdx.x % PDF_FOLD_WORDS), phase = threadIdx.x / PDF_FOLD_WORDS;
  unsigned long long n = 0ull;
  if (w < words) {
    for (unsigned s0 = phase; s0 < groups; s0 += PDF_FOLD_PHASES * PDF_FOLD_DEPTH) {
      unsigned x[PDF_FOLD_DEPTH];
#pragma unroll
      for (int u = 0; u < PDF_FOLD_DEPTH; ++u) {
        const unsigned s = s0 + (unsigned)u * PDF_FOLD_PHASES;
        x[u] = s < groups ? slabs[(size_t)s * words + w] : 0u;
      }
#pragma unroll
      for (int u = 0; u < PDF_FOLD_DEPTH; ++u) n += x[u];
    }
  }
  // (every lane of the wave is here: the lanes of words past the end carry 0)
  n += __shfl_xor(n, PDF_FOLD_WORDS, 64);
  n += __shfl_xor(n, 2 * PDF_FOLD_WORDS, 64);
  if (phase == 0 && w < words) out[w] = n;
}

// The launches of one sample of U into out[S.words]; scratch: groups * S.words u32 (the slabs)
inline int launch_monitor_pdf(rg_stream_t s, const DevParams& g, const PdfSet& S, int replicas, unsigned groups, const double* U, const StepClock* clk, unsigned* scratch, unsigned long long* out) {
  hipLaunchKernelGGL(monitor_pdf_count_kernel, dim3(groups), dim3(PDF_BLOCK), 0, s, g, S, replicas, U, clk, scratch);
  if (hipGetLastError() != hipSuccess) return -1;
  hipLaunchKernelGGL(monitor_pdf_fold_kernel, dim3((S.words + PDF_FOLD_WORDS - 1) / PDF_FOLD_WORDS), dim3(64), 0, s, S.words, groups, clk, (const unsigned*)scratch, out);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace rgpu_tiled
