// rg_options.h -- diagnostic options of librgpu.so (process-wide), set through rgpu_set_option (include/rgpu.h).
// A user needs none of them: each switches an optional fast path off, or pins a parameter of a launch plan, so that the tests can
// run a configuration both ways (tests/test_gpu_parity.py).  They replace the RGPU_NO_* / RGPU_XCD_SUB / RGPU_ZSEG / RGPU_CHUNKS
// environment switches of rounds 2-5; what is left in the environment is listed in include/rgpu.h ("Environment").
#pragma once
#include <cstring>

namespace rgpu {

struct Options {
  int spec = 1;           // kernels specialised for the solver configuration (0: the generic instantiations only)
  int ghost_images = 1;   // the fused 2D steps write the ghost images of their output (the next step's ghost fill is skipped)
  int step_clock = 1;     // the time step stays on the device between the steps of a batch (rgpu_run_steps)
  int xcd_sub = -1;       // sub-band size (cells) of the XCD-aware workgroup order of the flat kernels; -1: rgpu_create's default
  int zseg = 0;           // planes per z segment of the tiled sweeps; 0: planned per launch (tile_grid_plan)
  int chunks = -1;        // chunks of the two-stream schedule of the flat 3D MHD kernels; -1: ksize / 8; 1: one stream
  int history_batch = 1;  // rgpu_run_steps_history samples on the device inside the device-clock batches (0: the literal loop everywhere)
  int forcing_clock = 1;  // rgpu_run_steps* batch a lone 3D context with random / Ornstein-Uhlenbeck forcing: the forcing stages read the record (0: the literal loop)
  int member_params = 0;  // 1: the fused rounds of every ensemble read their constants from the per-member table (hip/ensemble_scan.h), equal sets or not
  int map_log_kib = 262144;   // byte budget (KiB) of the device log of the maps a batch samples (api/monitor.h; rgpu_run_steps_mapped)
  int map_x_tiled = -1;   // the kernel that sums a map along x (hip/monitor_maps.h): -1 by the thickness of the range, 0 direct, 1 tiled
  int pdf_replicas = -1;  // copies of the LDS table of the PDF monitor's count kernel (hip/monitor_pdf.h): -1 automatic, n forces the count (the same words)
  int pdf_groups = -1;    // workgroups of that kernel: -1 automatic, n forces the grid size (the same words)
  int spectrum_tile_y = -1;   // log2 of the lines a tile of the spectrum monitor's y pass holds (hip/monitor_spectrum.h): -1 the widest that fits, 0 .. 6 (the same doubles)
};
inline Options& options() { static Options o; return o; }
inline int* option_slot(const char* name) {
  Options& o = options();
  if (!name) return 0;
  if (!std::strcmp(name, "spec")) return &o.spec;
  if (!std::strcmp(name, "ghost_images")) return &o.ghost_images;
  if (!std::strcmp(name, "step_clock")) return &o.step_clock;
  if (!std::strcmp(name, "xcd_sub")) return &o.xcd_sub;
  if (!std::strcmp(name, "zseg")) return &o.zseg;
  if (!std::strcmp(name, "chunks")) return &o.chunks;
  if (!std::strcmp(name, "history_batch")) return &o.history_batch;
  if (!std::strcmp(name, "forcing_clock")) return &o.forcing_clock;
  if (!std::strcmp(name, "member_params")) return &o.member_params;
  if (!std::strcmp(name, "map_log_kib")) return &o.map_log_kib;
  if (!std::strcmp(name, "map_x_tiled")) return &o.map_x_tiled;
  if (!std::strcmp(name, "pdf_replicas")) return &o.pdf_replicas;
  if (!std::strcmp(name, "pdf_groups")) return &o.pdf_groups;
  if (!std::strcmp(name, "spectrum_tile_y")) return &o.spectrum_tile_y;
  return 0;
}

}  // namespace rgpu
