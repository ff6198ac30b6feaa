// api/history.h -- history diagnostics: the scratch layout and the launches of the row / column sums (kernels_history.h); the arithmetic
// behind the column sums is history_row.h.  See api/ctx.h.
#pragma once
namespace {
// ---- history diagnostics ------------------------------------------------------------------------------------------
// Scratch lives in the flux array F, which is dead between steps: rows [HIST_NQ][nk][isize], then the column sums
// [HIST_NQ][isize], then the two mean-velocity columns.
struct HistScratch { double* rows; double* cols; double* mean; size_t R; };
HistScratch hist_scratch(rgpu_ctx* c) {
  HistScratch h;
  const int nk = c->g.three_d ? c->g.nz : 1;
  h.R = (size_t)c->g.isize * nk;
  h.rows = c->F;
  h.cols = c->F + (size_t)HIST_NQ * h.R;
  h.mean = h.cols + (size_t)HIST_NQ * c->g.isize;
  return h;
}

int history_columns(rgpu_ctx* c, int parity, double* h_cols) {
  const HistScratch h = hist_scratch(c);
  K_hist_rows kr = {c->g, c->U[parity & 1], h.rows};
  K_hist_cols kc = {c->g, h.rows, h.cols, HIST_NQ};
  if (rg_launch<kBlock>(c->stream, (unsigned)h.R, kr) || rg_launch<kBlock>(c->stream, (unsigned)(HIST_NQ * c->g.isize), kc)) return -1;
  if (rg_copy_d2h(h_cols, h.cols, sizeof(double) * HIST_NQ * c->g.isize, c->stream) || rg_stream_sync(c->stream)) return -1;
  return 0;
}

int history_reynolds(rgpu_ctx* c, int parity, const double* h_mean_vx, const double* h_mean_vy, double dTau, double* h_cols) {
  const HistScratch h = hist_scratch(c);
  const size_t is = (size_t)c->g.isize;
  if (rg_copy_h2d(h.mean, h_mean_vx, sizeof(double) * is, c->stream) || rg_copy_h2d(h.mean + is, h_mean_vy, sizeof(double) * is, c->stream)) return -1;
  K_hist_reynolds kr = {c->g, c->U[parity & 1], h.mean, h.mean + is, dTau, h.rows};
  K_hist_cols kc = {c->g, h.rows, h.cols, 1};
  if (rg_launch<kBlock>(c->stream, (unsigned)h.R, kr) || rg_launch<kBlock>(c->stream, (unsigned)is, kc)) return -1;
  if (rg_copy_d2h(h_cols, h.cols, sizeof(double) * is, c->stream) || rg_stream_sync(c->stream)) return -1;
  return 0;
}

// history_turbulence: rows [HIST_TURB_NQ][nz][isize] and columns [HIST_TURB_NQ][isize] in the flux array, dead between steps (F has 15
// components per cell); the column sums come back in h_cols
int history_turbulence_columns(rgpu_ctx* c, int parity, double* h_cols) {
  const size_t is = (size_t)c->g.isize, R = is * c->g.nz;
  double* rows = c->F;
  double* cols = c->F + (size_t)HIST_TURB_NQ * R;
  K_hist_turb_rows kr = {c->g, c->U[parity & 1], rows};
  K_hist_cols kc = {c->g, rows, cols, HIST_TURB_NQ};
  if (rg_launch<kBlock>(c->stream, (unsigned)R, kr) || rg_launch<kBlock>(c->stream, (unsigned)(HIST_TURB_NQ * is), kc) ||
      rg_copy_d2h(h_cols, cols, sizeof(double) * HIST_TURB_NQ * is, c->stream) || rg_stream_sync(c->stream)) return -1;
  return 0;
}

// ---- the history row of a step inside a batch of device-clock steps (kernels_history.h) -----------------------------
// Queues, behind the tick of the step `nStep` (record c->clk_cur, the `slot`-th of the open batch), the five launches that take the
// row of rgpu_history_mri of U[nStep % 2] when the loop's condition holds for this step, and write record `slot` of the log (c->hist) either way.
// dt0, tHist0: the loop's *dt and *tHist at the head of the batch's first step (read by slot 0 only).
// Scratch in F exactly as hist_scratch lays it out (the Reynolds column sums go where the vx sums were).  F is dead here: the
// step before is complete in stream order (a batch is queued on the context stream alone: mhd3d_core picks mhd3d_serial while c->clk_cur
// is set, the fused 2D step is one launch), and the first kernel of the step that follows which touches F -- the 3D sweep
// (rgpu_tiled::mhd3d_sweep) -- writes every entry of F, emf that the shear remap and the update read; step_pre's ghost fill works on
// U alone and the fused 2D step does not use F at all.  It is the liveness rgpu_history_mri between two steps has always relied on.
int history_batch_queue(rgpu_ctx* c, int nStep, int slot, double dt0, double tHist0, double dtHist) {
  const HistScratch h = hist_scratch(c);
  const size_t is = (size_t)c->g.isize;
  double* rcol = h.cols + is;   // column 1 (the vx sums) has served once the means are formed
  const double* U = c->U[nStep & 1];
  const HistBatchGate gate = {c->clk_cur, slot ? c->clk.d + slot - 1 : 0, slot ? c->hist.d + slot - 1 : 0, dt0, tHist0, dtHist};
  const double dTau = rgpu_hist::dtau(c->p);
  const int nyz = c->p.ny * (c->g.three_d ? c->p.nz : 1);
  K_hist_batch_gated<K_hist_rows> k1 = {gate, {c->g, U, h.rows}};
  K_hist_batch_cols k2 = {gate, {c->g, h.rows, h.cols, HIST_NQ}, h.mean, nyz};
  K_hist_batch_gated<K_hist_reynolds> k3 = {gate, {c->g, U, h.mean, h.mean + is, dTau, h.rows}};
  K_hist_batch_gated<K_hist_cols> k4 = {gate, {c->g, h.rows, rcol, 1}};
  K_hist_batch_finish k5 = {gate, c->g.isize, c->g.gw, h.cols, rcol, dTau, nStep, c->hist.d + slot};
  if (rg_launch<kBlock>(c->stream, (unsigned)h.R, k1) || rg_launch<kBlock>(c->stream, (unsigned)(HIST_NQ * is), k2) ||
      rg_launch<kBlock>(c->stream, (unsigned)h.R, k3) || rg_launch<kBlock>(c->stream, (unsigned)is, k4) ||
      rg_launch<64>(c->stream, (unsigned)HIST_BATCH_NQ, k5)) return -1;
  ++c->hist_heads;
  return 0;
}

}  // namespace
