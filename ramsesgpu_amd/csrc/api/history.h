// api/history.h -- history diagnostics (row / column sums on the device) and the forcings.  See api/ctx.h.
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

// the volume element of the history sums, normalised by the box (MHDRunBase.cpp:3533-3536; 2D: :3351-3353)
double hist_dtau(const rgpu_ctx* c) {
  const rgpu_params& p = c->p;
  if (c->g.three_d) return p.dx * p.dy * p.dz / (p.xMax - p.xMin) / (p.yMax - p.yMin) / (p.zMax - p.zMin);
  return p.dx * p.dy / (p.xMax - p.xMin) / (p.yMax - p.yMin);
}

// ---- the history row of a step inside a batch of device-clock steps (hip/history_batch.h) ---------------------------
// Queues, behind the tick of the step `nStep` (record c->clk_cur, the `slot`-th of the open batch), the five launches that take the
// row of rgpu_history_mri of U[nStep % 2] when the loop's condition holds for this step, and write d_hist[slot] either way.
// dt0, tHist0: the loop's *dt and *tHist at the head of the batch's first step (read by slot 0 only).
// Scratch in F exactly as hist_scratch lays it out (the Reynolds column sums go where the vx sums were).  F is dead here: the
// step before is complete in stream order (a batch is queued on the context stream alone: mhd3d_core is `serial` while c->clk_cur
// is set, the fused 2D step is one launch), and the first kernel of the step that follows which touches F -- the 3D sweep
// (rgpu_tiled::mhd3d_sweep) -- writes every entry of F, emf that the shear remap and the update read; step_pre's ghost fill works on
// U alone and the fused 2D step does not use F at all.  It is the liveness rgpu_history_mri between two steps has always relied on.
int history_batch_queue(rgpu_ctx* c, int nStep, int slot, double dt0, double tHist0, double dtHist) {
  const HistScratch h = hist_scratch(c);
  const size_t is = (size_t)c->g.isize;
  double* rcol = h.cols + is;   // column 1 (the vx sums) has served once the means are formed
  const double* U = c->U[nStep & 1];
  const HistBatchGate gate = {c->clk_cur, slot ? c->d_clk + slot - 1 : 0, slot ? c->d_hist + slot - 1 : 0, dt0, tHist0, dtHist};
  const double dTau = hist_dtau(c);
  const int nyz = c->p.ny * (c->g.three_d ? c->p.nz : 1);
  K_hist_monitor_gated<K_hist_rows> k1 = {gate, {c->g, U, h.rows}};
  K_hist_monitor_cols k2 = {gate, {c->g, h.rows, h.cols, HIST_NQ}, h.mean, nyz};
  K_hist_monitor_gated<K_hist_reynolds> k3 = {gate, {c->g, U, h.mean, h.mean + is, dTau, h.rows}};
  K_hist_monitor_gated<K_hist_cols> k4 = {gate, {c->g, h.rows, rcol, 1}};
  K_hist_monitor_finish k5 = {gate, c->g.isize, c->g.gw, h.cols, rcol, dTau, nStep, c->d_hist + slot};
  if (rg_launch<kBlock>(c->stream, (unsigned)h.R, k1) || rg_launch<kBlock>(c->stream, (unsigned)(HIST_NQ * is), k2) ||
      rg_launch<kBlock>(c->stream, (unsigned)h.R, k3) || rg_launch<kBlock>(c->stream, (unsigned)is, k4) ||
      rg_launch<64>(c->stream, (unsigned)HIST_BATCH_NQ, k5)) return -1;
  ++c->hist_heads;
  return 0;
}

// ---- the monitor of a 2D state (kernels_monitor.h; rgpu_state_monitor) ----------------------------------------------
// Scratch in F like the history sums: the segment sums part[MON_NQ][nseg][nx], then the lane values [lanes][MON_NQ].  Steps 1 - 3 of
// the summation order on the device, the butterfly over the lane values on the host (the same additions, mon_combine).  Reads the
// state only: no ghost fill, nothing of c->rec or the CFL slots.
static_assert(MON_NQ == RGPU_MON_NQ && MON_ROWS == RGPU_MON_ROWS && MON_LANES == RGPU_MON_LANES, "include/rgpu.h states the summation order");
size_t monitor_scratch_doubles(const DevParams& g) {
  const size_t R = (size_t)mon_nseg(g.ny) * g.nx;
  return MON_NQ * (R + (size_t)(g.nx < MON_LANES ? g.nx : MON_LANES));
}
int state_monitor(rgpu_ctx* c, int parity, double* out) {
  const size_t R = (size_t)mon_nseg(c->g.ny) * c->g.nx;
  const int nl = c->g.nx < MON_LANES ? c->g.nx : MON_LANES;
  double* part = c->F;
  double* lanes = c->F + (size_t)MON_NQ * R;
  K_mon_rows kr = {c->g, c->U[parity & 1], part};
  K_mon_lanes kl = {c->g, part, lanes};
  double h[MON_LANES * MON_NQ];
  for (int l = 0; l < MON_LANES; ++l) mon_init(h + l * MON_NQ);   // (a lane without a column: the neutral elements)
  if (rg_launch<kBlock>(c->stream, (unsigned)R, kr) || rg_launch<kBlock>(c->stream, (unsigned)nl, kl) ||
      rg_copy_d2h(h, lanes, sizeof(double) * nl * MON_NQ, c->stream) || rg_stream_sync(c->stream)) return -1;
  mon_butterfly(h, out);
  return 0;
}

// random forcing: the two sums of compute_random_forcing_normalization over this domain's interior, reduced in the
// rows (along y) / columns (along z) / host (along x) order of the history sums
int forcing_sums(rgpu_ctx* c, int parity, double* out2) {
  const HistScratch h = hist_scratch(c);
  const size_t is = (size_t)c->g.isize;
  K_forcing_rows kr = {c->g, c->U[parity & 1], c->Frc, h.rows};
  K_hist_cols kc = {c->g, h.rows, h.cols, 2};
  if (rg_launch<kBlock>(c->stream, (unsigned)h.R, kr) || rg_launch<kBlock>(c->stream, (unsigned)(2 * is), kc)) return -1;
  std::vector<double> cols(2 * is);
  if (rg_copy_d2h(cols.data(), h.cols, sizeof(double) * 2 * is, c->stream) || rg_stream_sync(c->stream)) return -1;
  out2[0] = 0.0; out2[1] = 0.0;
  for (size_t i = 0; i < is; ++i) { out2[0] += cols[i]; out2[1] += cols[is + i]; }
  return 0;
}

double forcing_norm(const rgpu_params& p, const double* s, double dt) {   // HydroRunBase.cpp:1286-1293
  if (p.randomForcingEdot == 0) return 0.0;
  const long long nbCells = (long long)p.nx * p.ny * p.nz_global;
  return (std::sqrt(s[0] * s[0] + s[1] * dt * p.randomForcingEdot * 2 * nbCells) - s[0]) / s[1];
}

int add_forcing(rgpu_ctx* c, int parity, double norm) {
  c->rec.forget();
  K_add_forcing k = {c->g, c->U[parity & 1], c->Frc, norm};
  return launch_planes<kBlock, 1>(c->stream, c->g, clip(c->g.gw, c->g.ksize - c->g.gw, c->g.ksize), k);
}

// Ornstein-Uhlenbeck forcing on U[parity]: advance the modes on the host, then one kernel over the interior planes
int step_ou_forcing(rgpu_ctx* c, int parity, double dt) {
  if (!c->ou) return 0;
  c->rec.forget();
  Phase ph(c, RGPU_T_UPDATE);
  c->ou->update(dt, c->p.cIso);
  K_ou_forcing k = {c->g, c->U[parity & 1], c->ou->m, dt, c->p.yMin, c->p.zMin, c->p.slab_rank * c->p.nz};
  return launch_planes<kBlock, 1>(c->stream, c->g, clip(c->g.gw, c->g.ksize - c->g.gw, c->g.ksize), k);
}

int step_forcing(rgpu_ctx* c, int nStep, double dt) {
  if (!c->p.randomForcingEnabled) return 0;
  Phase ph(c, RGPU_T_UPDATE);
  double s[2];
  if (forcing_sums(c, (nStep + 1) % 2, s)) return -1;
  return add_forcing(c, (nStep + 1) % 2, forcing_norm(c->p, s, dt));
}

// every entry point makes the context's device current: a multi-GPU process (or a thread whose current device differs)
// would otherwise launch on the wrong device
struct K_selftest_arith {
  const double* num; const double* den; double* quot; double* quot2; double* root; double* root2;
  RG_DEVFN void operator()(unsigned i) const {
    quot[i] = rg_div(num[i], rg_recip(den[i]));
    quot2[i] = num[i] / den[i];
    root[i] = rg_sqrt(num[i]);
    root2[i] = sqrt(num[i]);
  }
};

// one sample = the four corner states of an edge (LL, RL, LR, RR: r p u v w a b c each) and their four electric fields, SoA: in[q * n + i]
struct K_selftest_alfven {
  DevParams g; const double* in; double* e_sel; double* e_ref; int* route; unsigned n;
  RG_DEVFN void operator()(unsigned i) const {
    Prim8 s[4];
    for (int q = 0; q < 4; ++q) {
      const double* x = in + (size_t)(8 * q) * n + i;
      s[q].r = x[0]; s[q].p = x[n]; s[q].u = x[2 * (size_t)n]; s[q].v = x[3 * (size_t)n]; s[q].w = x[4 * (size_t)n];
      s[q].a = x[5 * (size_t)n]; s[q].b = x[6 * (size_t)n]; s[q].c = x[7 * (size_t)n];
    }
    const double E0 = in[(size_t)32 * n + i], E1 = in[(size_t)33 * n + i], E2 = in[(size_t)34 * n + i], E3 = in[(size_t)35 * n + i];
    int r = 0;
    e_sel[i] = mag_hlld_2d<false>(g, s[0], s[1], s[2], s[3], E0, E1, E2, E3, &r);
    e_ref[i] = mag_hlld_2d<true>(g, s[0], s[1], s[2], s[3], E0, E1, E2, E3);
    route[i] = r;
  }
};

#define RG_CHECK_CTX(c) do { if (!(c)) return RGPU_EINVAL; if ((c)->device >= 0) rg_set_device((c)->device); } while (0)
#define RG_HIPFAIL(c, what) fail((c), RGPU_EHIP, std::string(what) + ": " + rg_last_error_string())

}  // namespace
