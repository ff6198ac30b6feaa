// api/forcing.h -- the forcing stages of the turbulence problems: random forcing (sums, normalisation, kick) and the
// Ornstein-Uhlenbeck process.  See api/ctx.h.
#pragma once
namespace {
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
  c->ou_stale = true;
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

// ---- the forcing stages inside a batch of device-clock steps (api/run_steps.h) ------------------------------------------------------
// What the stages above take from the host in every step -- the sums and the norm of the random forcing, the mode step of the
// Ornstein-Uhlenbeck process, dt -- is formed on the device with the host's expressions (kernels_bc.h: forcing_norm_finish, ou_mode_step;
// launchers.h), and the last kick of the step carries the CFL scan of the state it leaves, so that the next tick finds its maxima in
// the slots: nothing in a forced step needs the host between two steps.
//
// Which forced contexts the library's own loop batches (option "forcing_clock"): a lone, non-rotating 3D box whose sweep covers the grid,
// with nothing else in the step that keeps it out of a batch (entry_clock.h: clock_config_ok).  Asked by that loop only: rgpu_clock_capable
// and an rgpu_clock_open from outside answer as they did, their callers queue no forcing stage.
bool forcing_clock_ok(const rgpu_ctx* c) {
  const rgpu_params& p = c->p;
  if (!(p.randomForcingEnabled || p.ouForcingEnabled) || !rgpu::options().forcing_clock) return false;
  if (!c->g.three_d || c->g.rot || p.slab_count != 1) return false;
  if (c->timers_on || p.gravityEnabled != 0 || p.nu > 0 || (p.mhdEnabled && p.eta > 0)) return false;
  if (!rgpu_tiled::step_clock_supported()) return false;
  if (RG_SYNC_LAUNCH) return true;   // (host emulation: the record is resolved by value for every kernel)
  return p.mhdEnabled ? rgpu_tiled::mhd3d_sweep_covers(c->g) : rgpu_tiled::hydro3d_sweep_covers(c->g);
}

static_assert(sizeof(rgpu_ou::OuModes) == 2 * rgpu_ou::NDIM * rgpu_ou::NMODE * sizeof(double), "ou_tab starts with an OuModes");
enum { kOuRow = rgpu_ou::OuProcess::STEP_DEVIATES, kOuForceAt = rgpu_ou::NDIM * rgpu_ou::NMODE, kOuProjAt = 2 * rgpu_ou::NDIM * rgpu_ou::NMODE };

// what the open of a batch leaves for its close: where the generator stood, and for how many steps it drew
struct ForcingBatch { rgpu_ou::OuProcess::Gen gen0; int drawn = 0; };

// At the open of a batch of at most m steps: the device buffers (first use), the tables of the process if the host's copy is the newer
// one, and the deviates of m steps, row s for the step of slot s -- the generator moves on by m steps (forcing_batch_close)
int forcing_batch_open(rgpu_ctx* c, int m, ForcingBatch* fb) {
  if (c->p.randomForcingEnabled && !c->frc_norm.allocated() && c->frc_norm.alloc(1, false)) return -1;
  if (!c->ou) return 0;
  if (!c->ou_tab.allocated() && c->ou_tab.alloc(rgpu_ctx::kOuTab)) return -1;
  if (!c->ou_gauss.allocated() && c->ou_gauss.alloc((size_t)rgpu_ctx::kClockBatch * kOuRow)) return -1;
  if (c->ou_stale) {
    std::memcpy(c->ou_tab.h, &c->ou->m, sizeof(c->ou->m));
    std::memcpy(c->ou_tab.h + kOuProjAt, c->ou->proj, sizeof(c->ou->proj));
    if (c->ou_tab.upload(rgpu_ctx::kOuTab, c->stream)) return -1;
    c->ou_stale = false;
  }
  fb->gen0 = c->ou->gen();
  for (int s = 0; s < m; ++s) c->ou->draw_step(c->ou_gauss.h + (size_t)s * kOuRow);
  fb->drawn = m;
  if (c->ou_gauss.upload((size_t)m * kOuRow, c->stream) == 0) return 0;
  c->ou->set_gen(fb->gen0);
  return -1;
}
// a batch whose records could not be read: no step of it counts, the generator stands where it stood and the host's force is the one to trust
void forcing_batch_abandon(rgpu_ctx* c, const ForcingBatch& fb) {
  if (!c->ou) return;
  c->ou->set_gen(fb.gen0);
  c->ou_stale = true;
}

// The forcing stages of the step of slot `slot`, behind its core, in the order of step_forcing / step_ou_forcing: [rows, columns, norm,
// kick] [mode step, kick] on U[(nStep + 1) % 2].  The scratch of the sums is hist_scratch's, in F: dead behind the core, and used by
// the monitors' samples only behind this step, on the same stream.  The last kick goes through rg_reduce_max into slot 0 of the slots
// the tick of this step zeroed (a stopped step: every kernel here returns at once, the slots stay the stopping tick's)
int forcing_batch_step(rgpu_ctx* c, int nStep, int slot) {
  using namespace monitored_run;   // (launchers.h: the functors of these stages)
  const StepTime st = step_time(c, 0.0, 0.0);
  if (st.skip) return 0;
  const rgpu_params& p = c->p;
  const DevParams& g = c->g;
  const int par = (nStep + 1) % 2;
  double* U = c->U[par];
  const PlaneRange r = clip(g.gw, g.ksize - g.gw, g.ksize);
  auto scan = [&](const auto& k) { return rg_reduce_max(c->stream, (unsigned)(r.hi - r.lo) * g.sk, k, c->d_red, (unsigned)r.lo * g.sk, false); };
  if (p.randomForcingEnabled) {
    const HistScratch h = hist_scratch(c);
    K_if_running<K_forcing_rows> kr = {{g, U, c->Frc, h.rows}, st.clk};
    K_if_running<K_hist_cols> kc = {{g, h.rows, h.cols, 2}, st.clk};
    K_forcing_norm kn = {h.cols, g.isize, p.randomForcingEdot, (long long)p.nx * p.ny * p.nz_global, st.dt, c->frc_norm.d, st.clk};
    if (rg_launch<kBlock>(c->stream, (unsigned)h.R, kr) || rg_launch<kBlock>(c->stream, (unsigned)(2 * g.isize), kc) || rg_launch<kBlock>(c->stream, 1u, kn)) return -1;
    K_add_forcing_dev k = {g, U, c->Frc, c->frc_norm.d, st.clk};
    if (c->ou ? launch_planes<kBlock, 1>(c->stream, g, r, k) : p.mhdEnabled ? scan(K_add_forcing_scan<true>{k}) : scan(K_add_forcing_scan<false>{k})) return -1;
  }
  if (c->ou) {
    rgpu_ou::OuModes* M = reinterpret_cast<rgpu_ou::OuModes*>(c->ou_tab.d);
    K_ou_mode_step km = {M, c->ou_tab.d + kOuProjAt, c->ou_gauss.d + (size_t)slot * kOuRow, c->ou->coef(p.cIso), st.dt, st.clk};
    if (rg_launch<kBlock>(c->stream, (unsigned)rgpu_ou::NMODE, km)) return -1;
    K_ou_forcing_dev k = {g, U, M, st.dt, p.yMin, p.zMin, p.slab_rank * p.nz, st.clk};
    if (p.mhdEnabled ? scan(K_ou_forcing_scan<true>{k}) : scan(K_ou_forcing_scan<false>{k})) return -1;
  }
  c->rec.scanned(par, 1);
  return 0;
}

// Behind the steps of a batch, in front of the read-back of its records: the force of the process comes back in the same synchronisation
int forcing_batch_download(rgpu_ctx* c) {
  return c->ou ? rg_copy_d2h(c->ou_tab.h + kOuForceAt, c->ou_tab.d + kOuForceAt, sizeof(c->ou->m.force), c->stream) : 0;
}
// ... and behind it: `ran` steps ran.  The host's process takes the device's force; had the generator drawn for more steps than ran, it
// goes back to where it stood and draws again for those that did -- it stands where the literal loop's would
void forcing_batch_close(rgpu_ctx* c, const ForcingBatch& fb, int ran) {
  c->forcing_steps += ran;
  if (!c->ou) return;
  std::memcpy(c->ou->m.force, c->ou_tab.h + kOuForceAt, sizeof(c->ou->m.force));
  if (ran < fb.drawn) {
    double r[kOuRow];
    c->ou->set_gen(fb.gen0);
    for (int s = 0; s < ran; ++s) c->ou->draw_step(r);
  }
}

}  // namespace
