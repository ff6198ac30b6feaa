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

}  // namespace
