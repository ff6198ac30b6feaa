// api/monitor.h -- the monitor of a lone context on the host side (kernels_monitor.h): scratch extent and launches of one sample, for
// rgpu_state_monitor (2D), rgpu_state_monitor3d and a sample queued inside a device-clock batch (rgpu_run_steps_monitored); the same for
// the plane monitor (kernels_monitor_planes.h: rgpu_state_monitor_planes, rgpu_run_steps_monitored_planes) and for the map monitor
// (kernels_monitor_maps.h: rgpu_state_maps, rgpu_run_steps_mapped), for the PDF monitor (kernels_monitor_pdf.h: rgpu_state_pdfs,
// rgpu_run_steps_pdfs), for the spectrum monitor (kernels_monitor_spectrum.h: rgpu_state_spectra, rgpu_run_steps_spectra) and for the
// Helmholtz spectra (kernels_monitor_helm.h: rgpu_state_helm_spectra, rgpu_run_steps_helm_spectra).  See api/ctx.h.
#pragma once
namespace {
// One route for either dimension, a 2D state being a volume of one plane.  Everything on the device, the sum over the planes included,
// so that the same launches serve a sample queued inside a batch of device-clock steps: the gfx950 kernels of hip/monitor3d.h where the
// backend has them, else the flat functors.  Scratch in F, then the ten doubles of a sample taken outside a batch.  F is dead between
// two steps (see history_batch_queue, api/history.h; the hydro steps keep nothing in it either).  Reads the state only: no ghost fill,
// nothing of c->rec or the CFL slots.
static_assert(MON_NQ == RGPU_MON_NQ && MON_ROWS == RGPU_MON_ROWS && MON_LANES == RGPU_MON_LANES, "include/rgpu.h states the summation order");
// (also: whether the samples of this context can be taken inside its device-clock batches)
bool monitor_scratch_fits(rgpu_ctx* c) { return c->F && mon_scratch_doubles(c->g) + MON_NQ <= (size_t)c->g.fN * plan_for(c->p).f; }
// queues the sample of U into dst[MON_NQ] (device); clk != 0: the record that decides, on the device, whether it is taken
int monitor_queue(rgpu_ctx* c, const double* U, const StepClock* clk, double* dst) {
#ifdef RGPU_TILED_MONITOR3D
  return rgpu_tiled::launch_monitor_vol(c->stream, c->g, U, clk, c->F, dst);
#else
  // one plane: its V[0] is the result bit for bit (kernels_monitor.h, below the summation order) -- written to dst, no finish launch
  const int nz = mon_nplanes(c->g);
  double* cols = c->F;
  double* V = nz == 1 ? dst : cols + (size_t)MON_NQ * nz * c->g.nx;
  const unsigned ncols = (unsigned)nz * (unsigned)c->g.nx;
  K_mon_vol_cols<true> k3d = {c->g, U, cols, clk};
  K_mon_vol_cols<false> k2d = {c->g, U, cols, clk};
  K_mon_vol_fold k2 = {c->g.nx, nz, cols, V, clk};
  if ((c->g.three_d ? rg_launch<kBlock>(c->stream, ncols, k3d) : rg_launch<kBlock>(c->stream, ncols, k2d)) || rg_launch<64>(c->stream, (unsigned)nz, k2)) return -1;
  if (nz == 1) return 0;
  K_mon_vol_finish k3 = {nz, V, dst, clk};
  return rg_launch<64>(c->stream, (unsigned)MON_NQ, k3);
#endif
}
// rgpu_state_monitor (want3d == 0) and rgpu_state_monitor3d: the same sample, each entry refusing the other's contexts in its own words
int state_monitor(rgpu_ctx* c, bool want3d, int parity, double* out) {
  RG_CHECK_CTX(c);
  const std::string who = want3d ? "state_monitor3d" : "state_monitor";
  if (!out || !c->U[0]) return fail(c, RGPU_EINVAL, who + ": null pointer / context without state");
  if ((c->g.three_d != 0) != want3d)
    return fail(c, RGPU_EUNSUPPORTED, who + (want3d ? ": 3D contexts only (2D contexts have rgpu_state_monitor)" : ": 2D contexts only (3D contexts have rgpu_state_monitor3d)"));
  if (want3d && c->p.slab_count > 1) return fail(c, RGPU_EINVAL, who + ": single-domain contexts only (a slab holds a part of the box)");
  if (!monitor_scratch_fits(c)) return fail(c, RGPU_EINVAL, who + (want3d ? ": no scratch for the partial sums" : ": no scratch for the segment sums"));
  double* dst = c->F + mon_scratch_doubles(c->g);
  double h[MON_NQ];
  if (monitor_queue(c, c->U[parity & 1], 0, dst) || rg_copy_d2h(h, dst, sizeof(h), c->stream) || rg_stream_sync(c->stream)) return RG_HIPFAIL(c, who);
  for (int q = 0; q < MON_NQ; ++q) out[q] = h[q];
  return RGPU_OK;
}

// ---- the plane monitor (kernels_monitor_planes.h): the same consumer with another sample, nz rows of MONP_NQ doubles ---------------
static_assert(MONP_NQ == RGPU_MONP_NQ, "include/rgpu.h states the width of a plane row");
// (also: whether the samples of this context can be taken inside its device-clock batches)
bool monitor_planes_scratch_fits(rgpu_ctx* c) {
  return c->F && c->g.three_d && monp_scratch_doubles(c->g) + monp_sample_doubles(c->g) <= (size_t)c->g.fN * plan_for(c->p).f;
}
// queues the rows of U into dst[nz][MONP_NQ] (device); clk != 0: the record that decides, on the device, whether they are taken
int monitor_planes_queue(rgpu_ctx* c, const double* U, const StepClock* clk, double* dst) {
#ifdef RGPU_TILED_MONITOR_PROFILE
  return rgpu_tiled::launch_monitor_profile(c->stream, c->g, U, clk, c->F, dst);
#else
  K_mon_prof_cols k1 = {c->g, U, c->F, clk};
  K_mon_prof_fold k2 = {c->g.nx, c->g.nz, c->F, dst, clk};
  return (rg_launch<kBlock>(c->stream, (unsigned)c->g.nz * (unsigned)c->g.nx, k1) || rg_launch<64>(c->stream, (unsigned)c->g.nz, k2)) ? -1 : 0;
#endif
}
int state_monitor_planes(rgpu_ctx* c, int parity, double* out) {
  RG_CHECK_CTX(c);
  const std::string who = "state_monitor_planes";
  if (!out || !c->U[0]) return fail(c, RGPU_EINVAL, who + ": null pointer / context without state");
  if (!c->g.three_d) return fail(c, RGPU_EUNSUPPORTED, who + ": 3D contexts only (the rows are the interior planes of a volume)");
  if (c->p.slab_count > 1) return fail(c, RGPU_EINVAL, who + ": single-domain contexts only (a slab holds a part of the box)");
  if (!monitor_planes_scratch_fits(c)) return fail(c, RGPU_EINVAL, who + ": no scratch for the partial sums");
  double* dst = c->F + monp_scratch_doubles(c->g);
  if (monitor_planes_queue(c, c->U[parity & 1], 0, dst) || rg_copy_d2h(out, dst, monp_sample_doubles(c->g) * sizeof(double), c->stream) || rg_stream_sync(c->stream))
    return RG_HIPFAIL(c, who);
  return RGPU_OK;
}

// ---- the map monitor (kernels_monitor_maps.h): the same consumer with a third sample, nmaps pictures of MAP_NQ channels ------------
static_assert(MAP_NQ == RGPU_MAP_NQ, "include/rgpu.h states the channels of a map");
// "" for a spec this context can take, else what is wrong with it
std::string map_spec_error(const rgpu_ctx* c, const rgpu_map_spec& s) {
  if (s.axis < 0 || s.axis > 2) return "axis must be 0 (x), 1 (y) or 2 (z)";
  const int n = s.axis == 0 ? c->g.nx : s.axis == 1 ? c->g.ny : c->g.nz;
  if (!(0 <= s.lo && s.lo < s.hi && s.hi <= n)) return "the range must satisfy 0 <= lo < hi <= " + std::to_string(n);
  return "";
}
size_t map_doubles(const rgpu_ctx* c, const rgpu_map_spec& s) { return (size_t)MAP_NQ * map_pixels(map_geom(c->g, s.axis, s.lo, s.hi)); }
size_t maps_sample_doubles(const rgpu_ctx* c, int nmaps, const rgpu_map_spec* specs) {
  size_t n = 0;
  for (int m = 0; m < nmaps; ++m) n += map_doubles(c, specs[m]);
  return n;
}
// what rgpu_state_maps and rgpu_run_steps_mapped refuse alike, in this order; 0: the maps can be taken
int maps_refusal(rgpu_ctx* c, const std::string& who, int nmaps, const rgpu_map_spec* specs) {
  if (!c->U[0]) return fail(c, RGPU_EINVAL, who + ": context without state");
  if (!c->g.three_d) return fail(c, RGPU_EUNSUPPORTED, who + ": 3D contexts only (the download of a 2D state is its map)");
  if (c->p.slab_count > 1) return fail(c, RGPU_EINVAL, who + ": single-domain contexts only (a slab holds a part of the box)");
  if (nmaps < 1 || nmaps > RGPU_MAP_MAX) return fail(c, RGPU_EINVAL, who + ": nmaps must be 1 .. " + std::to_string(RGPU_MAP_MAX));
  for (int m = 0; m < nmaps; ++m) {
    const std::string why = map_spec_error(c, specs[m]);
    if (!why.empty()) return fail(c, RGPU_EINVAL, who + ": map " + std::to_string(m) + ": " + why);
  }
  return RGPU_OK;
}
// the device buffer the kernels of the maps write to, at least `doubles` long: grown between two batches or two calls, when nothing
// is in flight.  != 0: it is not there
int map_log_reserve(rgpu_ctx* c, size_t doubles) {
  if (c->monm.allocated() && c->monm_doubles >= doubles) return 0;
  c->monm.release();
  c->monm_doubles = 0;
  if (c->monm.alloc(doubles) == 0 && rg_memset_async(c->monm.d, 0, doubles * sizeof(double), c->stream) == 0) {
    c->monm_doubles = doubles;
    return 0;
  }
  c->monm.release();   // zeroed, or not there
  return -1;
}
// the doubles the option "map_log_kib" gives the log of a batch
size_t map_log_budget_doubles() {
  const int kib = rgpu::options().map_log_kib;
  return kib > 0 ? (size_t)kib * (1024 / sizeof(double)) : 0;
}
// queues the maps of U one after another into dst (device), one launch each; clk != 0: the record that decides, on the device,
// whether they are taken.  The one place that knows whether the backend has kernels of its own
int maps_queue(rgpu_ctx* c, const double* U, const StepClock* clk, int nmaps, const rgpu_map_spec* specs, double* dst) {
  for (int m = 0; m < nmaps; ++m) {
    const rgpu_map_spec& s = specs[m];
#ifdef RGPU_TILED_MONITOR_MAPS
    if (rgpu_tiled::launch_monitor_map(c->stream, c->g, s.axis, s.lo, s.hi, rgpu::options().map_x_tiled, U, clk, dst)) return -1;
#else
    const MapGeom g = map_geom(c->g, s.axis, s.lo, s.hi);
    K_mon_map k = {c->g, g, U, dst, clk};
    if (rg_launch<kBlock>(c->stream, (unsigned)map_pixels(g), k)) return -1;
#endif
    dst += map_doubles(c, s);
  }
  return 0;
}
int state_maps(rgpu_ctx* c, int parity, int nmaps, const rgpu_map_spec* specs, double* out) {
  RG_CHECK_CTX(c);
  const std::string who = "state_maps";
  if (!out || !specs) return fail(c, RGPU_EINVAL, who + ": null pointer");
  if (const int rc = maps_refusal(c, who, nmaps, specs)) return rc;
  const size_t n = maps_sample_doubles(c, nmaps, specs);
  if (map_log_reserve(c, n)) return RG_HIPFAIL(c, who + ": device buffer of the maps");
  if (maps_queue(c, c->U[parity & 1], 0, nmaps, specs, c->monm.d) || rg_copy_d2h(out, c->monm.d, n * sizeof(double), c->stream) || rg_stream_sync(c->stream))
    return RG_HIPFAIL(c, who);
  return RGPU_OK;
}

// ---- the PDF monitor (kernels_monitor_pdf.h): the same consumer with a fourth sample, the tables of counts of npdfs specs ------------
static_assert(PDF_NQ == RGPU_PDF_NQ && PDF_MAX == RGPU_PDF_MAX && PDF_MAX_WORDS == RGPU_PDF_MAX_WORDS, "include/rgpu.h states the channels and the budgets of the PDFs");
// whether x is a normal power of two; *e: its biased exponent
bool pdf_pow2(double x, int* e) {
  unsigned long long u;
  std::memcpy(&u, &x, sizeof(u));
  *e = (int)(u >> 52);   // (with the sign bit: a negative number fails the range test)
  return (u & ((1ull << 52) - 1)) == 0 && *e >= 1 && *e <= 2046;
}
// "" for an axis that can be taken, else what is wrong with it
std::string pdf_axis_error(const rgpu_pdf_axis& a) {
  if (a.channel < 0 || a.channel >= RGPU_PDF_NQ) return "channel must be 0 .. " + std::to_string(RGPU_PDF_NQ - 1);
  if (a.nbins < 1 || a.nbins > RGPU_PDF_MAX_WORDS) return "nbins must be at least 1 (and within the word budget)";
  if (a.scale == 0) return std::isfinite(a.lo) && std::isfinite(a.hi) && a.lo < a.hi ? "" : "a linear range must be finite with lo < hi";
  if (a.scale != 1) return "scale must be 0 (linear) or 1 (octave bins)";
  int elo = 0, ehi = 0;
  if (!pdf_pow2(a.lo, &elo) || !pdf_pow2(a.hi, &ehi) || !(a.lo < a.hi)) return "an octave range must have normal powers of two lo < hi";
  if (a.sub < 0 || a.sub > 6) return "sub must be 0 .. 6";
  if (a.nbins != (ehi - elo) << a.sub) return "nbins must be (log2 hi - log2 lo) << sub = " + std::to_string((ehi - elo) << a.sub);
  return "";
}
// (of a spec whose axes can be taken)
size_t pdf_spec_words(const rgpu_pdf_spec& s) { return (size_t)(s.a.nbins + 3) * (s.b.nbins == 0 ? (size_t)1 : (size_t)(s.b.nbins + 3)); }
std::string pdf_spec_error(const rgpu_pdf_spec& s) {
  std::string why = pdf_axis_error(s.a);
  if (!why.empty()) return "axis a: " + why;
  if (s.b.nbins != 0 && !(why = pdf_axis_error(s.b)).empty()) return "axis b: " + why;
  if (pdf_spec_words(s) > (size_t)RGPU_PDF_MAX_WORDS) return "more than " + std::to_string(RGPU_PDF_MAX_WORDS) + " words";
  return "";
}
PdfAxis pdf_axis_make(const rgpu_pdf_axis& a) {
  PdfAxis d = {a.channel, a.scale, a.nbins, 0, a.lo, a.hi, 0.0, 0ull};
  if (a.scale == 0) d.inv = (double)a.nbins / (a.hi - a.lo);
  else {
    d.shift = 52 - a.sub;
    std::memcpy(&d.key0, &a.lo, sizeof(d.key0));
    d.key0 >>= d.shift;
  }
  return d;
}
// the slabs of one workgroup's counts the flux array holds (u32 words, two to a double)
size_t pdf_scratch_groups(const rgpu_ctx* c, const PdfSet& S) { return c->F ? (size_t)c->g.fN * plan_for(c->p).f * 2 / S.words : 0; }
// what rgpu_state_pdfs and rgpu_run_steps_pdfs refuse alike, in this order; 0: the tables can be taken, and *S is what the kernels read
int pdfs_refusal(rgpu_ctx* c, const std::string& who, int npdfs, const rgpu_pdf_spec* specs, PdfSet* S) {
  if (!c->U[0]) return fail(c, RGPU_EINVAL, who + ": context without state");
  if (!c->g.three_d) return fail(c, RGPU_EUNSUPPORTED, who + ": 3D contexts only");
  if (c->p.slab_count > 1) return fail(c, RGPU_EINVAL, who + ": single-domain contexts only (a slab holds a part of the box)");
  if (npdfs < 1 || npdfs > RGPU_PDF_MAX) return fail(c, RGPU_EINVAL, who + ": npdfs must be 1 .. " + std::to_string(RGPU_PDF_MAX));
  size_t words = 0;
  for (int m = 0; m < npdfs; ++m) {
    const std::string why = pdf_spec_error(specs[m]);
    if (!why.empty()) return fail(c, RGPU_EINVAL, who + ": pdf " + std::to_string(m) + ": " + why);
    PdfTable& t = S->t[m];
    t.a = pdf_axis_make(specs[m].a);
    t.joint = specs[m].b.nbins != 0;
    t.b = t.joint ? pdf_axis_make(specs[m].b) : t.a;
    t.base = (unsigned)words;
    t.pitch = t.joint ? (unsigned)(specs[m].b.nbins + 3) : 1u;
    words += pdf_spec_words(specs[m]);
  }
  if (words > (size_t)RGPU_PDF_MAX_WORDS) return fail(c, RGPU_EINVAL, who + ": the specs have " + std::to_string(words) + " words together, more than " + std::to_string(RGPU_PDF_MAX_WORDS));
  S->n = npdfs;
  S->words = (unsigned)words;
  if (pdf_scratch_groups(c, *S) < 1) return fail(c, RGPU_EINVAL, who + ": no scratch for the partial counts");
  return RGPU_OK;
}
// the device buffer the samples are stored to, at least `words` long: grown between two batches or two calls, when nothing is in
// flight.  Not zeroed: every word that is read was stored by the fold kernel.  != 0: it is not there
int pdf_log_reserve(rgpu_ctx* c, size_t words) {
  if (c->monh.allocated() && c->monh_words >= words) return 0;
  c->monh.release();
  c->monh_words = 0;
  if (c->monh.alloc(words)) return -1;
  c->monh_words = words;
  return 0;
}
// queues the tables of U into dst[S.words] (device, 64-bit counts); clk != 0: the record that decides, on the device, whether they are
// taken.  The one place that knows whether the backend has kernels of its own
int pdfs_queue(rgpu_ctx* c, const double* U, const StepClock* clk, const PdfSet& S, double* dst) {
  unsigned long long* out = reinterpret_cast<unsigned long long*>(dst);
#ifdef RGPU_TILED_MONITOR_PDF
  const unsigned groups = rgpu_tiled::pdf_groups(c->g, rgpu::options().pdf_groups, pdf_scratch_groups(c, S));
  return rgpu_tiled::launch_monitor_pdf(c->stream, c->g, S, rgpu_tiled::pdf_replicas(S.words, rgpu::options().pdf_replicas), groups, U, clk, reinterpret_cast<unsigned*>(c->F), out);
#else
  K_mon_pdf_zero k0 = {S.words, out, clk};
  K_mon_pdf k1 = {c->g, S, U, out, clk};
  return (rg_launch<kBlock>(c->stream, S.words, k0) || rg_launch<kBlock>(c->stream, pdf_rows(c->g) * (unsigned)c->g.nx, k1)) ? -1 : 0;
#endif
}
// one sample of U[parity] outside a batch, of a set that was not refused
int pdfs_take(rgpu_ctx* c, const std::string& who, int parity, const PdfSet& S, void* out) {
  if (pdf_log_reserve(c, S.words)) return RG_HIPFAIL(c, who + ": device buffer of the counts");
  if (pdfs_queue(c, c->U[parity & 1], 0, S, c->monh.d) || rg_copy_d2h(out, c->monh.d, S.words * sizeof(unsigned long long), c->stream) || rg_stream_sync(c->stream))
    return RG_HIPFAIL(c, who);
  return RGPU_OK;
}
int state_pdfs(rgpu_ctx* c, int parity, int npdfs, const rgpu_pdf_spec* specs, unsigned long long* out) {
  RG_CHECK_CTX(c);
  const std::string who = "state_pdfs";
  if (!out || !specs) return fail(c, RGPU_EINVAL, who + ": null pointer");
  PdfSet S;
  if (const int rc = pdfs_refusal(c, who, npdfs, specs, &S)) return rc;
  return pdfs_take(c, who, parity, S, out);
}

// ---- the spectrum monitor (kernels_monitor_spectrum.h): the same consumer with a fifth sample, 2 S doubles per spec -------------------
static_assert(SPEC_NQ == RGPU_SPECTRUM_NQ && SPEC_MAX == RGPU_SPECTRUM_MAX && SPEC_MAX_SHELLS == RGPU_SPECTRUM_MAX_SHELLS && SPEC_MAX_WEIGHT == RGPU_SPECTRUM_MAX_WEIGHT,
              "include/rgpu.h states the channels and the limits of the spectra");
// "" for a box the transforms can take, else what is wrong with it
std::string spectrum_box_error(const rgpu_ctx* c) {
  const int n[3] = {c->g.nx, c->g.ny, c->g.nz};
  for (int a = 0; a < 3; ++a)
    if (spec_log2(n[a]) < 0) return std::string("n") + "xyz"[a] + " = " + std::to_string(n[a]) + " is not a power of two in 4 .. 1024";
  return "";
}
// "" for a spec this context can take, else what is wrong with it (the box can be taken)
std::string spectrum_spec_error(const rgpu_ctx* c, const rgpu_spectrum_spec& s) {
  if (s.channels == 0) return "the channel mask is empty";
  if (s.channels >> RGPU_SPECTRUM_NQ) return "the channel mask has bits beyond the " + std::to_string(RGPU_SPECTRUM_NQ) + " channels";
  const int w[3] = {s.wx, s.wy, s.wz};
  for (int a = 0; a < 3; ++a)
    if (w[a] < 0 || w[a] > RGPU_SPECTRUM_MAX_WEIGHT) return std::string("w") + "xyz"[a] + " must be 0 .. " + std::to_string(RGPU_SPECTRUM_MAX_WEIGHT);
  if (s.wx == 0 && s.wy == 0 && s.wz == 0) return "the weights are all zero";
  const unsigned long long shells = spec_shell_count(spec_box(c->g), s.wx, s.wy, s.wz);
  if (shells > (unsigned long long)RGPU_SPECTRUM_MAX_SHELLS) return std::to_string(shells) + " shells, more than " + std::to_string(RGPU_SPECTRUM_MAX_SHELLS);
  return "";
}
// the shells of a spec on this context, 0 if the context or the spec is refused
int spectrum_shells(const rgpu_ctx* c, const rgpu_spectrum_spec* s) {
  if (!c || !s || !c->U[0] || !c->g.three_d || c->p.slab_count > 1 || !spectrum_box_error(c).empty() || !spectrum_spec_error(c, *s).empty()) return 0;
  return (int)spec_shell_count(spec_box(c->g), s->wx, s->wy, s->wz);
}
// the device buffer the samples are stored to, at least `doubles` long: grown between two batches or two calls, when nothing is in
// flight.  Not zeroed: every double that is read was stored by the last kernel of a sample.  != 0: it is not there
int spectrum_log_reserve(rgpu_ctx* c, size_t doubles) {
  if (c->mons.allocated() && c->mons_doubles >= doubles) return 0;
  c->mons.release();
  c->mons_doubles = 0;
  if (c->mons.alloc(doubles)) return -1;
  c->mons_doubles = doubles;
  return 0;
}
// the twiddle factors on the device: computed and uploaded by the first call that needs them, kept with the context
int spectrum_twiddles(rgpu_ctx* c) {
  if (c->montw.allocated()) return 0;
  if (c->montw.alloc(2 * (size_t)SPEC_TW)) return -1;
  spec_twiddle_table(c->montw.h);
  if (c->montw.upload(2 * (size_t)SPEC_TW, c->stream) == 0) return 0;
  c->montw.release();
  return -1;
}
// what rgpu_state_spectra and rgpu_run_steps_spectra refuse alike, in this order; 0: the spectra can be taken, and *S is what the kernels read
int spectra_refusal(rgpu_ctx* c, const std::string& who, int nspec, const rgpu_spectrum_spec* specs, SpecSet* S) {
  if (!c->U[0]) return fail(c, RGPU_EINVAL, who + ": context without state");
  if (!c->g.three_d) return fail(c, RGPU_EUNSUPPORTED, who + ": 3D contexts only");
  const std::string box = spectrum_box_error(c);
  if (!box.empty()) return fail(c, RGPU_EUNSUPPORTED, who + ": " + box);
  if (c->p.slab_count > 1) return fail(c, RGPU_EINVAL, who + ": single-domain contexts only (a slab holds a part of the box)");
  if (nspec < 1 || nspec > RGPU_SPECTRUM_MAX) return fail(c, RGPU_EINVAL, who + ": nspec must be 1 .. " + std::to_string(RGPU_SPECTRUM_MAX));
  const SpecBox b = spec_box(c->g);
  unsigned doubles = 0, most = 0;
  for (int m = 0; m < nspec; ++m) {
    const std::string why = spectrum_spec_error(c, specs[m]);
    if (!why.empty()) return fail(c, RGPU_EINVAL, who + ": spectrum " + std::to_string(m) + ": " + why);
    SpecOne& o = S->s[m];
    o.channels = specs[m].channels; o.wx = specs[m].wx; o.wy = specs[m].wy; o.wz = specs[m].wz;
    o.shells = (int)spec_shell_count(b, o.wx, o.wy, o.wz);
    o.base = doubles;
    doubles += 2u * (unsigned)o.shells;
    if ((unsigned)o.shells > most) most = (unsigned)o.shells;
  }
  S->n = nspec;
  S->doubles = doubles;
  if (!c->F || spec_scratch_doubles(b, most) > (size_t)c->g.fN * plan_for(c->p).f) return fail(c, RGPU_EINVAL, who + ": no scratch for the transform and the partial sums");
  if (spectrum_twiddles(c)) return RG_HIPFAIL(c, who + ": table of the twiddle factors");
  return RGPU_OK;
}
// queues the spectra of U into dst[S.doubles] (device); clk != 0: the record that decides, on the device, whether they are taken.  The
// one place that knows whether the backend has kernels of its own
int spectra_queue(rgpu_ctx* c, const double* U, const StepClock* clk, const SpecSet& S, double* dst) {
#ifdef RGPU_TILED_MONITOR_SPECTRUM
  return rgpu_tiled::launch_monitor_spectrum(c->stream, c->g, S, rgpu::options().spectrum_tile_y, U, c->montw.d, clk, c->F, dst);
#else
  const SpecBox b = spec_box(c->g);
  const double N = (double)b.nx * (double)b.ny * (double)b.nz;
  for (int m = 0; m < S.n; ++m) {
    int ca[SPEC_NQ], cb[SPEC_NQ];
    const int nt = spec_pairs(S.s[m].channels, ca, cb);
    for (int t = 0; t < nt; ++t) {
      K_mon_spectrum_x kx = {c->g, b, ca[t], cb[t], U, c->montw.d, c->F, clk};
      K_mon_spectrum_line ky = {b, 1, c->montw.d, c->F, clk};
      K_mon_spectrum_line kz = {b, 2, c->montw.d, c->F, clk};
      K_mon_spectrum_bin kb = {b, S.s[m], t == 0 ? 1 : 0, 1.0 / (N * N), c->F, dst, clk};
      if (rg_launch<kBlock>(c->stream, (unsigned)(b.ny * b.nz), kx) || rg_launch<kBlock>(c->stream, (unsigned)(b.nx * b.nz), ky) || rg_launch<kBlock>(c->stream, (unsigned)(b.nx * b.ny), kz) ||
          rg_launch<kBlock>(c->stream, (unsigned)S.s[m].shells, kb))
        return -1;
    }
  }
  return 0;
#endif
}
// one sample of U[parity] outside a batch, of a set that was not refused
int spectra_take(rgpu_ctx* c, const std::string& who, int parity, const SpecSet& S, double* out) {
  if (spectrum_log_reserve(c, S.doubles)) return RG_HIPFAIL(c, who + ": device buffer of the spectra");
  if (spectra_queue(c, c->U[parity & 1], 0, S, c->mons.d) || rg_copy_d2h(out, c->mons.d, S.doubles * sizeof(double), c->stream) || rg_stream_sync(c->stream))
    return RG_HIPFAIL(c, who);
  return RGPU_OK;
}
int state_spectra(rgpu_ctx* c, int parity, int nspec, const rgpu_spectrum_spec* specs, double* out) {
  RG_CHECK_CTX(c);
  const std::string who = "state_spectra";
  if (!out || !specs) return fail(c, RGPU_EINVAL, who + ": null pointer");
  SpecSet S;
  if (const int rc = spectra_refusal(c, who, nspec, specs, &S)) return rc;
  return spectra_take(c, who, parity, S, out);
}

// ---- the Helmholtz spectra (kernels_monitor_helm.h): the same consumer with a sixth sample, 3 S doubles per spec ----------------------
static_assert(HELM_NF == RGPU_HELM_NF && HELM_MAX == RGPU_HELM_MAX, "include/rgpu.h states the fields and the limits of the Helmholtz spectra");
// "" for a spec this context can take, else what is wrong with it (the box can be taken)
std::string helm_spec_error(const rgpu_ctx* c, const rgpu_helm_spec& s) {
  if (s.field < 0 || s.field >= RGPU_HELM_NF) return "field must be 0 .. " + std::to_string(RGPU_HELM_NF - 1);
  const int w[3] = {s.wx, s.wy, s.wz};
  for (int a = 0; a < 3; ++a) {
    if (w[a] == 0) return std::string("w") + "xyz"[a] + " is zero (the weights give the wave vector its direction)";
    if (w[a] < 0 || w[a] > RGPU_SPECTRUM_MAX_WEIGHT) return std::string("w") + "xyz"[a] + " must be 1 .. " + std::to_string(RGPU_SPECTRUM_MAX_WEIGHT);
  }
  const unsigned long long shells = spec_shell_count(spec_box(c->g), s.wx, s.wy, s.wz);
  if (shells > (unsigned long long)RGPU_SPECTRUM_MAX_SHELLS) return std::to_string(shells) + " shells, more than " + std::to_string(RGPU_SPECTRUM_MAX_SHELLS);
  return "";
}
// the shells of a spec on this context, 0 if the context or the spec is refused
// the doubles of the flux array, the scratch of a sample
size_t helm_scratch_capacity(const rgpu_ctx* c) { return c->F ? (size_t)c->g.fN * plan_for(c->p).f : 0; }
int helm_shells(const rgpu_ctx* c, const rgpu_helm_spec* s) {
  if (!c || !s || !c->U[0] || !c->g.three_d || c->p.slab_count > 1 || !spectrum_box_error(c).empty() || !helm_spec_error(c, *s).empty()) return 0;
  const SpecBox b = spec_box(c->g);
  const unsigned shells = (unsigned)spec_shell_count(b, s->wx, s->wy, s->wz);
  return helm_bin_groups(b, shells, helm_scratch_capacity(c)) ? (int)shells : 0;   // (refused for its scratch: refused)
}
// the device buffer the samples are stored to: spectrum_log_reserve for a buffer of their own
int helm_log_reserve(rgpu_ctx* c, size_t doubles) {
  if (c->monv.allocated() && c->monv_doubles >= doubles) return 0;
  c->monv.release();
  c->monv_doubles = 0;
  if (c->monv.alloc(doubles)) return -1;
  c->monv_doubles = doubles;
  return 0;
}
// what rgpu_state_helm_spectra and rgpu_run_steps_helm_spectra refuse alike, in the order of spectra_refusal; 0: the spectra can be
// taken, and *S is what the kernels read
int helm_refusal(rgpu_ctx* c, const std::string& who, int nspec, const rgpu_helm_spec* specs, HelmSet* S) {
  if (!c->U[0]) return fail(c, RGPU_EINVAL, who + ": context without state");
  if (!c->g.three_d) return fail(c, RGPU_EUNSUPPORTED, who + ": 3D contexts only");
  const std::string box = spectrum_box_error(c);
  if (!box.empty()) return fail(c, RGPU_EUNSUPPORTED, who + ": " + box);
  if (c->p.slab_count > 1) return fail(c, RGPU_EINVAL, who + ": single-domain contexts only (a slab holds a part of the box)");
  if (nspec < 1 || nspec > RGPU_HELM_MAX) return fail(c, RGPU_EINVAL, who + ": nspec must be 1 .. " + std::to_string(RGPU_HELM_MAX));
  const SpecBox b = spec_box(c->g);
  unsigned doubles = 0;
  for (int m = 0; m < nspec; ++m) {
    const std::string why = helm_spec_error(c, specs[m]);
    if (!why.empty()) return fail(c, RGPU_EINVAL, who + ": spectrum " + std::to_string(m) + ": " + why);
    HelmOne& o = S->s[m];
    o.field = specs[m].field; o.wx = specs[m].wx; o.wy = specs[m].wy; o.wz = specs[m].wz;
    o.shells = (int)spec_shell_count(b, o.wx, o.wy, o.wz);
    o.base = doubles;
    doubles += 3u * (unsigned)o.shells;
    S->groups[m] = helm_bin_groups(b, (unsigned)o.shells, helm_scratch_capacity(c));
    if (S->groups[m] == 0) return fail(c, RGPU_EINVAL, who + ": spectrum " + std::to_string(m) + ": no scratch for the three transforms and the partial sums");
  }
  S->n = nspec;
  S->doubles = doubles;
  if (spectrum_twiddles(c)) return RG_HIPFAIL(c, who + ": table of the twiddle factors");
  return RGPU_OK;
}
// queues the Helmholtz spectra of U into dst[S.doubles] (device); clk as for spectra_queue.  The one place that knows whether the
// backend has kernels of its own
int helm_queue(rgpu_ctx* c, const double* U, const StepClock* clk, const HelmSet& S, double* dst) {
#ifdef RGPU_TILED_MONITOR_HELM
  return rgpu_tiled::launch_monitor_helm(c->stream, c->g, S, rgpu::options().spectrum_tile_y, U, c->montw.d, clk, c->F, dst);
#else
  const SpecBox b = spec_box(c->g);
  const size_t cells = (size_t)b.nx * b.ny * b.nz;
  const double N = (double)cells;
  for (int m = 0; m < S.n; ++m) {
    for (int a = 0; a < 3; ++a) {
      double* Z = c->F + 2 * cells * (size_t)a;
      K_mon_spectrum_x kx = {c->g, b, helm_first_channel(S.s[m].field) + a, -1, U, c->montw.d, Z, clk};
      K_mon_spectrum_line ky = {b, 1, c->montw.d, Z, clk};
      K_mon_spectrum_line kz = {b, 2, c->montw.d, Z, clk};
      if (rg_launch<kBlock>(c->stream, (unsigned)(b.ny * b.nz), kx) || rg_launch<kBlock>(c->stream, (unsigned)(b.nx * b.nz), ky) || rg_launch<kBlock>(c->stream, (unsigned)(b.nx * b.ny), kz)) return -1;
    }
    K_mon_helm_bin kb = {b, S.s[m], 1.0 / (N * N), c->F, c->F + 2 * cells, c->F + 4 * cells, dst, clk};
    if (rg_launch<kBlock>(c->stream, (unsigned)S.s[m].shells, kb)) return -1;
  }
  return 0;
#endif
}
// one sample of U[parity] outside a batch, of a set that was not refused
int helm_take(rgpu_ctx* c, const std::string& who, int parity, const HelmSet& S, double* out) {
  if (helm_log_reserve(c, S.doubles)) return RG_HIPFAIL(c, who + ": device buffer of the spectra");
  if (helm_queue(c, c->U[parity & 1], 0, S, c->monv.d) || rg_copy_d2h(out, c->monv.d, S.doubles * sizeof(double), c->stream) || rg_stream_sync(c->stream))
    return RG_HIPFAIL(c, who);
  return RGPU_OK;
}
int state_helm_spectra(rgpu_ctx* c, int parity, int nspec, const rgpu_helm_spec* specs, double* out) {
  RG_CHECK_CTX(c);
  const std::string who = "state_helm_spectra";
  if (!out || !specs) return fail(c, RGPU_EINVAL, who + ": null pointer");
  HelmSet S;
  if (const int rc = helm_refusal(c, who, nspec, specs, &S)) return rc;
  return helm_take(c, who, parity, S, out);
}

// ---- the samples of a batch: of the monitor, of the plane, map, PDF or spectrum monitor, or of the Helmholtz spectra ------------------
// which sample a call takes (and, for maps and PDFs, of what).  Samples are 8-byte words, doubles or counts: the loop only copies them
enum MonWhat { MON_MONITOR, MON_PLANES, MON_MAPS, MON_PDFS, MON_SPECTRA, MON_HELM };
struct MonSample { MonWhat what; int nmaps; const rgpu_map_spec* specs; const PdfSet* pdf; const SpecSet* spec; const HelmSet* helm; };
size_t monitor_sample_doubles(const rgpu_ctx* c, const MonSample& S) {
  if (S.what == MON_HELM) return (size_t)S.helm->doubles;
  if (S.what == MON_SPECTRA) return (size_t)S.spec->doubles;
  if (S.what == MON_PDFS) return (size_t)S.pdf->words;
  return S.what == MON_MAPS ? maps_sample_doubles(c, S.nmaps, S.specs) : S.what == MON_PLANES ? monp_sample_doubles(c->g) : (size_t)MON_NQ;
}
// whether the samples of this context can be taken inside its device-clock batches.  Maps need no scratch: one sample within the
// budget.  PDFs and both kinds of spectra: their scratch was checked with the specs
bool monitor_sample_fits(rgpu_ctx* c, const MonSample& S) {
  if (S.what == MON_PDFS || S.what == MON_SPECTRA || S.what == MON_HELM) return true;
  if (S.what == MON_MAPS) return c->g.three_d && monitor_sample_doubles(c, S) <= map_log_budget_doubles();
  return S.what == MON_PLANES ? monitor_planes_scratch_fits(c) : monitor_scratch_fits(c);
}
DeviceMirror<double>& monitor_batch_log(rgpu_ctx* c, const MonSample& S) { return S.what == MON_HELM ? c->monv : S.what == MON_SPECTRA ? c->mons : S.what == MON_PDFS ? c->monh : S.what == MON_MAPS ? c->monm : S.what == MON_PLANES ? c->monp : c->mon; }
// The slots of the log of a call that samples every `every` steps.  The monitor's: a slot per step of a batch.  The plane monitor's:
// a slot per sample that can fall into one batch.  The maps': as many, or as the budget holds if that is fewer (at least one:
// monitor_sample_fits)
size_t monitor_batch_slots(const rgpu_ctx* c, const MonSample& S, int every) {
  if (S.what == MON_MONITOR) return (size_t)rgpu_ctx::kClockBatch;
  const size_t slots = (size_t)rgpu_ctx::kClockBatch / (size_t)every + 1;
  if (S.what == MON_PLANES || S.what == MON_PDFS || S.what == MON_SPECTRA || S.what == MON_HELM) return slots;   // (a PDF sample is at most 128 KiB, the spectra 256 KiB, the Helmholtz spectra 384 KiB: no byte budget)
  const size_t held = map_log_budget_doubles() / monitor_sample_doubles(c, S);
  return held < slots ? held : slots;
}
// How many of the m steps behind step n0 a batch takes: it ends at the last step before the (slots + 1)-th step that is due, so that
// it holds no more samples than its log has slots (all m where the log has a slot for every sample of a full batch)
int monitor_batch_steps(const rgpu_ctx* c, const MonSample& S, int every, int n0, int m) {
  const long long over = ((long long)(n0 / every) + 1 + (long long)monitor_batch_slots(c, S, every)) * every;
  return over - 1 - n0 < m ? (int)(over - 1 - n0) : m;
}
// The log: grown (between two batches: nothing is in flight) if this call needs more than the last did
int monitor_batch_alloc(rgpu_ctx* c, const MonSample& S, int every) {
  const size_t slots = monitor_batch_slots(c, S, every);
  const size_t n = slots * monitor_sample_doubles(c, S);
  if (S.what == MON_MAPS) return map_log_reserve(c, n);
  if (S.what == MON_PDFS) return pdf_log_reserve(c, n);
  if (S.what == MON_SPECTRA) return spectrum_log_reserve(c, n);
  if (S.what == MON_HELM) return helm_log_reserve(c, n);
  DeviceMirror<double>& log = monitor_batch_log(c, S);
  if (S.what == MON_PLANES && log.allocated() && c->monp_slots < slots) log.release();
  if (log.allocated()) return 0;
  if (log.alloc(n) == 0 && rg_memset_async(log.d, 0, n * sizeof(double), c->stream) == 0) {
    if (S.what == MON_PLANES) c->monp_slots = slots;
    return 0;
  }
  log.release();   // zeroed, or not there
  return -1;
}
// Queues, behind the last kernel of the step whose record is c->clk_cur, the sample of U[parity], the state that step leaves: into
// slot k of the log -- k samples were queued in the open batch before it -- if the record says that the step ran.
int monitor_batch_queue(rgpu_ctx* c, const MonSample& S, int parity, int k) {
  double* dst = monitor_batch_log(c, S).d + (size_t)k * monitor_sample_doubles(c, S);
  const double* U = c->U[parity & 1];
  const int rc = S.what == MON_HELM ? helm_queue(c, U, c->clk_cur, *S.helm, dst) : S.what == MON_SPECTRA ? spectra_queue(c, U, c->clk_cur, *S.spec, dst) : S.what == MON_PDFS ? pdfs_queue(c, U, c->clk_cur, *S.pdf, dst) : S.what == MON_MAPS ? maps_queue(c, U, c->clk_cur, S.nmaps, S.specs, dst)
               : S.what == MON_PLANES ? monitor_planes_queue(c, U, c->clk_cur, dst) : monitor_queue(c, U, c->clk_cur, dst);
  if (rc == 0) ++(S.what == MON_HELM ? c->monv_samples : S.what == MON_SPECTRA ? c->mons_samples : S.what == MON_PDFS ? c->monh_samples : S.what == MON_MAPS ? c->monm_samples : S.what == MON_PLANES ? c->monp_samples : c->mon_samples);
  return rc;
}

}  // namespace
