#include "run_driver.h"
#include "hdf5_io.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <iterator>
#include <limits>
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <iomanip>
#include <iostream>
#include <sstream>
#include <stdexcept>

#include "init_conditions.h"

namespace rgpu_host {

GodunovRun::GodunovRun(const IniConfig& cfg, int slab_rank, int slab_count)
    : cfg_(cfg), ctx_(0), totalTime_(0.0), restart_has_ghosts_(false), warned_no_hdf5_(false), wrote_hdf5_(false), hooked_(false),
      noted_vtk_(false), noted_hist_(false) {
  std::memset(&hooks_, 0, sizeof(hooks_));
  params_from_config(cfg_, slab_rank, slab_count, &p_, &rs_);
  const int rc = rgpu_create(&p_, &ctx_);
  if (rc) {
    const std::string msg = ctx_ ? rgpu_last_error(ctx_) : "allocation failure";
    if (ctx_) rgpu_destroy(ctx_);
    ctx_ = 0;
    throw std::runtime_error("rgpu_create: " + msg);
  }
  h_U_.assign(rgpu_state_elems(&p_), 0.0);
}

GodunovRun::~GodunovRun() {
  if (ctx_) rgpu_destroy(ctx_);
}

void GodunovRun::check(int rc, const char* what) {
  if (rc) throw std::runtime_error(std::string(what) + ": " + rgpu_last_error(ctx_));
}

int GodunovRun::init_simulation() {
  int timeStep = 0;
  if (rs_.restartEnabled) {
    // restart run (HydroRunBase.cpp:7033-7066): the state comes from a file of an earlier run instead of the problem's
    // initial condition; the static gravity / forcing fields below are rebuilt as in a fresh run.  The reference reads
    // HDF5 (inputHdf5, :4818-5160): so does this driver for a .h5 name (hdf5_io.h, libhdf5 bound at run time); it also resumes
    // from its raw .rgr dump and from the .vti it writes (interior cells, raw doubles, step count and time in the header).
    std::fill(h_U_.begin(), h_U_.end(), 0.0);
    const std::string path = rs_.outputDir + "/" + rs_.restartFilename;
    restart_has_ghosts_ = false;
    const bool h5 = path.size() > 3 && path.substr(path.size() - 3) == ".h5";
    const bool dump = h5 || (path.size() > 4 && path.substr(path.size() - 4) == ".rgr");
    if (rs_.restartUpscale && slab()) throw std::runtime_error("restart_upscale is single-domain only");
    if (rs_.restartUpscale) {
      if (!dump) throw std::runtime_error("restart_upscale reads an .h5 file or a .rgr dump ([output] outputHdf5=yes in the coarse run)");
      if (p_.nx % 2 || p_.ny % 2 || (p_.nz_global != 1 && p_.nz % 2)) throw std::runtime_error("restart_upscale: nx, ny, nz must be even");
      inputRestartUpscaled(path, &restart_has_ghosts_);   // timeStep stays 0; the forcing process starts afresh (:7084-7088)
    } else {
      timeStep = dump ? inputRestart(path, &restart_has_ghosts_) : inputVtk(path);
      restore_forcing_process(timeStep);
    }
    std::cout << "### This is a restarted run ! Current time is " << totalTime_ << " (step " << timeStep << ") ###\n";
  } else {
    init_condition(cfg_, p_, h_U_.data());
  }
  check(rgpu_upload(ctx_, h_U_.data(), 1), "upload");
  if (p_.gravityEnabled == 2) {   // h_gravity of the problem, copied to the device once (d_gravity.copyFromHost)
    std::vector<double> hG(3 * (h_U_.size() / p_.nbVar));
    if (init_gravity_field(cfg_, p_, hG.data())) check(rgpu_set_gravity_field(ctx_, hG.data()), "set_gravity_field");
  }
  if (p_.randomForcingEnabled) {   // h_randomForcing -> d_randomForcing (HydroRunBase.cpp:7199-7209)
    std::vector<double> hF(3 * (h_U_.size() / p_.nbVar));
    if (init_forcing_field(cfg_, p_, hF.data())) check(rgpu_set_forcing_field(ctx_, hF.data()), "set_forcing_field");
  }
  return timeStep;
}

// collective outcome of a step that can fail on one rank alone: every rank throws if any rank failed
void GodunovRun::agree_or_throw(const std::string& local_error, const char* what) {
  if (!hooked_) { if (!local_error.empty()) throw std::runtime_error(local_error); return; }
  if (!hooks_.agree) {   // an older slab driver: barrier only (a failing rank then throws alone)
    if (!local_error.empty()) throw std::runtime_error(local_error);
    hook_check(hooks_.barrier(hooks_.self), "barrier");
    return;
  }
  const int failed = hooks_.agree(hooks_.self, local_error.empty() ? 0 : 1);
  if (failed < 0) hook_check(failed, what);
  if (failed > 0) {
    std::ostringstream m;
    m << what << ": " << failed << " of " << p_.slab_count << " ranks failed";
    if (!local_error.empty()) m << "; this rank (" << p_.slab_rank << "): " << local_error;
    throw std::runtime_error(m.str());
  }
}

void GodunovRun::hook_check(int rc, const char* what) {
  if (rc) throw std::runtime_error(std::string(what) + ": " + (hooks_.last_error ? hooks_.last_error(hooks_.self) : "slab driver error"));
}
void GodunovRun::note_once(bool* flag, const char* msg) {
  if (!*flag && p_.slab_rank == 0) std::cerr << msg << "\n";
  *flag = true;
}

void GodunovRun::make_all_boundaries(int parity) {
  if (hooked_) { hook_check(hooks_.make_all_boundaries(hooks_.self, parity, totalTime_, 0.0), "make_all_boundaries"); return; }
  check(rgpu_make_all_boundaries(ctx_, parity, totalTime_, 0.0), "make_all_boundaries");
}

double GodunovRun::compute_dt(int useU) {
  if (hooked_) { double d = 0.0; hook_check(hooks_.compute_dt(hooks_.self, useU, &d), "compute_dt"); return d; }
  const double dt = rgpu_compute_dt(ctx_, useU);
  if (!(dt == dt)) throw std::runtime_error(std::string("compute_dt: ") + rgpu_last_error(ctx_));
  return dt;
}

void GodunovRun::godunov_unsplit(int nStep, double dt) { check(rgpu_godunov_unsplit(ctx_, nStep, dt, totalTime_), "godunov_unsplit"); }

// MHDRunGodunov.cpp:4077-4089 / HydroRunGodunov.cpp:4082-4126 (unsplit branch)
void GodunovRun::oneStepIntegration(int& nStep, double& t, double& dt) {
  if (hooked_) { hook_check(hooks_.one_step_integration(hooks_.self, &nStep, &t, &dt), "oneStepIntegration"); return; }
  dt = compute_dt(nStep % 2);
  godunov_unsplit(nStep, dt);
  nStep++;
  t += dt;
}

void GodunovRun::copyGpuToCpu(int nStep) { check(rgpu_download(ctx_, h_U_.data(), nStep % 2), "download"); }

// Hand-written VTI writer of the reference (HydroRunBase.cpp:2681-2995): ImageData, PointData, appended raw
// little-endian Float64, one uint32 byte count per array, INTERIOR cells only, names density..bz -- the reference's bytes.
void GodunovRun::outputVtk(int nStep) {
  static const char* names[8] = {"density", "energy", "mx", "my", "mz", "bx", "by", "bz"};
  const int gw = p_.ghostWidth, nx = p_.nx, ny = p_.ny;
  const bool three_d = p_.nz_global != 1;
  const int nz = three_d ? p_.nz : 1;
  const size_t isize = nx + 2 * gw, jsize = ny + 2 * gw, ksize = three_d ? nz + 2 * gw : 1;
  const size_t ncell = isize * jsize * ksize;
  std::ostringstream fn;
  fn << rs_.outputDir << "/" << rs_.outputPrefix << "_" << std::setw(7) << std::setfill('0') << nStep << ".vti";
  std::ofstream out(fn.str().c_str(), std::ios::binary);
  if (!out) throw std::runtime_error("cannot write " + fn.str());
  if (rs_.outputVtkAscii) {   // [output] outputVtkAscii=yes: the reference's text form, byte for byte (HydroRunBase.cpp:2919-2973)
    out << "<?xml version=\"1.0\"?>\n<VTKFile type=\"ImageData\" version=\"0.1\" byte_order=\"LittleEndian\">\n";
    out << "  <ImageData WholeExtent=\"0 " << nx - 1 << " 0 " << ny - 1 << " 0 " << nz - 1 << "\" Origin=\"0 0 0\" Spacing=\"1 1 1\">\n";
    out << "  <Piece Extent=\"0 " << nx - 1 << " 0 " << ny - 1 << " 0 " << nz - 1 << "\">\n    <PointData>\n";
    for (int v = 0; v < p_.nbVar; ++v) {
      const char* nm = (p_.nbVar == 4 && v == 3) ? "my" : names[v];
      out << "      <DataArray type=\"Float64\" Name=\"" << nm << "\" format=\"ascii\" >\n";
      for (int k = 0; k < nz; ++k)
        for (int j = 0; j < ny; ++j) {
          const size_t kk = three_d ? k + gw : 0;
          const double* src = &h_U_[(gw) + isize * ((j + gw) + jsize * kk) + ncell * v];
          for (int i = 0; i < nx; ++i) out << std::setprecision(12) << src[i] << " ";
          out << "\n";
        }
      out << "      </DataArray>\n";
    }
    out << "    </PointData>\n    <CellData>\n    </CellData>\n  </Piece>\n  </ImageData>\n</VTKFile>\n";
    return;
  }
  // appended raw doubles: the bytes of the reference's file (no XML declaration in this mode), followed by ONE comment line
  // with what a restart needs besides the fields (the reference keeps them as HDF5 attributes "time step" / "total time")
  // the format's per-array byte count is a uint32 (the reference's files: HydroRunBase.cpp:2974-2995): >= 4 GiB per variable cannot
  // be described -- say so instead of writing a corrupt header (HDF5 output has no such limit)
  if (sizeof(double) * (size_t)nx * ny * nz > UINT32_MAX)
    throw std::runtime_error("outputVtk: " + std::to_string(sizeof(double) * (size_t)nx * ny * nz) + " bytes per variable exceed the uint32 byte count of the "
                             "appended-raw .vti format; use [output] outputHdf5=yes (or outputVtkAscii=yes) for this box");
  const uint32_t nbytes = static_cast<uint32_t>(sizeof(double) * nx * ny * nz);
  out << "<VTKFile type=\"ImageData\" version=\"0.1\" byte_order=\"LittleEndian\">\n";
  out << "  <ImageData WholeExtent=\"0 " << nx - 1 << " 0 " << ny - 1 << " 0 " << nz - 1 << "\" Origin=\"0 0 0\" Spacing=\"1 1 1\">\n";
  out << "  <Piece Extent=\"0 " << nx - 1 << " 0 " << ny - 1 << " 0 " << nz - 1 << "\">\n    <PointData>\n";
  for (int v = 0; v < p_.nbVar; ++v) {
    const char* nm = (p_.nbVar == 4 && v == 3) ? "my" : names[v];
    out << "     <DataArray type=\"Float64\" Name=\"" << nm << "\" format=\"appended\" offset=\""
        << static_cast<size_t>(v) * (nbytes + sizeof(uint32_t)) << "\" />\n";
  }
  out << "    </PointData>\n    <CellData>\n    </CellData>\n  </Piece>\n  </ImageData>\n  <AppendedData encoding=\"raw\">\n_";
  std::vector<double> line(nx);
  for (int v = 0; v < p_.nbVar; ++v) {
    out.write(reinterpret_cast<const char*>(&nbytes), sizeof(nbytes));
    for (int k = 0; k < nz; ++k)
      for (int j = 0; j < ny; ++j) {
        const size_t kk = three_d ? k + gw : 0;
        const double* src = &h_U_[(gw) + isize * ((j + gw) + jsize * kk) + ncell * v];
        out.write(reinterpret_cast<const char*>(src), sizeof(double) * nx);
      }
  }
  out << "  </AppendedData>\n</VTKFile>\n";
  char tail[160];
  std::snprintf(tail, sizeof(tail), "<!-- rgpu restart: nStep=%d totalTime=%a (%.17g) -->\n", nStep, totalTime_, totalTime_);
  out << tail;
}

// z-slab runs: HydroRunBaseMpi::outputVtk, hand-written branch (HydroRunBaseMpi.cpp:4167-4790) for the 1 x 1 x N topology of the
// slab driver -- every rank writes <prefix>_time<step>_mpi<rank>.vti with its own planes (ranks > 0: plus the plane below, the
// one-cell overlap the parallel image-data format wants), rank 0 the index <prefix>_time<step>.pvti.  Appended raw doubles or,
// [output] outputVtkAscii, text with the stream's default precision (the MPI writer sets none).
void GodunovRun::outputVtkSlab(int nStep) {
  static const char* names[8] = {"density", "energy", "mx", "my", "mz", "bx", "by", "bz"};
  const int gw = p_.ghostWidth, nx = p_.nx, ny = p_.ny, nz = p_.nz, rank = p_.slab_rank, count = p_.slab_count;
  const size_t isize = nx + 2 * gw, jsize = ny + 2 * gw, ksize = nz + 2 * gw;
  const size_t ncell = isize * jsize * ksize;
  std::ostringstream ts, rk;
  ts << std::setw(7) << std::setfill('0') << nStep;
  rk << std::setw(5) << std::setfill('0') << rank;
  const std::string stem = rs_.outputPrefix + "_time" + ts.str();
  std::string local_error;
  try {
    if (rank == 0) {
      const std::string hn = rs_.outputDir + "/" + stem + ".pvti";
      std::ofstream h(hn.c_str());
      if (!h) throw std::runtime_error("cannot write " + hn);
      h << "<?xml version=\"1.0\"?>\n<VTKFile type=\"PImageData\" version=\"0.1\" byte_order=\"LittleEndian\">\n";
      h << "  <PImageData WholeExtent=\"0 " << nx - 1 << " 0 " << ny - 1 << " 0 " << count * nz - 1
        << "\" GhostLevel=\"0\" Origin=\"0 0 0\" Spacing=\"1 1 1\">\n    <PPointData Scalars=\"Scalars_\">\n";
      for (int v = 0; v < p_.nbVar; ++v) h << "      <PDataArray type=\"Float64\" Name=\"" << names[v] << "\"/>\n";
      h << "    </PPointData>\n";
      for (int r = 0; r < count; ++r) {
        std::ostringstream pr;
        pr << std::setw(5) << std::setfill('0') << r;
        h << " <Piece Extent=\"0 " << nx - 1 << " 0 " << ny - 1 << " ";
        if (r == 0) h << 0 << " " << nz - 1 << " ";
        else h << r * nz - 1 << " " << r * nz + nz - 1 << " ";
        h << "\" Source=\"" << stem << "_mpi" << pr.str() << ".vti\"/>\n";
      }
      h << "</PImageData>\n</VTKFile>\n";
    }
    const std::string fn = rs_.outputDir + "/" + stem + "_mpi" + rk.str() + ".vti";
    std::ofstream out(fn.c_str(), std::ios::binary);
    if (!out) throw std::runtime_error("cannot write " + fn);
    const int zlo = (rank == 0) ? 0 : rank * nz - 1, zhi = (rank == 0) ? nz - 1 : rank * nz + nz - 1;
    const int k0 = (rank == 0) ? gw : gw - 1, k1 = (int)ksize - gw;   // array planes [k0, k1)
    if (rs_.outputVtkAscii) out << "<?xml version=\"1.0\"?>\n";
    out << "<VTKFile type=\"ImageData\" version=\"0.1\" byte_order=\"LittleEndian\">\n";
    out << "  <ImageData WholeExtent=\"0 " << nx - 1 << " 0 " << ny - 1 << " " << zlo << " " << zhi << "\" Origin=\"0 0 0\" Spacing=\"1 1 1\">\n";
    out << "  <Piece Extent=\"0 " << nx - 1 << " 0 " << ny - 1 << " " << zlo << " " << zhi << "\">\n    <PointData>\n";
    if (rs_.outputVtkAscii) {
      for (int v = 0; v < p_.nbVar; ++v) {
        out << "      <DataArray type=\"Float64\" Name=\"" << names[v] << "\" format=\"ascii\">\n";
        for (int k = k0; k < k1; ++k)
          for (int j = gw; j < (int)jsize - gw; ++j) {
            const double* src = &h_U_[gw + isize * (j + jsize * (size_t)k) + ncell * v];
            for (int i = 0; i < nx; ++i) out << src[i] << " ";
            out << "\n";
          }
        out << "      </DataArray>\n";
      }
      out << "    </PointData>\n    <CellData>\n    </CellData>\n  </Piece>\n  </ImageData>\n</VTKFile>\n";
    } else {
      const size_t tuples = (size_t)nx * ny * (size_t)(k1 - k0);
      if (tuples * sizeof(double) > UINT32_MAX)   // caught below: every rank then fails the output step together (hooks.agree)
        throw std::runtime_error("outputVtk: " + std::to_string(tuples * sizeof(double)) + " bytes per variable in this rank's piece exceed the uint32 byte "
                                 "count of the appended-raw .vti format; use [output] outputHdf5=yes for this box");
      const uint32_t nbytes = static_cast<uint32_t>(tuples * sizeof(double));
      for (int v = 0; v < p_.nbVar; ++v)
        out << "     <DataArray type=\"Float64\" Name=\"" << names[v] << "\" format=\"appended\" offset=\""
            << (size_t)v * tuples * sizeof(double) + (size_t)v * sizeof(uint32_t) << "\" />\n";
      out << "    </PointData>\n    <CellData>\n    </CellData>\n  </Piece>\n  </ImageData>\n  <AppendedData encoding=\"raw\">\n_";
      for (int v = 0; v < p_.nbVar; ++v) {
        out.write(reinterpret_cast<const char*>(&nbytes), sizeof(nbytes));
        for (int k = k0; k < k1; ++k)
          for (int j = gw; j < (int)jsize - gw; ++j)
            out.write(reinterpret_cast<const char*>(&h_U_[gw + isize * (j + jsize * (size_t)k) + ncell * v]), sizeof(double) * nx);
      }
      out << "  </AppendedData>\n</VTKFile>\n";
    }
    if (!out) throw std::runtime_error("writing " + fn + " failed");
  } catch (const std::exception& e) { local_error = e.what(); }
  agree_or_throw(local_error, "outputVtk");
}

// Xsmurf: one ASCII header line + the interior of ONE variable (the density: the reference's default argument) as raw doubles,
// written to the current directory (no outputDir in the name, HydroRunBase.cpp:2535)
void GodunovRun::outputXsm(int nStep) {
  const int gw = p_.ghostWidth, nx = p_.nx, ny = p_.ny;
  const bool three_d = p_.nz_global != 1;
  const int nz = three_d ? p_.nz : 1;
  const size_t isize = nx + 2 * gw, jsize = ny + 2 * gw;
  std::ostringstream fn;
  fn << rs_.outputPrefix << "_d_" << std::setw(7) << std::setfill('0') << nStep << ".xsm";
  std::ofstream out(fn.str().c_str(), std::ios::binary);
  if (!out) throw std::runtime_error("cannot write " + fn.str());
  if (three_d) out << "Binary 1 " << nx << "x" << ny << "x" << nz << " " << nx * ny * nz << "(" << sizeof(double) << " byte reals)\n";
  else out << "Binary 1 " << nx << "x" << ny << " " << nx * ny << "(" << sizeof(double) << " byte reals)\n";
  for (int k = 0; k < nz; ++k)
    for (int j = 0; j < ny; ++j) {
      const size_t kk = three_d ? k + gw : 0;
      out.write(reinterpret_cast<const char*>(&h_U_[gw + isize * ((j + gw) + jsize * kk)]), sizeof(double) * nx);
    }
}

// NRRD: a text header + the interior of each variable converted to 32-bit floats, one file per variable (d, p, u, v, w, a, b, c)
void GodunovRun::outputNrrd(int nStep) {
  static const char* prefix[8] = {"d", "p", "u", "v", "w", "a", "b", "c"};
  const int gw = p_.ghostWidth, nx = p_.nx, ny = p_.ny;
  const bool three_d = p_.nz_global != 1;
  const int nz = three_d ? p_.nz : 1;
  const size_t isize = nx + 2 * gw, jsize = ny + 2 * gw, ksize = three_d ? nz + 2 * gw : 1, ncell = isize * jsize * ksize;
  std::vector<float> row(nx);
  for (int v = 0; v < p_.nbVar; ++v) {
    const int pv = (p_.nbVar == 4 && v == 3) ? 3 : v;   // 2D hydro: d, p, u, v
    std::ostringstream fn;
    fn << rs_.outputDir << "/" << rs_.outputPrefix << "_" << prefix[pv] << "_" << std::setw(7) << std::setfill('0') << nStep << ".nrrd";
    std::ofstream out(fn.str().c_str(), std::ios::binary);
    if (!out) throw std::runtime_error("cannot write " + fn.str());
    out << "NRRD0004\n# Complete NRRD file format specification at:\n# http://teem.sourceforge.net/nrrd/format.html\ntype: float\n";
    if (three_d) out << "dimension: 3\nsizes: " << nx << " " << ny << " " << nz << "\nspace directions: (1,0,0) (0,1,0) (0,0,1)\n";
    else out << "dimension: 2\nsizes: " << nx << " " << ny << "\nspace directions: (1,0) (0,1)\n";
    out << "endian: little\nencoding: raw\n\n";
    for (int k = 0; k < nz; ++k)
      for (int j = 0; j < ny; ++j) {
        const size_t kk = three_d ? k + gw : 0;
        const double* src = &h_U_[gw + isize * ((j + gw) + jsize * kk) + ncell * v];
        for (int i = 0; i < nx; ++i) row[i] = (float)src[i];
        out.write(reinterpret_cast<const char*>(row.data()), sizeof(float) * nx);
      }
  }
}

H5Box GodunovRun::h5_box(int nx, int ny, int nz) const {
  H5Box b;
  b.nx = nx; b.ny = ny; b.nz = nz;
  b.ghostWidth = p_.ghostWidth; b.nbVar = p_.nbVar;
  b.three_d = p_.nz_global != 1; b.mhd = p_.mhdEnabled != 0;
  return b;
}

// [output] outputHdf5=yes: the reference's HDF5 file (hdf5_io.h) when libhdf5 can be loaded, the raw dump below otherwise
void GodunovRun::outputHdf5(int nStep) {
  const char* fmt = std::getenv("RGPU_RESTART_FORMAT");   // "rgr": the raw dump even when HDF5 is there
  std::string why;
  if (slab()) {   // (agreed by all ranks: libhdf5 may be missing on one node only)
    std::string local_error;
    if ((fmt && std::string(fmt) == "rgr") || !hdf5_available(&why))
      local_error = "outputs of a z-slab run go to one HDF5 file for the whole box: " + (why.empty() ? std::string("RGPU_RESTART_FORMAT=rgr is single-domain only") : why);
    agree_or_throw(local_error, "outputHdf5");
  }
  if (fmt && std::string(fmt) == "rgr") { outputRestart(nStep); return; }
  if (!hdf5_available(&why)) {
    if (!warned_no_hdf5_) { std::cerr << "outputHdf5: " << why << " -- writing raw .rgr dumps instead\n"; warned_no_hdf5_ = true; }
    outputRestart(nStep);
    return;
  }
  std::ostringstream fn;
  fn << rs_.outputDir << "/" << rs_.outputPrefix << "_" << std::setw(7) << std::setfill('0') << nStep << ".h5";
  const bool three_d = p_.nz_global != 1;
  if (slab()) {   // one file for the whole box: the slabs take turns, rank 0 creates it (hdf5_io.h)
    // A write can fail on ONE rank (disk full, file lock, libhdf5 missing on that node): the ranks agree on the outcome of
    // every turn (hooks.agree: a sum all-reduce of the failure flags in place of the bare barrier) and throw TOGETHER --
    // a rank that left this loop alone would leave the others waiting in the collective for ever.
    for (int r = 0; r < p_.slab_count; ++r) {
      std::string local_error;
      if (r == p_.slab_rank) {
        try {
          hdf5_write_slab(fn.str(), h_U_.data(), h5_box(p_.nx, p_.ny, p_.nz), p_.nz_global, p_.slab_rank, p_.slab_count, r == 0, rs_.ghostIncluded, nStep,
                          totalTime_, rs_.hdf5CompressionLevel);
        } catch (const std::exception& e) { local_error = e.what(); }
      }
      agree_or_throw(local_error, "outputHdf5");
    }
  } else {
    hdf5_write_state(fn.str(), h_U_.data(), h5_box(p_.nx, p_.ny, three_d ? p_.nz : 1), rs_.ghostIncluded, nStep, totalTime_, rs_.hdf5CompressionLevel);
  }
  wrote_hdf5_ = true;
}

// Raw restart dump: one text line "RGPU-RESTART 1 nx ny nz ghostWidth nbVar ghostIncluded nStep totalTime(hex float)",
// then nbVar arrays of little-endian doubles, x fastest -- the whole ghost-inclusive arrays when ghostIncluded (what a
// shearing-box run needs: the field on the first high x face is evolved by the CT update and not rebuilt by the ghost
// fill), the interior otherwise.  Stands in for outputHdf5 / inputHdf5 (HydroRunBase.cpp:3308-3640, 4818-5160).
void GodunovRun::outputRestart(int nStep) {
  const int gw = p_.ghostWidth, nx = p_.nx, ny = p_.ny;
  const bool three_d = p_.nz_global != 1;
  const int nz = three_d ? p_.nz : 1;
  const size_t isize = nx + 2 * gw, jsize = ny + 2 * gw, ksize = three_d ? nz + 2 * gw : 1;
  const size_t ncell = isize * jsize * ksize;
  std::ostringstream fn;
  fn << rs_.outputDir << "/" << rs_.outputPrefix << "_" << std::setw(7) << std::setfill('0') << nStep << ".rgr";
  std::ofstream out(fn.str().c_str(), std::ios::binary);
  if (!out) throw std::runtime_error("cannot write " + fn.str());
  char line[256];
  std::snprintf(line, sizeof(line), "RGPU-RESTART 1 %d %d %d %d %d %d %d %a\n", nx, ny, nz, gw, p_.nbVar, rs_.ghostIncluded ? 1 : 0, nStep, totalTime_);
  out << line;
  if (rs_.ghostIncluded) {
    out.write(reinterpret_cast<const char*>(h_U_.data()), sizeof(double) * ncell * p_.nbVar);
  } else {
    for (int v = 0; v < p_.nbVar; ++v)
      for (int k = 0; k < nz; ++k)
        for (int j = 0; j < ny; ++j) {
          const size_t kk = three_d ? k + gw : 0;
          out.write(reinterpret_cast<const char*>(&h_U_[gw + isize * ((j + gw) + jsize * kk) + ncell * v]), sizeof(double) * nx);
        }
  }
}

// Reads a dump of an nx x ny x nz box (ghost width and variables of this run) into dst, a ghost-inclusive array of that
// box; without ghosts in the file the ghost cells of dst are left as they are.
int GodunovRun::read_restart(const std::string& path, int nx_want, int ny_want, int nz_want, double* dst, bool* ghosts_read) {
  if (path.size() > 3 && path.substr(path.size() - 3) == ".h5") {   // inputHdf5 (HydroRunBase.cpp:4818-5155)
    double t = 0.0;
    const int step = slab() ? hdf5_read_slab(path, dst, h5_box(nx_want, ny_want, nz_want), p_.nz_global, p_.slab_rank, p_.slab_count, &t, ghosts_read)
                            : hdf5_read_state(path, dst, h5_box(nx_want, ny_want, nz_want), &t, ghosts_read);
    totalTime_ = rs_.restartResetTotalTime ? 0.0 : t;
    return step;
  }
  if (slab()) throw std::runtime_error("restart: a z-slab run resumes from the .h5 file of the whole box");
  std::ifstream in(path.c_str(), std::ios::binary);
  if (!in) throw std::runtime_error("restart: cannot read " + path);
  std::string line;
  std::getline(in, line);
  int ver = 0, nx = 0, ny = 0, nz = 0, gw = 0, nv = 0, gi = 0, nStep = 0;
  char hex[64] = {0};
  if (std::sscanf(line.c_str(), "RGPU-RESTART %d %d %d %d %d %d %d %d %63s", &ver, &nx, &ny, &nz, &gw, &nv, &gi, &nStep, hex) != 9 || ver != 1)
    throw std::runtime_error("restart: " + path + " is not a restart dump of this code");
  const bool three_d = p_.nz_global != 1;
  if (nx != nx_want || ny != ny_want || nz != nz_want || gw != p_.ghostWidth || nv != p_.nbVar)
    throw std::runtime_error("restart: " + path + " holds another box than expected from [mesh] nx, ny, nz / other variables");
  const size_t isize = nx + 2 * gw, jsize = ny + 2 * gw, ksize = three_d ? nz + 2 * gw : 1;
  const size_t ncell = isize * jsize * ksize;
  if (gi) {
    in.read(reinterpret_cast<char*>(dst), sizeof(double) * ncell * nv);
  } else {
    for (int v = 0; v < nv; ++v)
      for (int k = 0; k < nz; ++k)
        for (int j = 0; j < ny; ++j) {
          const size_t kk = three_d ? k + gw : 0;
          in.read(reinterpret_cast<char*>(&dst[gw + isize * ((j + gw) + jsize * kk) + ncell * v]), sizeof(double) * nx);
        }
  }
  if (!in) throw std::runtime_error("restart: " + path + " is truncated");
  if (ghosts_read) *ghosts_read = gi != 0;
  totalTime_ = rs_.restartResetTotalTime ? 0.0 : std::strtod(hex, 0);
  return nStep;
}

int GodunovRun::inputRestart(const std::string& path, bool* ghosts_read) {
  const bool three_d = p_.nz_global != 1;
  return read_restart(path, p_.nx, p_.ny, three_d ? p_.nz : 1, h_U_.data(), ghosts_read);
}

// [run] restart_upscale: the dump holds the same problem on nx/2 x ny/2 (x nz/2) cells; every cell of this run's arrays,
// ghosts included, takes the value of the coarse cell under it -- (index + ghostWidth) / 2 per direction -- except the
// face-centred field: a fine face lying on a coarse face takes that face's value, one in the middle of a coarse cell the
// mean of the two coarse faces around it along the component's own direction, which keeps div B = 0
// (HydroRunBase::upscale, HydroRunBase.cpp:5170-5278; call site :7047-7062).  In 2D Bz is cell-like.  The step count of
// the coarse run is not taken over (the reference drops inputHdf5's return value there), its time is.
void GodunovRun::inputRestartUpscaled(const std::string& path, bool* ghosts_read) {
  const bool three_d = p_.nz_global != 1;
  const int gw = p_.ghostWidth, nv = p_.nbVar;
  const int lnx = p_.nx / 2, lny = p_.ny / 2, lnz = three_d ? p_.nz / 2 : 1;
  const size_t li = lnx + 2 * gw, lj = lny + 2 * gw, lk = three_d ? lnz + 2 * gw : 1, lcell = li * lj * lk;
  std::vector<double> low(lcell * nv, 0.0);
  read_restart(path, lnx, lny, lnz, low.data(), ghosts_read);
  const size_t isize = p_.nx + 2 * gw, jsize = p_.ny + 2 * gw, ksize = three_d ? p_.nz + 2 * gw : 1, ncell = isize * jsize * ksize;
  const bool mhd = nv == 8;
  const int ncopy = mhd ? 5 : nv;   // cell-centred variables (2D MHD: density, energy and the three momenta)
  for (size_t k = 0; k < ksize; ++k) {
    const size_t kl = three_d ? (k + gw) / 2 : 0;
    for (size_t j = 0; j < jsize; ++j) {
      const size_t jl = (j + gw) / 2;
      for (size_t i = 0; i < isize; ++i) {
        const size_t il = (i + gw) / 2;
        const size_t hi = i + isize * (j + jsize * k), lo = il + li * (jl + lj * kl);
        for (int v = 0; v < ncopy; ++v) h_U_[hi + ncell * v] = low[lo + lcell * v];
        if (mhd) {
          const double* bx = &low[lcell * 5]; const double* by = &low[lcell * 6]; const double* bz = &low[lcell * 7];
          h_U_[hi + ncell * 5] = (i + gw == 2 * il) ? bx[lo] : (bx[lo] + bx[lo + 1]) / 2;
          h_U_[hi + ncell * 6] = (j + gw == 2 * jl) ? by[lo] : (by[lo] + by[lo + li]) / 2;
          if (!three_d) h_U_[hi + ncell * 7] = bz[lo];
          else h_U_[hi + ncell * 7] = (k + gw == 2 * kl) ? bz[lo] : (bz[lo] + bz[lo + li * lj]) / 2;
        }
      }
    }
  }
}

// Reads a .vti written by outputVtk (same box, same variables) into the interior of h_U_; returns the step count of the
// file and sets totalTime_ (0 / 0 for files without the restart comment).  Ghost cells stay zero: start() fills them.
int GodunovRun::inputVtk(const std::string& path) {
  std::ifstream in(path.c_str(), std::ios::binary);
  if (!in) throw std::runtime_error("restart: cannot read " + path);
  std::string blob((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
  const size_t mark = blob.find("<AppendedData encoding=\"raw\">");
  if (mark == std::string::npos) throw std::runtime_error("restart: " + path + " is not an appended-raw .vti");
  const std::string head = blob.substr(0, mark);
  int nStep = 0;
  double t = 0.0;
  {
    // the comment line after </VTKFile> (files of earlier versions carried it in the header)
    const std::string tail = blob.substr(blob.size() > 256 ? blob.size() - 256 : 0);
    const size_t ct = tail.find("rgpu restart: nStep="), ch = head.find("rgpu restart: nStep=");
    const char* at = ct != std::string::npos ? tail.c_str() + ct : ch != std::string::npos ? head.c_str() + ch : 0;
    if (at) {
      char hex[64] = {0};
      if (std::sscanf(at, "rgpu restart: nStep=%d totalTime=%63s", &nStep, hex) == 2) t = std::strtod(hex, 0);
    }
  }
  int e[6] = {0, 0, 0, 0, 0, 0};
  {
    const size_t w = head.find("WholeExtent=\"");
    if (w == std::string::npos || std::sscanf(head.c_str() + w, "WholeExtent=\"%d %d %d %d %d %d\"", &e[0], &e[1], &e[2], &e[3], &e[4], &e[5]) != 6)
      throw std::runtime_error("restart: no WholeExtent in " + path);
  }
  const int gw = p_.ghostWidth, nx = p_.nx, ny = p_.ny;
  const bool three_d = p_.nz_global != 1;
  const int nz = three_d ? p_.nz : 1;
  if (e[1] - e[0] + 1 != nx || e[3] - e[2] + 1 != ny || e[5] - e[4] + 1 != nz)
    throw std::runtime_error("restart: " + path + " holds another box than [mesh] nx, ny, nz");
  const size_t isize = nx + 2 * gw, jsize = ny + 2 * gw, ksize = three_d ? nz + 2 * gw : 1;
  const size_t ncell = isize * jsize * ksize;
  const size_t start = blob.find('_', mark) + 1;
  const size_t nbytes = sizeof(double) * nx * ny * nz;
  size_t pos = 0;
  int nvar = 0;
  while ((pos = head.find("format=\"appended\" offset=\"", pos)) != std::string::npos) {
    pos += std::strlen("format=\"appended\" offset=\"");
    const size_t off = std::strtoull(head.c_str() + pos, 0, 10);
    if (nvar >= p_.nbVar) throw std::runtime_error("restart: " + path + " holds more variables than this run");
    uint32_t count = 0;
    if (start + off + sizeof(count) + nbytes > blob.size()) throw std::runtime_error("restart: " + path + " is truncated");
    std::memcpy(&count, blob.data() + start + off, sizeof(count));
    if (count != nbytes) throw std::runtime_error("restart: unexpected array size in " + path);
    const char* src = blob.data() + start + off + sizeof(count);
    for (int k = 0; k < nz; ++k)
      for (int j = 0; j < ny; ++j) {
        const size_t kk = three_d ? k + gw : 0;
        std::memcpy(&h_U_[gw + isize * ((j + gw) + jsize * kk) + ncell * nvar], src + sizeof(double) * nx * (j + (size_t)ny * k), sizeof(double) * nx);
      }
    ++nvar;
  }
  if (nvar != p_.nbVar) throw std::runtime_error("restart: " + path + " holds fewer variables than this run");
  totalTime_ = rs_.restartResetTotalTime ? 0.0 : t;
  return nStep;
}

// the forcing process of a step, next to the fields (the reference: <prefix>_forcing_NNNNNNN.npz, output_forcing)
void GodunovRun::save_forcing_process(int nStep) {
  if (p_.ouForcingEnabled) {
    double st[RGPU_OU_STATE_DOUBLES];
    check(rgpu_ou_forcing_get_state(ctx_, st), "ou_forcing_get_state");
    std::ostringstream fo;
    fo << rs_.outputDir << "/" << rs_.outputPrefix << "_forcing_" << std::setw(7) << std::setfill('0') << nStep << ".txt";
    std::ofstream f(fo.str().c_str());
    if (!f) throw std::runtime_error("cannot write " + fo.str());
    char buf[64];
    for (int i = 0; i < RGPU_OU_STATE_DOUBLES; ++i) { std::snprintf(buf, sizeof(buf), "%a\n", st[i]); f << buf; }
  }
}

// the Ornstein-Uhlenbeck process of step nStep, if the earlier run wrote it (outputVtk / outputRestart do)
void GodunovRun::restore_forcing_process(int nStep) {
  if (p_.ouForcingEnabled) {   // the forcing process of that step, if the earlier run wrote it
    std::ostringstream fo;
    fo << rs_.outputDir << "/" << rs_.outputPrefix << "_forcing_" << std::setw(7) << std::setfill('0') << nStep << ".txt";
    std::ifstream f(fo.str().c_str());
    if (f) {
      double st[RGPU_OU_STATE_DOUBLES];
      std::string tok;
      int n = 0;
      while (n < RGPU_OU_STATE_DOUBLES && (f >> tok)) st[n++] = std::strtod(tok.c_str(), 0);
      if (n != RGPU_OU_STATE_DOUBLES) throw std::runtime_error("restart: " + fo.str() + " is incomplete");
      check(rgpu_ou_forcing_set_state(ctx_, st), "ou_forcing_set_state");
    } else {
      std::cerr << "restart: no " << fo.str() << ", the forcing process starts afresh\n";
    }
  }
}

// MHDRunGodunov.cpp:3801-4070 / HydroRunGodunov.cpp:3857-4080 (no restart, no history, VTI outputs only)
// history(nStep, dt): the history file of the MHD runs (MHDRunBase.cpp:3285-3619), one row per call, same columns and
// ostream formatting: MRI problems get history_mri's eleven columns, Orszag-Tang history_default's four, every other
// problem none (history_empty); the turbulence problems get history_turbulence's twenty columns.  The sums come from the device
// (rgpu_history_mri) instead of a copy of the state to the host.  The inertial-wave problem gets history_inertial_wave's
// probe row (:3414-3469): the velocity of one cell in units of cIso, read with rgpu_read_cell.
// Largest 3D box (cells) whose history the run loop takes through rgpu_run_steps_history: the largest size at which the batched call
// was MEASURED to beat the per-step loop (the table's MRI 128 x 256 x 128 row; at 512^3 the two are level and
// nothing in between was measured).  Move it with that table, not without.
static const long long kHistoryBatchMaxCells = 128LL * 256 * 128;

// which of the two rows built from rgpu_history_mri's eight sums a single-domain run of this problem writes
int GodunovRun::history_row_kind() const {
  if (!p_.mhdEnabled) return 0;
  const std::string problem = cfg_.get_string("hydro", "problem", "unknown");
  if (problem == "MRI" || problem == "Mri" || problem == "mri") return p_.nz_global == 1 ? 0 : 1;   // history_mri does nothing in 2D
  return (problem == "Orszag-Tang" || problem == "OrszagTang") ? 2 : 0;
}

// The history file, open for appending.  At t <= 0, the first row of a run, "# history" goes in first, followed by the line that names
// the row's columns where the row has one.
static std::ofstream open_history(const IniConfig& cfg, double t, const char* columns) {
  const std::string fileName = cfg.get_string("output", "outputDir", "./") + "/" + cfg.get_string("output", "outputPrefix", "output") +
                               "_" + cfg.get_string("history", "filename", "history.txt");
  std::ofstream histo(fileName.c_str(), std::ios::out | std::ios::app | std::ios::ate);
  if (t <= 0) {
    histo << "# history" << std::endl;
    histo << columns;
  }
  return histo;
}

// the row itself (and, at t <= 0, the header in front of it): h = the out[8] of rgpu_history_mri taken at time t, dt the last time step
void GodunovRun::write_history_row(bool mri, double t, double dt, const double* h) {
  std::ofstream histo = open_history(cfg_, t, mri ? "# totalTime dt mass maxwell reynolds maxwell+reynolds magp mean_Bx mean_By mean_Bz divB\n"
                                                  : "# totalTime dt mass divB\n");
  if (mri)
    histo << t << "\t" << dt << "\t" << h[0] << "\t" << h[1] << "\t" << h[2] << "\t" << h[1] + h[2] << "\t" << h[3] << "\t"
          << h[4] << "\t" << h[5] << "\t" << h[6] << "\t" << h[7] << "\n";
  else
    histo << t << "\t" << dt << "\t" << h[0] << "\t" << h[7] << "\n";
}

void GodunovRun::history(int nStep, double dt) {
  if (!p_.mhdEnabled) return;
  const std::string problem = cfg_.get_string("hydro", "problem", "unknown");
  const int kind = history_row_kind();   // the one place that classifies the problem name (an MRI problem in 2D has no row: 0)
  const bool mri = kind == 1;
  bool dflt = kind == 2;
  if (slab()) {
    // z-slab runs follow the history set-up of the MPI classes (HydroRunBaseMpi.cpp:10667-10730): MRI -> history_mhd_mri,
    // turbulence -> history_mhd_turbulence (16 columns, no DFT amplitudes), every other MHD problem -> history_mhd_default
    const bool turb = (problem == "turbulence" || problem == "turbulence-Ornstein-Uhlenbeck") && p_.nz_global != 1;
    if (turb && hooks_.history_turbulence) {
      double h[14];
      hook_check(hooks_.history_turbulence(hooks_.self, nStep % 2, h), "history");   // collective; rank 0's values are the row
      if (p_.slab_rank != 0) return;
      std::ofstream histo = open_history(cfg_, totalTime_, "# totalTime dt mass divB eKin eMag helicity mean_B mean_Bx mean_By mean_Bz mean_rhovx mean_rhovy mean_rhovz Ma_s Ma_alfven\n");
      histo << totalTime_ << "\t" << dt;
      for (int q = 0; q < 14; ++q) histo << "\t" << h[q];
      histo << "\n";
      return;
    }
    if (!mri) dflt = true;
  }
  const bool iwave = problem == "InertialWave" || problem == "inertialwave" || problem == "Inertial-Wave" ||
                     problem == "inertial-wave" || problem == "Inertialwave";
  if (iwave && !slab()) {
    double u[8];
    const int iPos = p_.ghostWidth + p_.nx / 2, kPos = p_.ghostWidth;
    if (p_.nz_global == 1) check(rgpu_read_cell(ctx_, nStep % 2, iPos, kPos, 0, u), "history");
    else check(rgpu_read_cell(ctx_, nStep % 2, iPos, 1, kPos, u), "history");
    std::ofstream histo = open_history(cfg_, totalTime_, "");   // (this row has no line of column names)
    const double rho = u[RGPU_ID], dvx = u[RGPU_IU] / rho, dvy = u[RGPU_IV] / rho;
    // the reference's row, missing separator between totalTime and dt included; fmt() = " " + setw(12) fixed, 8 digits
    histo << totalTime_ << "" << dt << " " << rho << " ";
    const std::ios_base::fmtflags flags = histo.flags();
    histo << " " << std::setw(12) << std::setprecision(8) << std::fixed << dvx / p_.cIso;
    histo.flags(flags);
    histo << " ";
    histo << " " << std::setw(12) << std::setprecision(8) << std::fixed << dvy / p_.cIso;
    histo.flags(flags);
    histo << "\n";
    return;
  }
  if (!slab() && (problem == "turbulence" || problem == "turbulence-Ornstein-Uhlenbeck")) {   // history_turbulence (MHDRunBase.cpp:3626-3810)
    if (p_.nz_global == 1) return;
    double h[18];
    check(rgpu_history_turbulence(ctx_, nStep % 2, h), "history");
    std::ofstream histo = open_history(cfg_, totalTime_, "# totalTime dt mass divB eKin eMag helicity mean_rho mean_B mean_Bx mean_By mean_Bz mean_rhovx mean_rhovy mean_rhovz Ma_s Ma_alfven coef_x coef_y coef_z\n");
    histo << totalTime_ << "\t" << dt;
    for (int q = 0; q < 18; ++q) histo << "\t" << h[q];
    histo << "\n";
    return;
  }
  if (!mri && !dflt) return;
  double h[8];
  if (slab()) hook_check(hooks_.history_mri(hooks_.self, nStep % 2, h), "history");   // the same sums on every rank; rank 0 writes
  else check(rgpu_history_mri(ctx_, nStep % 2, h), "history");
  if (p_.slab_rank != 0) return;
  write_history_row(mri, totalTime_, dt, h);
}

int GodunovRun::start(double* mcell_per_s, rgpuh_attach_fn attach, void* user) {
  int nStep = init_simulation();
  if (attach) {   // the slab driver takes over the stepping from here (rgpuh_run_hooked)
    rgpuh_step_hooks h;
    std::memset(&h, 0, sizeof(h));
    if (attach(user, ctx_, &h) || !h.make_all_boundaries || !h.compute_dt || !h.one_step_integration || !h.barrier)
      throw std::runtime_error(std::string("attaching the slab driver failed") + (h.last_error ? std::string(": ") + h.last_error(h.self) : std::string()));
    set_hooks(h);
  }
  if (slab() && !hooked_) throw std::runtime_error("a z-slab context needs the slab driver (rgpuh_run_hooked / euler_hip --slabs)");
  if (!(rs_.restartEnabled && restart_has_ghosts_)) {   // a restart file with ghosts needs no fill (MHDRunGodunov.cpp:3818-3824)
    make_all_boundaries(0);
    // h_U.copyTo(h_U2): refresh both device arrays from the ghost-filled one
    copyGpuToCpu(0);
    check(rgpu_upload(ctx_, h_U_.data(), 1), "upload");
  }
  if (!rs_.restartEnabled) totalTime_ = 0.0;   // a restarted run keeps the time of its file (MHDRunGodunov.cpp:3866-3880)
  double dt = compute_dt(0);
  if (p_.slab_rank == 0) std::cout << "Initial dt : " << std::setprecision(8) << dt << std::endl;
  double io_seconds = 0.0;
  // history cadence of MHDRunGodunov::start (MHDRunGodunov.cpp:3913-3916, 3975-3984)
  const bool historyEnabled = p_.mhdEnabled && cfg_.get_bool("history", "enabled", false);
  const double dtHist = cfg_.get_float("history", "dtHist", static_cast<float>(10 * dt));
  double tHist = totalTime_;   // MHDRunGodunov.cpp:3916
  // the head of a turn of the time loop takes a history row (MHDRunGodunov.cpp:3975-3984)
  const auto history_due = [&]() { return tHist == 0 || ((totalTime_ - dt <= tHist + dtHist) && (totalTime_ > tHist + dtHist)); };
  // z-slab runs: the MRI / Orszag-Tang history goes through the slab driver's global sums; the other problems' do not
  const bool slab_history_ok = slab() && hooks_.history_mri;   // (every MHD problem has a history in the MPI classes)
  // A single-domain run whose history row is the MRI or the default one takes its samples inside rgpu_run_steps_history: the turns up
  // to the next log line or output are one call, the cadence above is evaluated there (on the device inside the device-clock
  // batches) and the returned samples are written with the row writer of history().  The turbulence, inertial-wave and z-slab
  // histories (other sums, a probe cell, global sums through the slab driver) keep the per-step loop below.  So do the classes of run
  // where the batched call was not measured to beat that loop: 2D (the extra launches behind every tick cost what
  // the host turn did) and 3D boxes above kHistoryBatchMaxCells, the largest size at which it won (at 512^3 the two are level).
  const int history_kind = (historyEnabled && !hooked_ && !slab()) ? history_row_kind() : 0;
  const bool history_batched = history_kind != 0 && p_.nz_global != 1 && (long long)p_.nx * p_.ny * p_.nz <= kHistoryBatchMaxCells;
  std::vector<int> hist_step;
  std::vector<double> hist_t, hist_dt, hist_v;
  // [monitor] enabled=yes: <outputDir>/<outputPrefix>_<filename> gets the ten doubles of rgpu_state_monitor / rgpu_state_monitor3d
  // (include/rgpu.h, "monitors") after every step that brings nStep to a multiple of `every`, hydro and MHD, 2D and 3D, with 17
  // significant digits (the doubles round-trip).  The quiet turns go through rgpu_run_steps_monitored (the samples taken on the device
  // inside the device-clock batches); with a history file as well the loop keeps its history handling, is cut at the sampling steps
  // and takes the rows by the direct calls -- the same doubles either way.  Not for z-slab runs (a slab holds a part of the box).
  // With planes=yes as well (3D single-domain runs) <outputDir>/<outputPrefix>_monitor_planes.txt gets the sixteen doubles of every
  // interior plane (rgpu_state_monitor_planes, "plane monitors") at the same steps, one line per plane; the samples then come from
  // rgpu_run_steps_monitored_planes / rgpu_state_monitor_planes, and the rows of the monitor file are folded from the plane rows on
  // the host, ascending in k, by the identity of include/rgpu.h: the bytes a run without planes=yes writes.
  const bool monitorEnabled = cfg_.get_bool("monitor", "enabled", false);
  const int mon_every = monitorEnabled ? (int)cfg_.get_integer("monitor", "every", 10) : 0;
  if (monitorEnabled && mon_every < 1) throw std::runtime_error("[monitor] every must be at least 1");
  bool noted_mon = false;
  if (monitorEnabled && (slab() || hooked_)) note_once(&noted_mon, "z-slab run: the monitor file is not written");
  const bool monitor_on = monitorEnabled && !slab() && !hooked_;
  const std::string mon_path = monitor_on ? rs_.outputDir + "/" + rs_.outputPrefix + "_" + cfg_.get_string("monitor", "filename", "monitor.txt") : std::string();
  const auto monitor_rows = [&](int n, const int* step, const double* t, const double* v) {
    std::ofstream f(mon_path.c_str(), std::ios::app);
    if (!f) throw std::runtime_error("cannot write " + mon_path);
    char num[40];
    for (int k = 0; k < n; ++k) {
      f << step[k];
      std::snprintf(num, sizeof(num), " %.17g", t[k]);
      f << num;
      for (int q = 0; q < RGPU_MON_NQ; ++q) { std::snprintf(num, sizeof(num), " %.17g", v[(size_t)k * RGPU_MON_NQ + q]); f << num; }
      f << "\n";
    }
  };
  const bool planesWanted = monitorEnabled && cfg_.get_bool("monitor", "planes", false);
  bool noted_planes = false;
  if (planesWanted && monitor_on && p_.nz_global == 1) note_once(&noted_planes, "2D run: the plane monitor file is not written");
  const bool planes_on = planesWanted && monitor_on && p_.nz_global != 1;
  const std::string planes_path = planes_on ? rs_.outputDir + "/" + rs_.outputPrefix + "_monitor_planes.txt" : std::string();
  const size_t planes_nz = (size_t)p_.nz;
  // n samples of planes_nz rows each: the lines of the planes file, and the monitor rows they fold to
  const auto planes_rows = [&](int n, const int* step, const double* t, const double* v) {
    std::ofstream f(planes_path.c_str(), std::ios::app);
    if (!f) throw std::runtime_error("cannot write " + planes_path);
    std::vector<double> folded((size_t)n * RGPU_MON_NQ);
    char num[40];
    for (int k = 0; k < n; ++k) {
      double* a = &folded[(size_t)k * RGPU_MON_NQ];
      for (int q = 0; q < RGPU_MON_NQ; ++q) a[q] = (q == 7 || q == 8) ? std::numeric_limits<double>::infinity() : 0.0;
      for (size_t kk = 0; kk < planes_nz; ++kk) {
        const double* row = v + ((size_t)k * planes_nz + kk) * RGPU_MONP_NQ;
        f << step[k];
        std::snprintf(num, sizeof(num), " %.17g", t[k]);
        f << num << " " << kk;
        for (int q = 0; q < RGPU_MONP_NQ; ++q) { std::snprintf(num, sizeof(num), " %.17g", row[q]); f << num; }
        f << "\n";
        for (int q = 0; q < 7; ++q) a[q] = a[q] + row[q];
        a[7] = std::fmin(a[7], row[7]); a[8] = std::fmin(a[8], row[8]); a[9] = std::fmax(a[9], row[9]);
      }
    }
    f.close();
    monitor_rows(n, step, t, folded.data());
  };
  std::vector<double> planes_v;
  const auto monitor_direct = [&](int n) {   // the row of the current state U[n % 2]
    if (planes_on) {
      planes_v.resize(std::max(planes_v.size(), planes_nz * RGPU_MONP_NQ));
      check(rgpu_state_monitor_planes(ctx_, n % 2, planes_v.data()), "state_monitor_planes");
      planes_rows(1, &n, &totalTime_, planes_v.data());
      return;
    }
    double v[RGPU_MON_NQ];
    check(p_.nz_global != 1 ? rgpu_state_monitor3d(ctx_, n % 2, v) : rgpu_state_monitor(ctx_, n % 2, v), "state_monitor");
    monitor_rows(1, &n, &totalTime_, v);
  };
  if (monitor_on && !(totalTime_ > 0)) {   // the start of a run
    std::ofstream f(mon_path.c_str(), std::ios::trunc);
    if (!f) throw std::runtime_error("cannot write " + mon_path);
    f << "# nStep totalTime " RGPU_MON_NAMES "\n";
  }
  if (planes_on && !(totalTime_ > 0)) {
    std::ofstream f(planes_path.c_str(), std::ios::trunc);
    if (!f) throw std::runtime_error("cannot write " + planes_path);
    f << "# nStep totalTime k " RGPU_MONP_NAMES "\n";
  }
  std::vector<int> mon_step;
  std::vector<double> mon_t, mon_v;
  // [maps] enabled=yes every=N map0=z:16 map1=y:0-24 map2=x:all ... (up to map7, numbered from 0 without a gap): pictures of a 3D
  // single-domain run (include/rgpu.h, "map monitors") after every step that brings nStep to a multiple of `every`.  A map is
  // axis:index (a slice), axis:lo-hi (the cells lo .. hi - 1 summed along the axis) or axis:all.  Each sample of each map is one file
  // <outputDir>/<outputPrefix>_map<m>_<step, 7 digits>.npy -- NumPy format 1.0, '<f8', C order, shape (12, nv, nu), the channels
  // RGPU_MAP_NAMES -- and one line "step t map axis lo hi file" of <outputPrefix>_maps.txt, t with 17 significant digits.  Driven as
  // the [monitor] block drives its run: the quiet turns go through rgpu_run_steps_mapped (the maps taken on the device inside the
  // device-clock batches); with a history file the loop is cut at the sampling steps and takes the maps by rgpu_state_maps -- the
  // same doubles either way.  With [monitor] on as well the maps take the batches and the monitor rows come from the direct calls
  // (the same rows: a batch serves one consumer).  Not for z-slab, hooked or 2D runs.
  const bool mapsEnabled = cfg_.get_bool("maps", "enabled", false);
  const int maps_every = mapsEnabled ? (int)cfg_.get_integer("maps", "every", 10) : 0;
  if (mapsEnabled && maps_every < 1) throw std::runtime_error("[maps] every must be at least 1");
  bool noted_maps = false;
  if (mapsEnabled && (slab() || hooked_ || p_.nz_global == 1)) note_once(&noted_maps, p_.nz_global == 1 ? "2D run: the map files are not written" : "z-slab run: the map files are not written");
  std::vector<rgpu_map_spec> map_specs;
  std::vector<size_t> map_at(1, 0);   // map m of a sample begins at map_at[m]; map_at.back(): the doubles of a sample
  if (mapsEnabled && !slab() && !hooked_ && p_.nz_global != 1) {
    for (int m = 0; m < RGPU_MAP_MAX; ++m) {
      const std::string key = "map" + std::to_string(m), text = cfg_.get_string("maps", key, "");
      if (text.empty()) break;
      const int n[3] = {p_.nx, p_.ny, p_.nz};
      rgpu_map_spec sp = {-1, 0, 0};
      if (text.size() > 2 && text[1] == ':') sp.axis = text[0] == 'x' ? 0 : text[0] == 'y' ? 1 : text[0] == 'z' ? 2 : -1;
      const std::string range = sp.axis >= 0 ? text.substr(2) : std::string();
      char* end = 0;
      if (range == "all") { sp.lo = 0; sp.hi = n[sp.axis]; }
      else if (!range.empty()) {
        sp.lo = (int)std::strtol(range.c_str(), &end, 10);
        sp.hi = sp.lo + 1;
        if (*end == '-' && end != range.c_str()) { const char* second = end + 1; sp.hi = (int)std::strtol(second, &end, 10); if (end == second) sp.axis = -1; }
        if (*end != 0) sp.axis = -1;
      }
      const size_t doubles = rgpu_map_doubles(ctx_, &sp);
      if (doubles == 0) throw std::runtime_error("[maps] " + key + "=" + text + ": expected x|y|z followed by :index, :lo-hi (lo inclusive, hi exclusive) or :all, inside the box");
      map_specs.push_back(sp);
      map_at.push_back(map_at.back() + doubles);
    }
  }
  const bool maps_on = !map_specs.empty();
  const std::string maps_list = rs_.outputDir + "/" + rs_.outputPrefix + "_maps.txt";
  // n samples of all maps: the .npy files and their lines in the list
  const auto maps_files = [&](int n, const int* step, const double* t, const double* v) {
    std::ofstream list(maps_list.c_str(), std::ios::app);
    if (!list) throw std::runtime_error("cannot write " + maps_list);
    char num[64];
    for (int k = 0; k < n; ++k)
      for (size_t m = 0; m < map_specs.size(); ++m) {
        const rgpu_map_spec& sp = map_specs[m];
        const int nu = sp.axis == 0 ? p_.ny : p_.nx, nv = sp.axis == 2 ? p_.ny : p_.nz;
        std::snprintf(num, sizeof(num), "_map%d_%07d.npy", (int)m, step[k]);
        const std::string name = rs_.outputPrefix + num, path = rs_.outputDir + "/" + name;
        // NumPy format 1.0: magic, version, the length of the header (little endian), the header padded with spaces to a multiple of 64
        std::string head = "{'descr': '<f8', 'fortran_order': False, 'shape': (" + std::to_string(RGPU_MAP_NQ) + ", " + std::to_string(nv) + ", " + std::to_string(nu) + "), }";
        head.append(63 - (10 + head.size()) % 64, ' ');
        head += "\n";
        std::ofstream f(path.c_str(), std::ios::binary | std::ios::trunc);
        const char magic[10] = {'\x93', 'N', 'U', 'M', 'P', 'Y', 1, 0, (char)(head.size() & 0xff), (char)(head.size() >> 8)};
        f.write(magic, 10);
        f.write(head.data(), (std::streamsize)head.size());
        f.write(reinterpret_cast<const char*>(v + (size_t)k * map_at.back() + map_at[m]), (std::streamsize)((map_at[m + 1] - map_at[m]) * sizeof(double)));
        if (!f) throw std::runtime_error("cannot write " + path);
        std::snprintf(num, sizeof(num), " %.17g", t[k]);
        list << step[k] << num << " " << m << " " << "xyz"[sp.axis] << " " << sp.lo << " " << sp.hi << " " << name << "\n";
      }
  };
  std::vector<double> maps_v;
  std::vector<int> maps_step;
  std::vector<double> maps_t;
  const auto maps_direct = [&](int n) {   // the maps of the current state U[n % 2]
    maps_v.resize(std::max(maps_v.size(), map_at.back()));
    check(rgpu_state_maps(ctx_, n % 2, (int)map_specs.size(), map_specs.data(), maps_v.data()), "state_maps");
    maps_files(1, &n, &totalTime_, maps_v.data());
  };
  if (maps_on && !(totalTime_ > 0)) {   // the start of a run
    std::ofstream f(maps_list.c_str(), std::ios::trunc);
    if (!f) throw std::runtime_error("cannot write " + maps_list);
    f << "# nStep totalTime map axis lo hi file\n";
  }
  // [pdfs] enabled=yes every=N pdf0=rho:log2:-8:8:3 pdf1=rho:log2:-4:4:2,eint:lin:0:4:32 ... (up to pdf7, numbered from 0 without a
  // gap): histograms of a 3D single-domain run (include/rgpu.h, "PDF monitors") after every step that brings nStep to a multiple of
  // `every`.  An axis is channel:lin:lo:hi:nbins or channel:log2:emin:emax:sub (octave bins on |x| from 2^emin to 2^emax, 2^sub
  // sub-bins each), the channel a name of RGPU_PDF_NAMES; two axes joined by a comma are a joint PDF.  Each sample of each PDF is one
  // file <outputDir>/<outputPrefix>_pdf<m>_<step, 7 digits>.npy -- NumPy format 1.0, '<u8', C order, shape (na + 3,) or (na + 3, nb + 3)
  // -- and one line "step t pdf spec file" of <outputPrefix>_pdfs.txt, t with 17 significant digits.  Driven as [maps] is; a batch
  // serves one consumer, and the PDFs take the batches where the maps do not: otherwise they come from rgpu_state_pdfs at the
  // sampling steps -- the same words either way.  Not for z-slab, hooked or 2D runs.
  const bool pdfsEnabled = cfg_.get_bool("pdfs", "enabled", false);
  const int pdfs_every = pdfsEnabled ? (int)cfg_.get_integer("pdfs", "every", 10) : 0;
  if (pdfsEnabled && pdfs_every < 1) throw std::runtime_error("[pdfs] every must be at least 1");
  bool noted_pdfs = false;
  if (pdfsEnabled && (slab() || hooked_ || p_.nz_global == 1)) note_once(&noted_pdfs, p_.nz_global == 1 ? "2D run: the PDF files are not written" : "z-slab run: the PDF files are not written");
  std::vector<rgpu_pdf_spec> pdf_specs;
  std::vector<std::string> pdf_texts;
  std::vector<size_t> pdf_at(1, 0);   // table m of a sample begins at pdf_at[m]; pdf_at.back(): the words of a sample
  if (pdfsEnabled && !slab() && !hooked_ && p_.nz_global != 1) {
    // one axis out of its text; false: the text is not an axis (what the numbers may be is the library's to say)
    const auto parse_axis = [](const std::string& text, rgpu_pdf_axis* a) {
      std::vector<std::string> f;
      for (size_t at = 0;;) {
        const size_t colon = text.find(':', at);
        f.push_back(text.substr(at, colon == std::string::npos ? colon : colon - at));
        if (colon == std::string::npos) break;
        at = colon + 1;
      }
      if (f.size() != 5) return false;
      std::istringstream names(RGPU_PDF_NAMES);
      std::string name;
      a->channel = -1;
      for (int q = 0; names >> name; ++q) if (name == f[0]) a->channel = q;
      a->scale = f[1] == "lin" ? 0 : f[1] == "log2" ? 1 : -1;
      if (a->channel < 0 || a->scale < 0) return false;
      char* end = 0;
      double v[3];
      for (int k = 0; k < 3; ++k) {
        v[k] = std::strtod(f[2 + k].c_str(), &end);
        if (f[2 + k].empty() || *end != 0) return false;
      }
      if (a->scale == 0) { a->lo = v[0]; a->hi = v[1]; a->nbins = (int)v[2]; a->sub = 0; return v[2] == (double)a->nbins; }
      if (v[0] != std::floor(v[0]) || v[1] != std::floor(v[1]) || v[2] != std::floor(v[2]) || std::fabs(v[0]) > 1100 || std::fabs(v[1]) > 1100 || v[2] < 0 || v[2] > 6) return false;
      a->lo = std::ldexp(1.0, (int)v[0]); a->hi = std::ldexp(1.0, (int)v[1]); a->sub = (int)v[2];
      a->nbins = v[1] > v[0] ? ((int)v[1] - (int)v[0]) << a->sub : 0;
      return true;
    };
    size_t total = 0;
    for (int m = 0; m < RGPU_PDF_MAX; ++m) {
      const std::string key = "pdf" + std::to_string(m), text = cfg_.get_string("pdfs", key, "");
      if (text.empty()) break;
      rgpu_pdf_spec sp = {};
      const size_t comma = text.find(',');
      const bool ok = parse_axis(text.substr(0, comma), &sp.a) && (comma == std::string::npos || (parse_axis(text.substr(comma + 1), &sp.b) && sp.b.nbins != 0));
      const size_t words = ok ? rgpu_pdf_words(&sp) : 0;
      if (words == 0)
        throw std::runtime_error("[pdfs] " + key + "=" + text + ": expected channel:lin:lo:hi:nbins or channel:log2:emin:emax:sub (a channel of \"" RGPU_PDF_NAMES "\"; lo < hi; sub 0 .. 6), or two of them joined by a comma, within " + std::to_string(RGPU_PDF_MAX_WORDS) + " words");
      total += words;
      if (total > (size_t)RGPU_PDF_MAX_WORDS) throw std::runtime_error("[pdfs] " + key + ": the PDFs have more than " + std::to_string(RGPU_PDF_MAX_WORDS) + " words together");
      pdf_specs.push_back(sp);
      pdf_texts.push_back(text);
      pdf_at.push_back(total);
    }
  }
  const bool pdfs_on = !pdf_specs.empty();
  const std::string pdfs_list = rs_.outputDir + "/" + rs_.outputPrefix + "_pdfs.txt";
  // n samples of all PDFs: the .npy files and their lines in the list
  const auto pdfs_files = [&](int n, const int* step, const double* t, const unsigned long long* v) {
    std::ofstream list(pdfs_list.c_str(), std::ios::app);
    if (!list) throw std::runtime_error("cannot write " + pdfs_list);
    char num[64];
    for (int k = 0; k < n; ++k)
      for (size_t m = 0; m < pdf_specs.size(); ++m) {
        const rgpu_pdf_spec& sp = pdf_specs[m];
        std::snprintf(num, sizeof(num), "_pdf%d_%07d.npy", (int)m, step[k]);
        const std::string name = rs_.outputPrefix + num, path = rs_.outputDir + "/" + name;
        // NumPy format 1.0, as the maps' files: the header padded with spaces to a multiple of 64
        const std::string shape = sp.b.nbins == 0 ? std::to_string(sp.a.nbins + 3) + "," : std::to_string(sp.a.nbins + 3) + ", " + std::to_string(sp.b.nbins + 3);
        std::string head = "{'descr': '<u8', 'fortran_order': False, 'shape': (" + shape + "), }";
        head.append(63 - (10 + head.size()) % 64, ' ');
        head += "\n";
        std::ofstream f(path.c_str(), std::ios::binary | std::ios::trunc);
        const char magic[10] = {'\x93', 'N', 'U', 'M', 'P', 'Y', 1, 0, (char)(head.size() & 0xff), (char)(head.size() >> 8)};
        f.write(magic, 10);
        f.write(head.data(), (std::streamsize)head.size());
        f.write(reinterpret_cast<const char*>(v + (size_t)k * pdf_at.back() + pdf_at[m]), (std::streamsize)((pdf_at[m + 1] - pdf_at[m]) * sizeof(unsigned long long)));
        if (!f) throw std::runtime_error("cannot write " + path);
        std::snprintf(num, sizeof(num), " %.17g", t[k]);
        list << step[k] << num << " " << m << " " << pdf_texts[m] << " " << name << "\n";
      }
  };
  std::vector<unsigned long long> pdfs_v;
  std::vector<int> pdfs_step;
  std::vector<double> pdfs_t;
  const auto pdfs_direct = [&](int n) {   // the PDFs of the current state U[n % 2]
    pdfs_v.resize(std::max(pdfs_v.size(), pdf_at.back()));
    check(rgpu_state_pdfs(ctx_, n % 2, (int)pdf_specs.size(), pdf_specs.data(), pdfs_v.data()), "state_pdfs");
    pdfs_files(1, &n, &totalTime_, pdfs_v.data());
  };
  if (pdfs_on && !(totalTime_ > 0)) {   // the start of a run
    std::ofstream f(pdfs_list.c_str(), std::ios::trunc);
    if (!f) throw std::runtime_error("cannot write " + pdfs_list);
    f << "# nStep totalTime pdf spec file\n";
  }
  // [spectra] enabled=yes every=N spectrum0="w 1 1 1" spectrum1="b 4 1 4" ... (up to spectrum3, numbered from 0 without a gap):
  // shell-binned power spectra of a 3D single-domain run whose extents are powers of two (include/rgpu.h, "spectrum monitors") after
  // every step that brings nStep to a multiple of `every`.  A spec is "<channels> <wx> <wy> <wz>": the channels names of
  // RGPU_SPECTRUM_NAMES or the shorthands v, w, b, m (all three components) joined by commas, then the three integer weights.  Each
  // sample of each spec is one file <outputDir>/<outputPrefix>_spectrum<m>_<step, 7 digits>.npy -- NumPy format 1.0, '<f8', C order,
  // shape (2, S): the power, then the modes of each shell -- and one line "step t spectrum spec file" of <outputPrefix>_spectra.txt,
  // t with 17 significant digits.  Driven as [pdfs] is; a batch serves one consumer, and the spectra take the batches where neither
  // the maps nor the PDFs do.  Not for z-slab, hooked or 2D runs, nor for a box with an extent that is no power of two in 4 .. 1024:
  // noted once, the run goes on.
  const bool spectraEnabled = cfg_.get_bool("spectra", "enabled", false);
  const int spectra_every = spectraEnabled ? (int)cfg_.get_integer("spectra", "every", 10) : 0;
  if (spectraEnabled && spectra_every < 1) throw std::runtime_error("[spectra] every must be at least 1");
  bool noted_spectra = false;
  const auto pow2_extent = [](int n) { return n >= 4 && n <= 1024 && (n & (n - 1)) == 0; };
  const bool spectra_box = !slab() && !hooked_ && p_.nz_global != 1 && pow2_extent(p_.nx) && pow2_extent(p_.ny) && pow2_extent(p_.nz);
  if (spectraEnabled && !spectra_box)
    note_once(&noted_spectra, p_.nz_global == 1 ? "2D run: the spectrum files are not written" : (slab() || hooked_) ? "z-slab run: the spectrum files are not written"
                                                                                                 : "an extent of the box is not a power of two in 4 .. 1024: the spectrum files are not written");
  std::vector<rgpu_spectrum_spec> spectrum_specs;
  std::vector<std::string> spectrum_texts;
  std::vector<size_t> spectrum_at(1, 0);   // spec m of a sample begins at spectrum_at[m]; spectrum_at.back(): the doubles of a sample
  if (spectraEnabled && spectra_box) {
    // the mask of "<channels>"; 0: not a list of channels
    const auto parse_channels = [](const std::string& text) {
      unsigned mask = 0;
      for (size_t at = 0; at <= text.size();) {
        const size_t comma = text.find(',', at);
        const std::string one = text.substr(at, comma == std::string::npos ? comma : comma - at);
        std::istringstream names(RGPU_SPECTRUM_NAMES);
        std::string name;
        unsigned hit = 0;
        for (int q = 0; names >> name; ++q)
          if (name == one || (one.size() == 1 && name.size() == 2 && name[0] == one[0] && std::string("vwbm").find(one[0]) != std::string::npos)) hit |= 1u << q;
        if (!hit) return 0u;
        mask |= hit;
        if (comma == std::string::npos) break;
        at = comma + 1;
      }
      return mask;
    };
    for (int m = 0; m < RGPU_SPECTRUM_MAX; ++m) {
      const std::string key = "spectrum" + std::to_string(m);
      std::string text = cfg_.get_string("spectra", key, "");
      if (text.empty()) break;
      if (text.size() >= 2 && text.front() == '"' && text.back() == '"') text = text.substr(1, text.size() - 2);
      std::istringstream in(text);
      std::string channels, rest;
      rgpu_spectrum_spec sp = {};
      const bool ok = static_cast<bool>(in >> channels >> sp.wx >> sp.wy >> sp.wz) && !(in >> rest) && (sp.channels = parse_channels(channels)) != 0;
      const int shells = ok ? rgpu_spectrum_shells(ctx_, &sp) : 0;
      if (shells == 0)
        throw std::runtime_error("[spectra] " + key + "=" + text + ": expected \"<channels> <wx> <wy> <wz>\" (channels of \"" RGPU_SPECTRUM_NAMES "\" or v, w, b, m, joined by commas; weights 0 .. " +
                                 std::to_string(RGPU_SPECTRUM_MAX_WEIGHT) + ", not all zero; at most " + std::to_string(RGPU_SPECTRUM_MAX_SHELLS) + " shells)");
      spectrum_specs.push_back(sp);
      std::string word = text;   // (one word in the list: the blanks become colons)
      for (char& ch : word) if (ch == ' ' || ch == '\t') ch = ':';
      spectrum_texts.push_back(word);
      spectrum_at.push_back(spectrum_at.back() + 2 * (size_t)shells);
    }
  }
  const bool spectra_on = !spectrum_specs.empty();
  const std::string spectra_list = rs_.outputDir + "/" + rs_.outputPrefix + "_spectra.txt";
  // n samples of all spectra: the .npy files and their lines in the list
  const auto spectra_files = [&](int n, const int* step, const double* t, const double* v) {
    std::ofstream list(spectra_list.c_str(), std::ios::app);
    if (!list) throw std::runtime_error("cannot write " + spectra_list);
    char num[64];
    for (int k = 0; k < n; ++k)
      for (size_t m = 0; m < spectrum_specs.size(); ++m) {
        std::snprintf(num, sizeof(num), "_spectrum%d_%07d.npy", (int)m, step[k]);
        const std::string name = rs_.outputPrefix + num, path = rs_.outputDir + "/" + name;
        const size_t doubles = spectrum_at[m + 1] - spectrum_at[m];
        // NumPy format 1.0, as the maps' files: the header padded with spaces to a multiple of 64
        std::string head = "{'descr': '<f8', 'fortran_order': False, 'shape': (2, " + std::to_string(doubles / 2) + "), }";
        head.append(63 - (10 + head.size()) % 64, ' ');
        head += "\n";
        std::ofstream f(path.c_str(), std::ios::binary | std::ios::trunc);
        const char magic[10] = {'\x93', 'N', 'U', 'M', 'P', 'Y', 1, 0, (char)(head.size() & 0xff), (char)(head.size() >> 8)};
        f.write(magic, 10);
        f.write(head.data(), (std::streamsize)head.size());
        f.write(reinterpret_cast<const char*>(v + (size_t)k * spectrum_at.back() + spectrum_at[m]), (std::streamsize)(doubles * sizeof(double)));
        if (!f) throw std::runtime_error("cannot write " + path);
        std::snprintf(num, sizeof(num), " %.17g", t[k]);
        list << step[k] << num << " " << m << " " << spectrum_texts[m] << " " << name << "\n";
      }
  };
  std::vector<double> spectra_v, spectra_t;
  std::vector<int> spectra_step;
  const auto spectra_direct = [&](int n) {   // the spectra of the current state U[n % 2]
    spectra_v.resize(std::max(spectra_v.size(), spectrum_at.back()));
    check(rgpu_state_spectra(ctx_, n % 2, (int)spectrum_specs.size(), spectrum_specs.data(), spectra_v.data()), "state_spectra");
    spectra_files(1, &n, &totalTime_, spectra_v.data());
  };
  if (spectra_on && !(totalTime_ > 0)) {   // the start of a run
    std::ofstream f(spectra_list.c_str(), std::ios::trunc);
    if (!f) throw std::runtime_error("cannot write " + spectra_list);
    f << "# nStep totalTime spectrum spec file\n";
  }
  // [helmholtz] enabled=yes every=N spectrum0="w 1 1 1" spectrum1="b 4 1 4" ... (up to spectrum3, numbered from 0 without a gap): the
  // solenoidal and the compressive power per shell of a vector field (include/rgpu.h, "Helmholtz spectra") on the terms of [spectra].
  // A spec is "<field> <wx> <wy> <wz>": one of RGPU_HELM_NAMES (m, v, w, b), then the three integer weights, none of them zero.  Each
  // sample of each spec is one file <outputDir>/<outputPrefix>_helmholtz<m>_<step, 7 digits>.npy -- '<f8', C order, shape (3, S): the
  // solenoidal power, the compressive power, then the modes of each shell -- and one line "step t spectrum spec file" of
  // <outputPrefix>_helmholtz.txt.  A batch serves one consumer: the Helmholtz spectra take the batches where none of the maps, the
  // PDFs and the spectra does, ahead of the monitor.  Not for z-slab, hooked or 2D runs, nor for a box with an extent that is no
  // power of two in 4 .. 1024: noted once, the run goes on.
  const bool helmEnabled = cfg_.get_bool("helmholtz", "enabled", false);
  const int helm_every = helmEnabled ? (int)cfg_.get_integer("helmholtz", "every", 10) : 0;
  if (helmEnabled && helm_every < 1) throw std::runtime_error("[helmholtz] every must be at least 1");
  bool noted_helm = false;
  if (helmEnabled && !spectra_box)
    note_once(&noted_helm, p_.nz_global == 1 ? "2D run: the Helmholtz spectrum files are not written" : (slab() || hooked_) ? "z-slab run: the Helmholtz spectrum files are not written"
                                                                                                      : "an extent of the box is not a power of two in 4 .. 1024: the Helmholtz spectrum files are not written");
  std::vector<rgpu_helm_spec> helm_specs;
  std::vector<std::string> helm_texts;
  std::vector<size_t> helm_at(1, 0);   // spec m of a sample begins at helm_at[m]; helm_at.back(): the doubles of a sample
  if (helmEnabled && spectra_box) {
    for (int m = 0; m < RGPU_HELM_MAX; ++m) {
      const std::string key = "spectrum" + std::to_string(m);
      std::string text = cfg_.get_string("helmholtz", key, "");
      if (text.empty()) break;
      if (text.size() >= 2 && text.front() == '"' && text.back() == '"') text = text.substr(1, text.size() - 2);
      std::istringstream in(text);
      std::string field, rest, name;
      rgpu_helm_spec sp = {};
      bool ok = static_cast<bool>(in >> field >> sp.wx >> sp.wy >> sp.wz) && !(in >> rest);
      std::istringstream names(RGPU_HELM_NAMES);
      sp.field = -1;
      for (int q = 0; names >> name; ++q)
        if (name == field) sp.field = q;
      ok = ok && sp.field >= 0;
      const int shells = ok ? rgpu_helm_shells(ctx_, &sp) : 0;
      if (shells == 0)
        throw std::runtime_error("[helmholtz] " + key + "=" + text + ": expected \"<field> <wx> <wy> <wz>\" (a field of \"" RGPU_HELM_NAMES "\"; weights 1 .. " +
                                 std::to_string(RGPU_SPECTRUM_MAX_WEIGHT) + "; at most " + std::to_string(RGPU_SPECTRUM_MAX_SHELLS) + " shells)");
      helm_specs.push_back(sp);
      std::string word = text;   // (one word in the list: the blanks become colons)
      for (char& ch : word) if (ch == ' ' || ch == '\t') ch = ':';
      helm_texts.push_back(word);
      helm_at.push_back(helm_at.back() + 3 * (size_t)shells);
    }
  }
  const bool helm_on = !helm_specs.empty();
  const std::string helm_list = rs_.outputDir + "/" + rs_.outputPrefix + "_helmholtz.txt";
  // n samples of all Helmholtz spectra: the .npy files and their lines in the list
  const auto helm_files = [&](int n, const int* step, const double* t, const double* v) {
    std::ofstream list(helm_list.c_str(), std::ios::app);
    if (!list) throw std::runtime_error("cannot write " + helm_list);
    char num[64];
    for (int k = 0; k < n; ++k)
      for (size_t m = 0; m < helm_specs.size(); ++m) {
        std::snprintf(num, sizeof(num), "_helmholtz%d_%07d.npy", (int)m, step[k]);
        const std::string name = rs_.outputPrefix + num, path = rs_.outputDir + "/" + name;
        const size_t doubles = helm_at[m + 1] - helm_at[m];
        // NumPy format 1.0, as the maps' files: the header padded with spaces to a multiple of 64
        std::string head = "{'descr': '<f8', 'fortran_order': False, 'shape': (3, " + std::to_string(doubles / 3) + "), }";
        head.append(63 - (10 + head.size()) % 64, ' ');
        head += "\n";
        std::ofstream f(path.c_str(), std::ios::binary | std::ios::trunc);
        const char magic[10] = {'\x93', 'N', 'U', 'M', 'P', 'Y', 1, 0, (char)(head.size() & 0xff), (char)(head.size() >> 8)};
        f.write(magic, 10);
        f.write(head.data(), (std::streamsize)head.size());
        f.write(reinterpret_cast<const char*>(v + (size_t)k * helm_at.back() + helm_at[m]), (std::streamsize)(doubles * sizeof(double)));
        if (!f) throw std::runtime_error("cannot write " + path);
        std::snprintf(num, sizeof(num), " %.17g", t[k]);
        list << step[k] << num << " " << m << " " << helm_texts[m] << " " << name << "\n";
      }
  };
  std::vector<double> helm_v, helm_t;
  std::vector<int> helm_step;
  const auto helm_direct = [&](int n) {   // the Helmholtz spectra of the current state U[n % 2]
    helm_v.resize(std::max(helm_v.size(), helm_at.back()));
    check(rgpu_state_helm_spectra(ctx_, n % 2, (int)helm_specs.size(), helm_specs.data(), helm_v.data()), "state_helm_spectra");
    helm_files(1, &n, &totalTime_, helm_v.data());
  };
  if (helm_on && !(totalTime_ > 0)) {   // the start of a run
    std::ofstream f(helm_list.c_str(), std::ios::trunc);
    if (!f) throw std::runtime_error("cannot write " + helm_list);
    f << "# nStep totalTime spectrum spec file\n";
  }
  const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  while (totalTime_ < rs_.tEnd && nStep < rs_.nStepmax) {
    if (rs_.nLog > 0 && (nStep % rs_.nLog) == 0 && p_.slab_rank == 0)
      std::printf("  step=%9d t=%14.8f dt=%16.12f\n", nStep, totalTime_, dt);
    if (rs_.nOutput > 0 && (nStep % rs_.nOutput) == 0) {   // noutput <= 0: no output (the reference divides by zero here)
      const std::chrono::steady_clock::time_point w0 = std::chrono::steady_clock::now();
      const bool raw = (rs_.outputXsm || rs_.outputNrrd) && !slab();
      if (rs_.outputVtk || rs_.outputRestart || raw) copyGpuToCpu(nStep);
      if (raw && rs_.outputXsm) outputXsm(nStep);
      if (raw && rs_.outputNrrd) outputNrrd(nStep);
      if (rs_.outputVtk && !slab()) outputVtk(nStep);
      if (rs_.outputVtk && slab()) outputVtkSlab(nStep);
      if (rs_.outputRestart) outputHdf5(nStep);
      if ((rs_.outputVtk || rs_.outputRestart) && p_.slab_rank == 0) save_forcing_process(nStep);
      io_seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - w0).count();
      if (p_.slab_rank == 0) std::printf("  step=%9d t=%14.8f dt=%16.12f\n", nStep, totalTime_, dt);
    }
    if (historyEnabled && slab() && !slab_history_ok) note_once(&noted_hist_, "z-slab run: this problem's history file is not written");
    if (historyEnabled && !history_batched && (!slab() || slab_history_ok) && history_due()) {
      history(nStep, dt);
      tHist += dtHist;
    }
    // the turns of this loop up to the next one that logs, writes or records history do nothing but step: rgpu_run_steps runs them
    // (same states, same dt sequence; where a step is one fused kernel the time step stays on the device in between)
    int quiet = 1;
    if ((!hooked_ || hooks_.run_steps) && (!historyEnabled || history_batched)) {
      quiet = rs_.nStepmax - nStep;
      if (rs_.nLog > 0 && rs_.nLog - nStep % rs_.nLog < quiet) quiet = rs_.nLog - nStep % rs_.nLog;
      if (rs_.nOutput > 0 && rs_.nOutput - nStep % rs_.nOutput < quiet) quiet = rs_.nOutput - nStep % rs_.nOutput;
    }
    // a batch serves one consumer: where the maps take it, the monitor rows come from the direct calls
    const bool maps_batched = maps_on && !historyEnabled && quiet > 1;
    const bool pdfs_batched = pdfs_on && !historyEnabled && quiet > 1 && !maps_batched;
    const bool spectra_batched = spectra_on && !historyEnabled && quiet > 1 && !maps_batched && !pdfs_batched;
    const bool helm_batched = helm_on && !historyEnabled && quiet > 1 && !maps_batched && !pdfs_batched && !spectra_batched;
    const bool monitor_batched = monitor_on && !historyEnabled && quiet > 1 && !maps_batched && !pdfs_batched && !spectra_batched && !helm_batched;
    if (monitor_on && !monitor_batched && mon_every - nStep % mon_every < quiet) quiet = mon_every - nStep % mon_every;   // the direct call follows
    if (maps_on && !maps_batched && maps_every - nStep % maps_every < quiet) quiet = maps_every - nStep % maps_every;      // the direct call follows
    if (pdfs_on && !pdfs_batched && pdfs_every - nStep % pdfs_every < quiet) quiet = pdfs_every - nStep % pdfs_every;      // the direct call follows
    if (spectra_on && !spectra_batched && spectra_every - nStep % spectra_every < quiet) quiet = spectra_every - nStep % spectra_every;   // the direct call follows
    if (helm_on && !helm_batched && helm_every - nStep % helm_every < quiet) quiet = helm_every - nStep % helm_every;   // the direct call follows
    const int nStep_before = nStep;
    if (helm_batched) {
      int mn = 0;
      const size_t cap = (size_t)(quiet / helm_every + 1);
      if (helm_step.size() < cap) { helm_step.resize(cap); helm_t.resize(cap); }
      if (helm_v.size() < cap * helm_at.back()) helm_v.resize(cap * helm_at.back());
      const int rc = rgpu_run_steps_helm_spectra(ctx_, quiet, rs_.tEnd, &nStep, &totalTime_, &dt, 0, helm_every, (int)helm_specs.size(), helm_specs.data(), &mn, helm_step.data(), helm_t.data(), helm_v.data());
      helm_files(mn, helm_step.data(), helm_t.data(), helm_v.data());
      if (rc < 0) check(rc, "run_steps_helm_spectra");
    } else if (spectra_batched) {
      int mn = 0;
      const size_t cap = (size_t)(quiet / spectra_every + 1);
      if (spectra_step.size() < cap) { spectra_step.resize(cap); spectra_t.resize(cap); }
      if (spectra_v.size() < cap * spectrum_at.back()) spectra_v.resize(cap * spectrum_at.back());
      const int rc = rgpu_run_steps_spectra(ctx_, quiet, rs_.tEnd, &nStep, &totalTime_, &dt, 0, spectra_every, (int)spectrum_specs.size(), spectrum_specs.data(), &mn, spectra_step.data(), spectra_t.data(),
                                            spectra_v.data());
      spectra_files(mn, spectra_step.data(), spectra_t.data(), spectra_v.data());
      if (rc < 0) check(rc, "run_steps_spectra");
    } else if (pdfs_batched) {
      int mn = 0;
      const size_t cap = (size_t)(quiet / pdfs_every + 1);
      if (pdfs_step.size() < cap) { pdfs_step.resize(cap); pdfs_t.resize(cap); }
      if (pdfs_v.size() < cap * pdf_at.back()) pdfs_v.resize(cap * pdf_at.back());
      const int rc = rgpu_run_steps_pdfs(ctx_, quiet, rs_.tEnd, &nStep, &totalTime_, &dt, 0, pdfs_every, (int)pdf_specs.size(), pdf_specs.data(), &mn, pdfs_step.data(), pdfs_t.data(), pdfs_v.data());
      pdfs_files(mn, pdfs_step.data(), pdfs_t.data(), pdfs_v.data());
      if (rc < 0) check(rc, "run_steps_pdfs");
    } else if (maps_batched) {
      int mn = 0;
      const size_t cap = (size_t)(quiet / maps_every + 1);
      if (maps_step.size() < cap) { maps_step.resize(cap); maps_t.resize(cap); }
      if (maps_v.size() < cap * map_at.back()) maps_v.resize(cap * map_at.back());
      const int rc = rgpu_run_steps_mapped(ctx_, quiet, rs_.tEnd, &nStep, &totalTime_, &dt, 0, maps_every, (int)map_specs.size(), map_specs.data(), &mn, maps_step.data(), maps_t.data(), maps_v.data());
      maps_files(mn, maps_step.data(), maps_t.data(), maps_v.data());
      if (rc < 0) check(rc, "run_steps_mapped");
    } else if (monitor_batched && planes_on) {
      int mn = 0;
      const size_t cap = (size_t)(quiet / mon_every + 1);
      if (mon_step.size() < cap) { mon_step.resize(cap); mon_t.resize(cap); }
      if (planes_v.size() < cap * planes_nz * RGPU_MONP_NQ) planes_v.resize(cap * planes_nz * RGPU_MONP_NQ);
      const int rc = rgpu_run_steps_monitored_planes(ctx_, quiet, rs_.tEnd, &nStep, &totalTime_, &dt, 0, mon_every, &mn, mon_step.data(), mon_t.data(), planes_v.data());
      planes_rows(mn, mon_step.data(), mon_t.data(), planes_v.data());
      if (rc < 0) check(rc, "run_steps_monitored_planes");
    } else if (monitor_batched) {
      int mn = 0;
      const size_t cap = (size_t)(quiet / mon_every + 1);
      if (mon_step.size() < cap) { mon_step.resize(cap); mon_t.resize(cap); mon_v.resize(cap * RGPU_MON_NQ); }
      const int rc = rgpu_run_steps_monitored(ctx_, quiet, rs_.tEnd, &nStep, &totalTime_, &dt, 0, mon_every, &mn, mon_step.data(), mon_t.data(), mon_v.data());
      monitor_rows(mn, mon_step.data(), mon_t.data(), mon_v.data());
      if (rc < 0) check(rc, "run_steps_monitored");
    } else if (history_batched) {
      int hn = 0;
      if ((int)hist_step.size() < quiet) { hist_step.resize(quiet); hist_t.resize(quiet); hist_dt.resize(quiet); hist_v.resize((size_t)quiet * RGPU_HIST_NQ); }
      const int rc = rgpu_run_steps_history(ctx_, quiet, rs_.tEnd, &nStep, &totalTime_, &dt, 0, dtHist, &tHist, &hn, hist_step.data(), hist_t.data(), hist_dt.data(), hist_v.data());
      for (int k = 0; k < hn; ++k) write_history_row(history_kind == 1, hist_t[k], hist_dt[k], &hist_v[(size_t)k * RGPU_HIST_NQ]);
      if (rc < 0) check(rc, "run_steps_history");
    } else if (quiet > 1) {
      if (hooked_) {
        const int rc = hooks_.run_steps(hooks_.self, quiet, rs_.tEnd, &nStep, &totalTime_, &dt);
        if (rc < 0) hook_check(rc, "run_steps");
      } else {
        const int rc = rgpu_run_steps(ctx_, quiet, rs_.tEnd, &nStep, &totalTime_, &dt);
        if (rc < 0) check(rc, "run_steps");
      }
    } else {
      oneStepIntegration(nStep, totalTime_, dt);
    }
    if (monitor_on && !monitor_batched && nStep > nStep_before && nStep % mon_every == 0) monitor_direct(nStep);
    if (maps_on && !maps_batched && nStep > nStep_before && nStep % maps_every == 0) maps_direct(nStep);
    if (pdfs_on && !pdfs_batched && nStep > nStep_before && nStep % pdfs_every == 0) pdfs_direct(nStep);
    if (spectra_on && !spectra_batched && nStep > nStep_before && nStep % spectra_every == 0) spectra_direct(nStep);
    if (helm_on && !helm_batched && nStep > nStep_before && nStep % helm_every == 0) helm_direct(nStep);
  }
  check(rgpu_synchronize(ctx_), "synchronize");
  if (hooked_) hook_check(hooks_.barrier(hooks_.self), "barrier");
  {
    const std::chrono::steady_clock::time_point w0 = std::chrono::steady_clock::now();
    const bool raw = (rs_.outputXsm || rs_.outputNrrd) && !slab();
    if (rs_.outputVtk || rs_.outputRestart || raw) copyGpuToCpu(nStep);
    if (raw && rs_.outputXsm) outputXsm(nStep);
    if (raw && rs_.outputNrrd) outputNrrd(nStep);
    if (rs_.outputVtk && !slab()) outputVtk(nStep);
    if (rs_.outputVtk && slab()) outputVtkSlab(nStep);
    if (rs_.outputRestart) outputHdf5(nStep);
    if ((rs_.outputVtk || rs_.outputRestart) && p_.slab_rank == 0) save_forcing_process(nStep);
    // the XDMF index of the .h5 files of this run, in the current directory (MHDRunGodunov.cpp:4004)
    if (wrote_hdf5_ && p_.slab_rank == 0)
      xdmf_write_wrapper(rs_.outputPrefix, h5_box(p_.nx, p_.ny, (p_.nz_global != 1) ? p_.nz_global : 1), rs_.ghostIncluded, nStep, rs_.nOutput);
    io_seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - w0).count();
  }
  const double total = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  const double nz = (p_.nz_global != 1) ? p_.nz_global : 1;   // a slab reports the rate of the whole box
  const double rate = 1.0 * nStep * p_.nx * p_.ny * nz / (total - io_seconds);
  if (p_.slab_rank == 0) {
    std::cout << "DEBUG : totalTime " << std::setprecision(12) << totalTime_ << std::endl;
    std::cout << "####################################\nGlobal performance                  \n"
              << rate << " cell updates per seconds (based on wall time)\n####################################\n";
  }
  if (mcell_per_s) *mcell_per_s = rate / 1e6;
  return nStep;
}

}  // namespace rgpu_host

extern "C" int rgpuh_run_hooked(const char* ini_path, const char* overrides, int slab_rank, int slab_count, rgpuh_attach_fn attach,
                                rgpuh_detach_fn detach, void* user, double* mcell_per_s, char* err, int err_len) {
  int n = RGPU_EINVAL;
  try {
    if (!attach) throw std::runtime_error("run_hooked: no attach function");
    rgpu_host::IniConfig cfg;
    const int rc = cfg.load_file(ini_path ? ini_path : "");
    if (rc != 0) throw std::runtime_error(std::string("cannot read parameter file ") + (ini_path ? ini_path : "(null)"));
    if (overrides) cfg.apply_overrides(overrides);
    rgpu_host::GodunovRun run(cfg, slab_rank, slab_count);
    try {
      n = run.start(mcell_per_s, attach, user);
    } catch (...) {
      if (detach) detach(user);   // the slab driver refers to the context: release it before the run object goes
      throw;
    }
    if (detach) detach(user);
  } catch (const std::exception& e) {
    if (err && err_len > 0) std::snprintf(err, static_cast<size_t>(err_len), "%s", e.what());
    return RGPU_EINVAL;
  }
  return n;
}

extern "C" int rgpuh_run(const char* ini_path, const char* overrides, double* mcell_per_s, char* err, int err_len) {
  try {
    rgpu_host::IniConfig cfg;
    const int rc = cfg.load_file(ini_path ? ini_path : "");
    if (rc != 0) throw std::runtime_error(std::string("cannot read parameter file ") + (ini_path ? ini_path : "(null)"));
    if (overrides) cfg.apply_overrides(overrides);
    rgpu_host::GodunovRun run(cfg);
    return run.start(mcell_per_s);
  } catch (const std::exception& e) {
    if (err && err_len > 0) std::snprintf(err, static_cast<size_t>(err_len), "%s", e.what());
    return RGPU_EINVAL;
  }
}
