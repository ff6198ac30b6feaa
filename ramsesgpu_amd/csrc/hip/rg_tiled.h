// rg_tiled.h (HIP / gfx950) -- cooperative LDS-tiled kernels of the backend.  The step driver calls
//   rgpu_tiled::hydro3d_sweep(...)      whole 3D hydro step for a plane range
//   rgpu_tiled::mhd3d_sweep(...)        trace + Riemann problems of the 3D MHD step for a plane range
//   rgpu_tiled::mhd2d_step(...)         whole 2D MHD step
//   rgpu_tiled::hydro2d_step(...)       whole 2D hydro step
//   rgpu_tiled::hydro2d_ensemble_step(...) / mhd2d_ensemble_step(...)   the same for every member of an ensemble of 2D boxes (ensemble2d.h)
// each returning 0 = done, 1 = configuration not covered (the driver runs the flat per-cell kernels), < 0 = error.
#pragma once
#include "tiled_hydro.h"
#include "tiled_mhd.h"
#include "tiled_mhd2d.h"
#include "tiled_hydro2d.h"
#include "ensemble2d.h"
// the ensemble kernels exist (api/entry_ensemble.h: without this macro -- the test-only host emulation -- an ensemble steps member by member)
#define RGPU_TILED_ENSEMBLE2D 1
#include "monitor3d.h"
// the gfx950 kernels of a lone context's monitor exist (api/monitor.h: without this macro it runs the flat functors)
#define RGPU_TILED_MONITOR3D 1
#include "monitor_profile.h"
// the gfx950 kernels of the plane monitor exist (api/monitor.h: without this macro it runs the flat functors)
#define RGPU_TILED_MONITOR_PROFILE 1
#include "monitor_maps.h"
// the gfx950 kernels of the map monitor exist (api/monitor.h: without this macro it runs the flat functor)
#define RGPU_TILED_MONITOR_MAPS 1
#include "monitor_pdf.h"
// the gfx950 kernels of the PDF monitor exist (api/monitor.h: without this macro it runs the flat functors)
#define RGPU_TILED_MONITOR_PDF 1
#include "monitor_spectrum.h"
// the gfx950 kernels of the spectrum monitor exist (api/monitor.h: without this macro it runs the flat functors)
#define RGPU_TILED_MONITOR_SPECTRUM 1
#include "monitor_helm.h"
// the gfx950 kernels of the Helmholtz spectra exist (api/monitor.h: without this macro they run the flat functors)
#define RGPU_TILED_MONITOR_HELM 1
