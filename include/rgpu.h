/*
 * rgpu.h -- C ABI of the MI355X-native Godunov / MUSCL-Hancock unsplit time step
 *           (hydro HLLC/approx/HLL, MHD HLLD + constrained transport, shearing box).
 *
 * This is the drop-in boundary for ONE hot path of pkestene/ramsesGPU: the body of
 *   HydroRunBase::oneStepIntegration(int& nStep, real_t& t, real_t& dt)   (HydroRunBase.h:433)
 *     = compute_dt[_mhd](nStep % 2) + godunov_unsplit(nStep, dt)          (MHDRunGodunov.cpp:4077-4089,
 *                                                                           HydroRunGodunov.cpp:4082-4126)
 * plus the ghost fill it calls (make_all_boundaries / make_all_boundaries_shear).
 * The reference has no FFI; its seam is that C++ virtual interface with state in the protected members
 * h_U,h_U2,d_U,d_U2 (HydroRunBase.h:556-566).  A maintainer binds these entry points from the run classes
 * (see INTEGRATION.md).  Everything is plain C: pointers, sizes, doubles.  No torch / HIP types.
 *
 * Array layout (contract shared with the reference's HostArray/DeviceArray, Arrays.h:95-98,236-239):
 *   U[ i + isize*( j + jsize*( k + ksize*ivar ) ) ],  fp64, ghost cells included,
 *   isize = nx+2*ghostWidth, jsize = ny+2*ghostWidth, ksize = nz+2*ghostWidth (1 in 2D),
 *   component order ID,IP,IU,IV,IW,IA,IB,IC (constants.h:59-71); hydro uses the first 4 (2D) / 5 (3D).
 *   Sizes are 64-bit here (the reference's uint sizes overflow at 518^3 x 8).
 *
 * Error model: every int entry point returns 0 on success or a negative RGPU_E* code; the message is kept in
 * the context (rgpu_last_error).  The reference exit()s on CUDA failure (cutil_inline_runtime.h:167-174); a
 * library must not.  Not thread-safe per context (the reference is single-threaded per run object).
 * All entry points return with their results visible to the next call (internally asynchronous on one stream).
 */
#ifndef RGPU_H_
#define RGPU_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RGPU_ABI_VERSION 5   /* layout of rgpu_params; new entry points do not change it */

/* component indexes -- constants.h:59-71 */
enum { RGPU_ID = 0, RGPU_IP = 1, RGPU_IU = 2, RGPU_IV = 3, RGPU_IW = 4, RGPU_IA = 5, RGPU_IB = 6, RGPU_IC = 7 };

/* BoundaryConditionType -- constants.h:209-217 */
enum {
  RGPU_BC_UNDEFINED = 0, RGPU_BC_DIRICHLET = 1, RGPU_BC_NEUMANN = 2, RGPU_BC_PERIODIC = 3,
  RGPU_BC_SHEARINGBOX = 4,
  RGPU_BC_COPY = 5 /* ghost planes are supplied by a neighbour slab (or any external z driver).  The planes written into the ghost region of
                    * such a face must be COMPLETE planes of the neighbour's state -- its x / y ghost cells and corners included, i.e. taken
                    * after the neighbour's own x / y fill: the library fills x / y ghosts on the interior planes only and does not re-run
                    * the X / Y passes over received planes (librgpu_comm.so sends such planes) */,
  RGPU_BC_Z_STRATIFIED = 6 /* z faces of the vertically stratified MRI box (3D MHD, isothermal, Omega0 > 0):
                            * make_boundary2_z_stratified, make_boundary_base.h:1356-1647 */
};

/* RiemannSolverType -- constants.h:140-146 */
enum { RGPU_RS_APPROX = 0, RGPU_RS_HLL = 1, RGPU_RS_HLLC = 2, RGPU_RS_HLLD = 3, RGPU_RS_LLF = 4 };
/* MagneticRiemannSolverType -- constants.h:149-156 */
enum { RGPU_MAG_HLLD = 0, RGPU_MAG_HLLF = 1, RGPU_MAG_HLLA = 2, RGPU_MAG_ROE = 3, RGPU_MAG_LLF = 4, RGPU_MAG_UPWIND = 5 };

/* direction ids used by rgpu_make_boundaries -- constants.h:220 (XDIR=1,YDIR=2,ZDIR=3) */
enum { RGPU_XDIR = 1, RGPU_YDIR = 2, RGPU_ZDIR = 3 };

/* error codes */
enum {
  RGPU_OK = 0, RGPU_EINVAL = -1, RGPU_ENODEVICE = -2, RGPU_ENOMEM = -3, RGPU_EHIP = -4, RGPU_EUNSUPPORTED = -5
};

/*
 * Scalar knobs of one run: 1:1 with GlobalConstants (constants.h:277-317) and the HydroParameters members the
 * path reads (HydroParameters.h:73-136), with the derivations of HydroParameters.h:196-325 ALREADY APPLIED by
 * the host (float-parsed values widened to double, smallp/smallpp/gamma6 derived, MHD => ghostWidth 3, nbVar 8).
 */
typedef struct rgpu_params {
  int32_t abi_version;          /* must be RGPU_ABI_VERSION */
  int32_t nx, ny, nz;           /* interior cells of THIS domain (a z-slab when slab_count>1); nz=1 => 2D */
  int32_t ghostWidth;           /* 2 hydro, 3 MHD (HydroParameters.h:260-271) */
  int32_t nbVar;                /* 4 hydro 2D, 5 hydro 3D, 8 MHD (HydroParameters.h:204-235) */
  int32_t mhdEnabled;
  int32_t bc[6];                /* xmin,xmax,ymin,ymax,zmin,zmax (HydroParameters.h:253-258) */
  double  xMin, xMax, yMin, yMax, zMin, zMax;   /* GLOBAL box (HydroParameters.h:238-243) */
  double  dx, dy, dz;           /* HydroParameters.h:245-247 (dz from the GLOBAL nz) */
  double  cfl;                  /* HydroParameters.h:274-282 */
  double  gamma0, cIso, smallr, smallc, smalle, smallp, smallpp, gamma6;   /* HydroParameters.h:292-312 */
  double  Omega0;               /* [MHD] omega0 (HydroParameters.h:313) */
  double  slope_type;           /* HydroParameters.h:319-321 */
  int32_t niter_riemann, iorder;
  int32_t riemannSolver;        /* RGPU_RS_*  (HydroParameters.h:353-381) */
  int32_t magRiemannSolver;     /* RGPU_MAG_* (HydroParameters.h:388-417) */
  int32_t implementationVersion;/* [MHD] implementationVersion: 2D 0 or 1; 3D 3/4 (Omega0>0 forces 1/4, MHDRunGodunov.cpp:119-126) */
  int32_t unsplitVersion;       /* [hydro] unsplitVersion: 1 or 2 (HydroRunGodunov.cpp:1852-1866; 2 = direction-wise sweeps) */
  int32_t shearingBoxEnabled;   /* bc xmin==xmax==4 and Omega0>0 (MHDRunGodunov.cpp:97-103) */
  int32_t enableJet, ijet, offsetJet;  /* HydroParameters.h:435-444 */
  double  djet, ujet, pjet, cjet;
  /* z-slab decomposition (replaces the reference's MPI cartesian topology, HydroMpiParameters.cpp:44-80) */
  int32_t slab_rank, slab_count;/* 0,1 for a single device */
  int32_t nz_global;            /* == nz when slab_count==1 */
  int32_t gravityEnabled;       /* [gravity] static=yes, or forced by problem=Rayleigh-Taylor (HydroRunBase.cpp:250-260):
                                 * 1 = the uniform vector below, 2 = a per-cell field given with rgpu_set_gravity_field */
  /* uniform static gravity field ([gravity] static_field_x/y/z, HydroParameters.h:322-324): the reference keeps it in a
   * per-cell array h_gravity that its problems fill with exactly this vector (HydroRunBase.cpp:6336-6337, 6403-6405) */
  double  gravity_x, gravity_y, gravity_z;
  /* dissipative stage after the Godunov update (HydroParameters.h:327-328): kinematic viscosity [hydro] nu and
   * resistivity [MHD] eta; 0 = off */
  double  nu, eta;
  int32_t zStratifiedFloor;     /* [MRI] floor (HydroRunBase.cpp:2206): RGPU_BC_Z_STRATIFIED copies the density instead of
                                 * extrapolating the hydrostatic profile */
  int32_t randomForcingEnabled; /* problem "turbulence" (HydroRunBase.cpp:213-227): the static solenoidal driving field of
                                 * rgpu_set_forcing_field is added to the momenta at the end of every step, scaled so that
                                 * the kinetic energy input rate is randomForcingEdot (3D, no rotating frame) */
  double  randomForcingEdot;    /* [turbulence] edot, or the Mac Low (1999) estimate when negative (HydroRunBase.cpp:7175-7194) */
  /* problem "turbulence-Ornstein-Uhlenbeck" (HydroRunBase.cpp:230-247): 31 Fourier modes of a forcing field driven by an
   * Ornstein-Uhlenbeck process (ForcingOrnsteinUhlenbeck, Forcing_OrnsteinUhlenbeck.cpp) are advanced on the host every
   * step and their real-space sum accelerates the gas at the end of the step (3D, no rotating frame).  The context owns
   * the process (mode signs, projection tensor, the four-digit base-4096 seed of RandomGen); every z-slab runs the same one. */
  int32_t ouForcingEnabled;
  int32_t ouInitRandom;         /* [turbulence-Ornstein-Uhlenbeck] init_random (seed of the Gaussian generator) */
  double  ouTimeScaleTurb, ouAmplitudeTurb, ouKsi;   /* timeScaleTurb, amplitudeTurb, ksi (1 solenoidal .. 0 compressive) */
} rgpu_params;

typedef struct rgpu_ctx rgpu_ctx;

/* ---- life cycle ------------------------------------------------------------------------------------------ */

/* Allocates U, U2 and all scratch on the current HIP device.  Replaces the allocations of the HydroRunBase /
 * MHDRunGodunov constructors (HydroRunBase.cpp:92-300, MHDRunGodunov.cpp:128-418).  Fails with RGPU_ENODEVICE when
 * no GPU is present: there is NO CPU fallback.
 * Size limit: the kernels address a cell of one context with a 32-bit flat index (byte offsets and component strides are
 * 64-bit), so (nx + 2 gw)(ny + 2 gw)(nz + 2 gw) must stay below 2^32 - 1 cells PER CONTEXT -- 1619^3 with gw = 3; at the 34
 * doubles per cell of the 3D MHD step that is 1.17 TB, four times the 288 GB of one MI355X, so the memory is exhausted long
 * before the index.  rgpu_create checks it and fails with RGPU_EUNSUPPORTED ("more than 2^32 cells per device"); larger boxes
 * run as z-slabs (rgpu_comm.h), every slab its own context.  (The reference's 32-bit BYTE offsets overflow at 518^3 x 8.) */
int rgpu_create(const rgpu_params* p, rgpu_ctx** out);

/* Same, but U and U2 are device buffers owned by the caller (e.g. torch tensors) of rgpu_state_elems() doubles
 * each, and work is issued on the caller's hipStream_t (pass NULL for the default stream). */
int rgpu_create_external(const rgpu_params* p, double* dU, double* dU2, void* hip_stream, rgpu_ctx** out);

void rgpu_destroy(rgpu_ctx* c);

/* number of doubles in one state array: isize*jsize*ksize*nbVar */
size_t rgpu_state_elems(const rgpu_params* p);

/* bytes of device memory rgpu_create will allocate (U, U2 and scratch) */
size_t rgpu_device_bytes(const rgpu_params* p);

const char* rgpu_last_error(rgpu_ctx* c);

/* ---- host <-> device (init, output, history only; never inside the step) ---------------------------------- */

/* == d_U.copyFromHost(h_U) [+ d_U2] (MHDRunBase.cpp:1346-1351) */
int rgpu_upload(rgpu_ctx* c, const double* hU, int both);
/* == copyGpuToCpu(nStep) + getDataHost(nStep) (HydroRunBase.cpp:7217-7229, 2442-2447); parity = nStep%2 */
int rgpu_download(rgpu_ctx* c, double* hU, int parity);
/* Static gravity field of a context created with gravityEnabled = 2: hG[3][ksize][jsize][isize] (ghost cells included,
 * the z component ignored in 2D) = the reference's h_gravity / d_gravity (HydroRunBase.h, filled by the initial
 * conditions of Keplerian-disk, HydroRunBase.cpp:6489-6500, and of the stratified MRI box, MHDRunBase.cpp:3163-3211).
 * Until it is called the field is zero, like the reference's freshly allocated array. */
int rgpu_set_gravity_field(rgpu_ctx* c, const double* hG);
/* Driving of the "turbulence" problem (randomForcingEnabled): hF[3][ksize][jsize][isize] = the reference's
 * h_randomForcing / d_randomForcing (turbulenceInit.cpp, copied to the device at HydroRunBase.cpp:7206-7209).
 * rgpu_godunov_unsplit applies it after the dissipative stage like the reference (HydroRunGodunov.cpp:2930-2938,
 * mhd_godunov_unsplit_cpu_v3.cpp:696-704).  A z-slab driver does the same in pieces: rgpu_forcing_sums returns
 * out[2] = { sum rho v.f , sum rho f.f } over the interior of this domain (compute_random_forcing_normalization,
 * HydroRunBase.cpp:1201-1312; the other seven sums of the reference are debug output), the caller adds the slabs'
 * values, computes norm = (sqrt(s0^2 + s1 dt edot 2 nbCells) - s0) / s1 and calls rgpu_add_forcing
 * (add_random_forcing, HydroRunBase.cpp:1397-1428).  The sums are accumulated in a fixed order that is not the
 * reference's loop order: results agree with the reference to round-off, not bit for bit. */
int rgpu_set_forcing_field(rgpu_ctx* c, const double* hF);
/* ForcingOrnsteinUhlenbeck::add_forcing_field (Forcing_OrnsteinUhlenbeck.cpp:498-549, 597-686) on U[parity]: one
 * Ornstein-Uhlenbeck update of the 31 modes with time step dt (host; RandomGen::gaussDev), then momenta and total energy
 * of every interior cell get the real-space sum of the modes.  rgpu_godunov_unsplit calls it itself after the dissipative
 * stage like the reference (HydroRunGodunov.cpp:2940-2945, mhd_godunov_unsplit_cpu_v3.cpp:706-710); a z-slab driver calls
 * it on every slab (same process on every rank, no communication).  The device evaluates cos() with its own libm: states
 * agree with the reference to round-off (relative L2 ~1e-16 per step), not bit for bit.
 * rgpu_ou_forcing_state copies out mode[3][31], forcingField[3][31] (what output_forcing writes, :392-444). */
int rgpu_step_ou_forcing(rgpu_ctx* c, int parity, double dt);
int rgpu_ou_forcing_state(rgpu_ctx* c, double* mode93, double* forcingField93);
/* The whole process (modes, amplitudes, projection tensor, generator) as RGPU_OU_STATE_DOUBLES doubles, for restart files:
 * get before writing one, set after rgpu_create when resuming (the reference keeps a *_forcing_NNNNNNN.npz for the same
 * purpose, output_forcing / init_forcing(restart), Forcing_OrnsteinUhlenbeck.cpp:236-352, 392-444). */
#define RGPU_OU_STATE_DOUBLES 471
int rgpu_ou_forcing_get_state(rgpu_ctx* c, double* state);
int rgpu_ou_forcing_set_state(rgpu_ctx* c, const double* state);
int rgpu_forcing_sums(rgpu_ctx* c, int parity, double* out);
int rgpu_add_forcing(rgpu_ctx* c, int parity, double norm);
/* raw device pointers of U (parity 0) / U2 (parity 1), for zero-copy halo exchange */
double* rgpu_device_state(rgpu_ctx* c, int parity);
/* What a communication layer (include/rgpu_comm.h) needs to work on a context without host round trips: the parameters
 * the context was created with, the HIP stream its kernels are queued on (hipStream_t as void*), and the 8-byte device
 * slot the CFL scan leaves its maximum in (a non-negative double; rgpu_inv_dt_result reads it back) -- the operand
 * of the MAX all-reduce that replaces the reference's MPI allReduce of dt (HydroRunBaseMpi.cpp:509-513). */
int rgpu_get_params(rgpu_ctx* c, rgpu_params* out);
void* rgpu_stream_handle(rgpu_ctx* c);
double* rgpu_inv_dt_device_slot(rgpu_ctx* c);
/* The slot is the first of RGPU_DT_SLOTS doubles (zero at create): the update kernels that carry the CFL scan of the new state
 * spread their maxima over all of them (rgpu_inv_dt_fused_commit).  A communication layer all-reduces ALL RGPU_DT_SLOTS values,
 * whatever the step left in them -- a fixed count, so that ranks in different states (first step, a failed step piece) can never
 * post all-reduces of different sizes; rgpu_inv_dt_result reads the ones that are valid. */
#define RGPU_DT_SLOTS 1024
#define RGPU_CLOCK_BATCH 256   /* steps per batch of the device-side time step (rgpu_clock_open .. rgpu_clock_close) */

/* ---- the path ------------------------------------------------------------------------------------------- */

/* Ghost fill of one direction: make_boundaries(U, idim) (HydroRunBase.cpp:2276-2316), incl. make_jet.
 * Faces whose bc is RGPU_BC_COPY or RGPU_BC_SHEARINGBOX are left untouched. */
int rgpu_make_boundaries(rgpu_ctx* c, int parity, int idim);

/* Shearing-box remap of the x ghosts: MHDRunGodunov::make_boundaries_shear (MHDRunGodunov.cpp:3539-3759).
 * totalTime is the time at the START of the step that produced U[parity], dt its time step
 * (the remap uses totalTime+dt, :3554). */
int rgpu_make_boundaries_shear(rgpu_ctx* c, int parity, double totalTime, double dt);

/* make_all_boundaries (X,Y,Z; HydroRunBase.cpp:2333-2342) or, when shearingBoxEnabled and 3D,
 * make_all_boundaries_shear (Y, shear, Z, Y; MHDRunGodunov.cpp:3779-3793). */
int rgpu_make_all_boundaries(rgpu_ctx* c, int parity, double totalTime, double dt);

/* max over the interior of the inverse time step: the invDt of compute_dt (HydroRunBase.cpp:372-426) /
 * compute_dt_mhd (MHDRunBase.cpp:140-250) BEFORE "cfl / invDt"; with slabs the caller max-reduces it. */
int rgpu_compute_inv_dt(rgpu_ctx* c, int parity, double* invDt);

/* Tell the context that the caller changed U[0] / U[1] behind its back (arrays adopted with rgpu_create_external and
 * written by the host program; the reference has no counterpart: its compute_dt always rescans).  Where nothing modifies the
 * new state between the step and the next compute_dt, the step's last kernel carries the CFL scan and rgpu_compute_dt only
 * reads the result back; after this call the next rgpu_compute_dt scans the arrays again.  The ghost-fill entry points above
 * do it themselves when they can change what the scan reads (any face that is not periodic / copy / shearing, the jet). */
int rgpu_invalidate_dt(rgpu_ctx* c);

/* == compute_dt[_mhd](useU): cfl / invDt.  Returns NaN on error (see rgpu_last_error). */
double rgpu_compute_dt(rgpu_ctx* c, int useU);

/* == godunov_unsplit(nStep, dt) (MHDRunGodunov.cpp:572-617, HydroRunGodunov.cpp:419-441): reads U[nStep%2],
 * writes U[(nStep+1)%2].  Plain path fills the ghosts of the INPUT at entry; the rotating path (Omega0>0) fills
 * the ghosts of the OUTPUT at exit (MHDRunGodunov.cpp:2031-3440).  totalTime is needed by the shear remaps
 * (:3213, :3554).  With RGPU_BC_COPY z faces use the three calls below instead. */
int rgpu_godunov_unsplit(rgpu_ctx* c, int nStep, double dt, double totalTime);

/* The same step cut at the points where a z-slab driver exchanges ghost planes:
 *   plain   : pre (X,Y fill of input) -> [exchange z ghosts of input]  -> core -> post (nothing)
 *   rotating: pre (nothing)           -> core -> post_a (Y fill, shear remap of output)
 *                                     -> [exchange z ghosts of output] -> post_b (Y fill of output) */
int rgpu_step_pre   (rgpu_ctx* c, int nStep, double dt, double totalTime);
int rgpu_step_core  (rgpu_ctx* c, int nStep, double dt, double totalTime);
int rgpu_step_post_a(rgpu_ctx* c, int nStep, double dt, double totalTime);
int rgpu_step_post_b(rgpu_ctx* c, int nStep, double dt, double totalTime);

/* Plane-ranged pieces (3D contexts) for a slab driver that hides the halo exchange behind the update of the planes
 * nobody else needs ("boundary planes first"): with every ghost of the INPUT valid at entry,
 *   core_planes [0,2gw) and [nz,ksize)  -> fill_planes [gw,2gw) and [nz,nz+gw) -> start exchange of the OUTPUT
 *   core_planes [2gw,nz)                -> fill_planes [2gw,nz)                -> wait -> physical z faces
 * k_lo/k_hi are array plane indices (ghosts included), half open.
 * rgpu_step_core_planes completes the update of planes [k_lo,k_hi) of U[(nStep+1)%2] (every intermediate stage is
 * run on exactly the planes that update needs); rgpu_step_core == planes [0,ksize).
 * rgpu_step_fill_planes applies the in-plane part of the ghost fill to planes [k_lo,k_hi) of the OUTPUT state:
 * X,Y faces (HydroRunBase.cpp:2333-2342) or, shearing box, Y + shear remap + Y (MHDRunGodunov.cpp:3779-3793 with
 * the z copy commuted out: all three act within one z plane). */
int rgpu_step_core_planes(rgpu_ctx* c, int nStep, double dt, double totalTime, int k_lo, int k_hi);
/* The same piece in two halves, for solvers whose update is a kernel of its own (3D MHD): RGPU_CORE_FLUXES computes the
 * face fluxes and edge EMFs the update of planes [k_lo,k_hi) needs (one z-marching launch -- over the whole slab it costs one
 * pipeline fill instead of one per plane range), RGPU_CORE_UPDATE then completes planes [k_lo,k_hi) -- any sub-ranges of a
 * FLUXES range, in any order.  For every other solver FLUXES does nothing and UPDATE is rgpu_step_core_planes, so the
 * schedule  FLUXES [0,ksize) ; UPDATE boundary ranges ; exchange || UPDATE inner range  is valid for all of them. */
enum { RGPU_CORE_FLUXES = 1, RGPU_CORE_UPDATE = 2, RGPU_CORE_SCAN = 4 };
/* | RGPU_CORE_SCAN: the CFL scan of the new state rides in the update kernels of the pieces (no pass over U for the next
 * compute_dt): FLUXES | SCAN resets the context's RGPU_DT_SLOTS device slots, every UPDATE | SCAN accumulates the maxima of the
 * cells it updates, rgpu_inv_dt_fused_commit(ctx, parity of the new state) closes the accumulation and returns the number of
 * slots to all-reduce (rgpu_inv_dt_device_slot) before rgpu_inv_dt_result.  rgpu_inv_dt_fused_active tells right after the
 * FLUXES call whether the step can carry the scan; if not (dissipative stage, forcing, the rotating path with other x faces than the
 * shearing box's or with open y / z faces, flat kernels) scan with rgpu_inv_dt_accumulate as before. */
/* 1 when THIS context's configuration lets its update pieces carry the scan (depends on its boundary types: the end slabs of
 * a run may differ from the inner ones).  All ranks must pass the same flag combination and all-reduce the same number of
 * slots: the slab driver takes the minimum over the ranks once and drops RGPU_CORE_SCAN everywhere if any rank says 0. */
int rgpu_inv_dt_fusable(rgpu_ctx* c);
int rgpu_inv_dt_fused_active(rgpu_ctx* c, int parity);   /* after FLUXES | SCAN: 1 when this step's pieces carry the scan */
int rgpu_inv_dt_fused_commit(rgpu_ctx* c, int parity);
int rgpu_step_core_planes_split(rgpu_ctx* c, int nStep, double dt, double totalTime, int k_lo, int k_hi, int what);
/* The dissipative stage of the step ([hydro] nu / [MHD] eta > 0; no-op otherwise) on U[(nStep+1)%2], WITHOUT the ghost
 * fill that precedes it in rgpu_godunov_unsplit: a slab driver calls it between rgpu_step_core and rgpu_step_post_a after
 * it has filled the ghosts of the output itself (rgpu_make_boundaries / _shear + its z exchange), as the reference's MPI
 * classes do with make_all_boundaries(h_UNew) (mhd_godunov_unsplit_cpu_v3.cpp:662-668). */
int rgpu_step_dissipative(rgpu_ctx* c, int nStep, double dt, double totalTime);
int rgpu_step_fill_planes(rgpu_ctx* c, int nStep, double dt, double totalTime, int k_lo, int k_hi);
/* The same two pieces for TWO disjoint plane ranges at once -- the two boundary ranges of a slab, [0,2gw) + [nz,ksize) and
 * [gw,2gw) + [nz,nz+gw) -- so that what lies between the end of the flux sweep and the start of the halo exchange is a handful of
 * launches: the 3D MHD update kernel marches both ranges in one launch; the ghost fill of both ranges is one launch whenever the
 * x / y faces are mirror / copy / periodic or the shearing box with periodic y (one thread per ghost cell, every value a function
 * of interior cells of its plane: X, Y -- or Y, shear remap, Y -- need no ordering).  Same doubles as the one-range calls.
 * Either range may be empty.  (3D hydro: the sweep is the whole step -- both ranges in one launch of it.) */
int rgpu_step_core_planes_pair(rgpu_ctx* c, int nStep, double dt, double totalTime, int k_lo, int k_hi, int k_lo2, int k_hi2, int what);
int rgpu_step_fill_planes_pair(rgpu_ctx* c, int nStep, double dt, double totalTime, int k_lo, int k_hi, int k_lo2, int k_hi2);

/* rgpu_compute_inv_dt in pieces: accumulate the max over the cells of planes [k_lo,k_hi) into the context's device
 * slot (reset != 0 starts a new maximum), asynchronously on the context stream; rgpu_inv_dt_result synchronises
 * and returns it with the seeds of compute_dt[_mhd] applied.  Lets a slab driver scan each plane of the output
 * BEFORE its ghosts are refilled, which is the state the reference's compute_dt sees on the plain path
 * (oneStepIntegration: compute_dt, then godunov_unsplit fills the ghosts; MHDRunGodunov.cpp:4077-4089). */
int rgpu_inv_dt_accumulate(rgpu_ctx* c, int parity, int k_lo, int k_hi, int reset);
int rgpu_inv_dt_result(rgpu_ctx* c, double* invDt);

/* History diagnostics of the MHD runs, reduced on the device instead of copying the state to the host
 * (MHDRunBase::history_mri, MHDRunBase.cpp:3476-3619; history_default, :3311-3407 is its mass / divB subset).
 * rgpu_history_mri: out[8] = mass, maxwell stress, reynolds stress, magnetic pressure, mean Bx, By, Bz, sum of divB,
 * normalised like the reference's history file (single domain).  Sums are accumulated in a fixed order that is not the
 * reference's loop order: they agree with it to round-off.
 * Slab runs combine the two lower-level calls: rgpu_history_columns gives cols[9][isize] = sums over the interior y,z
 * extent of this domain of {rho, mx/rho, my/rho (every i), magp terms, maxwell term, Bx, By, Bz, divB (interior i)};
 * after an all-reduce, mean_vx/vy[i] = cols[1..2][i] / (ny * nz_global) feed rgpu_history_reynolds, which returns
 * cols[isize] = sum_jk rho * dTau * (vx - mean_vx)(vy - mean_vy). */
int rgpu_history_columns(rgpu_ctx* c, int parity, double* cols);
int rgpu_history_reynolds(rgpu_ctx* c, int parity, const double* mean_vx, const double* mean_vy, double dTau, double* cols);
int rgpu_history_mri(rgpu_ctx* c, int parity, double* out);
/* MHDRunBase::history_turbulence (MHDRunBase.cpp:3626-3810; problems "turbulence" and "turbulence-Ornstein-Uhlenbeck", 3D),
 * reduced on the device: out[18] = the columns of the reference's history file after totalTime and dt --
 * mass divB eKin eMag helicity mean_rho mean_B mean_Bx mean_By mean_Bz mean_rhovx mean_rhovy mean_rhovz Ma_s Ma_alfven
 * coef_x coef_y coef_z (the three high-k DFT amplitudes of Bx it monitors).  Single-domain contexts; fixed summation order,
 * device cos / sin: agreement with the reference to round-off. */
int rgpu_history_turbulence(rgpu_ctx* c, int parity, double* out);
/* The 18 raw sums behind rgpu_history_turbulence over the interior cells of this context -- also a slab's (its own planes):
 * the z-slab driver adds them up across the ranks (rgpu_comm_history_turbulence, the reference's history_mhd_turbulence of the
 * MPI classes, HydroRunBaseMpi.cpp:11346-11530). */
int rgpu_history_turbulence_sums(rgpu_ctx* c, int parity, double* sums18);
/* One cell of the state, out[nbVar] = U(i,j,k,:) with ghost-inclusive local indices: what history_inertial_wave
 * (MHDRunBase.cpp:3414-3469) probes -- U(ghostWidth + nx/2, ghostWidth) in 2D, U(ghostWidth + nx/2, 1, ghostWidth) in 3D --
 * without copying the whole array back (the reference calls copyGpuToCpu first). */
int rgpu_read_cell(rgpu_ctx* c, int parity, int i, int j, int k, double* out);

/* Reproducibility fingerprint of U[parity]: the sum, modulo 2^64, of the 64-bit patterns of every variable of every INTERIOR cell of
 * this context (a slab: its own planes).  Integer addition is associative: the value does not depend on how the box was cut into
 * slabs or tiles, so the sum of the slabs' checksums (mod 2^64) of an N-rank run equals the single-device run's whenever the states
 * are equal bit for bit -- which the z-slab driver promises (rgpu_comm.h).  bench.py prints it for every N.  (The reference compares
 * runs through its output files; this is the same check without the 8.9 GB copy, HydroRunBase.cpp:7217-7229 copyGpuToCpu.) */
int rgpu_state_checksum(rgpu_ctx* c, int parity, unsigned long long* out);

/* == oneStepIntegration(nStep, t, dt) (MHDRunGodunov.cpp:4077-4089) for a single device */
int rgpu_one_step_integration(rgpu_ctx* c, int* nStep, double* t, double* dt);

/* The body of the reference's time loop, "while (totalTime < tEnd && nStep < nStepmax) oneStepIntegration(nStep, totalTime, dt)"
 * (MHDRunGodunov.cpp:3921-3990, HydroRunGodunov.cpp:3960), for up to nsteps steps: returns the number of steps done (< nsteps only when
 * totalTime reached tEnd; pass HUGE_VAL for "no end") or a negative RGPU_E* code; *nStep, *t, *dt advance exactly as nsteps calls of
 * rgpu_one_step_integration would advance them -- same states, same dt sequence, bit for bit.  What it adds: where a step is ONE fused
 * kernel that leaves the CFL maxima and the ghost cells of its output on the device (2D hydro in a box of periodic, reflecting or
 * outflow faces; 2D MHD in an all-periodic box -- with a Neumann face its kernel writes no ghost images and the plain loop runs; no
 * gravity, no rotating frame) the time step itself stays on the device (csrc/hip/step_clock.h: dt = cfl / max 1/dt, the
 * loop condition and t += dt evaluated by a one-workgroup kernel between two steps) and a batch of steps is queued without a host round
 * trip -- at the shipped 2D sizes that round trip costs as much as a third of the step.  Since round 5 the 3D steps do the same (hydro,
 * plain / shearing-box MHD through the z-marching sweeps: rgpu_clock_capable; a rotating box with periodic x faces leaves no CFL maxima
 * behind -- the reference scans its refilled ghosts -- and runs the plain loop).  Driven turbulence -- a lone, non-rotating 3D context
 * with random forcing, Ornstein-Uhlenbeck forcing or both, no gravity, no dissipative stage, phase timers off -- is batched too (option
 * "forcing_clock"): the sums and the norm of the random forcing and the mode step of the Ornstein-Uhlenbeck process are formed on the
 * device with the host's expressions, from deviates the host draws ahead, and the last kick of a step carries the CFL scan of the
 * state it leaves; a state without CFL maxima in the slots (the first step of a run, the state a single step left) gets its scan
 * queued and the batch opens.  States, dt sequence and the process (rgpu_ou_forcing_get_state, generator included) are the plain
 * loop's, bit for bit.  Every other configuration runs the plain loop. */
int rgpu_run_steps(rgpu_ctx* c, int nsteps, double tEnd, int* nStep, double* t, double* dt);
/* ... the same, and dt_log[n] = the time step of the n-th step done (the "dt=" column of the reference's log, MHDRunGodunov.cpp:3958);
 * dt_log holds nsteps doubles or is NULL.  If a launch fails after some steps of a batch were queued, *nStep, *t, *dt (and dt_log)
 * are advanced for the steps that did run before the error is returned. */
int rgpu_run_steps_log(rgpu_ctx* c, int nsteps, double tEnd, int* nStep, double* t, double* dt, double* dt_log);
/* ... the same, with the history file's cadence inside (MHD, single domain): the loop of MHDRunGodunov.cpp:3975-3984,
 *     n = 0
 *     while n < nsteps and *t < tEnd:
 *         if *tHist == 0 or ((*t - *dt <= *tHist + dtHist) and (*t > *tHist + dtHist)):
 *             k = (*hist_n)++                      (hist_n starts at 0 in every call)
 *             hist_step[k] = *nStep; hist_t[k] = *t; hist_dt[k] = *dt
 *             hist[k][:] = rgpu_history_mri(c, *nStep % 2)
 *             *tHist += dtHist
 *         rgpu_one_step_integration(c, nStep, t, dt); n++
 *     return n
 * *nStep, *t, *dt, dt_log and the state advance exactly as in rgpu_run_steps_log; the sample steps and *tHist are those of the code
 * above, evaluated in doubles with those expressions in that order; hist[k] holds, bit for bit, the eight doubles rgpu_history_mri of
 * the same library returns on a lone context holding that state.  hist_step, hist_t, hist_dt hold nsteps entries, hist nsteps rows of
 * RGPU_HIST_NQ; dt_log may be NULL.  The reference's quirks stay: dtHist == 0 with *tHist == 0 samples before every step, and a step
 * that overshoots more than one interval can end the series.  A sample is taken only at the head of a turn that begins (*t < tEnd): the
 * state after the last step of a call is sampled by the next call, so a run cut into calls gives the series of one call.
 * Where the context takes its time step from the device (rgpu_device_time_step_ready: the 2D all-periodic MHD box; rgpu_clock_capable:
 * 3D MHD, plain, rotating and shearing box) the decision, the row and *tHist += dtHist are formed on the device behind each tick of the
 * batch (csrc/kernels_history.h: the kernels of rgpu_history_mri behind a gate, the host's small arithmetic in a finish kernel, a log
 * of RGPU_CLOCK_BATCH records read back once per batch with the clock records -- allocated by the first call that needs it, not part of
 * rgpu_device_bytes); every other configuration, and option "history_batch" = 0, takes the code above literally.
 * Errors: RGPU_EUNSUPPORTED for a hydro context; RGPU_EINVAL for a slab context (slab_count > 1, as rgpu_history_mri), a NULL pointer
 * among nStep, t, dt, tHist, hist_n, hist_step, hist_t, hist_dt, hist, or nsteps < 0.  When the call ends with a negative code, *hist_n
 * counts only samples whose values were written, and *nStep, *t, *dt, *tHist describe the steps that ran; the head sample of the step
 * that failed is among them on the literal path (it is taken before the step) and is not inside a device batch (the records behind
 * the last step that ran are not read). */
#define RGPU_HIST_NQ 8   /* the out[8] of rgpu_history_mri */
int rgpu_run_steps_history(rgpu_ctx* c, int nsteps, double tEnd, int* nStep, double* t, double* dt, double* dt_log,
                           double dtHist, double* tHist,          /* in / out */
                           int* hist_n, int* hist_step /* [nsteps] */, double* hist_t /* [nsteps] */,
                           double* hist_dt /* [nsteps] */, double* hist /* [nsteps][RGPU_HIST_NQ] */);
/* how many heads of rgpu_run_steps_history this context has queued on the device so far (one per step of a device-clock batch,
 * sampling or not; 0 where every call took the literal loop): lets a caller (and the tests) tell which path ran */
long rgpu_history_batch_heads(rgpu_ctx* c);
/* how many steps of this context ran inside device-clock batches of rgpu_run_steps* with a forcing stage queued behind their core (random
 * or Ornstein-Uhlenbeck forcing, option "forcing_clock"; 0 where every forced step took the literal loop): which path ran, as above */
long rgpu_forcing_batch_steps(rgpu_ctx* c);
/* 1 when the next step of rgpu_run_steps on the state U[parity] would take its time step from the device (see above), else 0:
 * lets a caller (and the tests) tell which loop runs.  A forced context (see rgpu_run_steps): 1 for a state that came out of a batch --
 * its CFL maxima are in the slots, the next rgpu_compute_dt fetches them and does not scan; 0 after a single step, and always with
 * option "forcing_clock" = 0. */
int rgpu_device_time_step_ready(rgpu_ctx* c, int parity);

/* The device-side time step as pieces, for a driver that queues whole batches of steps itself (the z-slab driver: all-reduce of the
 * 1/dt slots in place -> clock -> step pieces -> halo exchange, no host turn between steps; rgpu_run_steps is built on the same three).
 *   rgpu_clock_capable  1 when every kernel of this context's step that depends on dt or t can read them from a device record
 *                       (csrc/step_clock_rec.h): 2D fused steps; 3D hydro and MHD through the z-marching sweeps, incl. the rotating frame
 *                       and the shearing box (periodic y); no gravity, dissipative stage, forcing, phase timers.  (Forcing: the pieces
 *                       below include no forcing stage, so a forced context answers 0 here and rgpu_clock_open refuses it; the library's
 *                       own loop, rgpu_run_steps*, queues the forcing stages itself and batches such a context all the same.)
 *   rgpu_clock_open     starts a batch at time t0; steps stop being executed once t >= tEnd (HUGE_VAL: never).
 *   rgpu_clock_tick     queues the clock kernel of the NEXT step: folds the RGPU_DT_SLOTS device slots (which must hold the CFL maxima of
 *                       the step's input state -- all-reduced across slabs by the caller), zeroes them for the step's own scan, forms
 *                       dt = cfl / max(1/dt), dt/dx.., the rotating-frame coefficients, the shearing-box offsets, t += dt with the host's
 *                       expressions (the same doubles).  Until the next tick / close every rgpu_step_* piece of this context reads that
 *                       record on the device; its dt / totalTime arguments are ignored.  A step whose record says "stop" (t >= tEnd, or
 *                       1/dt not finite) and every step after it are no-ops that leave state, ghost cells and slots untouched.
 *   rgpu_clock_close    reads the records back (the one synchronisation of the batch): *ran = steps that ran, *t += their dt in order,
 *                       *dt_last, dt_log[0..ran) (may be NULL), *stop = 0 or why the batch stopped (1: tEnd, 2: dt is NaN, 3: 1/dt not
 *                       finite).  nStep0 = step number of the first step of the batch.  At most RGPU_CLOCK_BATCH ticks per batch. */
int rgpu_clock_capable(rgpu_ctx* c);
int rgpu_clock_open(rgpu_ctx* c, double t0, double tEnd);
int rgpu_clock_tick(rgpu_ctx* c);
int rgpu_clock_close(rgpu_ctx* c, int nStep0, int* ran, double* t, double* dt_last, double* dt_log, int* stop);
/* 1 when the host already KNOWS that the record of the last tick says "stop" -- never on the device backend (the record is formed
 * asynchronously; the batch's no-op steps are simply queued), always up to date on a synchronous backend (the test-only host emulation),
 * where a driver can end its batch at once.  The answer is the same on every slab of a run. */
int rgpu_clock_stopped(rgpu_ctx* c);
/* The same answer on ANY backend, at the price of a synchronisation: waits for the record of the last tick and returns its stop flag
 * (0 = the step runs, 1 / 2 / 3 as in rgpu_clock_close; < 0: error).  The slab driver checks the first step of every batch this way:
 * a rank that failed in an unbatched step has told the others through ONE poisoned all-reduce and left the loop. */
int rgpu_clock_check(rgpu_ctx* c);

/* ---- ensembles of 2D boxes ----------------------------------------------------------------------------------------------------
 * A fused 2D step is one kernel of 20-50 us that fills a fraction of the device (a 128^2 hydro box: ~100 of ~768 resident workgroups)
 * and 2D boxes do not shard (rgpu_comm.h).  What fills the device is MANY boxes: seeds of a perturbation, a parameter scan.  An
 * ensemble is `members` boxes of one shape and one solver configuration (*p, shared -- or one set per member that differs in
 * doubles only: rgpu_ensemble_create_scan, below), each with its own state, its own dt sequence
 * and its own end time, advanced by ONE step-kernel launch and ONE clock-kernel launch per step for all of them
 * (csrc/hip/ensemble2d.h: the member is the second grid dimension; the kernels run the single-box body, hence the same doubles).
 *
 *   rgpu_ensemble_create   2D only (nz_global == 1) with slab_count == 1, else RGPU_EUNSUPPORTED; members outside
 *                          1 .. RGPU_ENSEMBLE_MAX_MEMBERS: RGPU_EINVAL; no device: RGPU_ENODEVICE, as rgpu_create.  *out is returned
 *                          even on failure so that rgpu_ensemble_last_error can be read; the caller destroys it.
 *   rgpu_ensemble_member   member m as an ordinary rgpu_ctx over a slice of the ensemble's storage, on the ensemble's one stream
 *                          (BORROWED; NULL when m is out of range).  Every entry point of this header works on it unchanged --
 *                          rgpu_upload, rgpu_download, rgpu_make_all_boundaries, rgpu_compute_dt, rgpu_state_checksum, rgpu_read_cell,
 *                          rgpu_set_gravity_field, the histories, and rgpu_one_step_integration / rgpu_run_steps on that member alone --
 *                          except rgpu_destroy, which refuses a member (it returns without doing anything).
 *   rgpu_ensemble_destroy  frees the members and everything else.
 *   rgpu_ensemble_device_bytes   device memory of an ensemble (0: parameters rgpu_ensemble_create would refuse): what create allocates
 *                          plus the clock records of the fused rounds (RGPU_CLOCK_BATCH records of 128 bytes per member, allocated by
 *                          the first rgpu_ensemble_run_steps that takes a fused round, and as many again in pinned host memory).
 *   rgpu_ensemble_run_steps      for EVERY member m exactly what rgpu_run_steps_log(member m, nsteps, tEnd[m], &nStep[m], &t[m], &dt[m],
 *                          dt_log + m * nsteps) does on a lone context holding that member's state: the same states, nStep, t, dt and
 *                          dt sequence -- bit for bit in librgpu.so, to round-off (relative L2 <= 1e-12; mostly, not always, the same bits)
 *                          in librgpu_fast.so.  nStep, t, dt: [members], in / out.  tEnd: [members], or
 *                          NULL for "no end".  dt_log: [members][nsteps] or NULL.  done[m] = steps member m took in this call.
 *                          stop[m] (may be NULL) = 0, or why member m took fewer than nsteps: 1 = its t reached its tEnd (also when that
 *                          happened with its last step, or before the call: done[m] = 0), 2 = its dt is not a number, 3 = its 1/dt is
 *                          not finite (the codes of rgpu_clock_close).  A member stops with the last state it wrote while the others go
 *                          on.  Codes 2 and 3 are that member's business: the call still returns RGPU_OK, the code is in stop[m] and
 *                          the text in rgpu_last_error(member).  *fused_steps (may be NULL) = the step rounds that went through the
 *                          fused launch.  Returns RGPU_OK or a negative code (a launch or a plain single-member step failed: the
 *                          members are advanced for the steps that did run, as rgpu_run_steps_log does).
 * The fused launch covers what rgpu_device_time_step_ready covers on a 2D context (2D hydro with Dirichlet, Neumann or periodic faces,
 * no jet, no gravity; 2D MHD in an all-periodic non-rotating box; options step_clock, ghost_images and the tiled kernels on) and is
 * used for a round when every member that still runs is ready and the running members share a step parity; every other round -- each
 * member's first step of a run, uncovered configurations, members of mixed parity after different end times -- is taken member by
 * member through the single-context loop: a correct fallback, not an error.  One more state is mixed in that sense and nothing
 * re-aligns it: a 2D hydro member that was clock-ready when it was stepped ALONE (rgpu_run_steps on that member, or a member-by-member
 * round beside a member whose state had just been uploaded) has rotated through its three CFL slot arrays, because the lone loop folds
 * the clock into the step kernel on small grids; the fused launch addresses one array for all members, so from then on members whose
 * arrays differ are stepped one by one -- for the rest of that call and of later ones, until every member is uploaded afresh.
 * *fused_steps < the rounds taken (less each member's first) is how a caller sees it.  Batches of at most RGPU_CLOCK_BATCH rounds, one
 * read-back of the records per batch.  Afterwards every member's bookkeeping (CFL slots, ghost cells) is what the single-context
 * loop would have left: any later call on a member alone continues correctly.
 *
 * Parameter scans: rgpu_ensemble_create_scan takes one parameter set PER MEMBER (sets[m] for member m) instead of one for all.
 *   Shared, because they select code or shape: every int32_t field of rgpu_params, slope_type, and the four sign classes cIso > 0,
 *   Omega0 > 0, nu > 0, eta > 0.  A set that differs from sets[0] in one of them: RGPU_EINVAL, the message names the field and the
 *   first offending member.  A set rgpu_ensemble_create would refuse: that call's code.  sets == NULL: RGPU_EINVAL.
 *   May differ: every other double -- gamma0 (with smallp, smallpp, gamma6), cfl, cIso, smallr, smallc, smalle, the box extents and
 *   dx, dy, the jet, gravity, viscosity and forcing magnitudes.
 *   Everything else is the ensemble above: rgpu_ensemble_member / _members / _destroy / _last_error / _run_steps work unchanged, and
 *   rgpu_ensemble_run_steps gives member m exactly what rgpu_run_steps_log gives a lone context created from sets[m] (bit for bit in
 *   librgpu.so, relative L2 <= 1e-12 in librgpu_fast.so).  On the fused rounds every workgroup reads its member's constants
 *   (DevParams, the clock's constants, the rotating-frame coefficients: 384 bytes per member) from a table in device memory through
 *   scalar loads (csrc/hip/ensemble_scan.h) instead of the kernel arguments; the table is written once, by the first fused round (or rgpu_ensemble_monitor), and
 *   never again.  The same kernel bodies, the same placement on a CU as the uniform ensemble kernels in every instantiation (DESIGN
 *   3.6.1: no retreat was needed for the generic 2D MHD kernel).  A scan whose sets are all bytewise equal takes the by-value
 *   launch of rgpu_ensemble_create (unless option "member_params" is 1).  Where a configuration is off the fused path it is so for
 *   all members alike, and the member-by-member rounds use each member's own context.
 *   rgpu_ensemble_scan_device_bytes: 0 for input rgpu_ensemble_create_scan would refuse, else rgpu_ensemble_device_bytes of the
 *   shared shape plus the table. */
typedef struct rgpu_ensemble rgpu_ensemble;
#define RGPU_ENSEMBLE_MAX_MEMBERS 1024
int rgpu_ensemble_create(const rgpu_params* p, int members, rgpu_ensemble** out);
/* members parameter sets, sets[m] for member m */
int rgpu_ensemble_create_scan(const rgpu_params* sets, int members, rgpu_ensemble** out);
void rgpu_ensemble_destroy(rgpu_ensemble* e);
int rgpu_ensemble_members(rgpu_ensemble* e);
rgpu_ctx* rgpu_ensemble_member(rgpu_ensemble* e, int m);
size_t rgpu_ensemble_device_bytes(const rgpu_params* p, int members);
size_t rgpu_ensemble_scan_device_bytes(const rgpu_params* sets, int members);
const char* rgpu_ensemble_last_error(rgpu_ensemble* e);
int rgpu_ensemble_run_steps(rgpu_ensemble* e, int nsteps, const double* tEnd, int* nStep, double* t, double* dt, double* dt_log, int* done,
                            int* stop, int* fused_steps);

/* ---- monitors: per-member totals and extrema, reduced on the device --------------------------------------------------------------
 * What a user wants out of a run of 64 seeds or of a parameter scan is a time series per member; downloading every member's state
 * for it (64 members of 128^2, 8 variables: 67 MB per sample) would end the batch of queued rounds an ensemble exists for.  A monitor
 * is RGPU_MON_NQ = 10 doubles of a 2D state U[parity], hydro or MHD, taken over its nx x ny INTERIOR cells and raw (not multiplied by
 * dx dy):
 *     q  0 mass   1 mx   2 my   3 mz   4 E   5 ekin   6 emag        sums
 *        7 min_rho   8 min_eint                                     minima
 *        9 max_absdivb                                              maximum
 * Per-cell terms, with IEEE + - * / in exactly this order and no FMA contraction in either library (csrc/kernels_monitor.h):
 *     rho = U[ID], E = U[IP], mx = U[IU], my = U[IV], mz = U[IW] (hydro, nbVar == 4: +0.0)
 *     ekin = (0.5 * ((mx * mx + my * my) + mz * mz)) / rho
 *     MHD:   bxc = 0.5 * (Bx(i,j) + Bx(i+1,j)), byc = 0.5 * (By(i,j) + By(i,j+1)), bzc = U[IC],
 *            emag = 0.5 * ((bxc * bxc + byc * byc) + bzc * bzc),
 *            absdivb = | (Bx(i+1,j) - Bx(i,j)) / dx + (By(i,j+1) - By(i,j)) / dy |       (dx, dy: the context's own)
 *     hydro: emag = +0.0, absdivb = +0.0            (columns 3, 6 and 9 of a hydro state are exactly 0)
 *     eint = (E - ekin) - emag
 *   The high faces of the last interior row and column lie in the first ghost layer; they hold their constrained-transport value
 *   after every step and after a ghost fill, so no ghost fill is done (rgpu_history_* read the same faces).
 * Summation order: fixed by (nx, ny), RGPU_MON_ROWS and RGPU_MON_LANES alone -- not by the number of members, the member index,
 * the position in a batch, fused or member-by-member rounds, the by-value or table path, or the library.  No floating-point
 * atomics.  With ii = i - ghostWidth in [0, nx), jj = j - ghostWidth in [0, ny), every accumulator starting at +0.0 and taking
 * "a = a + x" in the order given:
 *     1. P[s][ii] = sum of the terms of column ii over jj = s * ROWS .. min(ny, (s + 1) * ROWS) - 1, ascending   (s < nseg = ceil(ny / ROWS))
 *     2. C[ii]    = sum of P[s][ii] over s = 0 .. nseg - 1, ascending
 *     3. L[l]     = sum of C[ii] over ii = l, l + LANES, l + 2 LANES, .. < nx, ascending                          (l < LANES; no such ii: +0.0)
 *     4. for off = LANES / 2, LANES / 4, .., 1:  L[l] <- L[l] + L[l ^ off] for all l at once;  the sum is L[0]
 *   (tests/monitor_checks.py is this order in numpy and reproduces every double.)  Whatever the order, |S - exact| <= N 2^-53 sum |terms|.
 * Extrema: fmin from +inf, fmax from +0.0 along the same route, order-free.  NaN: a NaN in a state propagates into the sums that
 * contain it as IEEE addition does; fmin / fmax return their other operand when one is NaN, so the extrema are those of the cells
 * whose term is a number (all terms NaN: +inf / +0.0 stay).  Members do not see each other: a poisoned member changes no other's values.
 *
 *   rgpu_state_monitor     out[RGPU_MON_NQ] of U[parity] of any 2D context, in any configuration (3D: RGPU_EUNSUPPORTED, see rgpu_state_monitor3d).  Reads the
 *                          state only: ghost cells, CFL slots and what the context knows about them stay as they are.  Synchronises.
 *   rgpu_ensemble_monitor  out[members][RGPU_MON_NQ] of every member's CURRENT state -- U[0] after rgpu_upload, U[nStep % 2] after steps
 *                          taken through rgpu_one_step_integration / rgpu_godunov_unsplit / rgpu_run_steps* on the member or
 *                          rgpu_ensemble_run_steps* -- with two launches for all members and one read-back.  The staged entry points
 *                          (rgpu_step_pre / _core / _post_*, the plane-ranged pieces, rgpu_clock_*) do NOT move what counts as a
 *                          member's current state: a caller that drives a member through them reads it with rgpu_state_monitor
 *                          and the parity it knows.
 *   rgpu_ensemble_run_steps_monitored   rgpu_ensemble_run_steps (same arguments, same states, dt sequences, done, stop, fused_steps) plus
 *                          sampling: member m is sampled after each of its steps that brings nStep[m] to a multiple of `every` -- its
 *                          own global step number, so the series does not depend on how a run is cut into calls and members with
 *                          different nStep are sampled at different rounds.  mon_n[m] = its samples in this call (<= cap = nsteps /
 *                          every + 1); sample k of member m: mon_step[m * cap + k] the step number, mon_t[m * cap + k] the
 *                          host-accumulated t[m] after that step (the double the loop returns), mon[(m * cap + k) * RGPU_MON_NQ + q] the
 *                          values.  A member that stops on reaching its tEnd is sampled if its last step qualifies; a member stopped
 *                          with code 2 or 3 gets no further samples.  every < 1 or a null monitor pointer: RGPU_EINVAL.
 *                          On fused rounds the host queues the monitor kernels (csrc/hip/ensemble_monitor.h) behind the step launch of
 *                          every round after which some running member qualifies; each workgroup decides from its member's clock record
 *                          and step number whether to sample; the values go to a device log that is copied back once per batch
 *                          with the clock records: no synchronisation inside a batch.  On member-by-member rounds the loop is cut at
 *                          the member's next sampling step and rgpu_state_monitor is called on its context (one synchronisation per
 *                          sample).  Both give the doubles of rgpu_state_monitor on a lone context holding that state.
 *   rgpu_ensemble_monitor_device_bytes   the extra device memory, allocated by the first call that samples on the device (per member:
 *                          the segment sums, RGPU_CLOCK_BATCH log slots, 8 bytes of bookkeeping; the log as many again in pinned host
 *                          memory).  rgpu_ensemble_device_bytes / _scan_device_bytes do not include it.  0 for refused parameters.
 *
 * The 3D monitor: the same ten quantities, names and RGPU_MON_NQ over the nx x ny x nz interior cells of U[parity] as the array stands
 * (no ghost fill; the high faces of the last interior row, column and plane come from the first ghost layer), raw.  Terms of cell
 * (i, j, k), IEEE + - * / in this order, no FMA contraction in either library:
 *     rho, E, mx, my as above, mz = U[IW] (3D hydro has five variables);  ekin = (0.5 * ((mx * mx + my * my) + mz * mz)) / rho
 *     MHD:   bxc, byc as above, bzc = 0.5 * (Bz(i,j,k) + Bz(i,j,k+1));  emag = 0.5 * ((bxc * bxc + byc * byc) + bzc * bzc)
 *            absdivb = | ((Bx(i+1,j,k) - Bx(i,j,k)) / dx + (By(i,j+1,k) - By(i,j,k)) / dy) + (Bz(i,j,k+1) - Bz(i,j,k)) / dz |
 *     hydro: emag = +0.0, absdivb = +0.0;   eint = (E - ekin) - emag
 * Summation order, fixed by (nx, ny, nz), RGPU_MON_ROWS and RGPU_MON_LANES alone: V[kk], kk = k - ghostWidth, is steps 1 - 4 above
 * applied to the nx x ny cells of interior plane kk; the result is V[0] + V[1] + .. ascending in kk from +0.0.  The extrema take the
 * same route with fmin from +inf / fmax from +0.0; the NaN rules are those above.  No floating-point atomics: the values do not depend
 * on the library, on whether the sample is taken inside or outside a batch, or on how the kernels cut the grid.
 * (tests/monitor3d_checks.py is this order in numpy.)
 *
 *   rgpu_state_monitor3d   out[RGPU_MON_NQ] of U[parity] of any single-domain 3D context, hydro or MHD, rotating and shearing box
 *                          included.  Reads the state only: ghost cells, CFL slots and what the context knows about them stay as they
 *                          are.  Synchronises.  2D context: RGPU_EUNSUPPORTED; slab context (slab_count > 1): RGPU_EINVAL, as
 *                          rgpu_history_mri; NULL pointer: RGPU_EINVAL.
 *   rgpu_run_steps_monitored   rgpu_run_steps_log (same states, same dt sequence, same return value) of a 2D or 3D context plus sampling,
 *                          with the semantics of rgpu_ensemble_run_steps_monitored for one member: a sample after each step that brings
 *                          *nStep to a multiple of `every`; *mon_n = the samples of this call (<= cap = nsteps / every + 1); sample k:
 *                          mon_step[k], mon_t[k] the host-accumulated *t after that step, mon[k * RGPU_MON_NQ + q] the values of
 *                          rgpu_state_monitor / rgpu_state_monitor3d on that state, bit for bit.  A step that reaches tEnd is sampled if
 *                          it qualifies, nothing is sampled after a stop, and after stop code 2 or 3 (a negative return) no further
 *                          samples are taken; *mon_n counts only samples whose values were written.  A run cut into calls gives the
 *                          series of one call.  dt_log may be NULL.
 *                          Where the context takes its time step from the device (rgpu_device_time_step_ready) the monitor kernels are
 *                          queued behind the last kernel of each qualifying step (csrc/hip/monitor3d.h; a 2D state is a volume of one
 *                          plane, whose sum over the planes is left out), return in their first instructions when the step's clock record says stop -- the
 *                          host knows the step number, only "did the step run" comes from the record, which on small 2D hydro grids is
 *                          written by that step's own kernel -- and write to a device log of RGPU_CLOCK_BATCH slots that is copied back
 *                          once per batch with the clock records: no synchronisation inside a batch.  Everywhere else (first steps,
 *                          gravity, the dissipative stage, forcing with option "forcing_clock" = 0,
 *                          a rotating 2D box, phase timers, option "step_clock" = 0) the call
 *                          is the literal loop: rgpu_one_step_integration, then rgpu_state_monitor / rgpu_state_monitor3d.
 *                          Partial sums go to the flux array, dead between steps; the log (RGPU_CLOCK_BATCH x RGPU_MON_NQ doubles)
 *                          and its pinned mirror are allocated by the first call that needs them, freed with the context, and
 *                          are not part of rgpu_device_bytes.
 *                          Errors: RGPU_EINVAL for every < 1 ("every" in the message), a NULL pointer among nStep, t, dt, mon_n,
 *                          mon_step, mon_t, mon, nsteps < 0, or a slab context.
 *   rgpu_monitor_batch_samples   how many samples this context has queued on the device inside its batches so far (0 where every call
 *                          took the literal loop): lets a caller (and the tests) tell which path ran, as rgpu_history_batch_heads. */
#define RGPU_MON_NQ 10
#define RGPU_MON_NAMES "mass mx my mz E ekin emag min_rho min_eint max_absdivb"   /* the RGPU_MON_NQ columns, in order */
#define RGPU_MON_ROWS 32    /* rows per segment of the summation order */
#define RGPU_MON_LANES 64   /* lanes of the summation order (one wavefront) */
int rgpu_state_monitor(rgpu_ctx* c, int parity, double* out /* [RGPU_MON_NQ] */);
int rgpu_ensemble_monitor(rgpu_ensemble* e, double* out /* [members][RGPU_MON_NQ] */);
int rgpu_ensemble_run_steps_monitored(rgpu_ensemble* e, int nsteps, const double* tEnd, int* nStep, double* t, double* dt,
                                      double* dt_log, int* done, int* stop, int* fused_steps,
                                      int every, int* mon_n /* [members] */, int* mon_step /* [members][cap] */,
                                      double* mon_t /* [members][cap] */, double* mon /* [members][cap][RGPU_MON_NQ] */);
size_t rgpu_ensemble_monitor_device_bytes(const rgpu_params* p, int members);
int rgpu_state_monitor3d(rgpu_ctx* c, int parity, double* out /* [RGPU_MON_NQ] */);
int rgpu_run_steps_monitored(rgpu_ctx* c, int nsteps, double tEnd, int* nStep, double* t, double* dt, double* dt_log,
                             int every, int* mon_n, int* mon_step /* [cap] */, double* mon_t /* [cap] */, double* mon /* [cap][RGPU_MON_NQ] */);
long rgpu_monitor_batch_samples(rgpu_ctx* c);

/* ---- plane monitors: z profiles of a 3D state, reduced on the device ----------------------------------------------------------------
 * What a 3D run is plotted from is resolved along z: the space-time diagram of the mean By(z, t) of an MRI box, the profiles of the
 * Maxwell and Reynolds stresses, the density profile of a stratified box, <rho>(z) and <rho^2>(z) of a mixing layer.  A plane monitor
 * is RGPU_MONP_NQ = 16 doubles for EVERY interior plane kk = k - ghostWidth in [0, nz) of U[parity] of a single-domain 3D context,
 * hydro or MHD, shearing box included, taken over the nx x ny interior cells of the plane and raw (not multiplied by dx dy):
 *     q  0 .. 9   the ten columns of the 3D monitor above (seven sums, min_rho, min_eint, max_absdivb), from the same per-cell terms
 *       10 bx   11 by   12 bz   13 bxby   14 rvxvy   15 rho2                                     sums
 * Terms of cell (i, j, k) of columns 10 - 15, IEEE + - * / in exactly this order, no FMA contraction in either library
 * (csrc/kernels_monitor_planes.h), with rho, mx, my, bxc, byc, bzc as defined for the 3D monitor:
 *     MHD:   bx = bxc, by = byc, bz = bzc (the cell-centred field), bxby = bxc * byc
 *     hydro: bx = by = bz = bxby = +0.0              (columns 6, 9 and 10 - 13 of a hydro state are exactly +0.0)
 *     rvxvy = (mx * my) / rho,   rho2 = rho * rho
 * Row kk: steps 1 - 4 of the summation order above (segments of RGPU_MON_ROWS rows, columns, RGPU_MON_LANES lanes, butterfly) applied
 * to the nx x ny cells of plane kk; columns 7, 8 and 9 take fmin / fmin / fmax along the same route.  There is no step 5 and there are
 * no floating-point atomics: a row depends on (nx, ny) and on its own plane only -- not on nz, the library, the position in a batch,
 * or how the kernels cut the grid.  No ghost fill is done; the high faces of the last interior row, column and plane come from the
 * first ghost layer, as for the monitors.  The NaN rules are the monitors', per plane: a NaN cell propagates into the sums of its
 * own plane that contain it, drops out of that plane's extrema, and changes no other row.
 * Identity: folding the rows ascending in kk from (+0.0 for the sums, +inf for the minima, +0.0 for the maximum) with + / fmin / fmax
 * gives, in columns 0 - 9, the ten doubles of rgpu_state_monitor3d on that state, bit for bit (row kk is V[kk] of its order).
 * (tests/monitor_planes_checks.py is this definition in numpy.)
 *
 *   rgpu_state_monitor_planes   out[nz][RGPU_MONP_NQ] of U[parity].  Reads the state only: ghost cells, CFL slots and what the context
 *                          knows about them stay as they are.  Synchronises.  2D context: RGPU_EUNSUPPORTED ("3D" in the message);
 *                          slab context (slab_count > 1): RGPU_EINVAL; NULL pointer: RGPU_EINVAL; partial sums that do not fit the
 *                          flux array: RGPU_EINVAL.
 *   rgpu_run_steps_monitored_planes   rgpu_run_steps_log (same states, same dt sequence, same return value) plus sampling, with the
 *                          semantics of rgpu_run_steps_monitored word for word: a sample after each step that brings *nStep to a
 *                          multiple of `every`; *mon_n = the samples of this call (<= cap = nsteps / every + 1); sample k: mon_step[k],
 *                          mon_t[k] the host-accumulated *t after that step, mon[(k * nz + kk) * RGPU_MONP_NQ + q] the rows of
 *                          rgpu_state_monitor_planes on that state, bit for bit.  A step that reaches tEnd is sampled if it qualifies,
 *                          nothing is sampled after a stop; *mon_n counts only samples whose values were written.  A run cut into
 *                          calls gives the series of one call.  dt_log may be NULL.
 *                          Where the context takes its time step from the device (rgpu_device_time_step_ready) the two kernels of a
 *                          sample (csrc/hip/monitor_profile.h) are queued behind the last kernel of each qualifying step, return in
 *                          their first instructions when the step's clock record says stop, and write to a device log that is copied
 *                          back once per batch with the clock records: no synchronisation inside a batch.  Everywhere else (first
 *                          steps, gravity, the dissipative stage, forcing with option "forcing_clock" = 0,
 *                          phase timers, option "step_clock" = 0) the call is the
 *                          literal loop: rgpu_one_step_integration, then rgpu_state_monitor_planes.  A call samples the monitor or
 *                          the planes, not both: the monitor's columns are the fold of the rows (the identity above).
 *                          Memory: the partial sums (RGPU_MONP_NQ x nz x ceil(ny / RGPU_MON_ROWS) x nx doubles, then the nz rows of
 *                          a sample taken outside a batch) go to the flux array, dead between steps.  The log -- RGPU_CLOCK_BATCH /
 *                          every + 1 slots of nz x RGPU_MONP_NQ doubles, the samples that can fall into one batch -- and its pinned
 *                          mirror of the same size are allocated by the first call that needs them, grown if a later call needs
 *                          more, freed with the context, and are not part of rgpu_device_bytes.
 *                          Errors: RGPU_EUNSUPPORTED for a 2D context; RGPU_EINVAL for every < 1 ("every" in the message), a NULL
 *                          pointer among nStep, t, dt, mon_n, mon_step, mon_t, mon, nsteps < 0, a slab context, or partial sums that
 *                          do not fit the flux array.
 *   rgpu_monitor_planes_batch_samples   how many plane samples this context has queued on the device inside its batches so far (0
 *                          where every call took the literal loop), as rgpu_monitor_batch_samples -- which these calls leave alone. */
#define RGPU_MONP_NQ 16
#define RGPU_MONP_NAMES "mass mx my mz E ekin emag min_rho min_eint max_absdivb bx by bz bxby rvxvy rho2"   /* the RGPU_MONP_NQ columns, in order */
int rgpu_state_monitor_planes(rgpu_ctx* c, int parity, double* out /* [nz][RGPU_MONP_NQ] */);
int rgpu_run_steps_monitored_planes(rgpu_ctx* c, int nsteps, double tEnd, int* nStep, double* t, double* dt, double* dt_log,
                                    int every, int* mon_n, int* mon_step /* [cap] */, double* mon_t /* [cap] */,
                                    double* mon /* [cap][nz][RGPU_MONP_NQ] */);
long rgpu_monitor_planes_batch_samples(rgpu_ctx* c);

/* ---- map monitors: slices and projections of a 3D state, taken on the device ---------------------------------------------------------
 * What one looks at first in a 3D run is a picture: the mid-plane density of an implosion or a jet, an x-z cut of By in an MRI box,
 * the column density of a turbulent box along each axis.  A map is a 2D array of RGPU_MAP_NQ = 12 channels taken from U[parity] of a
 * single-domain 3D context as the array stands, hydro or MHD, shearing box included.  No ghost fill is done; the high faces of the last
 * interior row, column and plane come from the first ghost layer, as for the monitors.  A map is given by a spec:
 *     axis   0 = x, 1 = y, 2 = z: the direction summed over (w)
 *     lo, hi the range [lo, hi) of interior indices along it, 0 <= lo < hi <= n_axis
 * Channels, in the order of RGPU_MAP_NAMES: channel q of a cell is column {0, 1, 2, 3, 4, 5, 6, 8, 10, 11, 12, 15}[q] of the plane
 * monitor's per-cell terms above (rho = its "mass" term, eint = its "min_eint" term (E - ekin) - emag, rho2 = rho * rho): the same
 * operations in the same order, no FMA contraction in either library (csrc/kernels_monitor_maps.h picks them, it restates nothing).
 * For a hydro state the channels emag, bx, by, bz are exactly +0.0.
 * Pixel: out[q][v][u] = the sum over w = lo .. hi - 1 of channel q of the cell, ascending in w, from +0.0, "a = a + x" at every step;
 * no floating-point atomics, no segments, no butterfly.  The remaining axes (u, v), u varying fastest in memory:
 *     axis z: u = i, v = j, [12][ny][nx]      axis y: u = i, v = k, [12][nz][nx]      axis x: u = j, v = k, [12][nz][ny]
 * A slice is the map whose range holds one cell, hi == lo + 1: +0.0 + term, the term itself (a term of -0.0 becomes +0.0).  One
 * definition and one code path for slices and projections.  A value depends on the state and the spec only -- not on the library, on
 * whether the sample is taken inside a batch, on which kernel ran, or on how the kernels cut the grid.
 * NaN: IEEE addition.  A NaN term makes the one pixel whose column holds it NaN in the channels that contain it and changes nothing
 * else: a NaN density gives NaN in rho, ekin, eint and rho2 of that pixel; mx, my, mz, E, emag, bx, by, bz keep their numbers.
 * Against the monitor: the sum over the pixels of each of channels 0 - 6 of the full z map lies within N 2^-53 sum|terms| (N = nx ny
 * nz), the bound of any summation order stated for the monitors above, of the same column of rgpu_state_monitor3d.
 * (tests/monitor_maps_checks.py is this definition in numpy.)
 *
 *   rgpu_map_doubles       the doubles of the map of *spec on this context, RGPU_MAP_NQ x nv x nu; 0 for a spec (or a context) that
 *                          rgpu_state_maps would refuse.
 *   rgpu_state_maps        nmaps maps of U[parity], one after another in `out` (map m at the sum of rgpu_map_doubles of the specs
 *                          before it).  Reads the state only: ghost cells, CFL slots and what the context knows about them stay as
 *                          they are.  One launch per map, each writing straight to its place in a device buffer (the head of the map
 *                          log below, grown to one sample where it is smaller, whatever the budget); one read-back for all maps.
 *                          Synchronises.
 *   rgpu_run_steps_mapped  rgpu_run_steps_log (same states, same dt sequence, same return value) plus sampling, with the semantics of
 *                          rgpu_run_steps_monitored_planes word for word: a sample (all nmaps maps) after each step that brings
 *                          *nStep to a multiple of `every`; *mon_n = the samples of this call (<= cap = nsteps / every + 1); sample
 *                          k: mon_step[k], mon_t[k] the host-accumulated *t after that step, maps + k * W (W = the sum of
 *                          rgpu_map_doubles over the specs) what rgpu_state_maps gives on that state, bit for bit.  A step that
 *                          reaches tEnd is sampled if it qualifies, nothing is sampled after a stop; *mon_n counts only samples whose
 *                          values were written.  A run cut into calls gives the series of one call.  dt_log may be NULL.
 *                          Where the context takes its time step from the device (rgpu_device_time_step_ready) the kernels of a
 *                          sample (csrc/hip/monitor_maps.h) are queued behind the last kernel of each qualifying step, return in
 *                          their first instructions when the step's clock record says stop, and write to a device log that is copied
 *                          back once per batch with the clock records: no synchronisation inside a batch.  Everywhere else (first
 *                          steps, gravity, the dissipative stage, forcing with option "forcing_clock" = 0,
 *                          phase timers, option "step_clock" = 0) the call is the
 *                          literal loop: rgpu_one_step_integration, then rgpu_state_maps.
 *                          Memory: maps need no scratch, the flux array is not used.  The log of a batch has a byte budget, option
 *                          "map_log_kib" (default 262144: 256 MiB on the device and as much pinned): slots = min(RGPU_CLOCK_BATCH /
 *                          every + 1, budget / bytes of a sample), and a batch is cut so that it holds no more samples than slots.
 *                          A sample larger than the budget: the literal loop.  The log and its pinned mirror are allocated by the
 *                          first call that needs them, grown between batches if a later call needs more, freed with the context,
 *                          and are not part of rgpu_device_bytes.
 *   rgpu_map_batch_samples how many samples (of nmaps maps each) this context has queued on the device inside its batches so far (0
 *                          where every call took the literal loop), as rgpu_monitor_planes_batch_samples.  These calls leave
 *                          rgpu_monitor_batch_samples and rgpu_monitor_planes_batch_samples alone.
 *   Errors (nothing has run, *mon_n == 0): RGPU_EUNSUPPORTED for a 2D context ("3D" in the message: a download is its map);
 *                          RGPU_EINVAL for a slab context (slab_count > 1), a NULL pointer among nStep, t, dt, specs, mon_n,
 *                          mon_step, mon_t, maps / out, nsteps < 0, every < 1 ("every" in the message), nmaps outside 1 ..
 *                          RGPU_MAP_MAX, an axis outside 0 .. 2 or a range that is not 0 <= lo < hi <= n_axis (the message names
 *                          the index of the offending map, "map 2: ..."). */
#define RGPU_MAP_NQ 12
#define RGPU_MAP_NAMES "rho mx my mz E ekin emag eint bx by bz rho2"   /* the RGPU_MAP_NQ channels, in order */
#define RGPU_MAP_MAX 8                                                /* specs per call */
typedef struct { int axis; int lo; int hi; } rgpu_map_spec;   /* axis 0 = x, 1 = y, 2 = z: the direction summed over; [lo, hi) in interior indices along it */
size_t rgpu_map_doubles(rgpu_ctx* c, const rgpu_map_spec* spec);
int rgpu_state_maps(rgpu_ctx* c, int parity, int nmaps, const rgpu_map_spec* specs, double* out);
int rgpu_run_steps_mapped(rgpu_ctx* c, int nsteps, double tEnd, int* nStep, double* t, double* dt, double* dt_log,
                          int every, int nmaps, const rgpu_map_spec* specs, int* mon_n, int* mon_step /* [cap] */, double* mon_t /* [cap] */,
                          double* maps /* [cap][sum of rgpu_map_doubles] */);
long rgpu_map_batch_samples(rgpu_ctx* c);

/* ---- PDF monitors: histograms of a 3D state, counted on the device ---------------------------------------------------------------------
 * The distribution is the fourth shape of the family: the density PDF of a turbulent box, the PDF of |B|, of the magnetic energy or of
 * |div B| in an MRI run, and the joint PDFs -- rho against eint, rho against emag.  A PDF is a table of 64-bit COUNTS over the nx ny nz
 * interior cells of U[parity] of a single-domain 3D context as the array stands, hydro or MHD, shearing box included.  No ghost fill
 * is done; the high faces of the last interior row, column and plane come from the first ghost layer, as for the monitors.  Counts
 * are integers and do not depend on the order of arrival: a table depends on the state and the spec only -- not on the library, on
 * which kernel variant ran, on the grid size, or on whether and where in a batch the sample is taken.
 * Channels, in the order of RGPU_PDF_NAMES: channel q < 12 of a cell is column {0, 1, 2, 3, 4, 5, 6, 8, 10, 11, 12, 9}[q] of the plane
 * monitor's per-cell terms above (rho = its "mass" term, eint = its "min_eint" term (E - ekin) - emag, absdivb = its "max_absdivb"
 * term): the same operations in the same order, no FMA contraction in either library (csrc/kernels_monitor_pdf.h picks them, it
 * restates nothing).  Channel 12: v2 = (ekin + ekin) / rho, the speed squared, from those terms, not contracted.  For a hydro state
 * emag, bx, by, bz and absdivb are exactly +0.0; they may be histogrammed and land in `under` or in the bin that holds 0.
 * An axis: { channel; scale; nbins; sub; lo; hi }.  A value x of the channel falls into one of nbins + 3 classes: the bins 0 .. nbins - 1,
 * then under (nbins), over (nbins + 1) and nan (nbins + 2).  x != x gives nan, tested first.  Otherwise
 *   scale == 0, linear: finite lo < hi and nbins >= 1 (sub is ignored).  x < lo: under.  x >= hi: over.  Else the bin is the integer
 *       part of (x - lo) * inv, at most nbins - 1, where inv = (double)nbins / (hi - lo) is computed once on the host; the subtraction
 *       and the product are IEEE operations, not contracted, in both libraries.
 *   scale == 1, octave bins on |x|, each octave cut into 2^sub sub-bins of equal width; no logarithm is evaluated.  lo and hi are
 *       normal powers of two, lo < hi; 0 <= sub <= 6; nbins == (log2 hi - log2 lo) << sub, anything else is refused.  |x| < lo:
 *       under (zeros and subnormals too).  |x| >= hi: over (infinity too).  Else the bin is (bits(|x|) >> (52 - sub)) - (bits(lo)
 *       >> (52 - sub)), integer arithmetic on the IEEE representation.  Bin b is [lo 2^o (1 + r / 2^sub), lo 2^o (1 + (r + 1) / 2^sub))
 *       with o = b >> sub, r = b mod 2^sub: the edges are exactly representable, so a true log-PDF follows from the counts and the
 *       known widths.
 * A spec: { a; b }.  b.nbins == 0: the 1D histogram of a, a.nbins + 3 words in class order (b is not looked at).  Else the joint
 * table, (a.nbins + 3) x (b.nbins + 3) words, the word of a cell at ia * (b.nbins + 3) + ib; the tail classes are its last three rows
 * and columns.  Identities: the words of every spec sum to nx ny nz; the sum of a joint table over ib is the 1D histogram of a, word
 * for word.  (tests/monitor_pdf_checks.py is this definition in numpy.)
 *
 *   rgpu_pdf_words         the words of *spec; 0 for a spec that is refused (a bad axis, more than RGPU_PDF_MAX_WORDS words, NULL).
 *   rgpu_state_pdfs        npdfs tables of U[parity], one after another in `out` (table m at the sum of rgpu_pdf_words of the specs
 *                          before it).  The state is read ONCE however many specs the call has -- hence the shared word budget,
 *                          RGPU_PDF_MAX_WORDS for all specs of a call together: the counts of a workgroup are kept in LDS.  Reads
 *                          the state only: ghost cells, CFL slots and what the context knows about them stay as they are.  Two
 *                          launches (csrc/hip/monitor_pdf.h), partial counts in the flux array, which is dead between two steps.
 *                          Synchronises.
 *   rgpu_run_steps_pdfs    rgpu_run_steps_log (same states, same dt sequence, same return value) plus sampling, with the semantics of
 *                          rgpu_run_steps_mapped word for word: a sample (all npdfs tables) after each step that brings *nStep to a
 *                          multiple of `every`; *mon_n = the samples of this call (<= cap = nsteps / every + 1); sample k:
 *                          mon_step[k], mon_t[k] the host-accumulated *t after that step, pdfs + k * W (W = the sum of
 *                          rgpu_pdf_words over the specs) what rgpu_state_pdfs gives on that state, word for word.  A step that
 *                          reaches tEnd is sampled if it qualifies, nothing is sampled after a stop; *mon_n counts only samples
 *                          whose values were written.  A run cut into calls gives the series of one call.  dt_log may be NULL.
 *                          Where the context takes its time step from the device (rgpu_device_time_step_ready) the kernels of a
 *                          sample are queued behind the last kernel of each qualifying step, return in their first instructions when
 *                          the step's clock record says stop, and store to a device log that is copied back once per batch with the
 *                          clock records: no synchronisation inside a batch, no zeroing of the log.  Everywhere else (first steps,
 *                          gravity, the dissipative stage, forcing with option "forcing_clock" = 0,
 *                          phase timers, option "step_clock" = 0) the call is the literal
 *                          loop: rgpu_one_step_integration, then rgpu_state_pdfs.  The log has RGPU_CLOCK_BATCH / every + 1 slots
 *                          (a sample is at most 128 KiB), is allocated by the first call that needs it, grown between batches if a
 *                          later call needs more, freed with the context, and is not part of rgpu_device_bytes.
 *   rgpu_pdf_batch_samples how many samples this context has queued on the device inside its batches so far (0 where every call
 *                          took the literal loop).  These calls leave the other monitors' counters alone.
 *   Errors (nothing has run, *mon_n == 0): RGPU_EUNSUPPORTED for a 2D context ("3D" in the message); RGPU_EINVAL for a slab context
 *                          (slab_count > 1), a NULL pointer among nStep, t, dt, specs, mon_n, mon_step, mon_t, pdfs / out, nsteps
 *                          < 0, every < 1 ("every" in the message), npdfs outside 1 .. RGPU_PDF_MAX, a bad axis -- channel, scale,
 *                          range, the power-of-two rule, nbins, sub (the message names the spec, "pdf 1: ...") -- more than
 *                          RGPU_PDF_MAX_WORDS words in all, or a flux array too small for one workgroup's counts. */
#define RGPU_PDF_NQ 13
#define RGPU_PDF_NAMES "rho mx my mz E ekin emag eint bx by bz absdivb v2"   /* the RGPU_PDF_NQ channels, in order */
#define RGPU_PDF_MAX 8                                                      /* specs per call */
#define RGPU_PDF_MAX_WORDS 16384                                            /* words of all specs of a call together */
typedef struct { int channel; int scale; int nbins; int sub; double lo; double hi; } rgpu_pdf_axis;
typedef struct { rgpu_pdf_axis a, b; } rgpu_pdf_spec;   /* b.nbins == 0: a 1D histogram of a; else the joint one */
size_t rgpu_pdf_words(const rgpu_pdf_spec* spec);
int rgpu_state_pdfs(rgpu_ctx* c, int parity, int npdfs, const rgpu_pdf_spec* specs, unsigned long long* out);
int rgpu_run_steps_pdfs(rgpu_ctx* c, int nsteps, double tEnd, int* nStep, double* t, double* dt, double* dt_log,
                        int every, int npdfs, const rgpu_pdf_spec* specs, int* mon_n, int* mon_step /* [cap] */, double* mon_t /* [cap] */,
                        unsigned long long* pdfs /* [cap][sum of rgpu_pdf_words] */);
long rgpu_pdf_batch_samples(rgpu_ctx* c);

/* ---- spectrum monitors: shell-binned power spectra of a 3D state, taken on the device -------------------------------------------------
 * The power per wave-number shell is the fifth shape of the family: E(k) of a turbulent box, the kinetic, magnetic and density spectra
 * of an MRI run, the one-dimensional spectra along an axis.  The box is a single-domain 3D context whose nx, ny, nz are each a power
 * of two from 4 to 1024, and it is treated as PERIODIC in all three directions whatever its boundary conditions are: only the
 * N = nx ny nz interior cells of U[parity] are read, as the array stands, hydro or MHD.  No ghost fill is done; the cell-centred B of
 * the last interior row, column and plane takes its high faces from the first ghost layer, as for the plane monitor.  In a shearing
 * box the transform is the plain lab-frame one: no remap to shearing coordinates is done, so between the periodic points of the shear
 * the x direction is not periodic and the spectra along x carry the jump.
 * Channels, in the order of RGPU_SPECTRUM_NAMES: rho, mx my mz and bx by bz are columns 0, 1 2 3 and 10 11 12 of the plane monitor's
 * per-cell terms above (csrc/kernels_monitor_spectrum.h picks them, it restates nothing); v = m / rho; w = m / sqrt(rho), the
 * density-weighted velocity, whose spectrum sums to twice the kinetic energy per cell.  v and w are formed from those terms with the
 * library's division and square root (exactly rounded in librgpu.so, within a few ulp in librgpu_fast.so), not contracted.  For a hydro
 * state bx, by, bz are exactly +0.0.
 * A spec: { channels; wx, wy, wz }.  `channels` is a non-empty bit mask over the RGPU_SPECTRUM_NQ channels (bit q: channel q); the
 * weights are integers 0 .. RGPU_SPECTRUM_MAX_WEIGHT, not all zero.  With u_c a channel,
 *   u^_c(k) = (1 / N) sum_x u_c(x) exp(-2 pi i (kx i / nx + ky j / ny + kz k / nz)),
 * k the integer wave vector, k_a folded to -n_a / 2 .. n_a / 2 - 1.  The shell of a mode is defined in integers: with
 * q = (wx kx)^2 + (wy ky)^2 + (wz kz)^2, shell s is the s >= 0 with s^2 - s + 1 <= q <= s^2 + s (shell 0: q = 0).  That is
 * round(sqrt(q)) with every edge exact; no square root is evaluated.  A spec has S = shell(sum_a (w_a n_a / 2)^2) + 1 shells, at most
 * RGPU_SPECTRUM_MAX_SHELLS.  Its output is 2 S doubles:
 *   P[s] = sum over the modes k of shell s, over the channels c of the mask, of |u^_c(k)|^2
 *   M[s] = the number of modes of shell s, as a double (an exact integer).
 * Weights (1, 1, 1): the isotropic spectrum in units of the fundamental; (4, 1, 4): physical shells of a 1 : 4 : 1 box in units of
 * 2 pi / Ly; (0, 1, 0): the one-dimensional spectrum along y, summed over kx and kz, the shell |ky|.  Identities: sum_s P[s] =
 * (1 / N) sum_x sum_c u_c^2 (Parseval) to rounding; sum_s M[s] = N exactly.
 * How it is computed (csrc/hip/monitor_spectrum.h): per pair of channels a, b of the mask in ascending order (an odd
 * last one with zero) ONE complex transform of Z = a + i b -- every shell is symmetric under k -> -k, so the shell sums of |Z^|^2 are
 * those of |a^|^2 + |b^|^2 -- in three passes of radix-2 line transforms, x, y, z, each with the whole line in LDS, twiddle factors
 * from one table computed on the host; the z pass bins |Z^|^2 without writing Z^ back.  All work lies in the flux array, which is
 * dead between two steps.
 * Reproducibility: within one library the same state and spec give the same doubles bit for bit, on every call, wherever in a batch
 * the sample is taken, whatever other specs share the call, and for every value of option "spectrum_tile_y".  No floating-point
 * atomics: in a workgroup a shell has one owner per part of a tile's columns (parts and tiles assigned by the box and the spec alone),
 * who adds tile after tile, column after column, |kz| ascending, +kz before -kz; the partial sums are added in the order workgroup,
 * part, in sixteen runs whose sums are added ascending, and the result is stored.  M is the same in both libraries, word for
 * word.  P differs between librgpu.so, librgpu_fast.so and another FFT by rounding: the transforms are backward stable, |dP[s]| <=
 * e (P[s] + 2 sqrt(P[s] Ptot)) + e^2 Ptot with e the relative L2 error of the transforms (tests: e = 1e-12; measured: DESIGN 3.4.6).
 *
 *   rgpu_spectrum_shells        S of *spec on this context; 0 for a context or a spec that is refused.
 *   rgpu_state_spectra          nspec outputs of U[parity], one after another in `out` (spec m at the sum of 2 S of the specs before
 *                               it: P[0 .. S), then M[0 .. S)).  Reads the state only: ghost cells, CFL slots and what the context knows
 *                               about them stay as they are.  Synchronises.
 *   rgpu_run_steps_spectra      rgpu_run_steps_log (same states, same dt sequence, same return value) plus sampling, with the semantics
 *                               of rgpu_run_steps_pdfs word for word: a sample (all nspec outputs) after each step that brings *nStep to
 *                               a multiple of `every`; *mon_n = the samples of this call (<= cap = nsteps / every + 1); sample k:
 *                               mon_step[k], mon_t[k] the host-accumulated *t after that step, spectra + k * W (W = the sum of 2 S over
 *                               the specs) what rgpu_state_spectra gives on that state, bit for bit.  A step that reaches tEnd is
 *                               sampled if it qualifies, nothing is sampled after a stop; *mon_n counts only samples whose values were
 *                               written.  A run cut into calls gives the series of one call.  dt_log may be NULL.  Where the context
 *                               takes its time step from the device (rgpu_device_time_step_ready) the kernels of a sample are queued
 *                               behind the last kernel of each qualifying step, return in their first instructions when the step's clock
 *                               record says stop, and store to a device log that is copied back once per batch with the clock records.
 *                               Everywhere else the call is the literal loop: rgpu_one_step_integration, then rgpu_state_spectra.  The
 *                               log has RGPU_CLOCK_BATCH / every + 1 slots, is allocated by the first call that needs it, grown between
 *                               batches if a later call needs more, freed with the context, and is not part of rgpu_device_bytes; nor
 *                               is the table of twiddle factors (8 KiB, uploaded by the first call that needs it, freed with the context).
 *   rgpu_spectrum_batch_samples how many samples this context has queued on the device inside its batches so far (0 where every call
 *                               took the literal loop).  These calls leave the other monitors' counters alone.
 *   Errors (nothing has run, *mon_n == 0): RGPU_EUNSUPPORTED for a 2D context ("3D" in the message) and for an extent that is not a
 *                               power of two in 4 .. 1024 (the message names it, "nx = 65 ..."); RGPU_EINVAL for a slab context
 *                               (slab_count > 1), a NULL pointer among nStep, t, dt, specs, mon_n, mon_step, mon_t, spectra / out,
 *                               nsteps < 0, every < 1 ("every" in the message), nspec outside 1 .. RGPU_SPECTRUM_MAX, an empty mask or
 *                               one with bits beyond the channels, a weight outside 0 .. RGPU_SPECTRUM_MAX_WEIGHT, all weights zero,
 *                               more than RGPU_SPECTRUM_MAX_SHELLS shells (the message names the spec, "spectrum 1: ..."), or a flux
 *                               array too small for the transform and the partial sums. */
#define RGPU_SPECTRUM_NQ 13
#define RGPU_SPECTRUM_NAMES "rho mx my mz vx vy vz wx wy wz bx by bz"   /* the RGPU_SPECTRUM_NQ channels, in order */
#define RGPU_SPECTRUM_MAX 4                                            /* specs per call */
#define RGPU_SPECTRUM_MAX_SHELLS 4096                                  /* shells of one spec */
#define RGPU_SPECTRUM_MAX_WEIGHT 64                                    /* largest weight of an axis */
typedef struct { unsigned channels; int wx, wy, wz; } rgpu_spectrum_spec;
int rgpu_spectrum_shells(rgpu_ctx* c, const rgpu_spectrum_spec* spec);
int rgpu_state_spectra(rgpu_ctx* c, int parity, int nspec, const rgpu_spectrum_spec* specs, double* out);
int rgpu_run_steps_spectra(rgpu_ctx* c, int nsteps, double tEnd, int* nStep, double* t, double* dt, double* dt_log,
                           int every, int nspec, const rgpu_spectrum_spec* specs, int* mon_n, int* mon_step /* [cap] */, double* mon_t /* [cap] */,
                           double* spectra /* [cap][sum of 2 S] */);
long rgpu_spectrum_batch_samples(rgpu_ctx* c);

/* ---- Helmholtz spectra: solenoidal and compressive power of a vector field per shell, taken on the device ---------------------------
 * The sixth shape of the family: how the power of a vector field splits, shell by shell, into the part transverse to the wave vector
 * (solenoidal) and the part along it (compressive) -- the diagnostic of a driven run (what its forcing really injects: DESIGN 3.4.8),
 * the sound-wave content of w = m / sqrt(rho), the distance of the cell-centred B from the divergence-free face field.
 * rgpu_state_spectra cannot give it: it packs two real channels into one complex transform, so the components of a vector never meet
 * at the same mode.
 * Context: that of the spectrum monitors above, word for word -- a lone single-domain 3D context, extents powers of two in 4 .. 1024,
 * the box taken as periodic, the interior cells of U[parity] as the array stands, the plain lab-frame transform in a shearing box.
 * A spec: { field; wx, wy, wz }.  `field` indexes RGPU_HELM_NAMES: m, v, w, b are the channel triples 1-3, 4-6, 7-9 and 10-12 of
 * RGPU_SPECTRUM_NAMES, formed by the same code (csrc/kernels_monitor_helm.h picks them, it restates nothing).  The weights are
 * integers 1 .. RGPU_SPECTRUM_MAX_WEIGHT; a zero weight is refused, because here the weights also give the wave vector its direction
 * and a dropped axis has none.
 * With u^_a(k), a = x, y, z, the transforms of the three components as defined above and k_a the SIGNED folded wave number
 * (-n_a / 2 .. n_a / 2 - 1: the Nyquist index counts as -n_a / 2), kappa_a = w_a k_a (an exact double), q = kappa_x^2 + kappa_y^2 +
 * kappa_z^2 is the integer of the spectrum monitors, the shell of q follows from the same integer rule, and a spec has the same S.
 * Per mode, without contraction and in this order (helm_mode, the one definition every kernel uses):
 *   d = (kappa_x u^_x + kappa_y u^_y) + kappa_z u^_z                 real and imaginary part separately
 *   c = kappa x u^: c_x = kappa_y u^_z - kappa_z u^_y, c_y = kappa_z u^_x - kappa_x u^_z, c_z = kappa_x u^_y - kappa_y u^_x
 *   q > 0:  L = (d.re^2 + d.im^2) / q,  T = ((|c_x|^2 + |c_y|^2) + |c_z|^2) / q      the division is the library's own (rg_div)
 *   q = 0:  L = +0.0,  T = (|u^_x|^2 + |u^_y|^2) + |u^_z|^2                          the mean flow counts as solenoidal, in shell 0
 * Both parts are computed directly, never one as the difference of the total and the other: a nearly pure field does not lose its
 * small part to cancellation.  The output of a spec is 3 S doubles:
 *   Psol[s] = sum of T over the modes of shell s,  Pcomp[s] = sum of L,  M[s] = the number of modes, as a double (an exact integer).
 * Identities: sum_s (Psol[s] + Pcomp[s]) = (1 / N) sum_x |u(x)|^2 to rounding (|kappa x u^|^2 + |kappa . u^|^2 = q |u^|^2, Parseval);
 * Psol[s] + Pcomp[s] agrees with P[s] of rgpu_state_spectra for the same three channels and weights within the bound below (twice
 * it: each side has its own rounding); M equals that call's M word for word.
 * How it is computed (csrc/hip/monitor_helm.h): per spec three transforms, one per component with imaginary part zero,
 * into three arrays in the flux array.  The x and y passes are the spectrum monitor's kernels as they are; a z pass writes the first
 * two arrays back; the binning pass transforms the third in LDS, reads the other two at the same mode, replaces each element of its
 * tile by (T, L) and then bins with the owners, the column and the |kz| order of the spectrum monitor; a fold stores.
 * Reproducibility: as for the spectrum monitors -- within one library the same doubles bit for bit on every call, wherever in a batch
 * the sample is taken, whatever other specs share the call, and for every value of option "spectrum_tile_y"; no floating-point
 * atomics, no zeroing pass; M the same in both libraries, word for word.  For each of Psol and Pcomp, against another FFT:
 * |dP_c[s]| <= e (P_c[s] + 2 sqrt(P_c[s] Ptot)) + e^2 Ptot with Ptot = sum_s (Psol + Pcomp) -- the bound of the spectra carries over
 * because both projections are contractions of u^ (tests: e = 1e-12; measured: DESIGN 3.4.8).
 *
 *   rgpu_helm_shells            S of *spec on this context; 0 for a context or a spec that is refused, for its scratch included.
 *   rgpu_state_helm_spectra     nspec outputs of U[parity], one after another in `out` (spec m at the sum of 3 S of the specs before it:
 *                               Psol[0 .. S), Pcomp[0 .. S), M[0 .. S)).  Reads the state only.  Synchronises.
 *   rgpu_run_steps_helm_spectra rgpu_run_steps_spectra word for word with W = the sum of 3 S over the specs: the same states, dt
 *                               sequence and return value as rgpu_run_steps_log, a sample after each step that brings *nStep to a
 *                               multiple of `every`, each what rgpu_state_helm_spectra gives on that state, bit for bit; inside the
 *                               device-clock batches the kernels of a sample are queued behind the qualifying step, gated by its clock
 *                               record, and the log (RGPU_CLOCK_BATCH / every + 1 slots, a buffer of its own, not part of
 *                               rgpu_device_bytes) is copied back once per batch; everywhere else the literal loop.  The table of
 *                               twiddle factors is the spectrum monitors'.
 *   rgpu_helm_batch_samples     how many samples this context has queued on the device inside its batches so far.  These calls leave
 *                               the other monitors' counters alone, and the other monitors leave this one alone.
 *   Errors (nothing has run, *mon_n == 0): those of the spectrum monitors -- RGPU_EUNSUPPORTED for a 2D context and for an extent that
 *                               is not a power of two in 4 .. 1024; RGPU_EINVAL for a slab context, a NULL pointer, nsteps < 0,
 *                               every < 1, nspec outside 1 .. RGPU_HELM_MAX, more than RGPU_SPECTRUM_MAX_SHELLS shells, a flux array too
 *                               small for the three transforms and the partial sums of one workgroup (where it is too small for
 *                               those of all workgroups of the binning pass, fewer run: the count follows from the box, the spec
 *                               and the flux array of the context alone, and is part of the fixed summation order) -- and RGPU_EINVAL for `field` outside
 *                               0 .. RGPU_HELM_NF - 1, a zero weight ("zero" in the message) or a weight outside
 *                               1 .. RGPU_SPECTRUM_MAX_WEIGHT (the message names the spec, "spectrum 1: ..."). */
#define RGPU_HELM_NF 4
#define RGPU_HELM_NAMES "m v w b"   /* the RGPU_HELM_NF vector fields, in order */
#define RGPU_HELM_MAX 4             /* specs per call */
typedef struct { int field; int wx, wy, wz; } rgpu_helm_spec;
int rgpu_helm_shells(rgpu_ctx* c, const rgpu_helm_spec* spec);
int rgpu_state_helm_spectra(rgpu_ctx* c, int parity, int nspec, const rgpu_helm_spec* specs, double* out);
int rgpu_run_steps_helm_spectra(rgpu_ctx* c, int nsteps, double tEnd, int* nStep, double* t, double* dt, double* dt_log,
                                int every, int nspec, const rgpu_helm_spec* specs, int* mon_n, int* mon_step /* [cap] */, double* mon_t /* [cap] */,
                                double* spectra /* [cap][sum of 3 S] */);
long rgpu_helm_batch_samples(rgpu_ctx* c);

/* Self-test of the device arithmetic the parity contract rests on: for n operand pairs computes on the device
 *   quot[i]  = rg_div(num[i], rg_recip(den[i]))   the shared-reciprocal division of csrc/hip/rg_backend.h
 *   quot2[i] = num[i] / den[i]                    the compiler's IEEE division
 *   root[i]  = rg_sqrt(num[i]),  root2[i] = sqrt(num[i])
 * (host arrays).  Inside the documented operand range all four equal the correctly rounded results bit for bit. */
int rgpu_selftest_arith(int n, const double* num, const double* den, double* quot, double* quot2, double* root, double* root2);

/* Self-test of the one place where the exact library departs from the reference's instruction sequence on data-dependent grounds:
 * the Alfven speeds of the 2D HLLD edge solver (mag_riemann2d_hlld, riemann_mhd.h:727-738) are formed for the WINNER of each group
 * of four |b| / sqrt(rho) candidates, picked on the operands (csrc/dev_numerics.h: alfven_pick / alfven_duel); a lane whose ordering
 * is closer than the error bound sends its wave down the reference's sequence.  For n samples -- SoA, states36[q * n + i]: the four
 * corner states LL, RL, LR, RR of an edge (r p u v w a b c each, q = 0..31) and their electric fields ELL, ERL, ELR, ERR (q = 32..35)
 * -- the device evaluates the solver twice, e_select[i] through the selection and e_reference[i] through the reference's sequence,
 * with the knobs of *p (gamma0, cIso, smallc, ...); route[i] = 1 when sample i's wave (64 consecutive samples) took the reference's
 * sequence anyway.  e_select must equal e_reference bit for bit (tests/test_gpu_parity.py: >= 1e7 random and adversarial states).
 * The contracted library has no selection: both outputs come from the same sequence and route is 1. */
int rgpu_selftest_alfven(const rgpu_params* p, int n, const double* states36, double* e_select, double* e_reference, int* route);

/* ---- Environment and options ------------------------------------------------------------------------------------------------
 * Environment variables the libraries read (all optional; everything else is an argument of an entry point):
 *   RGPU_TILED=0              librgpu.so: the flat per-cell kernels everywhere instead of the LDS-tiled cooperative ones (a second,
 *                             independently tested implementation of every step; 3-10x slower).  On the device the default suite
 *                             runs it in a child process, one case per step family against the oracle
 *                             (tests/test_flat_path_gpu.py: test_flat_kernels_everywhere_vs_oracle); contexts with a per-cell gravity
 *                             field take the same kernels in any process
 *   RGPU_COMM_SCHEDULE=1|2    librgpu_comm.so: step schedule of the slab driver where the caller leaves the choice to it (rgpu_comm_set_overlap(-1), rgpu_comm.h)
 *   RGPU_COMM_PACK=0          ... one send / recv per variable and face instead of the packed exchange
 *   RGPU_HALO_PRIO=high|low   ... priority of the halo stream (default: normal)
 *   RGPU_COMM_ONE_STREAM=1    ... halo traffic on the compute stream (no overlap): fallback should two streams on one RCCL
 *                             communicator misbehave on a given node
 *   RGPU_HDF5_LIB=<path>      host layer: the libhdf5 to load (default: the system's)
 *   RGPU_RESTART_FORMAT=...   host layer: what rgpuh_* writes for restarts (run_driver.h)
 * Diagnostic options (process-wide; tests run a configuration both ways through them -- a user needs none):
 *   "spec" (1)          kernels specialised for the solver configuration; 0: the generic instantiations
 *   "ghost_images" (1)  the fused 2D steps write the ghost images of their output; 0: the next step fills the ghost cells
 *   "step_clock" (1)    the time step stays on the device between the steps of rgpu_run_steps; 0: one host turn per step
 *   "xcd_sub" (-1)      sub-band size (cells) of the XCD-aware workgroup order of the flat kernels, read by rgpu_create; 0: linear
 *   "zseg" (0)          planes per z segment of the tiled sweeps; 0: planned per launch
 *   "chunks" (-1)       chunks of the two-stream schedule of the flat 3D MHD kernels, read by rgpu_create; 1: one stream
 *   "history_batch" (1) rgpu_run_steps_history samples on the device inside the device-clock batches; 0: its literal loop everywhere
 *   "forcing_clock" (1) rgpu_run_steps* batch a lone 3D context with random / Ornstein-Uhlenbeck forcing; 0: its literal loop
 *   "member_params" (0) 1: the fused rounds of EVERY ensemble read their constants from the per-member table (the path of a
 *                       parameter scan), even when all sets are equal: the table path and the by-value path on one workload
 *   "map_log_kib" (262144) byte budget, in KiB, of the device log of the maps a batch of rgpu_run_steps_mapped samples ("map monitors")
 *   "map_x_tiled" (-1)  which kernel sums a map along x: -1 by the thickness of the range, 0 the direct one, 1 the tiled one (the same bits)
 *   "pdf_replicas" (-1) copies of the LDS table of counts the PDF monitor's kernel keeps: -1 automatic, n forces the count (the same words)
 *   "pdf_groups" (-1)   workgroups of that kernel: -1 automatic, n forces the grid size (the same words)
 *   "spectrum_tile_y" (-1) log2 of the adjacent x a tile of the spectrum monitor's y pass holds: -1 the widest that fits, 0 .. 6 forces it (the same doubles)
 * rgpu_set_option returns the previous value (-1: unknown name; the options above are never negative except "as created" and the
 * defaults of "map_x_tiled", "pdf_replicas", "pdf_groups" and "spectrum_tile_y"). */
int rgpu_set_option(const char* name, int value);
int rgpu_get_option(const char* name);

/* name of the device backend the library was built for ("hip-gfx950") */
const char* rgpu_backend_name(void);

/* floating-point arithmetic of the kernels in this library:
 *   "exact"       librgpu.so       no FMA contraction, correctly rounded division / square root, the reference's operand
 *                                  order: results bit-identical to the reference's CPU path
 *   "contracted"  librgpu_fast.so  the same sources with FMA contraction, a division within 18 ulp (measured; half of the
 *                                  quotients correctly rounded, 93 % within 2 ulp) and a square root within 1 ulp: results agree
 *                                  with the reference to round-off (relative L2 < 1e-12 on every golden fixture), ~20 %
 *                                  faster on the 3D MHD step.  Same ABI: link one or the other. */
const char* rgpu_arithmetic(void);

/* block until all queued work of this context is complete */
int rgpu_synchronize(rgpu_ctx* c);

/* ---- instrumentation (the reference's DO_TIMING phase timers, MHDRunGodunov.h:382-430) ------------------- */

enum {
  RGPU_T_BOUNDARIES = 0, RGPU_T_PRIM, RGPU_T_ELEC, RGPU_T_TRACE, RGPU_T_FLUX, RGPU_T_EMF, RGPU_T_UPDATE,
  RGPU_T_SHEAR, RGPU_T_DT, RGPU_T_DISSIPATIVE, RGPU_T_SWEEP, RGPU_T_COUNT
};
/* RGPU_T_FLUX is the Riemann phase: face fluxes and edge EMFs are one kernel (RGPU_T_EMF stays 0).
 * RGPU_T_SWEEP is the LDS-tiled, z-marching fused kernel (hydro 3D: the whole step; 3D MHD: trace + Riemann problems).
 * enable!=0 brackets every phase with hipEvents (serialises the stream; off by default) */
int rgpu_enable_timers(rgpu_ctx* c, int enable);
/* accumulated seconds per phase since creation / last reset; n <= RGPU_T_COUNT */
int rgpu_get_timers(rgpu_ctx* c, double* secs, int n);
int rgpu_reset_timers(rgpu_ctx* c);
const char* rgpu_timer_name(int which);

/* name / average duration [ms] / launch count of the dominant kernel of the last timed steps, measured with
 * hipEvents on the context's stream (used by bench.py's roofline object) */
int rgpu_dominant_kernel(rgpu_ctx* c, char* name, int name_len, double* avg_ms, long* launches);

/* ---- host side of the reference interface (C++ lives in csrc/host; these are its C entry points) ---------- */

/* Parse an .ini file exactly like ConfigMap + HydroParameters (float-parsed knobs, case-insensitive keys,
 * ConfigMap.cpp:41-49, INIReader.cpp:94-101) with optional "section.key=value;..." overrides. */
int rgpuh_params_from_ini(const char* ini_path, const char* overrides, rgpu_params* out, char* err, int err_len);

/* the [run] section the reference's start() loop reads: nstepmax, tend, noutput (HydroRunBase.cpp:224-232) */
int rgpuh_run_settings(const char* ini_path, const char* overrides, int* nStepmax, double* tEnd, int* nOutput,
                       char* err, int err_len);

/* Fill hU (rgpu_state_elems doubles, zeroed first) with the initial condition named by [hydro] problem:
 * jet, implode (HydroRunBase.cpp:5282-5350, 5449-5536), Orszag-Tang, Brio-Wu, MRI
 * (MHDRunBase.cpp:1378-1475, 1870-2080, 2677-2758).  For a slab, only planes of this slab are produced
 * (the MRI drand48 stream is skipped ahead so that every slab draws the numbers the single-domain run would). */
int rgpuh_init_condition(const char* ini_path, const char* overrides, const rgpu_params* p, double* hU,
                         char* err, int err_len);

/* Fill hG (3 * cells doubles: x, y, z component, ghost cells included; zeroed first) with the static gravity field the
 * problem's init routine writes into h_gravity: Keplerian-disk (HydroRunBase.cpp:6489-6500, 6575-6597).  Returns 1 when the problem defines a field (params_from_ini then says gravityEnabled = 2), 0 when it does not,
 * a negative RGPU_E* on error. */
int rgpuh_init_gravity(const char* ini_path, const char* overrides, const rgpu_params* p, double* hG,
                       char* err, int err_len);

/* Same for the static driving field of the "turbulence" problem (turbulenceInit.cpp; params_from_ini then says
 * randomForcingEnabled = 1): hF = 3 * cells doubles.  Returns 1 / 0 / negative like rgpuh_init_gravity. */
int rgpuh_init_forcing(const char* ini_path, const char* overrides, const rgpu_params* p, double* hF,
                       char* err, int err_len);

/* Run [run] nstepmax / tend like MHDRunGodunov::start / HydroRunGodunov::start on one GPU; writes .vti outputs
 * when [output] outputVtk=yes.  Returns steps done (>=0) or a negative error. Mcell-updates/s is printed like
 * MHDRunGodunov.cpp:4064-4068. */
int rgpuh_run(const char* ini_path, const char* overrides, double* mcell_per_s, char* err, int err_len);

/* The run loop of rgpuh_run with the stepping delegated -- the seam of the z-slab front end (include/rgpu_comm.h fills the
 * hooks with the slab driver; euler_hip --slabs N).  The run builds the context of slab `slab_rank` of `slab_count` and its
 * initial state (initial condition, or [run] restart from the .h5 of the whole box), calls attach(user, ctx, &hooks), then
 * runs the reference's time loop through the hooks: ghost fill, dt, one step; outputs go to ONE HDF5 file per output step for
 * the whole box (the ranks take turns, hooks.barrier between them) and are identical to the single-domain files; detach(user)
 * at the end.  Returns the number of steps or a negative error code (message in err). */
typedef struct rgpuh_step_hooks {
  void* self;
  int (*make_all_boundaries)(void* self, int parity, double totalTime, double dt);
  int (*compute_dt)(void* self, int useU, double* dt);
  int (*one_step_integration)(void* self, int* nStep, double* totalTime, double* dt);
  int (*barrier)(void* self);
  const char* (*last_error)(void* self);
  int (*history_mri)(void* self, int parity, double* out8);   /* optional (may be 0): rgpu_history_mri over the whole box */
  /* optional (may be 0; then barrier is used): collective over all ranks, returns the NUMBER of ranks that passed
   * local_failed != 0 (or a negative code when the transport itself failed).  The run loop calls it where one rank alone
   * can fail -- file output -- so that every rank throws together instead of one leaving the others in a collective. */
  int (*agree)(void* self, int local_failed);
  /* optional: the 14 numbers after "totalTime dt" of the MPI classes' turbulence history row (rgpu_comm_history_turbulence) */
  int (*history_turbulence)(void* self, int parity, double* out14);
  /* optional: the loop body for a run of quiet steps (rgpu_comm_run_steps; contract of rgpu_run_steps: steps done or a negative code) */
  int (*run_steps)(void* self, int nsteps, double tEnd, int* nStep, double* totalTime, double* dt);
} rgpuh_step_hooks;
typedef int (*rgpuh_attach_fn)(void* user, rgpu_ctx* ctx, rgpuh_step_hooks* hooks);
typedef void (*rgpuh_detach_fn)(void* user);
int rgpuh_run_hooked(const char* ini_path, const char* overrides, int slab_rank, int slab_count, rgpuh_attach_fn attach,
                     rgpuh_detach_fn detach, void* user, double* mcell_per_s, char* err, int err_len);

#ifdef __cplusplus
}
#endif
#endif /* RGPU_H_ */
