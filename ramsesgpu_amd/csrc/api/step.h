// api/step.h -- what every core of the step shares: the ghost-fill pieces (pre / post / plane-ranged / full), the plane-range
// helpers, and the fused CFL scan: which kernel family may carry it (the policy functions) and what one core call does about it
// (ScanPlan).  The cores follow in api/step_hydro.h and api/step_mhd.h, their dispatch in api/step_core.h.  See api/ctx.h.
#pragma once
namespace {
// ---- the step -------------------------------------------------------------------------------------------------
int step_pre(rgpu_ctx* c, int nStep) {
  if (c->g.rot) return 0;
  if (c->rec.ghosts_valid(nStep % 2)) return 0;   // the kernel that wrote this state filled its ghost cells too (periodic images)
  Phase ph(c, RGPU_T_BOUNDARIES);
  double* in = c->U[nStep % 2];
  FillXY f;
  if (z_fill_is_planewise(c) && fill_xy_plan(c, 0.0, 0.0, &f)) {   // X and Y in one launch over the interior planes, then Z copies whole planes
    if (launch_fill_xy(c, in, f, c->g.three_d ? c->g.gw : 0, c->g.three_d ? c->g.ksize - c->g.gw : 1, 0, 0)) return -1;
  } else if (do_make_boundaries(c, in, RGPU_XDIR) || do_make_boundaries(c, in, RGPU_YDIR)) return -1;
  if (c->g.three_d && do_make_boundaries(c, in, RGPU_ZDIR)) return -1;
  return 0;
}

int step_post_a(rgpu_ctx* c, int nStep, double dt_arg, double t_arg) {
  if (!c->g.rot) return 0;
  const StepTime st = step_time(c, dt_arg, t_arg);
  if (st.skip) return 0;
  const double dt = st.dt, totalTime = st.t;
  Phase ph(c, RGPU_T_BOUNDARIES);
  double* out = c->U[(nStep + 1) % 2];
  FillXY f;
  if (z_fill_is_planewise(c) && fill_xy_plan(c, totalTime, dt, &f))   // Y, shear, [Z], Y (or X, Y) as one pass over the interior planes; post_b adds Z
    return launch_fill_xy(c, out, f, c->g.three_d ? c->g.gw : 0, c->g.three_d ? c->g.ksize - c->g.gw : 1, 0, 0);
  if (c->g.shearbox && c->g.three_d) {
    if (do_make_boundaries(c, out, RGPU_YDIR)) return -1;
    return do_make_boundaries_shear(c, out, totalTime, dt);
  }
  if (do_make_boundaries(c, out, RGPU_XDIR) || do_make_boundaries(c, out, RGPU_YDIR)) return -1;
  return 0;
}

int step_post_b(rgpu_ctx* c, int nStep) {
  if (!c->g.rot) return 0;
  Phase ph(c, RGPU_T_BOUNDARIES);
  double* out = c->U[(nStep + 1) % 2];
  if (c->g.three_d && do_make_boundaries(c, out, RGPU_ZDIR)) return -1;
  FillXY f;
  if (c->g.shearbox && c->g.three_d && !(z_fill_is_planewise(c) && fill_xy_plan(c, 0.0, 0.0, &f))) return do_make_boundaries(c, out, RGPU_YDIR);
  return 0;   // (fused post_a: the z ghost planes are copies of complete planes, the last Y pass has nothing left to do)
}

// In-plane part of the ghost fill of the step's OUTPUT state, restricted to planes [a,b) (and [a2,b2)): what a z-slab driver applies
// to the planes it is about to send, so that the neighbour receives finished planes (x / y ghosts and corners
// included) and never has to touch its z ghost planes again.  x and y fills (and the shear remap) act within one
// z plane, hence plane-wise { Y, shear, Y } + copying planes equals the reference's { Y, shear, Z, Y } sequence.
int step_fill_planes(rgpu_ctx* c, int nStep, double dt_arg, double t_arg, int a, int b, int a2 = 0, int b2 = 0) {
  const StepTime st = step_time(c, dt_arg, t_arg);
  if (st.skip) return 0;
  const double dt = st.dt, totalTime = st.t;
  Phase ph(c, RGPU_T_BOUNDARIES);
  double* out = c->U[(nStep + 1) % 2];
  FillXY f;
  if (fill_xy_plan(c, totalTime, dt, &f)) return launch_fill_xy(c, out, f, a, b, a2, b2);
  for (int n = 0; n < 2; ++n) {
    const int lo = n ? a2 : a, hi = n ? b2 : b;
    if (hi <= lo) continue;
    if (c->g.rot && c->g.shearbox) {
      if (do_make_boundaries(c, out, RGPU_YDIR, lo, hi) || do_make_boundaries_shear(c, out, totalTime, dt, lo, hi) ||
          do_make_boundaries(c, out, RGPU_YDIR, lo, hi)) return -1;
    } else if (do_make_boundaries(c, out, RGPU_XDIR, lo, hi) || do_make_boundaries(c, out, RGPU_YDIR, lo, hi)) return -1;
  }
  return 0;
}

// The full ghost fill of a state from outside the step kernels: { Y, shear, Z, Y } for the 3D shearing box, { X, Y, [Z] } otherwise
int fill_all_ghosts(rgpu_ctx* c, double* U, double totalTime, double dt) {
  if (c->g.shearbox && c->g.three_d)
    return do_make_boundaries(c, U, RGPU_YDIR) || do_make_boundaries_shear(c, U, totalTime, dt) ||
           do_make_boundaries(c, U, RGPU_ZDIR) || do_make_boundaries(c, U, RGPU_YDIR);
  return do_make_boundaries(c, U, RGPU_XDIR) || do_make_boundaries(c, U, RGPU_YDIR) || (c->g.three_d && do_make_boundaries(c, U, RGPU_ZDIR));
}

// ---- plane-range helpers -----------------------------------------------------------------------------------------
// Every kernel body works on a flat cell index and guards its own (i,j,k) validity, so a stage can be run on any
// range of z planes.  The step is expressed as "complete the UPDATE of planes [a,b)"; each stage then has to cover
//   update [a,b) <- flux/emf [a,b+1) <- trace [a-1,b+1) <- elec [a-1,b+2), prim [a-2,b+2)      (3D MHD)
//   update [a,b) <- flux [a,b+1) <- trace [a-1,b+1) <- prim [a-2,b+2)                           (hydro)
// clipped to the array.  Values are deterministic functions of the (unchanging) input state, so computing a plane
// twice in two calls is harmless; a z-slab driver uses this to update the planes that do not depend on the
// neighbours' ghost planes while the halo exchange is still in flight.
struct PlaneRange { int lo, hi; };
inline PlaneRange clip(int lo, int hi, int ksize) {
  PlaneRange r = {lo < 0 ? 0 : lo, hi > ksize ? ksize : hi};
  if (r.hi < r.lo) r.hi = r.lo;
  return r;
}
template <int BLOCK, int MINW, class K>
int launch_planes(rg_stream_t s, const DevParams& g, PlaneRange r, const K& k) {
  if (r.hi <= r.lo) return 0;
  return rg_launch_planes<BLOCK, MINW>(s, (unsigned)r.lo * g.sk, g.sk, (unsigned)(r.hi - r.lo), k, (unsigned)g.xcd_sub);
}

// ---- what the kernel that writes the new state carries along ---------------------------------------------------------------
// The CFL scan of the new state rides in that kernel when nothing modifies the state afterwards (no dissipative stage, no forcing)
// and the next compute_dt reads exactly what the kernel wrote.  One function per step family: how many slots of d_red the kernel
// fills (0: the scan is left to compute_dt).  They depend on the context's configuration alone; slabs of one run may answer
// differently (the slab driver agrees on the minimum once, at rgpu_comm_create, through rgpu_inv_dt_fusable).
bool no_later_write(const rgpu_params& p, bool mhd) { return !(p.nu > 0) && !(mhd && p.eta > 0) && !p.randomForcingEnabled && !p.ouForcingEnabled; }
bool periodic_xy(const rgpu_params& p) { return p.bc[0] == RGPU_BC_PERIODIC && p.bc[1] == RGPU_BC_PERIODIC && p.bc[2] == RGPU_BC_PERIODIC && p.bc[3] == RGPU_BC_PERIODIC; }
// hydro 3D, the LDS-tiled sweep: whole-domain steps, and slab pieces (RGPU_CORE_SCAN) accumulating into the same slot
int hydro3d_sweep_scan(const rgpu_ctx* c) { return no_later_write(c->p, false) && rgpu_tiled::hydro3d_sweep_covers(c->g) && c->g.grav_on != 2 ? 1 : 0; }
// hydro 2D (fused step or flat update) and the flat 3D update (RGPU_TILED=0, per-cell gravity field): whole-domain steps
int hydro_flat_scan(const rgpu_ctx* c) { return no_later_write(c->p, false) ? RG_DT_SLOTS : 0; }
// 2D MHD (fused step or flat update): the plain path only.  On the rotating path the reference refills the ghosts before it scans, and
// no face type makes the refilled Bx on the high x face the value the CT update left there: the emf carries xPos (the shear terms), so
// even the periodic image, one box length away, differs (a last-column cell that sets the time step showed it:
// tests/test_cfl_plant_emu.py, orszag-tang with MHD.omega0)
int mhd2d_scan(const rgpu_ctx* c) { return c->g.grav_on != 2 && no_later_write(c->p, true) && !c->g.rot ? RG_DT_SLOTS : 0; }
// 3D MHD slab pieces (RGPU_CORE_SCAN): the field on the three high faces keeps its CT value -- always on the plain path (the reference
// scans before the ghosts are refilled); on the rotating path when y, z are periodic (bit-identical copies) and x is the shearing box
// (its fill skips the first outer Bx face).  Not with periodic x faces: the emf of the high x face carries another xPos than its image's.
// A z face shared with a neighbour slab (RGPU_BC_COPY) counts as periodic.
int mhd3d_pieces_scan(const rgpu_ctx* c) {
  const auto& bc = c->p.bc;
  auto zok = [](int b) { return b == RGPU_BC_PERIODIC || b == RGPU_BC_COPY; };
  const bool rot_ok = bc[0] == RGPU_BC_SHEARINGBOX && bc[1] == RGPU_BC_SHEARINGBOX && bc[2] == RGPU_BC_PERIODIC &&
                      bc[3] == RGPU_BC_PERIODIC && zok(bc[4]) && zok(bc[5]);
  return c->g.grav_on != 2 && no_later_write(c->p, true) && (!c->g.rot || rot_ok) ? RG_DT_SLOTS : 0;
}
// 3D MHD whole domain: as the pieces, but the whole-slab step of a rotating slab leaves the scan to the driver
int mhd3d_scan(const rgpu_ctx* c) { return c->g.rot && (c->p.bc[4] == RGPU_BC_COPY || c->p.bc[5] == RGPU_BC_COPY) ? 0 : mhd3d_pieces_scan(c); }
// The 2D fused kernels write the ghost images of their output too when they scan it, the faces are plain and there is no jet (the
// next step_pre skips its fill).  Hydro: Dirichlet, Neumann or periodic faces (the kernel's mask of face types, 0: no images);
// MHD: periodic faces, not on the rotating frame.
int hydro2d_images(const rgpu_ctx* c) {
  if (!rgpu::options().ghost_images || !hydro_flat_scan(c) || c->p.enableJet || c->g.nx < c->g.gw || c->g.ny < c->g.gw) return 0;
  int images = 1 << 12;
  for (int f = 0; f < 4; ++f) {
    const int bc = c->p.bc[f];
    if (bc != RGPU_BC_DIRICHLET && bc != RGPU_BC_NEUMANN && bc != RGPU_BC_PERIODIC) return 0;
    images |= bc << (2 * f);
  }
  return images;
}
bool mhd2d_images(const rgpu_ctx* c) {
  return rgpu::options().ghost_images && !c->g.rot && mhd2d_scan(c) && !c->p.enableJet && c->g.nx >= c->g.gw && c->g.ny >= c->g.gw && periodic_xy(c->p);
}
// zero the slots a fused scan is about to fill -- unless a clock kernel of this step already did
int zero_scan_slots(rgpu_ctx* c) { return c->clk_cur ? 0 : rg_memset_async(c->d_red, 0, RG_DT_SLOTS * sizeof(unsigned long long), c->stream); }

// What ONE call of a core does about the fused scan of the state U[parity] it writes, given how many slots its kernel family fills
// (`family_slots`, a policy function above; 0: it cannot scan) and the RGPU_CORE_* flags of the call:
//   whole step (no FLUXES / UPDATE flag, all planes)   the slots are zeroed, the kernel fills them, success records scanned(parity, n)
//   RGPU_CORE_FLUXES | RGPU_CORE_SCAN                  the slots are zeroed and armed for the pieces that follow; a family that cannot
//                                                      scan disarms
//   RGPU_CORE_UPDATE | RGPU_CORE_SCAN                  the kernel accumulates into the slots while they are armed for this parity, else
//                                                      the call disarms (the slab driver commits the pieces: StateRecord::commit)
//   anything else                                      no scan, the record is left alone
// begin() goes before the launch (again before a second kernel that takes over from one that answered "not covered": the slots are
// zeroed again), slots() is what the kernel gets, done() follows a launch that succeeded and ran.
class ScanPlan {
  enum Role { kNone, kWhole, kArm, kPiece, kLostPiece };   // kLostPiece: an UPDATE | SCAN piece that cannot accumulate
  rgpu_ctx* c_; int n_, par_; Role role_;
 public:
  ScanPlan(rgpu_ctx* c, int family_slots, bool whole, int flags, int parity) : c_(c), n_(family_slots), par_(parity) {
    const int what = flags & ~RGPU_CORE_SCAN;
    if (what == 0) role_ = whole && n_ ? kWhole : kNone;
    else if (!(flags & RGPU_CORE_SCAN)) role_ = kNone;
    else role_ = what == RGPU_CORE_FLUXES ? kArm : n_ && c->rec.armed(par_) ? kPiece : kLostPiece;
  }
  unsigned long long* slots() const { return (role_ == kWhole || role_ == kPiece) ? c_->d_red : 0; }
  int begin() {   // != 0: failed
    if (role_ == kArm || role_ == kLostPiece) c_->rec.disarm();
    if ((role_ == kWhole || (role_ == kArm && n_)) && zero_scan_slots(c_)) return -1;
    if (role_ == kArm && n_) c_->rec.arm(par_);
    return 0;
  }
  void done() { if (role_ == kWhole) c_->rec.scanned(par_, n_); }
  void not_covered() { if (role_ == kPiece) c_->rec.disarm(); }   // other kernels take over: no accumulated scan for this step
};

}  // namespace
