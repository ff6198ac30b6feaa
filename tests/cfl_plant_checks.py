"""The CFL scan that rides in the step kernels, pinned by planting the fastest cell of the box where a kernel could lose it: checks
shared by the CPU emulation tests (tests/test_cfl_plant_emu.py) and the GPU ones (tests/test_cfl_plant_gpu.py).

Every kernel that writes a new state leaves the maximum of sum_d (c + |v_d|) / delta_d over its cells in RG_DT_SLOTS device slots, and
the next compute_dt only reads them back.  A reduction shows nothing but its maximum: a wrong term, mask or slot in one cell is
invisible unless that cell is the fastest of the box.  So the state here is a uniform background at rest with ONE fast cell, and the
cell is put on every face, corner line, tile seam, partial last tile and z-segment seam in turn.

  planted_state       rho = 1, p = 1, v = 0, face field (0.3, 0.2, 0.1); the planted cell carries p = 5 and |v| = 4 along a direction
                      tangential to the face it lies on, so that the pulse stays in the outermost layer
  planted_reference   the oracle's two steps from that state, with the generator's proof: in the oracle's state after step 1 -- the
                      state whose scan gives the second dt, which is asserted -- replacing the target set (the cell and its neighbours
                      along the listed directions) by a far background cell drops the oracle's 1/dt to <= MASK_CAP of its value.
                      A plant that has gone soft fails as PlantError, not as a pass
  check_planted_dt    a library's two dts == the oracle's; the value the step left behind == a fresh scan of the same state == the
                      oracle's scan; which of the two paths (fused slots or scan kernel) the second dt took is asserted against
                      expect_fused, the rules of csrc/api/step.h; run_steps(2) on a fresh context ends at the same time (the device
                      clock folds the slots itself)

Cells are (ix, iy, iz) in interior coordinates.  A Plant is (name, cell, v, axes): v = (axis, sign) of the velocity, axes the directions
along which the cell's two neighbours belong to the target set."""
import collections

import numpy as np

import ensemble_checks as ec
import parity_checks as pc
from conftest import ini
from ramsesgpu_amd.ensemble import Ensemble
from ramsesgpu_amd.solver import Solver, interior

MASK_CAP = 0.8          # the oracle's 1/dt with the target set masked, over its unmasked value
DT_RTOL = 1e-11         # the contracted library's dt against the oracle's (parity_checks.check_run_vs_oracle)
X, Y, Z = 0, 1, 2
PERIODIC, SHEARINGBOX = 3, 4     # RGPU_BC_PERIODIC, RGPU_BC_SHEARINGBOX (include/rgpu.h)

Plant = collections.namedtuple("Plant", "name cell v axes")


class PlantError(AssertionError):
    """the generator's own claim does not hold (the planted cell is not what sets the time step): never a pass"""


# every masking ratio measured in this process: (case, plant name, ratio)
RATIOS = []


def bc_ov(xmin, xmax, ymin, ymax, zmin=None, zmax=None):
    ov = "mesh.boundary_xmin=%d;mesh.boundary_xmax=%d;mesh.boundary_ymin=%d;mesh.boundary_ymax=%d" % (xmin, xmax, ymin, ymax)
    if zmin is not None:
        ov += ";mesh.boundary_zmin=%d;mesh.boundary_zmax=%d" % (zmin, zmax)
    return ov


REFLECT2 = bc_ov(1, 1, 1, 1)
OUTFLOW2 = bc_ov(2, 2, 2, 2)
PERIODIC2 = bc_ov(3, 3, 3, 3)
REFLECT3 = bc_ov(1, 1, 1, 1, 1, 1)
OUTFLOW3 = bc_ov(2, 2, 2, 2, 2, 2)
PERIODIC3 = bc_ov(3, 3, 3, 3, 3, 3)
OPEN_Z = "mesh.boundary_zmin=2;mesh.boundary_zmax=2"


# ---- which path the second dt takes: the rules of csrc/api/step.h (hydro_flat_scan, hydro3d_sweep_scan, mhd2d_scan, mhd3d_scan),
# the `scan` column of parity_checks.FUSED_BOOKKEEPING (test_expect_fused_agrees_with_the_bookkeeping_table) -----------------------
def expect_fused(p):
    """does a whole-box step of this configuration leave the CFL scan of its output in the device slots"""
    mhd = bool(p.mhdEnabled)
    if p.nu > 0 or (mhd and p.eta > 0) or p.randomForcingEnabled or p.ouForcingEnabled:
        return False                     # a later stage rewrites the state
    if not mhd:
        return True
    if p.gravityEnabled == 2:
        return False
    if not p.Omega0 > 0:
        return True                      # plain path: the reference scans before the ghosts are refilled
    # rotating path: the reference scans the refilled ghosts.  Only the shearing box keeps the CT value of Bx on the high x face (a
    # periodic image lies one box length away, and the emf carries xPos), and only periodic y / z images are bit-identical copies
    bc = list(p.bc)
    return bool(p.three_d) and bc[0] == SHEARINGBOX and bc[1] == SHEARINGBOX and all(b == PERIODIC for b in bc[2:6])


# ---- where to plant ----------------------------------------------------------------------------------------------------------------
def tile_shape(p):
    """(cells per tile in x, in y, the seam pairs of the first tile in x, in y, cells the tiles cover beyond nx / ny) of the step
    family's tiled kernel (the header of tests/test_stress_states.py)"""
    if not p.mhdEnabled:
        return 16, 16, (15, 16), (15, 16), 0
    if p.three_d:
        return 16, 8, (15, 16), (7, 8), 1        # face columns gw .. nx + gw: nx + 1 of them
    return 15, 7, (14, 15), (6, 7), 1            # 15 x 7 finished cells of 16 x 8; nx + 1 by ny + 1 cells to finish


def _inward(i, n):
    return 1 if i < n // 2 else -1


def plants(p, groups=("low", "high", "seams"), zseam=None):
    """the Plants of a box: low / high = the faces and the corner line of that side, seams = the first tile's seams, the first cell of
    a partial last tile and (zseam = z) the planes z - 1 and z.  Names are stable ids"""
    nx, ny, nz = p.nx, p.ny, (p.nz if p.three_d else 1)
    three = bool(p.three_d)
    mx, my, mz = nx // 2, ny // 2, (nz // 2 if three else 0)
    has_w = p.nbVar >= 5
    tang_z = (Z,) if three else ()
    out = []
    for side in ("low", "high"):
        if side not in groups:
            continue
        ix, iy, iz = (0, 0, 0) if side == "low" else (nx - 1, ny - 1, nz - 1)
        out.append(Plant("x-" + side, (ix, my, mz), (Y, 1), (Y,) + tang_z))
        out.append(Plant("y-" + side, (mx, iy, mz), (X, 1), (X,) + tang_z))
        if three:
            out.append(Plant("z-" + side, (mx, my, iz), (X, 1), (X, Y)))
            out.append(Plant("edge-" + side, (ix, iy, mz), (Z, 1), ()))       # along the edge; the cell alone
        elif has_w:
            out.append(Plant("corner-" + side, (ix, iy, 0), (Z, 1), ()))      # out of the plane; the cell alone
        else:
            # 2D hydro has no z momentum: along x, inwards, in the outermost y layer
            out.append(Plant("corner-" + side, (ix, iy, 0), (X, _inward(ix, nx)), (X,)))
    if "seams" in groups:
        tx, ty, sx, sy, extra = tile_shape(p)
        # along the seam line where there is a z momentum (3D: along z; 2D MHD: out of the plane), else along x
        along = (Z, 1) if has_w else (X, 1)
        allax = (X, Y) + tang_z
        for i in sx:
            for j in sy:
                if i < nx and j < ny:
                    out.append(Plant("seam-%d-%d" % (i, j), (i, j, mz), along, allax))
        lx, ly = min(((nx + extra - 1) // tx) * tx, nx - 1), min(((ny + extra - 1) // ty) * ty, ny - 1)
        if lx > 0 and ly > 0:
            out.append(Plant("last-tile", (lx, ly, mz), along if has_w else (X, -1), allax))
        if zseam is not None:
            assert three and 0 < zseam < nz
            for k in (zseam - 1, zseam):
                out.append(Plant("zseam-%d" % k, (mx, my, k), (X, 1), allax))
    return out


def plant_named(p, name, zseam=None):
    for q in plants(p, zseam=zseam):
        if q.name == name:
            return q
    raise KeyError(name)


def _index(p, cell):
    gw = p.ghostWidth
    ix, iy, iz = cell
    return (iz + gw if p.three_d else 0, iy + gw, ix + gw)


def planted_state(p, plant):
    """the uniform background at rest with the planted cell: p = 5, |v| = 4 along plant.v.  Isothermal configurations ignore the
    pressure; the velocity alone plants the maximum"""
    nv, ks, js, is_ = p.shape
    rho = np.ones((ks, js, is_))
    pres = np.ones((ks, js, is_))
    vel = np.zeros((3, ks, js, is_))
    B = None
    if nv == 8:
        B = np.empty((3, ks, js, is_))
        B[0], B[1], B[2] = 0.3, 0.2, 0.1
    idx = _index(p, plant.cell)
    axis, sign = plant.v
    assert axis != Z or nv >= 5, plant
    pres[idx] = 5.0
    vel[(axis,) + idx] = 4.0 * sign
    return pc._assemble(p, rho, vel, pres, B)


def target_set(p, plant):
    """array indices of the planted cell and its two neighbours along each of plant.axes, inside the interior"""
    n = (p.nx, p.ny, p.nz if p.three_d else 1)
    cells = [tuple(plant.cell)]
    for ax in plant.axes:
        for s in (-1, 1):
            c = list(plant.cell)
            c[ax] += s
            if 0 <= c[ax] < n[ax]:
                cells.append(tuple(c))
    return [_index(p, c) for c in cells]


def far_cell(p, plant):
    n = (p.nx, p.ny, p.nz if p.three_d else 1)
    return _index(p, tuple((c + m // 2) % m for c, m in zip(plant.cell, n)))


def masking_ratio(oracle, p, U, cells, far):
    """the oracle's 1/dt of U with every variable of `cells` replaced by the cell `far`'s, over its 1/dt of U"""
    whole = oracle.compute_inv_dt(p, U)
    M = U.copy()
    for c in cells:
        M[(slice(None),) + c] = U[(slice(None),) + far]
    return oracle.compute_inv_dt(p, M) / whole


_REF = {}      # the last case's references (the exact and the contracted library ask for the same ones in a row), read-only


def planted_reference(lib, oracle, base, ov, plant, nsteps=2):
    """(p, U0, the oracle's dts, its state after the last step, its 1/dt of that state) with the generator's proofs.  The caller has
    handed the oracle the gravity / forcing fields of the case (attach_gravity)"""
    key = (base, ov, plant, nsteps)
    if key in _REF:
        return _REF[key]
    p = lib.params_from_ini(ini(base), ov)
    U0 = planted_state(p, plant)
    U1, d1, _ = oracle.run_sequential(p, U0, 1)
    U2, dts, _ = oracle.run_sequential(p, U0, nsteps)
    what = "%s [%s] planted at %s %r" % (base, ov, plant.name, plant.cell)
    if not (np.isfinite(U2).all() and len(dts) == nsteps and dts[0] == d1[0]):
        raise PlantError(what + ": the oracle's run is not finite")
    # the state that is masked is the one the reference scans for its second dt
    inv1 = oracle.compute_inv_dt(p, U1)
    if not p.cfl / inv1 == dts[1]:
        raise PlantError("%s: cfl / the oracle's scan of its state after step 1 = %r, its second dt %r" % (what, p.cfl / inv1, dts[1]))
    ratio = masking_ratio(oracle, p, U1, target_set(p, plant), far_cell(p, plant))
    RATIOS.append((base + "[" + ov + "]", plant.name, float(ratio)))
    print("planted CFL: %s: 1/dt with the target set masked / unmasked = %.3f" % (what, ratio))
    if not ratio <= MASK_CAP:
        raise PlantError("%s: masking the target set leaves %.3f of the oracle's 1/dt (cap %.2f): the planted cell does not set the time step"
                         % (what, ratio, MASK_CAP))
    U0.flags.writeable = False
    U2.flags.writeable = False
    if len(_REF) >= 64:
        _REF.clear()
    _REF[key] = (p, U0, [float(d) for d in dts], U2, oracle.compute_inv_dt(p, U2))
    return _REF[key]


def _close(a, b):
    return abs(a / b - 1.0) < DT_RTOL


def _left_behind(lib, sv, par):
    """(1/dt the next compute_dt returns, 1/dt of a fresh scan, did the first come from the slots the step's kernel filled)"""
    if "emulation" in lib.backend:
        # a fast cell written behind the library's back: a scan sees it, a value read back from the slots does not
        U = pc._host_state(lib, sv, par)
        gw = sv.p.ghostWidth
        cell = (gw if sv.p.three_d else 0, gw, gw)
        saved = U[2][cell]
        U[2][cell] = 1e4 * U[0][cell]
        first = sv.compute_inv_dt(par)
        assert lib.lib.rgpu_invalidate_dt(sv.ctx) == 0
        seen = sv.compute_inv_dt(par)
        U[2][cell] = saved
        assert lib.lib.rgpu_invalidate_dt(sv.ctx) == 0
        fresh = sv.compute_inv_dt(par)
        assert seen > fresh, "the probe cell is not visible to a scan"
        fused = first != seen
        return (first if fused else fresh), fresh, fused
    sv.enable_timers(True)
    sv.reset_timers()
    first = sv.compute_inv_dt(par)
    fused = sv.timers()["dt"] == 0.0
    assert lib.lib.rgpu_invalidate_dt(sv.ctx) == 0
    sv.reset_timers()
    fresh = sv.compute_inv_dt(par)
    scanned = sv.timers()["dt"] > 0.0
    sv.enable_timers(False)
    assert scanned, "rgpu_invalidate_dt did not make compute_inv_dt scan"
    return first, fresh, fused


def check_planted_dt(lib, oracle, base, ov, cells, exact=True, zseam=None):
    """every Plant of `cells` in turn on one context (see the module's header).  Returns [(plant name, fused)]"""
    p = lib.params_from_ini(ini(base), ov)
    want_fused = expect_fused(p)
    out = []
    sv = Solver(p, lib)
    try:
        pc.attach_gravity(lib, base, ov, p, sv=sv, oracle=oracle)
        for plant in cells:
            what = "%s [%s] planted at %s %r, %s library" % (base, ov, plant.name, plant.cell, lib.arithmetic)
            _, U0, dts_ref, U2, inv_ref = planted_reference(lib, oracle, base, ov, plant)
            dts = [float(d) for d in sv.start(U0, 2)]
            par = sv.nStep % 2
            left, fresh, fused = _left_behind(lib, sv, par)
            print("planted CFL: %s: dts %r (oracle %r), 1/dt left %r fresh %r oracle %r, %s" % (what, dts, dts_ref, left, fresh, inv_ref, "fused" if fused else "scanned"))
            if exact:
                assert dts == dts_ref, "%s: dt sequence %r, the oracle's %r" % (what, dts, dts_ref)
                assert left == fresh, "%s: the step left 1/dt = %r, a fresh scan of the same state gives %r" % (what, left, fresh)
                assert fresh == inv_ref, "%s: 1/dt of the state after two steps %r, the oracle's %r" % (what, fresh, inv_ref)
            else:
                assert all(_close(a, b) for a, b in zip(dts, dts_ref)) and len(dts) == 2, "%s: dt sequence %r, the oracle's %r" % (what, dts, dts_ref)
                assert _close(left, fresh), "%s: the step left 1/dt = %r, a fresh scan of the same state gives %r" % (what, left, fresh)
                assert _close(fresh, inv_ref), "%s: 1/dt of the state after two steps %r, the oracle's %r" % (what, fresh, inv_ref)
            assert fused == want_fused, "%s: the value compute_dt returns after the step was %s, expected %s" % (
                what, "read back from the slots" if fused else "scanned", "a read-back" if want_fused else "a scan")
            t_end = sv.totalTime
            # the same two steps with the time step kept on the device where the step allows it
            sv2 = Solver(p, lib)
            try:
                pc.attach_gravity(lib, base, ov, p, sv=sv2)
                sv2.start(U0, 0)
                assert sv2.run_steps(2) == 2, what
                if exact:
                    assert sv2.totalTime == t_end and list(sv2.dt_log) == dts, "%s: run_steps(2) ends at %r with %r, start(U0, 2) at %r with %r" % (
                        what, sv2.totalTime, sv2.dt_log, t_end, dts)
                else:
                    assert _close(sv2.totalTime, t_end), "%s: run_steps(2) ends at %r, start(U0, 2) at %r" % (what, sv2.totalTime, t_end)
            finally:
                sv2.close()
            out.append((plant.name, fused))
    finally:
        sv.close()
        oracle.set_gravity_field(None)
        oracle.set_forcing_field(None)
    return out


def check_planted_case(lib, oracle, base, ov, group, exact=True, zseg=None):
    """check_planted_dt over one group of plants (plants()); zseg: the launch option "zseg" set to it (read at rgpu_create) and
    restored, with the planes zseg - 1 and zseg planted too"""
    p = lib.params_from_ini(ini(base), ov)
    if zseg is None:
        return check_planted_dt(lib, oracle, base, ov, plants(p, (group,)), exact)
    cells = [q for q in plants(p, (group,), zseam=zseg) if q.name.startswith("zseam") or group != "seams"]
    old = lib.set_option("zseg", zseg)
    try:
        return check_planted_dt(lib, oracle, base, ov, cells, exact)
    finally:
        lib.set_option("zseg", old)


GROUPS = ("low", "high", "seams")


def case_ids(cases):
    return ["%s[%s]-%s" % (b, o, g) for b, o, g in cases]


def grouped(shapes, groups=GROUPS):
    return [(s[0], s[1], g) for s in shapes for g in groups]


# ---- shapes ------------------------------------------------------------------------------------------------------------------------
# the small boxes of the emulation file: every step family over periodic, reflecting and outflow faces, the shearing box, the rotating
# periodic box, and configurations that do not fuse (the flat scan kernel is what they test)
EMU_SHAPES = [
    ("implode3d", "mesh.nx=40;mesh.ny=24;mesh.nz=1;hydro.riemannSolver=hllc"),                   # 2D hydro, reflecting
    ("implode3d", "mesh.nx=40;mesh.ny=24;mesh.nz=1;" + OUTFLOW2),
    ("kelvin_helmholtz_gpu_2d", "mesh.nx=40;mesh.ny=24"),                                        # 2D hydro, periodic
    ("kelvin_helmholtz_gpu_2d", "mesh.nx=40;mesh.ny=24;hydro.nu=0.01"),                          # not fused: viscous stage
    ("Keplerian_disk2d", "mesh.nx=40;mesh.ny=24"),                                               # per-cell gravity field (fused in hydro)
    ("mhd_BrioWu", "mesh.nx=40;mesh.ny=24"),                                                     # 2D MHD, outflow
    ("orszag-tang", "mesh.nx=40;mesh.ny=24;" + REFLECT2),
    ("orszag-tang", "mesh.nx=40;mesh.ny=24"),                                                    # periodic
    ("orszag-tang", "mesh.nx=40;mesh.ny=24;MHD.omega0=0.4"),                                     # rotating, periodic: not fused
    ("orszag-tang", "mesh.nx=40;mesh.ny=24;MHD.omega0=0.4;" + OUTFLOW2),                         # rotating, open: not fused
    ("orszag-tang", "mesh.nx=40;mesh.ny=24;MHD.eta=0.01"),                                       # not fused: resistive stage
    ("implode3d", "mesh.nx=20;mesh.ny=18;mesh.nz=10;hydro.riemannSolver=hllc"),                  # 3D hydro, reflecting
    ("implode3d", "mesh.nx=20;mesh.ny=18;mesh.nz=10;" + OUTFLOW3),
    ("implode3d", "mesh.nx=20;mesh.ny=18;mesh.nz=10;" + PERIODIC3),
    ("orszag-tang3d", "mesh.nx=20;mesh.ny=18;mesh.nz=10"),                                       # 3D MHD, periodic
    ("orszag-tang3d", "mesh.nx=20;mesh.ny=18;mesh.nz=10;" + REFLECT3),
    ("orszag-tang3d", "mesh.nx=20;mesh.ny=18;mesh.nz=10;" + OUTFLOW3),
    ("orszag-tang3d", "mesh.nx=20;mesh.ny=18;mesh.nz=10;MHD.omega0=0.3"),                        # rotating periodic box: not fused
    ("mhd_mri_3d", "mesh.nx=20;mesh.ny=18;mesh.nz=10"),                                          # shearing box
    ("mhd_mri_3d", "mesh.nx=20;mesh.ny=18;mesh.nz=10;" + OPEN_Z),                                # shearing box, open z: not fused
    ("mhd_mri_3d", "mesh.nx=20;mesh.ny=18;mesh.nz=10;gravity.static=yes"),                       # per-cell gravity field: not fused
    ("orszag-tang3d", "mesh.nx=20;mesh.ny=18;mesh.nz=10;hydro.nu=0.005"),                        # not fused: viscous stage
]

# more slots than RG_DT_SLOTS: 2D MHD with more than 512 tiles, 2D hydro with more than 256; both more than 65536 cells, which wraps
# the flat kernels' (idx >> 6) & 1023.  Planted in the first and in the last tile
WRAP_SHAPES = [
    ("orszag-tang", "mesh.nx=480;mesh.ny=126"),              # 33 x 18 = 594 tiles of 15 x 7; 486 x 132 = 64152 cells with ghosts
    ("kelvin_helmholtz_gpu_2d", "mesh.nx=272;mesh.ny=256"),  # 17 x 16 = 272 tiles of 16 x 16; more than 65536 cells
]
# ... and a 2D MHD box of more than 65536 cells for the flat update (the 594-tile one stays just below)
WRAP_SHAPES_FLAT = WRAP_SHAPES + [("orszag-tang", "mesh.nx=480;mesh.ny=140")]


def wrap_tiles(p):
    tx, ty, _, _, extra = tile_shape(p)
    return -(-(p.nx + extra) // tx) * -(-(p.ny + extra) // ty)


def wrap_plants(p):
    """the low and high corner lines (first and last tile) and the cells beside them"""
    return [q for q in plants(p, ("low", "high")) if q.name.startswith("corner")] + [
        Plant("first-tile", (1, 1, 0), (X, 1), (X, Y)), Plant("last-tile-inner", (p.nx - 2, p.ny - 2, 0), (X, -1), (X, Y))]


# ---- ensembles: a different planted cell per member --------------------------------------------------------------------------------
ENSEMBLE_SHAPES = [
    ("kelvin_helmholtz_gpu_2d", "mesh.nx=40;mesh.ny=24"),       # 2D hydro: 3 x 2 tiles of 16 x 16
    ("orszag-tang", "mesh.nx=46;mesh.ny=23"),                   # 2D MHD: partial last tiles in x and y
]
ENSEMBLE_STEPS = 3
SCAN_SETS = ["hydro.cfl=0.3;hydro.gamma0=1.8", "hydro.cfl=0.45;hydro.gamma0=1.3", "hydro.cfl=0.2;hydro.gamma0=1.55", "hydro.cfl=0.4;hydro.gamma0=1.4"]


def ensemble_plants(p):
    """low corner, high corner, a seam, mid-box"""
    tx, ty, sx, sy, _ = tile_shape(p)
    along = (Z, 1) if p.nbVar >= 5 else (X, 1)
    return [plant_named(p, "corner-low"), plant_named(p, "corner-high"), plant_named(p, "seam-%d-%d" % (sx[1], sy[0])),
            Plant("mid", (p.nx // 2, p.ny // 2, 0), along, (X, Y))]


def _proven_states(lib, oracle, base, ovs, ps, cells):
    """member m's planted state under ITS parameter set, each with the generator's proof"""
    return [np.array(planted_reference(lib, oracle, base, ovs[m], cells[m])[1]) for m in range(len(cells))]


def check_planted_ensemble(lib, oracle, base, ov, exact=True):
    """4 members, each with another planted cell: dt sequence and final state of every member over ENSEMBLE_STEPS steps == a lone
    context's == the oracle's (ensemble_checks.check_ensemble)"""
    p = lib.params_from_ini(ini(base), ov)
    cells = ensemble_plants(p)
    states = _proven_states(lib, oracle, base, [ov] * len(cells), [p] * len(cells), cells)
    done, stop, fused = ec.check_ensemble(lib, oracle, base, ov, len(cells), ENSEMBLE_STEPS, exact=exact, states=states)
    assert done == [ENSEMBLE_STEPS] * len(cells) and stop == [0] * len(cells)
    return fused


def check_planted_scan(lib, oracle, base, ov, exact=True):
    """a parameter scan (another cfl and gamma0 per member), each member with another planted cell: every member == a lone context
    created from its set == the oracle's run with its set"""
    ovs = [ov + ";" + s for s in SCAN_SETS]
    ps = [lib.params_from_ini(ini(base), o) for o in ovs]
    cells = ensemble_plants(ps[0])
    states = _proven_states(lib, oracle, base, ovs, ps, cells)
    refs = [oracle.run_sequential(ps[m], states[m], ENSEMBLE_STEPS) for m in range(len(ps))]
    assert len({float(r[1][0]) for r in refs}) == len(ps), "the parameter sets do not tell the members apart"
    ens = Ensemble.scan(ps, lib)
    try:
        ens.start(states)
        done, stop, fused = ens.run_steps(ENSEMBLE_STEPS)
        for m in range(len(ps)):
            want = ec.lone_run(lib, ps[m], states[m], ENSEMBLE_STEPS)
            ec.assert_member(ens.member(m), done[m], want, "planted scan %s[%s] member %d" % (base, ovs[m], m), exact, refs[m])
        assert list(stop) == [0] * len(ps)
    finally:
        ens.close()
    return fused


# ---- slab pieces: the world-1 schedule of tests/slab_harness.py from a planted state ----------------------------------------------
SLAB_SHAPES = [
    ("implode3d", "mesh.nx=20;mesh.ny=18;mesh.nz=40;hydro.riemannSolver=hllc"),
    ("orszag-tang3d", "mesh.nx=20;mesh.ny=18;mesh.nz=40"),
]


def slab_plants(p):
    """iz = 0 and nz - 1, the first and last plane of the interior piece (array planes [2 gw, nz): iz = gw and nz - gw - 1), mid-box"""
    gw, nz = p.ghostWidth, p.nz
    mx, my = p.nx // 2, p.ny // 2
    allax = (X, Y, Z)
    return [Plant("z-low", (mx, my, 0), (X, 1), (X, Y)), Plant("z-high", (mx, my, nz - 1), (X, 1), (X, Y)),
            Plant("inner-first", (mx, my, gw), (X, 1), allax), Plant("inner-last", (mx, my, nz - gw - 1), (X, 1), allax),
            Plant("mid", (mx, my, nz // 2), (X, 1), allax)]


def check_planted_slab(lib, oracle, base, ov, overlap):
    """SlabRun's two steps from each planted state: dts == oracle.run_sequential's, the state too"""
    import torch
    from slab_harness import SlabRun
    p = lib.params_from_ini(ini(base), ov)
    for plant in slab_plants(p):
        _, U0, dts_ref, U2, _ = planted_reference(lib, oracle, base, ov, plant)
        run = SlabRun(ini(base), ov, library=lib, device="cuda:0", overlap=overlap, initial_state=U0)
        try:
            run.init_simulation()
            dts = [run.oneStepIntegration() for _ in range(2)]
            torch.cuda.synchronize()
            got = run.local_interior().cpu().numpy()
        finally:
            run.close()
        what = "slab schedule (%s) %s [%s] planted at %s %r" % ("overlap" if overlap else "serial", base, ov, plant.name, plant.cell)
        assert dts == dts_ref, "%s: dt sequence %r, the oracle's %r" % (what, dts, dts_ref)
        pc.assert_same(got, interior(U2, p), what)
