"""The operator-split viscous / resistive stage (csrc/kernels_dissipative.h, launcher dissipative_nd in csrc/api/step_core.h) on rough states:
checks shared by the CPU emulation tests (tests/test_dissipative_emu.py) and the GPU ones (tests/test_dissipative_gpu.py).

  ROUGH_RUNS    three steps from a random state on ONE context, the stage behind shapes that cross tile seams, use the MhLastX column,
                z-segment starts and partial last tiles (the shapes of tests/test_stress_states.py): steps 2 and 3 run on scratch arrays
                the earlier steps have used (the resistive CT update reads the emf one cell beyond what the emf kernel writes and
                relies on that strip of its scratch being zero)
  STAGE_ALONE   rgpu_step_dissipative alone against the oracle's stage (orc_dissipative_stage) on the same ghost-filled array, at a
                diffusion number of 0.1, and two properties that need no second implementation of the arithmetic: the resistive CT
                update keeps the discrete div B, the flux form keeps the totals of a periodic box.

The device kernels and the oracle's stage are the same direction-generic restatement written twice, so kernel-vs-oracle equality
cannot see an error they share; the fixtures written by the reference itself (oracle/gen_golden.py, the *_visc* / *_res* cases) and
the two properties are what stands against that."""
import math

import numpy as np

import parity_checks as pc
from conftest import ini
from ramsesgpu_amd.solver import Solver, interior
from test_ensemble_gpu import MIXED_FACES

V = "hydro.nu=0.01"
R = "MHD.eta=0.02"
OPEN = "mesh.boundary_xmin=2;mesh.boundary_xmax=2;mesh.boundary_ymin=1;mesh.boundary_ymax=2;mesh.boundary_zmin=1;mesh.boundary_zmax=1"
MIXED = MIXED_FACES    # reflecting / outflow / periodic faces mixed


def _ov(*parts):
    return ";".join(parts)


ROUGH_RUNS = [
    # ---- 3D MHD sweep + resistive / viscous stage ----
    ("orszag-tang3d", _ov("mesh.nx=33;mesh.ny=17;mesh.nz=20", V, R)),                     # partial x / y tiles, up to 2 z segments
    ("orszag-tang3d", _ov("mesh.nx=32;mesh.ny=24;mesh.nz=14", V, R, "hydro.cIso=0.9")),   # periodic layers copied; isothermal: no energy flux
    ("orszag-tang3d", _ov("mesh.nx=32;mesh.ny=32;mesh.nz=12", R, OPEN)),                  # MhLastX, a one-row last tile, non-periodic faces under the resistive ranges
    ("mhd_mri_3d", _ov("mesh.nx=48;mesh.ny=40;mesh.nz=12;MHD.omega0=0.3", V, R)),         # shearing box: the shear remap runs before the stage
    ("mhd_mri_3d", _ov("mesh.nx=12;mesh.ny=10;mesh.nz=9;MHD.omega0=0.3;gravity.static=yes", V, R)),   # flat 3D kernels: T holds trace data
    # ---- 2D MHD step ----
    ("orszag-tang", _ov("mesh.nx=46;mesh.ny=23", V, R)),
    ("orszag-tang", _ov("mesh.nx=36;mesh.ny=29", V, R, "MHD.omega0=0.4")),                # the 2D rotating call site
    ("mhd_BrioWu", _ov("mesh.nx=32;mesh.ny=17", V, R, "mesh.boundary_xmin=1")),           # flat 2D kernels
    ("mhd_BrioWu", _ov("mesh.nx=32;mesh.ny=17", R)),                                      # tiled, Neumann faces
    # ---- 3D hydro sweep ----
    ("implode3d", _ov("mesh.nx=33;mesh.ny=17;mesh.nz=30", V, "hydro.riemannSolver=hllc")),
    ("implode3d", _ov("mesh.nx=20;mesh.ny=36;mesh.nz=14", V, "hydro.riemannSolver=hll;mesh.boundary_xmin=3;mesh.boundary_xmax=3;mesh.boundary_ymin=2")),
    # ---- 2D hydro step: the stage rewrites the interior after the kernel wrote the output's ghost images ----
    ("blast2d", _ov("mesh.nx=37;mesh.ny=29", V, MIXED)),
    ("kelvin_helmholtz_gpu_2d", _ov("mesh.nx=40;mesh.ny=24", V)),
    ("hydro_sod2d", _ov("mesh.nx=70;mesh.ny=50", V)),
]
ROUGH_IDS = ["%s[%s]" % c for c in ROUGH_RUNS]
ROUGH_STEPS = 3
NON_VACUITY = 1e-4    # relative L2 by which the run with the stage must differ from the run without, in at least one variable

_ROUGH_CACHE = {}


def var_names(p):
    return pc.OT_VARS if p.nbVar == 8 else ("density", "energy", "mx", "my", "mz")[:p.nbVar]


def rough_reference(lib, oracle, base, ov):
    """(p, U0, oracle's state after ROUGH_STEPS steps, its dts, filled U0, oracle's first step) of one ROUGH_RUNS case, with the
    non-vacuity assertion: the same run with nu = eta = 0 differs by a relative L2 >= NON_VACUITY in at least one variable.  The last
    case is kept (the exact and the contracted library ask for the same one in a row) and handed out read-only"""
    key = (base, ov)
    if key in _ROUGH_CACHE:
        return _ROUGH_CACHE[key]
    p = lib.params_from_ini(ini(base), ov)
    assert p.nu > 0 or (p.mhdEnabled and p.eta > 0), (base, ov)
    U0 = pc.random_state(p, seed=5, mach=1.0)
    pc.attach_gravity(lib, base, ov, p, oracle=oracle)
    try:
        ref, dts, _ = oracle.run(p, U0, ROUGH_STEPS)
        assert np.isfinite(ref).all() and len(dts) == ROUGH_STEPS, (base, ov)
        q = p.copy()
        q.nu = 0.0
        q.eta = 0.0
        plain, _, _ = oracle.run(q, U0, ROUGH_STEPS)
        moved = {n: float(pc.rel_l2(interior(ref, p)[v], interior(plain, p)[v])) for v, n in enumerate(var_names(p))}
        h2 = min(p.dx, p.dy, p.dz) ** 2 if p.three_d else min(p.dx, p.dy) ** 2
        D = max(p.nu, p.eta if p.mhdEnabled else 0.0) * np.asarray(dts) / h2
        print("dissipative stage on %s [%s]: diffusion number %.3f .. %.3f, moves the state by (relative L2) %s"
              % (base, ov, D.min(), D.max(), " ".join("%s %.1e" % kv for kv in moved.items())))
        assert max(moved.values()) >= NON_VACUITY, "%s [%s]: the stage moves no variable by %.0e: %s" % (base, ov, NON_VACUITY, moved)
        # the first step alone (the contracted library's comparison): ghosts filled as start() does, the run's first dt
        U = U0.copy()
        oracle.make_all_boundaries(p, U, 0.0, 0.0)
        first = oracle.godunov_unsplit(p, U.copy(), float(dts[0]), 0.0)
    finally:
        oracle.set_gravity_field(None)
        oracle.set_forcing_field(None)
    for a in (U0, ref, U, first):
        a.flags.writeable = False
    _ROUGH_CACHE.clear()
    _ROUGH_CACHE[key] = (p, U0, ref, [float(d) for d in dts], U, first)
    return _ROUGH_CACHE[key]


def first_difference(got, ref):
    """'(v, k, j, i) got ref' of the first differing double"""
    idx = tuple(int(x[0]) for x in np.nonzero(got != ref))
    return "%r: %r != %r" % (idx, got[idx], ref[idx])


def check_rough_run(lib, oracle, base, ov, exact=True):
    """exact: start(U0, 3) on one context == the oracle's run, every interior double and every dt.  Otherwise (contracted library): the
    first step through godunov_unsplit within parity_checks.assert_close_specific; returns its per-variable errors"""
    p, U0, ref, dts_ref, U, first = rough_reference(lib, oracle, base, ov)
    what = "%s [%s] with the dissipative stage, random state" % (base, ov)
    sv = Solver(p, lib)
    try:
        pc.attach_gravity(lib, base, ov, p, sv=sv)
        if exact:
            dts = sv.start(U0, ROUGH_STEPS)
            got = interior(sv.getDataHost(), p)
        else:
            sv.upload(U, both=True)
            sv.godunov_unsplit(0, dts_ref[0], 0.0)
            got = sv.getDataHost(1)
    finally:
        sv.close()
    if exact:
        want = interior(ref, p)
        assert np.isfinite(got).all(), what + ": non-finite values"
        nbad = int((got != want).sum())
        assert nbad == 0, "%s: %d of %d doubles differ after %d steps; first at %s" % (what, nbad, want.size, ROUGH_STEPS, first_difference(got, want))
        assert [float(d) for d in dts] == dts_ref, "%s: dt sequences differ: %r, the oracle's %r" % (what, dts, dts_ref)
        return None
    rho = pc._flux_partner_density(p, first[0])
    errs = pc.assert_close_specific(interior(got, p), interior(first, p), p, what + ", first step", rho=interior(rho[None], p)[0])
    if p.mhdEnabled and p.Omega0 > 0:
        pc.assert_close_specific(got, first, p, what + ", first step incl. ghosts")
    return errs


def record(what, errs):
    """print the contracted library's specific-form errors (pytest -s shows them)"""
    if errs is not None:
        print("contracted, specific-form relative L2: %s: %s" % (what, " ".join("%s %.2e" % kv for kv in errs.items())))


# ---- the stage alone ----------------------------------------------------------------------------------------------------------
STAGE_ALONE = [
    ("orszag-tang3d", _ov("mesh.nx=33;mesh.ny=17;mesh.nz=20", V, R)),       # 3D, periodic
    ("orszag-tang3d", _ov("mesh.nx=32;mesh.ny=32;mesh.nz=12", R, OPEN)),    # 3D, open / reflecting faces
    ("orszag-tang", _ov("mesh.nx=46;mesh.ny=23", V, R)),                    # 2D MHD, periodic
    ("blast2d", _ov("mesh.nx=37;mesh.ny=29", V, MIXED)),                    # 2D hydro, mixed faces
    # periodic boxes with the viscous stage alone: the conservation property with the energy (see totals_change)
    ("kelvin_helmholtz_gpu_2d", _ov("mesh.nx=40;mesh.ny=24", V)),
    ("orszag-tang3d", _ov("mesh.nx=33;mesh.ny=17;mesh.nz=20", V)),
]
STAGE_STATES = ("random", "contrast")
STAGE_CASES = [(b, o, s) for b, o in STAGE_ALONE for s in STAGE_STATES]
STAGE_IDS = ["%s[%s]-%s" % c for c in STAGE_CASES]
# a property applies where there is a resistive stage or every face is periodic (decided from the names so that collection needs no
# library; check_stage_properties asserts that one does)
PROPERTY_CASES = [c for c in STAGE_CASES if c[0] != "blast2d"]
PROPERTY_IDS = ["%s[%s]-%s" % c for c in PROPERTY_CASES]
STAGE_D = 0.1       # diffusion number max(nu, eta) dt / min(h)^2 of the stage-alone calls
STAGE_T0 = 2.0
EPS = float(np.finfo(np.float64).eps)

_STAGE_CACHE = {}


def stage_dt(p):
    h2 = min(p.dx, p.dy, p.dz) ** 2 if p.three_d else min(p.dx, p.dy) ** 2
    return STAGE_D * h2 / max(p.nu, p.eta if p.mhdEnabled else 0.0)


def stage_input(lib, oracle, base, ov, state):
    """(p, ghost-filled state, dt, the oracle's stage on it), kept for the last case, read-only"""
    key = (base, ov, state)
    if key not in _STAGE_CACHE:
        p = lib.params_from_ini(ini(base), ov)
        U = pc.random_state(p, seed=5, mach=1.0) if state == "random" else pc.stress_state(p, 5, state)
        dt = stage_dt(p)
        oracle.make_all_boundaries(p, U, STAGE_T0, dt)
        ref = oracle.dissipative_stage(p, U.copy(), dt, STAGE_T0)
        assert np.isfinite(ref).all(), (base, ov, state)
        assert not np.array_equal(interior(ref, p), interior(U, p))
        U.flags.writeable = False
        ref.flags.writeable = False
        _STAGE_CACHE.clear()
        _STAGE_CACHE[key] = (p, U, dt, ref)
    return _STAGE_CACHE[key]


def device_stage(lib, p, U, dt):
    """rgpu_step_dissipative(0, dt, t0) on a fresh context holding U in both parities: acts on U[1], no ghost fill"""
    sv = Solver(p, lib)
    try:
        sv.upload(U, both=True)
        sv.step_dissipative(0, dt, STAGE_T0)
        return sv.getDataHost(1)
    finally:
        sv.close()


def written_mask(p):
    """[nbVar][k][j][i] bool: the cells the reference's loops write -- the interior, plus for the field components the CT update touches
    (all three in 3D, Bx and By in 2D) the upper face layer i = nx + gw, j = ny + gw, k = nz + gw (its loops run to size - gw inclusive)"""
    gw = p.ghostWidth
    m = np.zeros(p.shape, bool)
    kint = slice(gw, -gw) if p.three_d else slice(None)
    m[:, kint, gw:-gw, gw:-gw] = True
    if p.mhdEnabled and p.eta > 0:
        kext = slice(gw, p.nz + gw + 1) if p.three_d else slice(None)
        m[5:(8 if p.three_d else 7), kext, gw:p.ny + gw + 1, gw:p.nx + gw + 1] = True
    return m


def check_stage_alone(lib, oracle, base, ov, state, exact=True):
    """the device's stage == the oracle's on the cells the reference writes (exact: equal bits; otherwise the project's specific-form
    tolerance), every other cell left as uploaded.  Returns the contracted library's errors"""
    p, U, dt, ref = stage_input(lib, oracle, base, ov, state)
    got = device_stage(lib, p, U, dt)
    what = "%s [%s] dissipative stage alone on the %s state" % (base, ov, state)
    m = written_mask(p)
    assert np.isfinite(got).all(), what + ": non-finite values"
    assert np.array_equal(got[~m], U[~m]), "%s: %d cells outside the reference's loop ranges were written" % (what, int((got[~m] != U[~m]).sum()))
    if exact:
        nbad = int((got[m] != ref[m]).sum())
        assert nbad == 0, "%s: %d of %d doubles differ; first at %s" % (what, nbad, int(m.sum()), first_difference(np.where(m, got, 0.0), np.where(m, ref, 0.0)))
        return None
    rho = pc._flux_partner_density(p, ref[0])
    errs = pc.assert_close_specific(interior(got, p), interior(ref, p), p, what, rho=interior(rho[None], p)[0])
    if p.mhdEnabled and p.eta > 0:
        # the field with its upper face layer, over the square root of the same density
        for v in range(5, 8 if p.three_d else 7):
            s = 1.0 / np.sqrt(rho[m[v]])
            e = float(pc.rel_l2(got[v][m[v]] * s, ref[v][m[v]] * s))
            assert e < pc.L2_TOLERANCE, "%s: %s with its upper face layer, specific-form relative L2 %.3e" % (what, pc.OT_VARS[v], e)
            errs[pc.OT_VARS[v] + "+face"] = e
    return errs


# ---- two properties that hold whatever the arithmetic of the fluxes --------------------------------------------------------------
# Bound of both: 4 x what the oracle's own output shows on the same input (the device differs from it in summation order and
# contraction only) + 64 eps x the sum of the magnitudes of the terms, so that a lucky zero of the oracle cannot make the bound vanish.
# The floor alone is already above what rounding can do: every face value enters the divergence / the total once per neighbour with a
# relative rounding error of a few eps/2 (the CT increment and the flux difference are rounded relative to themselves, and both are
# smaller than the values they are added to at a diffusion number of 0.1 on states without a density contrast).

def cell_divergence(p, U):
    """(div B per interior cell, sum of the magnitudes of its terms per cell): (Bx(i+1) - Bx(i)) / dx + ... on the face field"""
    gw = p.ghostWidth
    kint = slice(gw, -gw) if p.three_d else slice(None)
    c = (kint, slice(gw, -gw), slice(gw, -gw))
    xp = (kint, slice(gw, -gw), slice(gw + 1, p.nx + gw + 1))
    yp = (kint, slice(gw + 1, p.ny + gw + 1), slice(gw, -gw))
    d = (U[5][xp] - U[5][c]) / p.dx + (U[6][yp] - U[6][c]) / p.dy
    mag = (np.abs(U[5][xp]) + np.abs(U[5][c])) / p.dx + (np.abs(U[6][yp]) + np.abs(U[6][c])) / p.dy
    if p.three_d:
        zp = (slice(gw + 1, p.nz + gw + 1), slice(gw, -gw), slice(gw, -gw))
        d = d + (U[7][zp] - U[7][c]) / p.dz
        mag = mag + (np.abs(U[7][zp]) + np.abs(U[7][c])) / p.dz
    return d, mag


def divergence_change(p, before, after):
    """(max over the interior cells of |div B after - div B before|, 64 eps x the largest sum of term magnitudes of a cell)"""
    d0, m0 = cell_divergence(p, before)
    d1, m1 = cell_divergence(p, after)
    return float(np.abs(d1 - d0).max()), 64.0 * EPS * float(np.maximum(m0, m1).max())


def totals_change(p, before, after):
    """{variable: (|total after - total before| over the interior, 64 eps x the sum of |term| of both totals)}, the totals summed
    exactly (math.fsum): what is measured is the stage's own rounding, not the measurement's.  Density, momenta, and -- without a
    resistive stage -- the energy.  With eta > 0 the reference's total energy is NOT kept: its resistive energy flux reads the field
    after the CT update, whose ghost cells (and the transverse components of the upper face layer, updated from an emf that does not
    exist there) are not those of the periodic images, so the fluxes through the two ends of a row differ -- 7e-5 of the sum of |E|
    on the random state of the 33 x 17 x 20 box.  The fixtures written by the reference pin that behaviour; it is no property"""
    out = {}
    a, b = interior(after, p), interior(before, p)
    resistive = bool(p.mhdEnabled) and p.eta > 0
    for v, n in enumerate(var_names(p)[:5]):
        if n == "energy" and resistive:
            continue
        change = abs(math.fsum(a[v].ravel()) - math.fsum(b[v].ravel()))
        out[n] = (change, 64.0 * EPS * float(np.abs(a[v]).sum() + np.abs(b[v]).sum()))
    return out


def fully_periodic(p):
    return all(p.bc[f] == 3 for f in range(6 if p.three_d else 4))   # RGPU_BC_PERIODIC, include/rgpu.h


def check_stage_properties(lib, oracle, base, ov, state):
    """the resistive CT update keeps the per-cell div B, the flux form keeps the totals of a fully periodic box: the device's change of
    either <= 4 x the oracle's on the same input + the floor.  Returns {quantity: (device, oracle, bound)} (printed)"""
    p, U, dt, ref = stage_input(lib, oracle, base, ov, state)
    got = device_stage(lib, p, U, dt)
    what = "%s [%s] dissipative stage alone on the %s state" % (base, ov, state)
    facts = {}
    if p.mhdEnabled and p.eta > 0:
        (dev, floor), (orc, _) = divergence_change(p, U, got), divergence_change(p, U, ref)
        facts["max |change of div B|"] = (dev, orc, 4.0 * orc + floor)
    if fully_periodic(p):
        dv, oc = totals_change(p, U, got), totals_change(p, U, ref)
        for n in dv:
            facts["total " + n] = (dv[n][0], oc[n][0], 4.0 * oc[n][0] + dv[n][1])
    assert facts, what + ": no property applies"
    print("%s (%s): %s" % (what, lib.arithmetic, "; ".join("%s: device %.2e oracle %.2e bound %.2e" % ((k,) + v) for k, v in facts.items())))
    bad = {k: v for k, v in facts.items() if not v[0] <= v[2]}
    assert not bad, "%s: beyond round-off (device, oracle, bound): %s" % (what, bad)
    return facts


def oracle_property_values(lib, oracle, base, ov, state):
    """the oracle's own change of div B and of the totals (what the bounds are four times of)"""
    p, U, dt, ref = stage_input(lib, oracle, base, ov, state)
    out = {}
    if p.mhdEnabled and p.eta > 0:
        out["max |change of div B|"] = divergence_change(p, U, ref)
    if fully_periodic(p):
        for n, v in totals_change(p, U, ref).items():
            out["total " + n] = v
    return out
