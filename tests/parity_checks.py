"""Parity checks shared by the CPU emulation tests (tests/test_kernels_emu.py, not gpu) and the real thing
(tests/test_gpu_parity.py, -m gpu).  Every check drives a library through the C ABI (ramsesgpu_amd.solver) and
compares with the oracle (tests/oracle_api.py) or with fixtures produced by the reference binary.

Bar (stated once, used everywhere): BIT-IDENTICAL doubles.  The path is fp64; north_star asks for
"Orszag-Tang L2 error vs euler_cpu < 1e-12" -- `assert_same` reports that relative L2 too, and fails on the
stricter bit-identity."""
import math

import numpy as np

from conftest import golden_cases, ini, load_golden
from ramsesgpu_amd import _capi
from ramsesgpu_amd.solver import Solver, interior

L2_TOLERANCE = 1e-12   # north_star's tolerance; the tests demand 0


def rel_l2(a, b):
    num = np.sqrt(((a - b) ** 2).sum())
    den = np.sqrt((b ** 2).sum())
    return num / den if den > 0 else num


def assert_same(got, ref, what, exact=True):
    """bit-identical, except (exact=False) for runs with (a) the random forcing of the "turbulence" problem: its
    normalisation is a sum over the whole domain that the reference accumulates sequentially and the device in a
    fixed parallel order; (b) the Ornstein-Uhlenbeck forcing: 31 cos() per cell from the device's libm instead of
    glibc's.  Those agree to round-off -- well inside the stated L2 tolerance -- not bit for bit"""
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(got).all(), "%s: non-finite values" % what
    err = rel_l2(got, ref)
    assert err < L2_TOLERANCE, "%s: relative L2 %.3e exceeds the stated tolerance %.0e" % (what, err, L2_TOLERANCE)
    if not exact:
        return
    nbad = int((got != ref).sum())
    assert nbad == 0, "%s: %d of %d doubles differ (max abs %.3e, rel L2 %.3e)" % (what, nbad, ref.size, np.abs(got - ref).max(), err)


def attach_gravity(lib, base, ov, p, sv=None, oracle=None):
    """per-cell gravity field of the problem (params.gravityEnabled == 2), handed to the solver and / or the oracle"""
    G = lib.init_gravity(ini(base), ov, p)
    if sv is not None and G is not None:
        sv.set_gravity_field(G)
    if oracle is not None:
        oracle.set_gravity_field(G)
    F = lib.init_forcing(ini(base), ov, p)   # and the static driving field of the "turbulence" problem
    if sv is not None and F is not None:
        sv.set_forcing_field(F)
    if oracle is not None:
        oracle.set_forcing_field(F)
    return G


# ---- 1. fixtures produced by the reference binary --------------------------------------------------------------
def assert_dt_log(dts, log_dt, p, what, exact=True):
    """the time steps of a run against the reference's own log (oracle/gen_golden.py: line n + 1 of the log carries the dt of step n).
    The log is printed with 12 decimals by the MHD run class and with 8 by the hydro one, so the bound is the print's rounding,
    0.6 units of the last decimal (as tests/test_oracle_golden.py takes it for the oracle) -- relative 1e-11 for a dt of 0.05 in MHD,
    not bit equality -- plus, for the contracted library, its relative 1e-11 (check_run_vs_oracle)"""
    n = min(len(dts), len(log_dt) - 1)
    if n <= 0:
        return
    got, ref = np.asarray(dts[:n], dtype=np.float64), np.asarray(log_dt[1:n + 1], dtype=np.float64)
    unit = 0.6e-12 if p.mhdEnabled else 0.6e-8
    bound = unit * max(1.0, float(ref.max())) + (0.0 if exact else 1e-11 * np.abs(ref))
    bad = np.abs(got - ref) > bound
    assert not bad.any(), "%s: dt of step %d is %r, the reference's log says %r" % (what, int(np.argmax(bad)), got[np.argmax(bad)], ref[np.argmax(bad)])


def check_golden_case(lib, name, exact=True):
    """exact=False: the contracted-arithmetic variant of the library -- the stated L2 tolerance instead of equal bits"""
    case = golden_cases()[name]
    p = lib.params_from_ini(ini(case["base"]), case["overrides"])
    g = load_golden(name)
    for s in case["steps"]:
        U0 = lib.init_condition(ini(case["base"]), case["overrides"], p)
        sv = Solver(p, lib)
        try:
            attach_gravity(lib, case["base"], case["overrides"], p, sv=sv)
            dts = sv.start(U0, s)
            assert_dt_log(dts, g["log_dt"], p, "%s, %d steps" % (name, s), exact=exact)
            assert_same(interior(sv.getDataHost(), p), g["step_%d" % s], "%s step %d vs reference" % (name, s),
                        exact=exact and not (p.randomForcingEnabled or p.ouForcingEnabled))
            if s == max(case["steps"]) and np.isfinite(g["total_time"]):
                assert abs(sv.totalTime - float(g["total_time"])) <= 1e-11 * max(1.0, abs(sv.totalTime))
        finally:
            sv.close()


# ---- 2. against the oracle on the same seeded inputs ---------------------------------------------------------
def random_state(p, seed, mach=1.5):
    """a physically admissible but rough state (exercises limiter branches, supersonic Riemann fans, floors)"""
    rng = np.random.RandomState(seed)
    nv, ks, js, is_ = p.shape
    rho = 0.5 + 1.5 * rng.rand(ks, js, is_)
    vel = mach * (2 * rng.rand(3, ks, js, is_) - 1)
    pres = 0.2 + rng.rand(ks, js, is_)
    U = np.zeros(p.shape)
    U[0] = rho
    U[2] = rho * vel[0]
    U[3] = rho * vel[1]
    ekin = 0.5 * rho * (vel[0] ** 2 + vel[1] ** 2)
    if nv >= 5:
        if p.three_d or nv == 8:
            U[4] = rho * vel[2]
            ekin = ekin + 0.5 * rho * vel[2] ** 2
    emag = 0.0
    if nv == 8:
        B = 0.7 * (2 * rng.rand(3, ks, js, is_) - 1)
        U[5:8] = B
        emag = 0.5 * (B ** 2).sum(0) * 1.5   # generous: cell-centred averages are smaller than face values
    U[1] = pres / (p.gamma0 - 1.0) + ekin + emag
    return U


def check_boundaries(lib, oracle, base, ov, seed=1):
    p = lib.params_from_ini(ini(base), ov)
    U = random_state(p, seed)
    sv = Solver(p, lib)
    try:
        for idim in (1, 2, 3) if p.three_d else (1, 2):
            ref = U.copy()
            oracle.make_boundaries(p, ref, idim)
            sv.upload(U, both=False)
            sv.make_boundaries(0, idim)
            assert_same(sv.getDataHost(0), ref, "%s make_boundaries(dir %d)" % (base, idim))
        times = [(3.7, 0.9), (0.0, 0.0)]
        if p.shearingBoxEnabled and p.Omega0 > 0 and p.three_d:
            # ... and a (t, dt) whose shift lies in the last row, jplus == ny - 1: half a cell before the wrap of ylen, one wrap behind it
            rate, ylen = 1.5 * p.Omega0 * (p.dx * p.nx), p.dy * p.ny
            t_last = (2.0 * ylen - 0.5 * p.dy) / rate
            assert int(math.fmod(rate * t_last, ylen) / p.dy) == p.ny - 1, (base, ov)
            times.append((t_last - 0.9, 0.9))
        for t, dt in times:
            ref = U.copy()
            oracle.make_all_boundaries(p, ref, t, dt)
            sv.upload(U, both=False)
            sv.make_all_boundaries(0, t, dt)
            assert_same(sv.getDataHost(0), ref, "%s make_all_boundaries at (t, dt) = (%r, %r)" % (base, t, dt))
    finally:
        sv.close()


def check_compute_dt(lib, oracle, base, ov, seed=2):
    p = lib.params_from_ini(ini(base), ov)
    U = random_state(p, seed)
    sv = Solver(p, lib)
    try:
        sv.upload(U, both=True)
        for useU in (0, 1):
            got = sv.compute_dt(useU)
            ref = oracle.compute_dt(p, U)
            assert got == ref, "%s compute_dt(%d): %r != %r" % (base, useU, got, ref)
    finally:
        sv.close()


def check_single_step_random(lib, oracle, base, ov, seed=3, mach=1.5, t0=2.0):
    """one godunov_unsplit on a rough random state, interior (and evolved faces) compared"""
    p = lib.params_from_ini(ini(base), ov)
    U = random_state(p, seed, mach)
    oracle.make_all_boundaries(p, U, t0, 0.0)
    dt = 0.3 * oracle.compute_dt(p, U)
    sv = Solver(p, lib)
    try:
        attach_gravity(lib, base, ov, p, sv=sv, oracle=oracle)
        sv.upload(U, both=True)
        sv.godunov_unsplit(0, dt, t0)
        got = sv.getDataHost(1)
        ref = oracle.godunov_unsplit(p, U.copy(), dt, t0)
        assert_same(interior(got, p), interior(ref, p), "%s [%s] single step on random state" % (base, ov))
        if p.mhdEnabled and p.Omega0 > 0:
            # rotating path fills the ghosts of the OUTPUT at step end: the whole array is defined
            assert_same(got, ref, "%s single rotating step incl. ghosts" % base)
    finally:
        sv.close()


# ---- stress states: the floors, degenerate and tied branches the smooth problems and random_state never reach ------------------------
# Every family is seeded, admissible to the oracle (check_single_step_stress asserts its output finite) and checks on the numpy side
# that it holds what it claims (StressStateError otherwise): a family that has gone soft fails as a generator error, not as a pass.
STRESS_FAMILIES = ("rough", "contrast", "lowbeta", "floor", "patches")


class StressStateError(AssertionError):
    pass


def stress_families(p):
    """the families that apply to a configuration: lowbeta needs a magnetic field, and an isothermal sound speed that leaves beta
    below 1e-3 under |B| ~ 1"""
    return [f for f in STRESS_FAMILIES if f != "lowbeta" or (p.nbVar == 8 and 2.0 * p.cIso * p.cIso < 1e-3)]


_MHD_BASES = ("orszag-tang", "orszag-tang3d", "mhd_BrioWu", "mhd_mri_3d", "mhd_mri_3d_stratified", "mhd_inertialWave_2d")


def stress_cases(shapes):
    """[(base, ov, family)] for [(base, ov, ...)]: every family that applies (stress_families, decided here from the names so that
    collection needs no library: the tests assert that it agrees)"""
    out = []
    for s in shapes:
        base, ov = s[0], s[1]
        cs = [float(kv.split("=")[1]) for kv in ov.split(";") if kv.startswith("hydro.cIso=")]
        cs = cs[-1] if cs else (0.001 if base.startswith("mhd_mri_3d") else 0.0)
        for f in STRESS_FAMILIES:
            if f != "lowbeta" or (base in _MHD_BASES and 2.0 * cs * cs < 1e-3):
                out.append((base, ov, f))
    return out


def _plus1(a, axis):
    """a[.., i + 1, ..] along axis, the last layer repeated (it only feeds the outermost ghost layer)"""
    out = np.empty_like(a)
    n = a.shape[axis]
    src = [slice(None)] * a.ndim
    dst = [slice(None)] * a.ndim
    src[axis], dst[axis] = slice(1, n), slice(0, n - 1)
    out[tuple(dst)] = a[tuple(src)]
    src[axis], dst[axis] = slice(n - 1, n), slice(n - 1, n)
    out[tuple(dst)] = a[tuple(src)]
    return out


def centred_field(p, B):
    """the cell-centred field of the MHD primitives (dev_numerics.h: mhd_prim): the mean of the cell's low face and the +1 neighbour's;
    in 2D the z neighbour counts as 0.  B: [3][k][j][i] face field"""
    bx = 0.5 * (B[0] + _plus1(B[0], 2))
    by = 0.5 * (B[1] + _plus1(B[1], 1))
    bz = 0.5 * (B[2] + _plus1(B[2], 0)) if p.three_d else 0.5 * B[2]
    return np.array([bx, by, bz])


def _assemble(p, rho, vel, pres, B=None, emag=None):
    """conservative state from primitives; the energy uses the centred field exactly as the primitives recover it (or emag)"""
    nv = p.nbVar
    U = np.zeros(p.shape)
    U[0] = rho
    U[2] = rho * vel[0]
    U[3] = rho * vel[1]
    ekin = 0.5 * rho * (vel[0] ** 2 + vel[1] ** 2)
    if nv >= 5:
        U[4] = rho * vel[2]
        ekin = ekin + 0.5 * rho * vel[2] ** 2
    if nv == 8:
        U[5:8] = B
        if emag is None:
            emag = 0.5 * (centred_field(p, B) ** 2).sum(0)
    else:
        emag = 0.0
    U[1] = pres / (p.gamma0 - 1.0) + ekin + emag
    return U


def stress_pressure(p, U):
    """the pressure the primitives recover from U (before the floor), in the kernel's order of operations; ghosts included"""
    r = U[0]
    u, v = U[2] / r, U[3] / r
    eken = 0.5 * (u * u + v * v)
    if p.nbVar >= 5:
        w = U[4] / r
        eken = 0.5 * (u * u + v * v + w * w)
    emag = 0.5 * (centred_field(p, U[5:8]) ** 2).sum(0) if p.nbVar == 8 else 0.0
    return (p.gamma0 - 1.0) * r * ((U[1] - emag) / r - eken)


def _interior_cells(p, a):
    gw = p.ghostWidth
    return a[gw:-gw, gw:-gw, gw:-gw] if p.three_d else a[:, gw:-gw, gw:-gw]


def stress_stats(p, U):
    """what the generator checks: floored fraction, tied fraction, low-beta fraction, density ratio (interior cells)"""
    r = _interior_cells(p, U[0])
    if p.cIso > 0:
        pres = p.cIso * p.cIso * U[0]
        pfloor = np.zeros(U[0].shape, bool)
    else:
        pres = stress_pressure(p, U)
        pfloor = pres <= U[0] * p.smallp
    floored = float(((_interior_cells(p, U[0]) <= p.smallr) | _interior_cells(p, pfloor)).mean())
    # all 2 ndim neighbours equal in every variable: cells one layer inside the interior (their neighbours are interior cells)
    gw = p.ghostWidth
    axes = (1, 2, 3) if p.three_d else (2, 3)
    tied = np.ones(U.shape[1:], bool)
    for ax in axes:
        tied &= (np.roll(U, 1, ax) == U).all(0) & (np.roll(U, -1, ax) == U).all(0)
    inner = tied[gw + 1:-gw - 1, gw + 1:-gw - 1, gw + 1:-gw - 1] if p.three_d else tied[:, gw + 1:-gw - 1, gw + 1:-gw - 1]
    if p.nbVar == 8:
        b2 = (centred_field(p, U[5:8]) ** 2).sum(0)
        lowbeta = float((_interior_cells(p, 2.0 * np.maximum(pres, U[0] * p.smallp) < 1e-3 * b2)).mean())
    else:
        lowbeta = 0.0
    return {"floored": floored, "tied": float(inner.mean()) if inner.size else 0.0, "lowbeta": lowbeta,
            "density_ratio": float(r.max() / r.min())}


def stress_state(p, seed, family):
    """a seeded state of one family (STRESS_FAMILIES), ghosts included (the caller fills them):
      rough     random_state at Mach 3
      contrast  rho and p log-uniform over 6 decades, |v| <= 10, |B| <= 3
      lowbeta   (MHD) p ~ 1e-4 under |B| ~ 1: the pressure is what is left of E - ekin - emag
      floor     ~20 % of cells at rho in {smallr / 2, smallr, 2 smallr} (pressure ~ rho, field ~ sqrt(rho): sound and Alfven speeds of
                order 1, or they set a dt of 1e-7), ~30 % with E = ekin + emag exactly (every operand a short dyadic number: the recovered
                pressure is exactly 0 and floored to rho smallp)
      patches   piecewise-uniform blocks of 4 cells per direction: neighbours tie exactly (zero limited slopes); whole blocks with a velocity
                component exactly 0 and fields that are purely normal (one component only) or without a normal component (adiabatic
                only: the isothermal HLLD step of the reference is not finite at a zero normal field)"""
    if family not in STRESS_FAMILIES:
        raise ValueError(family)
    if family == "lowbeta" and p.nbVar != 8:
        raise ValueError("lowbeta is an MHD family")
    rng = np.random.RandomState(1000 + 17 * seed + STRESS_FAMILIES.index(family))
    nv, ks, js, is_ = p.shape
    mhd = nv == 8
    cells = (ks, js, is_)

    def uni(lo, hi, n=None):
        return rng.uniform(lo, hi, ((n,) if n else ()) + cells)

    if family == "rough":
        U = random_state(p, seed, mach=3.0)
    elif family == "contrast":
        rho, pres = 10.0 ** uni(-3, 3), 10.0 ** uni(-3, 3)
        vel = uni(-1, 1, 3) * (10.0 / np.sqrt(3.0))
        B = uni(-1, 1, 3) * (3.0 / np.sqrt(3.0)) if mhd else None
        U = _assemble(p, rho, vel, pres, B)
    elif family == "lowbeta":
        b0 = rng.normal(size=3)
        b0 /= np.sqrt((b0 ** 2).sum())
        B = b0[:, None, None, None] * uni(0.8, 1.2) + 0.05 * uni(-1, 1, 3)
        U = _assemble(p, uni(0.5, 2.0), uni(-1, 1, 3), 1e-4 * uni(0.5, 1.5), B)
    elif family == "floor":
        q = 1.0 / 16.0                                          # dyadic grid: every product and sum below is exact
        kind = rng.rand(*cells)
        light = kind < 0.24
        # not in the last interior layer: its +1 face is a ghost face, which the ghost fill may take from an unscaled image
        gw = p.ghostWidth
        for ax in ((0, 1, 2) if p.three_d else (1, 2)):
            idx = [slice(None)] * 3
            idx[ax] = slice(cells[ax] - gw - 1, None)
            light[tuple(idx)] = False
        zero_p = (kind >= 0.24) & (kind < 0.54)
        rho = np.where(zero_p, 2.0 ** rng.randint(-1, 2, cells), uni(0.5, 2.0))
        rho = np.where(light, p.smallr * np.array([0.5, 1.0, 2.0])[rng.randint(0, 3, cells)], rho)
        vel = np.round(uni(-3, 3, 3) / q) * q
        pres = np.where(light, rho * uni(0.3, 1.0), uni(0.2, 1.2))
        pres = np.where(zero_p, 0.0, pres)
        B = None
        if mhd:
            B = np.round(uni(-0.7, 0.7, 3) / q) * q
            # faces of the light cells (the cell's low face and the +1 neighbour's) scaled by a power of two ~ sqrt(smallr)
            s = 2.0 ** np.round(0.5 * np.log2(p.smallr))
            for c, ax in enumerate((2, 1, 0)):
                if c == 2 and not p.three_d:
                    B[c] = np.where(light, B[c] * s, B[c])
                    continue
                lo = np.roll(light, 1, ax)                      # the face i is the +1 face of cell i - 1
                B[c] = np.where(light | lo, B[c] * s, B[c])
        U = _assemble(p, rho, vel, pres, B)
    else:   # patches
        gw = p.ghostWidth
        nb = [(n + 3) // 4 + 2 for n in cells]

        def blocks(a):
            """[..][bk][bj][bi] -> cells, block origin at the first interior cell"""
            for ax, n in zip((-3, -2, -1), cells):
                a = np.repeat(a, 4, axis=ax)
                off = (4 - gw % 4) % 4 if (ax != -3 or p.three_d) else 0
                a = np.take(a, range(off, off + n), axis=ax)
            return a

        bshape = tuple(nb) if p.three_d else (1, nb[1], nb[2])
        rho = blocks(rng.uniform(0.5, 2.0, bshape))
        pres = blocks(rng.uniform(0.2, 1.2, bshape))
        v = rng.uniform(-2.0, 2.0, (3,) + bshape) * (rng.rand(3, *bshape) >= 0.35)
        vel = blocks(v)
        B = None
        if mhd:
            b = rng.uniform(-0.7, 0.7, (3,) + bshape)
            mode = rng.randint(0, 5, bshape)                     # 0: all three, 1-3: only x / y / z (purely normal), 4: no x component
            if p.cIso > 0:
                # isothermal HLLD has no answer for a zero normal field (the reference's step is NaN there): all three components
                mode[:] = 0
            for c in range(3):
                b[c] = np.where((mode >= 1) & (mode <= 3) & (mode != c + 1), 0.0, b[c])
            b[0] = np.where(mode == 4, 0.0, b[0])
            B = blocks(b)
        # the block's own field in the energy: U is uniform inside a block (the last cell's recovered pressure differs, may be floored)
        U = _assemble(p, rho, vel, pres, B, emag=None if B is None else 0.5 * (B ** 2).sum(0))
    # ---- what the family claims ----
    st = stress_stats(p, U)
    want = {"floor": ("floored", 0.08 if p.cIso > 0 else 0.3), "patches": ("tied", 0.08 if p.three_d else 0.15),
            "lowbeta": ("lowbeta", 0.5)}
    if family in want:
        k, lo = want[family]
        if not st[k] >= lo:
            raise StressStateError("stress_state(%s): %s fraction %.3f < %.2f" % (family, k, st[k], lo))
    if family == "contrast" and not st["density_ratio"] >= 1e5:
        raise StressStateError("stress_state(contrast): density ratio %.3g < 1e5" % st["density_ratio"])
    if not np.isfinite(U).all():
        raise StressStateError("stress_state(%s): non-finite values" % family)
    return U


_STRESS_CACHE = {}


def stress_reference(oracle, lib, base, ov, family, seed=3, t0=2.0):
    """(p, ghost-filled state, dt, oracle's step) for one case, with the generator's oracle-side checks: dt not below 1e-3 x the rough
    family's on the same box, a finite step.  The last case is kept: the exact and contracted libraries run the same case in a row."""
    key = (base, ov, family, seed, t0)
    if key in _STRESS_CACHE:
        return _STRESS_CACHE[key]
    p = lib.params_from_ini(ini(base), ov)
    attach_gravity(lib, base, ov, p, oracle=oracle)
    dts = {}
    for fam in ("rough", family):
        U = stress_state(p, seed, fam)
        oracle.make_all_boundaries(p, U, t0, 0.0)
        dts[fam] = oracle.compute_dt(p, U)
    if not dts[family] >= 1e-3 * dts["rough"]:
        raise StressStateError("stress_state(%s) on %s [%s]: the oracle's dt %.3g is below 1e-3 x the rough family's %.3g"
                               % (family, base, ov, dts[family], dts["rough"]))
    dt = 0.3 * dts[family]
    ref = oracle.godunov_unsplit(p, U.copy(), dt, t0)
    if not np.isfinite(ref).all():
        raise StressStateError("stress_state(%s) on %s [%s]: the oracle's step is not finite" % (family, base, ov))
    _STRESS_CACHE.clear()
    _STRESS_CACHE[key] = (p, U, dt, ref)
    return _STRESS_CACHE[key]


def _flux_partner_density(p, r):
    """max |rho| over a cell and its face neighbours (the cells whose fluxes update it), not below smallr"""
    m = np.abs(r)
    for ax in ((0, 1, 2) if p.three_d else (1, 2)):
        for s in (1, -1):
            m = np.maximum(m, np.abs(np.roll(r, s, ax)))
    return np.maximum(m, p.smallr)


def assert_close_specific(got, ref, p, what, rho=None):
    """the contracted library's bar on states whose density spans decades: relative L2 < L2_TOLERANCE per variable in specific form --
    rho; momenta and energy over a density; the field over its square root -- so that dense cells cannot hide light ones.  Every value
    finite.  Returns {variable: relative L2}.
    The density of a cell's specific form is the largest |rho| of the oracle's among the cell and its face neighbours, not below smallr:
    the update of a light cell sums fluxes of its neighbours, so a 1-ulp difference in the flux of a neighbour 1e6 times denser is a 1e-10
    change of the light cell's own specific momentum.  Measured on MI355X with the cell's own |rho| instead: up to 3.6e-10 (floor family,
    approx solver) and 1.3e-12 .. 1.7e-12 (contrast), ten cells or fewer carrying the whole error, every one a light cell beside a
    cell 1e3 .. 1e10 times denser; with the flux partner's density the same runs give <= 4.5e-16.  A light cell among light cells is still
    judged at its own scale.  (The oracle's own step leaves rho <= 0 in a few floored cells, hence |rho| and smallr.)  rho: that density,
    when got / ref are the interior of arrays whose ghost cells hold the neighbours of the edge cells"""
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(got).all(), "%s: non-finite values" % what
    r = _flux_partner_density(p, ref[0]) if rho is None else rho
    errs = {}
    for v in range(p.nbVar):
        scale = 1.0 if v == 0 else (1.0 / np.sqrt(r) if v >= 5 else 1.0 / r)
        name = OT_VARS[v] if p.nbVar == 8 else ("density", "energy", "mx", "my", "mz")[v]
        errs[name] = float(rel_l2(got[v] * scale, ref[v] * scale))
    bad = {k: e for k, e in errs.items() if not e < L2_TOLERANCE}
    assert not bad, "%s: specific-form relative L2 above %.0e: %s" % (what, L2_TOLERANCE, {k: "%.3e" % e for k, e in bad.items()})
    return errs


def check_single_step_stress(lib, oracle, base, ov, family, exact=True, seed=3, t0=2.0):
    """one godunov_unsplit from a stress state (ghosts filled by the oracle, dt = 0.3 x the oracle's CFL dt); the interior compared --
    and the whole array on the rotating path, which fills the ghosts of its output.  exact: every double equal; otherwise
    assert_close_specific.  Returns the specific-form relative L2 per variable (exact=False) or None."""
    p, U, dt, ref = stress_reference(oracle, lib, base, ov, family, seed, t0)
    sv = Solver(p, lib)
    try:
        attach_gravity(lib, base, ov, p, sv=sv)
        sv.upload(U, both=True)
        sv.godunov_unsplit(0, dt, t0)
        got = sv.getDataHost(1)
    finally:
        sv.close()
    what = "%s [%s] single step on the %s stress state" % (base, ov, family)
    whole = bool(p.mhdEnabled) and p.Omega0 > 0
    if exact:
        assert_same(interior(got, p), interior(ref, p), what)
        if whole:
            assert_same(got, ref, what + " incl. ghosts")
        return None
    rho = _flux_partner_density(p, ref[0])
    errs = assert_close_specific(interior(got, p), interior(ref, p), p, what, rho=interior(rho[None], p)[0])
    if whole:
        assert_close_specific(got, ref, p, what + " incl. ghosts")
    return errs


def near_uniform_state(p, seed, eps):
    """a uniform magnetised flow + perturbations of relative size eps in every variable: with eps around 1e-12 the candidates of the
    Alfven-speed maxima of the 2D HLLD edge solver (dev_numerics.h: alfven_pick / alfven_duel) lie within, at and beyond the margins
    below which the solver falls back to the reference's own sequence -- lanes of one wave take different routes; eps = 0: every
    candidate pair ties exactly"""
    rng = np.random.RandomState(seed)
    nv, ks, js, is_ = p.shape
    def pert():
        return 1.0 + eps * (2 * rng.rand(ks, js, is_) - 1)
    rho = 1.3 * pert()
    vel = [0.31 * pert(), -0.17 * pert(), 0.23 * pert()]
    U = np.zeros(p.shape)
    U[0] = rho
    U[2], U[3] = rho * vel[0], rho * vel[1]
    ekin = 0.5 * rho * (vel[0] ** 2 + vel[1] ** 2)
    if nv == 8 or p.three_d:
        U[4] = rho * vel[2]
        ekin = ekin + 0.5 * rho * vel[2] ** 2
    emag = 0.0
    if nv == 8:
        B = [0.45 * pert(), 0.36 * pert(), -0.52 * pert()]
        for c in range(3):
            U[5 + c] = B[c]
        emag = 0.5 * (B[0] ** 2 + B[1] ** 2 + B[2] ** 2)
    U[1] = 0.9 * pert() / (p.gamma0 - 1.0) + ekin + emag
    return U


def check_single_step_near_uniform(lib, oracle, base, ov, eps, seed=11, t0=0.0):
    """one godunov_unsplit from near_uniform_state, every double compared (the Alfven selection must return the reference's bits
    whichever route a lane takes)"""
    p = lib.params_from_ini(ini(base), ov)
    U = near_uniform_state(p, seed, eps)
    oracle.make_all_boundaries(p, U, t0, 0.0)
    dt = 0.4 * oracle.compute_dt(p, U)
    sv = Solver(p, lib)
    try:
        sv.upload(U, both=True)
        sv.godunov_unsplit(0, dt, t0)
        got = sv.getDataHost(1)
        ref = oracle.godunov_unsplit(p, U.copy(), dt, t0)
        assert_same(interior(got, p), interior(ref, p), "%s [%s] single step from a near-uniform state, eps = %g" % (base, ov, eps))
    finally:
        sv.close()


def check_run_vs_oracle(lib, oracle, base, ov, nsteps, exact=True, out=None):
    """exact=False: the contracted-arithmetic variant of the library -- relative L2 < 1e-12 on the state, dt within 1e-11.
    out: a dict that receives what the library returned ("state": the interior, "dts", "t"), before anything is compared"""
    p = lib.params_from_ini(ini(base), ov)
    U0 = lib.init_condition(ini(base), ov, p)
    attach_gravity(lib, base, ov, p, oracle=oracle)
    ref, dts_ref, t_ref = oracle.run(p, U0, nsteps)
    sv = Solver(p, lib)
    try:
        attach_gravity(lib, base, ov, p, sv=sv)
        dts = sv.start(U0, nsteps)
        if out is not None:
            out.update(state=interior(sv.getDataHost(), p).copy(), dts=list(dts), t=sv.totalTime)
        if not exact:
            assert np.abs(np.array(dts) / np.asarray(dts_ref) - 1.0).max() < 1e-11, "%s: dt sequences differ beyond round-off" % base
            assert_same(interior(sv.getDataHost(), p), interior(ref, p), "%s [%s] %d steps vs oracle" % (base, ov, nsteps), exact=False)
            return p
        if p.randomForcingEnabled or p.ouForcingEnabled:   # round-off level agreement only (see assert_same)
            np.testing.assert_allclose(np.array(dts), dts_ref, rtol=1e-12, atol=0)
            assert_same(interior(sv.getDataHost(), p), interior(ref, p), "%s [%s] %d steps vs oracle" % (base, ov, nsteps), exact=False)
            return
        assert np.array_equal(np.array(dts), dts_ref), "%s: dt sequences differ" % base
        assert_same(interior(sv.getDataHost(), p), interior(ref, p), "%s [%s] %d steps vs oracle" % (base, ov, nsteps))
        assert sv.totalTime == t_ref
    finally:
        sv.close()
    return p


# configurations without a golden fixture: solver options / boundary types / shapes
ORACLE_RUNS = [
    # 2D MHD: other Riemann solvers, slope types, rectangular grids, smallest legal grid
    ("orszag-tang", "mesh.nx=24;mesh.ny=16;hydro.riemannSolver=hll", 4),
    ("orszag-tang", "mesh.nx=16;mesh.ny=24;hydro.riemannSolver=llf", 4),
    ("orszag-tang", "mesh.nx=16;mesh.ny=16;hydro.slope_type=1.0", 4),
    ("orszag-tang", "mesh.nx=16;mesh.ny=16;hydro.traceVersion=0", 3),          # slope_type forced to 0
    ("orszag-tang", "mesh.nx=3;mesh.ny=3", 3),
    ("orszag-tang", "mesh.nx=16;mesh.ny=16;hydro.riemannSolver=hllc", 2),       # MHD + hllc => zero hydro flux quirk
    ("mhd_BrioWu", "mesh.nx=20;mesh.ny=12;BrioWu.direction=3", 5),
    # 3D MHD plain: boundary types, solvers, isothermal
    ("mhd_BrioWu", "mesh.nx=12;mesh.ny=10;mesh.nz=8;BrioWu.direction=0;MHD.implementationVersion=4", 4),
    ("mhd_BrioWu", "mesh.nx=8;mesh.ny=12;mesh.nz=10;BrioWu.direction=2;MHD.implementationVersion=3;mesh.boundary_zmin=1;mesh.boundary_zmax=1", 4),
    ("orszag-tang3d", "mesh.nx=10;mesh.ny=8;mesh.nz=6;hydro.riemannSolver=hll", 3),
    ("orszag-tang3d", "mesh.nx=8;mesh.ny=8;mesh.nz=8;hydro.cIso=0.9;hydro.slope_type=1.0", 3),
    ("orszag-tang3d", "mesh.nx=3;mesh.ny=3;mesh.nz=3", 2),
    # 3D MHD rotating: without shearing box (periodic x), other sizes
    ("orszag-tang3d", "mesh.nx=8;mesh.ny=12;mesh.nz=6;MHD.omega0=0.05", 4),
    ("mhd_mri_3d", "mesh.nx=6;mesh.ny=8;mesh.nz=10;MHD.omega0=0.01;MRI.amp=0.2", 6),
    # hydro: 3D jet (inflow after the z fill), 2D solvers / slopes
    ("jet2d_cpu", "mesh.nx=12;mesh.ny=12;mesh.nz=12;mesh.zmax=1;jet.ijet=3;jet.offsetJet=2", 6),
    ("implode3d", "mesh.nx=12;mesh.ny=8;mesh.nz=1;hydro.riemannSolver=hll;hydro.slope_type=2.0", 5),
    ("implode3d", "mesh.nx=10;mesh.ny=10;mesh.nz=10;hydro.traceVersion=0;hydro.riemannSolver=hllc", 4),
    ("implode3d", "mesh.nx=2;mesh.ny=2;mesh.nz=2", 3),
    # the other EMF solvers and the positivity-preserving slopes on further paths
    ("mhd_mri_3d", "mesh.nx=6;mesh.ny=8;mesh.nz=10;MHD.magRiemannSolver=hlla;MRI.amp=0.2", 5),     # rotating + shear terms of the EMF
    ("mhd_mri_3d", "mesh.nx=6;mesh.ny=8;mesh.nz=6;MHD.magRiemannSolver=llf", 4),
    ("mhd_BrioWu", "mesh.nx=16;mesh.ny=12;BrioWu.direction=1;MHD.magRiemannSolver=llf", 5),
    ("mhd_BrioWu", "mesh.nx=16;mesh.ny=12;BrioWu.direction=1;MHD.magRiemannSolver=hllf;hydro.slope_type=3.0", 5),
    ("orszag-tang3d", "mesh.nx=8;mesh.ny=6;mesh.nz=10;hydro.slope_type=3.0;MHD.magRiemannSolver=hllf;hydro.cIso=0.8", 3),
    ("mhd_BrioWu", "mesh.nx=10;mesh.ny=8;mesh.nz=8;BrioWu.direction=2;MHD.implementationVersion=3;hydro.slope_type=3.0", 4),
    # per-cell gravity field (Keplerian disk): other solvers, direction-wise update, viscosity, 3D
    ("Keplerian_disk2d", "mesh.nx=14;mesh.ny=10;hydro.riemannSolver=approx", 5),
    ("Keplerian_disk2d", "mesh.nx=10;mesh.ny=12;mesh.nz=6;hydro.riemannSolver=hll;hydro.unsplitVersion=2;hydro.nu=0.003", 4),
    ("Keplerian_disk2d", "mesh.nx=12;mesh.ny=12;gravity.static=no", 3),
    # driven turbulence (round-off agreement): other sizes / solvers, zero input rate, with viscosity
    ("turbulence_hydro", "mesh.nx=10;mesh.ny=8;mesh.nz=12;hydro.riemannSolver=hll", 4),
    ("turbulence_hydro", "mesh.nx=8;mesh.ny=8;mesh.nz=8;turbulence.edot=0.0;hydro.nu=0.001", 3),
    ("turbulence_mhd", "mesh.nx=8;mesh.ny=10;mesh.nz=8;hydro.slope_type=2.0;turbulence.beta=2.0;MHD.eta=1e-4", 4),
    # stratified MRI box: other solvers, unsmoothed gravity, floor
    ("mhd_mri_3d_stratified", "mesh.nx=6;mesh.ny=8;mesh.nz=16;hydro.slope_type=2.0;MRI.amp=0.4;MHD.magRiemannSolver=hllf;hydro.riemannSolver=hll", 4),
    ("mhd_mri_3d_stratified", "mesh.nx=8;mesh.ny=6;mesh.nz=12;hydro.slope_type=1.0;MRI.amp=0.4;MRI.smoothGravity=no;MRI.floor=yes;mesh.zmin=-1.5;mesh.zmax=1.5", 4),
    # 2D branch of the rotating-frame step: other solvers / slopes / boundaries, implementationVersion 0 + gravity knobs ignored
    ("orszag-tang", "mesh.nx=16;mesh.ny=20;MHD.omega0=0.4;hydro.slope_type=3.0;MHD.magRiemannSolver=hlla", 5),
    ("mhd_BrioWu", "mesh.nx=20;mesh.ny=12;BrioWu.direction=1;MHD.omega0=0.25;hydro.riemannSolver=llf;MHD.magRiemannSolver=llf;mesh.boundary_ymin=1;mesh.boundary_ymax=1", 5),
    ("mhd_inertialWave_2d", "mesh.nx=8;mesh.ny=6;MHD.implementationVersion=0", 6),
]

RANDOM_STEPS = [
    ("orszag-tang", "mesh.nx=20;mesh.ny=14", 1.5),
    ("orszag-tang", "mesh.nx=14;mesh.ny=20;hydro.riemannSolver=hll", 3.0),
    ("mhd_BrioWu", "mesh.nx=16;mesh.ny=16", 2.5),
    ("orszag-tang", "mesh.nx=18;mesh.ny=14;MHD.omega0=0.6;hydro.cIso=0.7", 2.0),
    ("orszag-tang3d", "mesh.nx=10;mesh.ny=8;mesh.nz=6", 1.5),
    ("orszag-tang3d", "mesh.nx=6;mesh.ny=10;mesh.nz=8;hydro.riemannSolver=llf", 3.0),
    ("mhd_mri_3d", "mesh.nx=8;mesh.ny=10;mesh.nz=6;hydro.cIso=0.8;MHD.omega0=0.3", 1.0),
    ("mhd_mri_3d_stratified", "mesh.nx=8;mesh.ny=10;mesh.nz=8;hydro.slope_type=2.0;hydro.cIso=0.8;MHD.omega0=0.3", 1.0),
    ("mhd_mri_3d", "mesh.nx=8;mesh.ny=10;mesh.nz=6;hydro.cIso=0.8;MHD.omega0=0.3;mesh.boundary_xmin=3;mesh.boundary_xmax=3", 1.0),
    ("implode3d", "mesh.nx=10;mesh.ny=8;mesh.nz=6;hydro.riemannSolver=hllc", 3.0),
    ("implode3d", "mesh.nx=10;mesh.ny=8;mesh.nz=6", 3.0),
    ("implode3d", "mesh.nx=10;mesh.ny=8;mesh.nz=6;hydro.riemannSolver=hll;hydro.slope_type=2.0", 3.0),
    ("implode3d", "mesh.nx=12;mesh.ny=10;mesh.nz=1;hydro.riemannSolver=hllc", 3.0),
    ("jet2d_cpu", "mesh.nx=12;mesh.ny=16;jet.ijet=3;jet.offsetJet=2", 2.0),
]

BOUNDARY_CASES = [
    ("orszag-tang", "mesh.nx=8;mesh.ny=6"), ("mhd_BrioWu", "mesh.nx=6;mesh.ny=8"), ("jet2d_cpu", "mesh.nx=10;mesh.ny=8;jet.ijet=3;jet.offsetJet=2"),
    ("implode3d", "mesh.nx=6;mesh.ny=5;mesh.nz=4"), ("orszag-tang3d", "mesh.nx=6;mesh.ny=5;mesh.nz=4"),
    ("mhd_mri_3d", "mesh.nx=6;mesh.ny=8;mesh.nz=4;MHD.omega0=0.4"),
    ("mhd_mri_3d", "mesh.nx=6;mesh.ny=8;mesh.nz=4;MHD.omega0=1.0"),      # fastshear: at (3.7, 0.9) the shift has wrapped ylen
    ("mhd_BrioWu", "mesh.nx=4;mesh.ny=5;mesh.nz=6;mesh.boundary_xmin=1;mesh.boundary_ymax=1;mesh.boundary_zmin=3;mesh.boundary_zmax=3"),
]


# The bench's launch geometry: the LDS-tiled kernels' full-width tile rows, several rounds of workgroups and a sub-segmented last
# round, on planes of > 32768 cells.  Few planes keep the oracle at seconds per step.  (These contexts run the tiled sweeps, which
# neither read "xcd_sub" nor take the chunked two-stream schedule: the XCD-aware workgroup order of rg_launch_planes belongs to the
# flat kernels' launch_planes calls and the chunk schedule to the flat 3D MHD kernels -- per-cell gravity field or RGPU_TILED=0 --
# and both are pinned at this plane size by tests/test_flat_path_gpu.py.)
BENCH_GEOMETRY = [
    ("mhd_mri_3d", "mesh.nx=512;mesh.ny=512;mesh.nz=16", 2),
    # the x-y cross-section of BASELINE config 5 (512 x 1024 x 512 over 8 GPUs): 33 x 129 tiles of the MHD sweep
    ("mhd_mri_3d", "mesh.nx=512;mesh.ny=1024;mesh.nz=16", 2),
    ("orszag-tang3d", "mesh.nx=256;mesh.ny=256;mesh.nz=24", 2),
    ("implode3d", "mesh.nx=512;mesh.ny=512;mesh.nz=8;hydro.riemannSolver=hllc", 2),
]


def check_core_plane_pieces(lib, base, ov, state=None, oracle=None):
    """rgpu_step_core_planes over a partition of [0,ksize) (odd cuts, out of order) == rgpu_step_core; so is the split form
    (rgpu_step_core_planes_split: the fluxes of the whole box once, then the update piece by piece -- the slab driver's order).
    state: a stress_state family (STRESS_FAMILIES) instead of the initial condition; oracle: the whole call is also compared with the
    oracle's step from the same state (dt equal, every double of the interior equal; the whole array on the rotating path).
    A per-cell gravity field of the problem is attached (flat kernels: a piece of >= 16 planes takes the chunked two-stream schedule
    of mhd3d_core from its own first plane)"""
    p = lib.params_from_ini(ini(base), ov)
    U0 = lib.init_condition(ini(base), ov, p) if state is None else stress_state(p, 3, state)
    ks = p.nz + 2 * p.ghostWidth
    cuts = [0, 1, 7, 8, ks - 15, ks]
    pieces = list(reversed(list(zip(cuts[:-1], cuts[1:]))))
    outs = []
    attach_gravity(lib, base, ov, p, oracle=oracle)
    for mode in ("whole", "pieces", "split"):
        sv = Solver(p, lib)
        attach_gravity(lib, base, ov, p, sv=sv)
        sv.upload(U0)
        sv.make_all_boundaries(0, 0.0, 0.0)
        dt = sv.compute_dt(0)
        if mode == "whole" and oracle is not None:
            filled = sv.getDataHost(0)
        sv.step_pre(0, dt, 0.0)
        if mode == "whole":
            sv.step_core(0, dt, 0.0)
        elif mode == "pieces":
            for a, b in pieces:
                sv.step_core_planes(0, dt, 0.0, a, b)
        else:
            sv.step_core_planes_split(0, dt, 0.0, 0, ks, 1)
            for a, b in pieces:
                sv.step_core_planes_split(0, dt, 0.0, a, b, 2)
        sv.step_post_a(0, dt, 0.0)
        sv.step_post_b(0, dt, 0.0)
        outs.append(sv.getDataHost(1))
        sv.close()
        if mode == "whole" and oracle is not None:
            ref = U0.copy()
            oracle.make_all_boundaries(p, ref, 0.0, 0.0)
            assert_same(filled, ref, "%s [%s] ghost fill before the step" % (base, ov))
            assert dt == oracle.compute_dt(p, ref), (dt, oracle.compute_dt(p, ref))
            ref = oracle.godunov_unsplit(p, ref, dt, 0.0)
            assert_same(interior(outs[0], p), interior(ref, p), "%s [%s] whole step_core vs oracle (%s)" % (base, ov, state or "initial condition"))
            if p.mhdEnabled and p.Omega0 > 0:
                assert_same(outs[0], ref, "%s [%s] whole step_core vs oracle incl. ghosts" % (base, ov))
    assert np.array_equal(outs[0], outs[1])
    assert np.array_equal(outs[0], outs[2])


HISTORY_CASES = [
    ("mhd_mri_3d", "mesh.nx=8;mesh.ny=16;mesh.nz=8;MRI.amp=0.2", 6),
    ("orszag-tang3d", "mesh.nx=12;mesh.ny=10;mesh.nz=8", 3),
    ("orszag-tang", "mesh.nx=24;mesh.ny=16", 4),                       # 2D: history_default's mass / divB
    ("mhd_BrioWu", "mesh.nx=16;mesh.ny=12;mesh.nz=8;BrioWu.direction=0;MHD.implementationVersion=4", 3),
]


def check_history(lib, oracle, base, ov, nsteps):
    """device-reduced history diagnostics (rgpu_history_mri) == the oracle's sequential restatement of
    MHDRunBase::history_mri to round-off: the device adds in a different (fixed) order, so every sum is compared with
    a tolerance of 1e-12 x the sum of the magnitudes of its terms"""
    p = lib.params_from_ini(ini(base), ov)
    sv = Solver(p, lib)
    sv.start(lib.init_condition(ini(base), ov, p), nsteps)
    U = sv.getDataHost()
    got = sv.history_mri()
    sv.close()
    ref = dict(zip(Solver.HISTORY_NAMES, oracle.history_mri(p, U)))
    I = interior(U, p)
    cells = I[0].size
    dtau = 1.0 / cells          # dx*dy*dz / box volume
    b = np.abs(I[5:8]).sum() * dtau + 1e-300
    b2 = (I[5:8] ** 2).sum() * dtau + 1e-300
    mom = np.abs(I[2] * I[3] / I[0]).sum() * dtau + 1e-300
    scale = {"mass": ref["mass"], "maxwell": b2, "reynolds": mom, "magp": b2, "mean_Bx": b, "mean_By": b, "mean_Bz": b,
             "divB": np.abs(I[5:8]).sum() * 6.0 / min(p.dx, p.dy) + 1e-300}
    for k in Solver.HISTORY_NAMES:
        assert abs(got[k] - ref[k]) <= 1e-12 * scale[k], (k, got[k], ref[k], scale[k])


TURB_HISTORY_CASES = [
    ("turbulence_mhd_ou", "mesh.nx=12;mesh.ny=10;mesh.nz=8;turbulence-Ornstein-Uhlenbeck.bx=0.01;turbulence-Ornstein-Uhlenbeck.by=0.02", 5),
    ("turbulence_mhd", "mesh.nx=12;mesh.ny=12;mesh.nz=12", 4),
]


def check_history_turbulence(lib, oracle, base, ov, nsteps):
    """device-reduced history_turbulence (rgpu_history_turbulence) == the oracle's sequential restatement of
    MHDRunBase::history_turbulence to round-off (fixed parallel summation order, device cos / sin): every column is compared
    with a tolerance of 1e-11 x the magnitude of the terms of its sum"""
    p = lib.params_from_ini(ini(base), ov)
    sv = Solver(p, lib)
    try:
        attach_gravity(lib, base, ov, p, sv=sv)
        sv.start(lib.init_condition(ini(base), ov, p), nsteps)
        U = sv.getDataHost()
        got = sv.history_turbulence()
    finally:
        sv.close()
    ref = oracle.history_turbulence(p, U)
    gw = p.ghostWidth
    I = U[:, gw:-gw, gw:-gw, gw:-gw]
    dTau = p.dx * p.dy * p.dz / (p.xMax - p.xMin) / (p.yMax - p.yMin) / (p.zMax - p.zMin)
    bmax, mmax = np.abs(U[5:8]).max(), np.abs(I[2:5]).max()
    n = I[0].size
    mag = {1: bmax / min(p.dx, p.dy, p.dz) * n, 4: mmax * bmax * n * dTau, 10: mmax * n * dTau, 11: mmax * n * dTau, 12: mmax * n * dTau,
           15: bmax * n * dTau, 16: bmax * n * dTau, 17: bmax * n * dTau, 7: bmax * n * dTau, 8: bmax * n * dTau, 9: bmax * n * dTau}
    for q, (a, b) in enumerate(zip(got, ref)):
        tol = 1e-11 * max(abs(b), mag.get(q, 0.0))
        assert abs(a - b) <= tol, "history_turbulence column %d: device %r oracle %r tol %g" % (q, a, b, tol)


# ---- gates at the BASELINE sizes, for the exact library (equal bits) and for the tolerance-grade one (relative L2 < 1e-12) ----
OT_VARS = ["density", "energy", "mx", "my", "mz", "bx", "by", "bz"]


def orszag_tang_gate(lib, oracle, exact):
    """data/orszag-tang.ini as shipped (512^2, nstepmax = 50) against the oracle: north_star's gate, relative L2 < 1e-12 per
    variable; exact=True additionally demands every double and every dt equal.  Returns {variable: relative L2}."""
    p = lib.params_from_ini(ini("orszag-tang"))
    assert (p.nx, p.ny) == (512, 512)
    U0 = lib.init_condition(ini("orszag-tang"), "", p)
    ref, dts_ref, _ = oracle.run(p, U0, 50)
    sv = Solver(p, lib)
    try:
        dts = sv.start(U0, 50)
        got, ref = interior(sv.getDataHost(), p), interior(ref, p)
    finally:
        sv.close()
    errs = {}
    for v, name in enumerate(OT_VARS):
        errs[name] = float(rel_l2(got[v], ref[v]))
        assert errs[name] < L2_TOLERANCE, "Orszag-Tang %s: relative L2 %.3e" % (name, errs[name])
    if exact:
        assert np.array_equal(got, ref) and np.array_equal(np.array(dts), dts_ref)
    else:
        assert np.abs(np.array(dts) / dts_ref - 1.0).max() < 1e-11
    return errs


def divB_max(U, p):
    gw = p.ghostWidth
    bx, by, bz = U[5], U[6], U[7]
    s = (slice(gw, -gw),) * 3
    sx = (slice(gw, -gw), slice(gw, -gw), slice(gw + 1, -gw + 1 if gw > 1 else None))
    sy = (slice(gw, -gw), slice(gw + 1, -gw + 1 if gw > 1 else None), slice(gw, -gw))
    sz = (slice(gw + 1, -gw + 1 if gw > 1 else None), slice(gw, -gw), slice(gw, -gw))
    d = (bx[sx] - bx[s]) / p.dx + (by[sy] - by[s]) / p.dy + (bz[sz] - bz[s]) / p.dz
    return float(np.abs(d).max())


def mri_headline_size_properties(lib):
    """512^3 MRI (the bench workload): div B at round-off, mass conserved to round-off, finite fields"""
    ov = "mesh.nx=512;mesh.ny=512;mesh.nz=512"
    p = lib.params_from_ini(ini("mhd_mri_3d"), ov)
    U0 = lib.init_condition(ini("mhd_mri_3d"), ov, p)
    sv = Solver(p, lib)
    try:
        sv.start(U0, 0)
        A = sv.getDataHost()
        m0 = interior(A, p)[0].sum(dtype=np.longdouble)
        b_scale = float(np.abs(A[7]).max()) / p.dx
        d0 = divB_max(A, p)
        del U0, A
        for _ in range(3):
            sv.oneStepIntegration()
        B = sv.getDataHost()
    finally:
        sv.close()
    assert np.isfinite(B).all()
    m1 = interior(B, p)[0].sum(dtype=np.longdouble)
    assert abs(float((m1 - m0) / m0)) < 1e-13
    assert divB_max(B, p) <= max(d0, 1e-13 * b_scale) + 1e-12 * b_scale


def implode_bench_size_properties(lib):
    """256^3 implode, HLLC, reflecting walls: mass and energy conserved to round-off, x <-> y symmetry of the solution"""
    ov = "mesh.nx=256;mesh.ny=256;mesh.nz=256;hydro.riemannSolver=hllc"
    p = lib.params_from_ini(ini("implode3d"), ov)
    U0 = lib.init_condition(ini("implode3d"), ov, p)
    sv = Solver(p, lib)
    try:
        sv.start(U0, 5)
        A = interior(sv.getDataHost(), p)
    finally:
        sv.close()
    I0 = interior(U0, p)
    for v in (0, 1):
        a, b = A[v].sum(dtype=np.longdouble), I0[v].sum(dtype=np.longdouble)
        assert abs(float((a - b) / b)) < 1e-13
    # x <-> y transposition symmetry: density invariant, mx <-> my
    assert np.allclose(A[0], A[0].transpose(0, 2, 1), rtol=0, atol=1e-12)
    assert np.allclose(A[2], A[3].transpose(0, 2, 1), rtol=0, atol=1e-12)


def long_run_error_growth(lib, oracle, base, ov, nsteps, every):
    """relative L2 (all variables together) of `lib` against the oracle after every `every` steps of one run -- how round-off
    differences of the tolerance-grade arithmetic grow on a long run.  Returns [(step, relative L2, max |dt / dt_ref - 1|)]."""
    p = lib.params_from_ini(ini(base), ov)
    U0 = lib.init_condition(ini(base), ov, p)
    out = []
    sv = Solver(p, lib)
    try:
        sv.start(U0, 0)      # the init part of start(): ghost fill of the initial state, both arrays
        dts = []
        for n in range(1, nsteps + 1):
            dts.append(sv.oneStepIntegration())
            if n % every == 0 or n == nsteps:
                ref, dts_ref, _ = oracle.run(p, U0, n)
                got = interior(sv.getDataHost(), p)
                out.append((n, float(rel_l2(got, interior(ref, p))), float(np.abs(np.array(dts) / np.asarray(dts_ref)[:n] - 1.0).max())))
    finally:
        sv.close()
    return out


def check_public_ghost_fill_invalidates_fused_dt(lib, oracle, base, ov):
    """ADVICE (round 2): the step's last kernel leaves the CFL maximum of the new state in a device slot and the next compute_dt
    only reads it back.  A ghost fill called from OUTSIDE the step with a non-periodic MHD face overwrites the field the CT update
    left on the first high ghost face, which compute_dt_mhd reads: the slot is then stale.  After rgpu_make_all_boundaries the
    library must scan again -- the value must equal the oracle's compute_dt of the downloaded state -- and rgpu_invalidate_dt must
    do the same for a host program that wrote into the arrays itself."""
    p = lib.params_from_ini(ini(base), ov)
    U0 = lib.init_condition(ini(base), ov, p)
    sv = Solver(p, lib)
    try:
        sv.start(U0, 3)                               # three steps: the slot holds the scan of the state after step 3
        par = sv.nStep % 2
        sv.make_all_boundaries(par, sv.totalTime, 0.0)   # public ghost fill of the CURRENT state
        got = sv.compute_inv_dt(par)
        ref = oracle.compute_inv_dt(p, sv.getDataHost(par))
        assert got == ref, (got, ref)
        # rgpu_invalidate_dt (a host program that wrote into adopted arrays calls it): the next compute_dt scans again
        sv.oneStepIntegration()
        par = sv.nStep % 2
        ref = oracle.compute_inv_dt(p, sv.getDataHost(par))
        sv.enable_timers(True)
        sv.reset_timers()
        fused = sv.compute_inv_dt(par)                 # read back from the slot the update kernel filled: no scan kernel
        t_fused = sv.timers().get("dt", 0.0)
        assert lib.lib.rgpu_invalidate_dt(sv.ctx) == 0
        rescanned = sv.compute_inv_dt(par)
        t_scan = sv.timers().get("dt", 0.0)
        sv.enable_timers(False)
        assert fused == ref and rescanned == ref, (fused, rescanned, ref)
        if "emulation" not in lib.backend:             # (the emulation backend has no phase timers)
            assert t_fused == 0.0 and t_scan > 0.0, (t_fused, t_scan)
    finally:
        sv.close()



# ---- what a step leaves behind for the next one: the CFL scan in the device slots, the ghost images, rgpu_inv_dt_fusable ----------
# One rgpu_godunov_unsplit per case, then: does the next compute_dt scan, does the next step_pre fill ghosts (not on the rotating
# frame, where step_pre does nothing), and (3D) rgpu_inv_dt_fusable before and after the step.  Columns: scan -- the step's kernel
# leaves the CFL maxima of its output (both builds); images -- the tiled 2D kernel writes the output's ghost images (None: rotating
# frame); fusable -- (flat kernels, tiled kernels), None in 2D.
FUSED_BOOKKEEPING = [
    ("hydro2d-periodic", "kelvin_helmholtz_gpu_2d", "mesh.nx=24;mesh.ny=16", True, True, None),
    ("hydro2d-dirichlet", "hydro_sod2d", "mesh.nx=20;mesh.ny=16", True, True, None),
    ("hydro2d-jet", "jet2d_cpu", "mesh.nx=24;mesh.ny=16", True, False, None),
    ("hydro2d-gravity", "rayleigh_taylor_gpu_2d", "mesh.nx=16;mesh.ny=24", True, True, None),
    ("hydro2d-gravity-field", "Keplerian_disk2d", "mesh.nx=20;mesh.ny=20", True, False, None),
    ("mhd2d-periodic", "orszag-tang", "mesh.nx=24;mesh.ny=20", True, True, None),
    ("mhd2d-neumann", "mhd_BrioWu", "mesh.nx=24;mesh.ny=16", True, False, None),
    ("mhd2d-dirichlet", "orszag-tang", "mesh.nx=24;mesh.ny=20;mesh.boundary_xmin=1;mesh.boundary_xmax=1;mesh.boundary_ymin=1;mesh.boundary_ymax=1", True, False, None),
    # rotating frame: the reference scans the refilled ghosts, and the emf of the high x face carries another xPos than its periodic image's
    ("mhd2d-rotating", "mhd_inertialWave_2d", "mesh.nx=16;mesh.ny=16", False, None, None),
    ("mhd3d-rotating-periodic", "orszag-tang3d", "mesh.nx=8;mesh.ny=8;mesh.nz=8;MHD.omega0=0.3", False, None, (0, 0)),
    ("mhd2d-eta", "orszag-tang", "mesh.nx=24;mesh.ny=20;MHD.eta=0.01", False, False, None),
    ("hydro3d-implode", "implode3d", "mesh.nx=8;mesh.ny=8;mesh.nz=8", True, False, (0, 1)),
    ("hydro3d-gravity", "rayleigh_taylor_gpu_3d", "mesh.nx=8;mesh.ny=8;mesh.nz=12", True, False, (0, 1)),
    ("hydro3d-forcing", "turbulence_hydro", "mesh.nx=8;mesh.ny=8;mesh.nz=8", False, False, (0, 0)),
    ("mhd3d-orszag-tang", "orszag-tang3d", "mesh.nx=8;mesh.ny=8;mesh.nz=8", True, False, (1, 1)),
    ("mhd3d-mri", "mhd_mri_3d", "mesh.nx=8;mesh.ny=12;mesh.nz=8", True, None, (1, 1)),
    ("mhd3d-mri-gravity-field", "mhd_mri_3d", "mesh.nx=6;mesh.ny=8;mesh.nz=6;gravity.static=yes", False, None, (0, 0)),
    ("mhd3d-mri-open-z", "mhd_mri_3d", "mesh.nx=8;mesh.ny=12;mesh.nz=8;mesh.boundary_zmin=2;mesh.boundary_zmax=2", False, None, (0, 0)),
    ("mhd3d-nu", "orszag-tang3d", "mesh.nx=8;mesh.ny=8;mesh.nz=8;hydro.nu=0.005", False, False, (0, 0)),
    # the viscous stage rewrites the interior after the tiled 2D hydro kernel wrote the output's ghost images: the next step_pre must fill
    ("hydro2d-nu", "kelvin_helmholtz_gpu_2d", "mesh.nx=24;mesh.ny=16;hydro.nu=0.01", False, False, None),
]


def _host_state(lib, sv, parity):
    """emulation build: the "device" state is host memory, written here without telling the library"""
    import ctypes as C
    n = int(np.prod(sv.p.shape))
    return np.ctypeslib.as_array((C.c_double * n).from_address(lib.lib.rgpu_device_state(sv.ctx, parity))).reshape(tuple(sv.p.shape))


def check_fused_bookkeeping(lib, case):
    import os
    _, base, ov, scan, images, fusable = case
    emu = "emulation" in lib.backend
    tiled = not emu and os.environ.get("RGPU_TILED", "1").strip() != "0"
    p = lib.params_from_ini(ini(base), ov)
    U0 = lib.init_condition(ini(base), ov, p)
    rot = bool(p.mhdEnabled) and p.Omega0 > 0
    sv = Solver(p, lib)
    try:
        attach_gravity(lib, base, ov, p, sv)
        sv.start(U0, 0)
        before = lib.lib.rgpu_inv_dt_fusable(sv.ctx)
        dt = sv.compute_dt(0)
        sv.godunov_unsplit(0, dt, 0.0)
        after = lib.lib.rgpu_inv_dt_fusable(sv.ctx)
        gw = p.ghostWidth
        cell = (gw, gw, gw) if p.three_d else (0, gw, gw)
        ghost = (gw, gw, 0) if p.three_d else (0, gw, 0)
        if emu:
            # a fast cell in the new state: a scan sees it, a maximum left by the step's kernel does not
            U = _host_state(lib, sv, 1)
            saved = U[2][cell]
            U[2][cell] = 1e4 * U[0][cell]
            got = sv.compute_inv_dt(1)
            assert lib.lib.rgpu_invalidate_dt(sv.ctx) == 0
            fresh = sv.compute_inv_dt(1)
            U[2][cell] = saved
            assert lib.lib.rgpu_invalidate_dt(sv.ctx) == 0
            assert fresh > sv.compute_inv_dt(1)      # (the fast cell is visible)
            scans = got == fresh
            fills = None
            if not rot:
                U[0][ghost] = -12345.0
                sv.step_pre(1, dt, dt)
                fills = U[0][ghost] != -12345.0
        else:
            sv.enable_timers(True)
            sv.reset_timers()
            sv.compute_inv_dt(1)
            scans = sv.timers()["dt"] > 0.0
            sv.reset_timers()
            sv.step_pre(1, dt, dt)
            fills = None if rot else sv.timers()["boundaries"] > 0.0
            sv.enable_timers(False)
    finally:
        sv.close()
    want_fills = None if rot else not (images and tiled and lib.get_option("ghost_images") != 0)
    assert (scans, fills) == (not scan, want_fills), ("next compute_dt scans, next step_pre fills", (scans, fills), (not scan, want_fills))
    if p.three_d:
        assert before == after == fusable[1 if tiled else 0], ("rgpu_inv_dt_fusable before / after the first step", before, after)

# ---- the shared division / square root (rgpu_selftest_arith: rg_div(rg_recip), rg_sqrt; the compiler's "/" and sqrt) --------------
def arith_operands():
    """random operands over 2^+-400 (both signs) and edge operands: exact quotients, powers of two, near-ties, tiny / huge in range"""
    rng = np.random.RandomState(7)
    n = 1 << 20
    num = (rng.rand(n) + 0.5) * np.exp2(rng.randint(-400, 400, n)) * np.where(rng.rand(n) < 0.5, -1.0, 1.0)
    den = (rng.rand(n) + 0.5) * np.exp2(rng.randint(-400, 400, n)) * np.where(rng.rand(n) < 0.5, -1.0, 1.0)
    edge_n = np.array([1.0, 3.0, 1.0, 2.0, 10.0, 1e-300, 1e300, 7.0, 0.1, 5e-324 * 2 ** 60, 1.0 + 2 ** -52, 9.0, 1e200, 1e-200])
    edge_d = np.array([3.0, 1.0, 7.0, 2.0 ** 300, 0.1, 1e-10, 1e10, 7.0, 0.3, 3.0, 1.0 - 2 ** -53, 3.0, 1e-90, 1e95])
    num[:edge_n.size], den[:edge_d.size] = edge_n, edge_d
    return num, den


def selftest_arith(lib, num, den):
    """(rg_div(n, rg_recip(d)), n / d, rg_sqrt(n), sqrt(n)) on the device"""
    import ctypes as C
    n = num.size
    quot, quot2, root, root2 = (np.empty(n) for _ in range(4))
    P = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    lib.lib.rgpu_selftest_arith.restype = C.c_int
    lib.lib.rgpu_selftest_arith.argtypes = [C.c_int] + [C.POINTER(C.c_double)] * 6
    assert lib.lib.rgpu_selftest_arith(n, P(num), P(den), P(quot), P(quot2), P(root), P(root2)) == 0
    return quot, quot2, root, root2


def ulp_distance(got, want):
    """distance in units in the last place between finite doubles (the number of representable doubles between them)"""
    def key(x):
        i = x.view(np.int64)
        return np.where(i < 0, np.int64(-0x8000000000000000) - i, i)   # monotonic in the value, -0 == +0
    with np.errstate(over="ignore"):
        return np.abs(key(got) - key(want))


# ---- direct differential test of the Alfven selection in the 2D HLLD edge solver (rgpu_selftest_alfven) -------------------------
def alfven_samples(n, seed):
    """(kept for the last few (n, seed): the four parameter sets of the selection test run on the same samples; read-only)"""
    key = (int(n), int(seed))
    if key not in _ALFVEN_SAMPLES:
        while len(_ALFVEN_SAMPLES) >= 3:
            _ALFVEN_SAMPLES.pop(next(iter(_ALFVEN_SAMPLES)))
        S, kind = _alfven_samples(n, seed)
        S.flags.writeable = False
        kind.flags.writeable = False
        _ALFVEN_SAMPLES[key] = (S, kind)
    return _ALFVEN_SAMPLES[key]


_ALFVEN_SAMPLES = {}


def _alfven_samples(n, seed):
    """n edge problems (SoA [36, n]): half random rough states, half adversarial -- built to sit on the selection's margins:
      * dv / dS = 1 +- k 2^-52 (k <= 2^14): a uniform flow (the star ratio t = dv / dS is exactly 1) whose velocities are nudged
        by k ulp, so that candidates and their star partners tie, nearly tie, or differ by a hair more than the 2^-40 margin;
      * equal candidates (all four states identical, or pairwise identical);
      * |b| from 1e-120 to 1e3, density ratios 2^+-60 between the states;
      * the kinds interleaved lane by lane, so that a wave of 64 samples holds both routes."""
    rng = np.random.RandomState(seed)
    S = np.empty((36, n))
    kind = rng.randint(0, 8, n)                    # per LANE: neighbours in a wave differ
    # base: random states
    for q in range(4):
        S[8 * q + 0] = np.exp(rng.uniform(-2, 2, n))            # r
        S[8 * q + 1] = np.exp(rng.uniform(-3, 2, n))            # p
        S[8 * q + 2:8 * q + 5] = rng.normal(0, 1.5, (3, n))     # u v w
        S[8 * q + 5:8 * q + 8] = rng.normal(0, 1.0, (3, n))     # a b c
    uni = kind >= 2                                # adversarial kinds start from a uniform flow: copy state 0 into the others
    for q in range(1, 4):
        S[8 * q:8 * q + 8, uni] = S[0:8, uni]
    ulp = 2.0 ** -52
    k = np.floor(np.exp2(rng.uniform(0, 14, n))) * np.where(rng.rand(n) < 0.5, -1.0, 1.0)
    # kind 2: exactly uniform (every pair ties).  3: one velocity of one state nudged by k ulp.  4: all velocities of two states nudged
    m = kind == 3
    q3 = rng.randint(0, 4, n); c3 = rng.randint(2, 4, n)
    for q in range(4):
        for c in (2, 3):
            sel = m & (q3 == q) & (c3 == c)
            S[8 * q + c, sel] *= 1.0 + k[sel] * ulp
    m = kind == 4
    for q in (1, 2):
        for c in (2, 3):
            S[8 * q + c, m] *= 1.0 + k[m] * ulp * (1 if q == 1 else -1)
    # kind 5: pairwise identical states (LL == LR, RL == RR) with a k-ulp density nudge across the pair
    m = kind == 5
    S[8:16, m] = S[0:8, m] * 1.0
    S[8:9, m] *= 1.0 + k[m] * ulp
    S[16:24, m] = S[0:8, m]
    S[24:32, m] = S[8:16, m]
    # kind 6: field scaled over 1e-120 .. 1e3 (all states alike, so that candidates stay comparable), velocities nudged
    m = kind == 6
    scale = np.exp(rng.uniform(np.log(1e-120), np.log(1e3), n))
    for q in range(4):
        S[8 * q + 5:8 * q + 8, m] *= scale[m]
        S[8 * q + 2, m] *= 1.0 + (q - 1.5) * k[m] * ulp
    # kind 7: density ratios 2^+-60 between the states (pressure follows, so that sound speeds stay finite), random fields
    m = kind == 7
    for q in range(1, 4):
        e = rng.randint(-60, 61, n).astype(float)
        S[8 * q + 0, m] = S[0, m] * np.exp2(e[m])
        S[8 * q + 1, m] = S[1, m] * np.exp2(e[m])
        S[8 * q + 5:8 * q + 8, m] = rng.normal(0, 1.0, (3, int(m.sum())))
    # kind 1 (random): field scale over a wide range too
    m = kind == 1
    scale = np.exp(rng.uniform(np.log(1e-120), np.log(1e3), n))
    for q in range(4):
        S[8 * q + 5:8 * q + 8, m] *= scale[m]
    # electric fields of the corner states, E = u b - v a (riemann_mhd.h:1115-1140)
    for q in range(4):
        S[32 + q] = S[8 * q + 2] * S[8 * q + 6] - S[8 * q + 3] * S[8 * q + 5]
    return np.ascontiguousarray(S), kind


def check_alfven_selftest(lib, n, seed, smallc, iso=False):
    """e_select == e_reference, bit for bit; returns (waves on the selection route, waves on the reference route)"""
    import ctypes as C
    from conftest import ini
    p = lib.params_from_ini(ini("mhd_mri_3d" if iso else "orszag-tang3d"), "mesh.nx=8;mesh.ny=8;mesh.nz=8")
    p.smallc = smallc
    S, kind = alfven_samples(n, seed)
    e_sel, e_ref = np.empty(n), np.empty(n)
    route = np.empty(n, dtype=np.int32)
    f = lib.lib.rgpu_selftest_alfven
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int)]
    P = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    rc = f(C.byref(p), n, P(S), P(e_sel), P(e_ref), route.ctypes.data_as(C.POINTER(C.c_int)))
    assert rc == 0, rc
    a, b = e_sel.view(np.uint64), e_ref.view(np.uint64)
    bad = (a != b) & ~(np.isnan(e_sel) & np.isnan(e_ref))
    assert not bad.any(), "%d of %d edge problems differ between the selection and the reference's sequence; first: sample %d kind %d: %r vs %r" % (
        int(bad.sum()), n, int(np.argmax(bad)), int(kind[np.argmax(bad)]), e_sel[np.argmax(bad)], e_ref[np.argmax(bad)])
    assert np.isfinite(e_ref).mean() > 0.9, "the samples are mostly not finite: %r" % np.isfinite(e_ref).mean()
    return int((route == 0).sum()), int((route == 1).sum()), kind, route


def check_fused_fill(lib, oracle, base, ov, seed=5, t0=3.7, dt=0.9):
    """rgpu_step_fill_planes_pair (one launch for x and y faces / the shearing-box remap, corners included, two plane ranges) against the
    oracle's separate passes -- X then Y, or the whole shearing-box sequence Y, shear, Z, Y -- on a random state: every ghost cell of the
    planes asked for equal, every other plane untouched"""
    p = lib.params_from_ini(ini(base), ov)
    U = random_state(p, seed)
    gw, ks = p.ghostWidth, p.nz + 2 * p.ghostWidth
    ref = U.copy()
    shear = bool(p.shearingBoxEnabled)
    if shear:
        oracle.make_all_boundaries(p, ref, t0, dt)
    else:
        oracle.make_boundaries(p, ref, 1)
        oracle.make_boundaries(p, ref, 2)
    r1, r2 = (gw, 2 * gw), (p.nz, p.nz + gw)            # the planes a slab sends
    if r2[0] < r1[1]:
        r1, r2 = (gw, p.nz + gw), (0, 0)
    sv = Solver(p, lib)
    try:
        sv.upload(U, both=True)
        sv.step_fill_planes_pair(1, dt, t0, r1, r2)      # step 1 writes U[0]
        got = sv.getDataHost(0)
        planes = list(range(*r1)) + list(range(*r2))
        for k in range(ks):
            if k in planes:
                assert np.array_equal(got[:, k], ref[:, k]), "%s: plane %d differs from the separate passes in %d doubles" % (base, k, int((got[:, k] != ref[:, k]).sum()))
            else:
                assert np.array_equal(got[:, k], U[:, k]), "%s: plane %d outside the ranges was touched" % (base, k)
        sv.upload(U, both=True)                          # one range, all interior planes
        sv.step_fill_planes_pair(1, dt, t0, (gw, ks - gw), (0, 0))
        got = sv.getDataHost(0)
        assert np.array_equal(got[:, gw:ks - gw], ref[:, gw:ks - gw])
    finally:
        sv.close()


# ---- 4. a step of any size against the oracle, z window by z window ----------------------------------------------------------
# A cell's new value depends only on the planes within ghostWidth of it.  So one step of a box too large for a single oracle call
# is checked in z windows: each window is the window's planes plus ghostWidth planes of the box on each side, cut from the state
# the step starts from, and orc_godunov_unsplit_zwindow steps it without refilling those z ghost planes.  Stitched together, the
# windows are the whole-box step, every double (tests/test_zwindow_oracle.py).

def zwindow(p, U, k0, w):
    """(params, state) of the z window of interior planes [k0, k0 + w) of the ghost-inclusive 3D state U: a copy of p with nz = w and
    zMin / zMax moved by k0 dz (nz_global stays the box's, so that a window of one plane is still a 3D step), and planes
    k0 .. k0 + w + 2 gw of U with all of x and y"""
    assert p.three_d and 0 <= k0 and w >= 1 and k0 + w <= p.nz, (k0, w, p.nz)
    q = type(p).from_buffer_copy(p)
    q.nz = w
    q.zMin = p.zMin + k0 * p.dz
    q.zMax = p.zMin + (k0 + w) * p.dz
    return q, np.ascontiguousarray(U[:, k0:k0 + w + 2 * p.ghostWidth])


def window_threads(oracle, q):
    """threads of one window's oracle step: Oracle._mt_threads (up to 16, the threaded 3D MHD step's scope), 1 outside it"""
    return max(1, oracle._mt_threads(q))


def step_in_windows(oracle, p, U, dt, t, widths, nthreads=None):
    """yields (k0, w, Unew of the window) for the windows of `widths` (a partition of [0, nz)), one after another: the oracle's
    global state is not proven thread-safe.  nthreads None: window_threads per window"""
    assert sum(widths) == p.nz and min(widths) >= 1, (widths, p.nz)
    k0 = 0
    try:
        for w in widths:
            q, Uw = zwindow(p, U, k0, w)
            nt = window_threads(oracle, q) if nthreads is None else nthreads
            out = oracle.godunov_unsplit_zwindow(q, Uw, dt, t, nt)
            del Uw
            yield k0, w, out
            k0 += w
    finally:
        oracle.release_zwindow()


WINDOW_SCRATCH = 24e9   # bytes of host scratch for one window's threaded oracle step (MtWork + the window's copies)


def window_widths(p, scratch=WINDOW_SCRATCH):
    """a partition of [0, nz) into near-equal windows whose oracle step stays within `scratch` bytes: MtWork's 182 doubles per cell
    plus the window's input and output, over w + 2 gw planes"""
    plane = (p.nx + 2 * p.ghostWidth) * (p.ny + 2 * p.ghostWidth)
    per_cell = 8 * (182 + 2 * p.nbVar)
    wmax = max(1, int(scratch // (per_cell * plane)) - 2 * p.ghostWidth)
    n = -(-p.nz // wmax)
    return [p.nz * (i + 1) // n - p.nz * i // n for i in range(n)]


def _mirror_tile_grid_plan(nbx, nby, span, slots, min_planes, fill):
    """tile_grid_plan of hip/tiled_hydro.h (one range, no RGPU_ZSEG): (nseg, ipx, full, tail)"""
    tiles = nbx * nby
    best_n, best_tail, best = 1, 1, 1e300
    nmax = 1 if span // min_planes < 1 else min(span // min_planes, 64)
    for n in range(1, nmax + 1):
        items = tiles * n
        ipx = (items + 7) // 8
        full = (ipx // slots) * slots
        rem = ipx - full
        ln = span / n
        tail = 1
        if rem > 0:
            tail = max(1, min(slots // rem, int(ln / min_planes)))
        t = (full // slots) * (ln + fill) + ((ln / tail + fill) * ((rem * tail + slots - 1) // slots) if rem > 0 else 0.0)
        if t < best * 0.995:
            best, best_n, best_tail = t, n, tail
    nseg = max(1, min(best_n, span))
    ipx = (tiles * nseg + 7) // 8
    full = (ipx // slots) * slots
    return nseg, ipx, full, (best_tail if ipx - full > 0 else 1)


def _segment_starts(nbx, nby, za, span, slots, min_planes, fill):
    """the first plane of every z segment and last-round sub-segment of one launch (tile_item of hip/tiled_hydro.h)"""
    nseg, ipx, full, tail = _mirror_tile_grid_plan(nbx, nby, span, slots, min_planes, fill)
    tiles = nbx * nby
    starts = set()
    for xcd in range(8):
        for item in range(xcd * ipx, min((xcd + 1) * ipx, tiles * nseg)):
            seg = item // tiles
            a0 = za + span * seg // nseg
            b0 = za + span * (seg + 1) // nseg
            nsub = tail if item - xcd * ipx >= full else 1
            starts.update(a0 + (b0 - a0) * s // nsub for s in range(nsub))
    return nseg, tail, sorted(starts)


def sweep_plan_facts(p):
    """{launch: (segments, last-round split, [first plane of each segment, ghost-inclusive])} of one whole-box step: the tiled 3D MHD
    sweep (MhMain and, without a periodic x image, MhLastX; hip/tiled_mhd.h launch_mhd3d_sweep) and the 3-plane update, or the tiled 3D
    hydro sweep (launch_hydro3d_sweep), at the default options"""
    gw, isz, jsz, ks = p.ghostWidth, p.nx + 2 * p.ghostWidth, p.ny + 2 * p.ghostWidth, p.nz + 2 * p.ghostWidth
    out = {}
    if not p.mhdEnabled:
        nbx, nby = (isz - 1 + 13) // 14, (jsz - 1 + 13) // 14
        nseg, tail, st = _segment_starts(nbx, nby, gw, ks - 2 * gw, 64, 12, 2)
        out["hydro3d_sweep"] = (nseg, tail, st)
        return out
    rot = p.Omega0 > 0
    periodic = 3                                             # RGPU_BC_PERIODIC, include/rgpu.h
    per = [p.bc[2 * d] == periodic and p.bc[2 * d + 1] == periodic for d in range(2)]
    copy_x = per[0] and not rot and p.nx % 16 == 0 and p.nx >= 16
    copy_y = per[1] and p.ny % 8 == 0 and p.ny >= 8
    nbx = (isz - 2 * gw + 1 + 15) // 16 - (1 if copy_x else 0)
    nby = (jsz - 2 * gw + 1 + 7) // 8 - (1 if copy_y else 0)
    lastx = not copy_x and p.nx % 16 == 0 and nbx >= 2
    if lastx:
        nbx -= 1
    span = ks - 2 * gw + 1                                   # the Riemann planes gw .. ksize - gw
    out["mhd3d_sweep MhMain"] = _segment_starts(nbx, nby, gw, span, 32, 8, 2)
    if lastx:
        out["mhd3d_sweep MhLastX"] = _segment_starts(1, (jsz - 2 * gw + (0 if copy_y else 1) + 31) // 32, gw, span, 32, 8, 2)
    out["mhd3d update"] = (-(-ks // 3), 1, list(range(0, ks, 3)))
    return out


def offset_crossing_planes(p):
    """[(array, what, component, plane)] of the device layout (api/ctx.h fill_dev_params): the planes (ghost-inclusive) where an
    element index of U, F or emf crosses 2^31, and where its byte offset crosses each power of two from 2^32 up"""
    gw, isz, jsz, ks = p.ghostWidth, p.nx + 2 * p.ghostWidth, p.ny + 2 * p.ghostWidth, p.nz + 2 * p.ghostWidth
    ncell, sk = isz * jsz * ks, isz * jsz
    arrays = [("U", p.nbVar, ncell, 0, sk)]
    if p.mhdEnabled:
        fsj = (isz + 15) // 16 * 16
        foff = (16 - gw % 16) % 16
        fsk = fsj * jsz
        fN = (fsk * ks + foff + 15) & ~15
        arrays += [("F", 15, fN, foff, fsk), ("emf", 3, fN, foff, fsk)]
    out = []
    for name, ncomp, pitch, off, kstride in arrays:
        total = ncomp * pitch
        lines = [("2^31 elements", 2 ** 31)] + [("2^%d bytes" % b, 2 ** (b - 3)) for b in range(32, 64) if 2 ** (b - 3) < total]
        for what, e in lines:
            if e >= total:
                continue
            v, r = divmod(e, pitch)
            k = min(max((r - off) // kstride, 0), ks - 1)
            out.append((name, what, v, k))
    return out


def _first_diff(got, ref, k_first, interior_xy, gw):
    """(v, k, j, i) of the first differing double, ghost-inclusive indices of the box"""
    v, k, j, i = (int(x[0]) for x in np.nonzero(got != ref))
    return (v, k + k_first, j + (gw if interior_xy else 0), i + (gw if interior_xy else 0))


def check_step_in_windows(lib, oracle, base, ov, K, exact, widths=None):
    """one step of a box of any size against the oracle, window by window: the step after K steps of the bench's path.
      A: start(U0, 0) + run_steps(K) (time step on the device, fused CFL scan): U_K with its ghosts, t_K and the last dt.
      B: a fresh context from the same U0, run_steps(K + 1) in one call: U_{K+1} and dt_{K+1}.  One context open at a time.
      dt_{K+1} == the oracle's compute_dt of U_K as downloaded (contracted: relative difference < 1e-12).
      U_K's ghosts: rotating path, equal to the oracle's make_all_boundaries of U_K with step K's own arguments (the device's end-of-step
      fill, shear remap included); plain path, filled by the oracle as the device step does at its start.
      Windows (window_widths, or `widths`) tile [0, nz); each is stepped by the oracle with dt_{K+1}, t_K.  Compared: the window's planes
      over all of x and y (rotating path: with the x / y ghost columns).  exact: every double; otherwise the specific-form relative L2
      per variable over the whole box < L2_TOLERANCE.
      Every offset-crossing plane (offset_crossing_planes) and every segment start of the sweep launches (sweep_plan_facts) lies inside
      a compared window.  Returns a dict of facts (also printed)."""
    import resource
    import time
    t_start = time.time()
    p = lib.params_from_ini(ini(base), ov)
    assert p.three_d
    gw, nz = p.ghostWidth, p.nz
    rot = bool(p.mhdEnabled) and p.Omega0 > 0
    what = "%s [%s], %s library, step %d" % (base, ov, lib.arithmetic, K + 1)
    U0 = lib.init_condition(ini(base), ov, p)
    sv = Solver(p, lib)
    try:
        sv.start(U0, 0)
        assert sv.run_steps(K) == K
        dts_a, t_K = list(sv.dt_log), sv.totalTime
        UK = sv.getDataHost()
    finally:
        sv.close()
    sv = Solver(p, lib)
    try:
        sv.start(U0, 0)
        del U0
        assert sv.run_steps(K + 1) == K + 1
        dts_b = list(sv.dt_log)
        UK1 = sv.getDataHost()
    finally:
        sv.close()
    t_gpu = time.time() - t_start
    assert dts_b[:K] == dts_a, (what, dts_a, dts_b)
    t = 0.0
    for d in dts_a[:-1]:
        t += d                                               # the oracle's loop: t at the start of step K
    t_prev = t
    t += dts_a[-1]
    assert t == t_K, (what, t, t_K)
    dt1 = dts_b[K]
    dt_ref = oracle.compute_dt(p, UK)
    if exact:
        assert dt1 == dt_ref, "%s: dt %r, the oracle's on U_K %r" % (what, dt1, dt_ref)
    else:
        assert abs(dt1 / dt_ref - 1.0) < 1e-12, "%s: dt %r, the oracle's on U_K %r" % (what, dt1, dt_ref)
    # ghosts of U_K
    if rot:
        regions = [(slice(None), slice(0, gw)), (slice(None), slice(-gw, None)),
                   (slice(None), slice(gw, -gw), slice(0, gw)), (slice(None), slice(gw, -gw), slice(-gw, None)),
                   (slice(None), slice(gw, -gw), slice(gw, -gw), slice(0, gw)), (slice(None), slice(gw, -gw), slice(gw, -gw), slice(-gw, None))]
        dev = [UK[r].copy() for r in regions]
        oracle.make_all_boundaries(p, UK, t_prev, dts_a[-1])
        for r, g in zip(regions, dev):
            ref = UK[r]
            if exact:
                nbad = int((g != ref).sum())
                assert nbad == 0, "%s: %d of %d ghost doubles of U_K differ from the oracle's fill %r" % (what, nbad, ref.size, r)
            else:
                assert_close_specific(g, ref, p, what + ": ghosts of U_K %r" % (r,), rho=np.maximum(np.abs(ref[0]), p.smallr))
        del dev
    else:
        oracle.make_all_boundaries(p, UK, 0.0, 0.0)
    # windows
    widths = window_widths(p) if widths is None else widths
    t_orc = time.time()
    num = np.zeros(p.nbVar)
    den = np.zeros(p.nbVar)
    worst = (-1.0, None)
    nbad_total, first = 0, None
    for k0, w, out in step_in_windows(oracle, p, UK, dt1, t_K, widths):
        got = UK1[:, gw + k0:gw + k0 + w]
        ref = out[:, gw:gw + w]
        xy = (slice(None), slice(None)) if rot else (slice(gw, -gw), slice(gw, -gw))
        got, ref = got[(slice(None), slice(None)) + xy], ref[(slice(None), slice(None)) + xy]
        assert np.isfinite(got).all(), "%s: non-finite values in planes %d .. %d" % (what, k0, k0 + w - 1)
        if exact:
            ne = got != ref
            nb = int(ne.sum())
            if nb and first is None:
                first = _first_diff(got, ref, gw + k0, not rot, gw)
            nbad_total += nb
        else:
            r = _flux_partner_density(p, out[0])[(slice(gw, gw + w),) + xy]
            wl2 = 0.0
            for v in range(p.nbVar):
                s = 1.0 if v == 0 else (1.0 / np.sqrt(r) if v >= 5 else 1.0 / r)
                d = (got[v] - ref[v]) * s
                a = ref[v] * s
                dn, dd = float((d * d).sum()), float((a * a).sum())
                num[v] += dn
                den[v] += dd
                wl2 = max(wl2, np.sqrt(dn / dd) if dd > 0 else np.sqrt(dn))
            if wl2 > worst[0]:
                worst = (wl2, (k0, w))
        del out, got, ref
    t_orc = time.time() - t_orc
    names = OT_VARS if p.nbVar == 8 else ("density", "energy", "mx", "my", "mz")
    facts = {"case": what, "windows": widths, "gpu_s": round(t_gpu, 1), "oracle_s": round(t_orc, 1), "dt": dt1}
    if exact:
        assert nbad_total == 0, "%s: %d of %d compared doubles differ from the oracle; first at (v, k, j, i) = %r" % (
            what, nbad_total, p.nbVar * nz * (UK1.shape[2] if rot else p.ny) * (UK1.shape[3] if rot else p.nx), first)
    else:
        errs = {names[v]: float(np.sqrt(num[v] / den[v])) if den[v] > 0 else float(np.sqrt(num[v])) for v in range(p.nbVar)}
        facts["rel_l2_specific"] = errs
        facts["worst_window"] = {"planes": worst[1], "rel_l2": worst[0]}
        bad = {k: e for k, e in errs.items() if not e < L2_TOLERANCE}
        assert not bad, "%s: specific-form relative L2 above %.0e: %s" % (what, L2_TOLERANCE, bad)
    # the planes that matter at this size lie inside compared windows
    starts = np.cumsum([0] + list(widths[:-1]))
    covered = lambda k: any(s <= k - gw < s + w for s, w in zip(starts, widths))   # noqa: E731
    nearest = lambda k: min(max(k, gw), gw + nz - 1)                               # a ghost plane: the interior plane that reads it
    cross = offset_crossing_planes(p)
    plan = sweep_plan_facts(p)
    for a, line, v, k in cross:
        assert covered(nearest(k)), (what, a, line, v, k)
    for launch, (nseg, tail, st) in plan.items():
        for k in st:
            assert covered(nearest(k)), (what, launch, k)
    facts["offset_crossings"] = ["%s %s: component %d, plane %d" % c for c in cross]
    facts["segments"] = {k: {"segments": v[0], "last_round_split": v[1], "starts": v[2] if len(v[2]) <= 40 else v[2][:20] + ["..."] + v[2][-5:]}
                         for k, v in plan.items()}
    facts["wall_s"] = round(time.time() - t_start, 1)
    facts["peak_rss_gb"] = round(resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1e6, 1)   # of the process so far
    print("step in windows:", facts)
    return facts
