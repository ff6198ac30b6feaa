"""The shearing box at every phase of its shift: checks and case lists shared by the CPU emulation tests (tests/test_shear_phase_emu.py)
and the GPU ones (tests/test_shear_phase_gpu.py).

Each step of the rotating shearing box consumes two time-dependent row offsets, both from
    deltay = fmod(1.5 Omega0 xlen t, ylen),  jplus = (int)(deltay / dy),  eps = fmod(deltay, dy) / dy
-- the flux / emf remap at t + dt/2 and the x-ghost remap at t + dt -- and that arithmetic is written out on the host (api/step_mhd.h:
shear_remap_at; api/boundaries.h twice), on the device (step_clock_rec.h: step_clock_form, read by the kernels of a device-clock batch) and in the slab
driver's clock; the consumers index rows with a periodic wrap.  An off-by-one row, a wrong wrap or a device / host fmod mismatch shows
only where jplus is near ny - 1, where the fmod(., ylen) wrap falls between t + dt/2 and t + dt, or where a batch starts at t != 0.
So the runs here are PLANTED: t0 is chosen from the oracle's own dt sequence so that the K steps have a named property (PLANTS), the
property is recomputed from the oracle loop (PlantError otherwise: a plant that has gone soft fails loudly), and the states vary at O(1)
from row to row (parity_checks.stress_state), which `sensitivity` proves on the oracle alone: its ghost fill one row further differs
in the x-ghost columns by a relative L2 of at least 1e6 x the tolerance applied -- "within tolerance" then means "the right row".

  phase(p, t)        (jplus, eps_max) of the shift at time t, a numpy / math.fmod restatement in the expression order of step_clock_form.
                     Used to plant and to assert what a case claims, never as the expected value of the product: that is the oracle
  reference(...)     the oracle loop from t0 (compute_dt / godunov_unsplit after make_all_boundaries(t0, 0)): times, dts, states, the
                     planted step; with the plant's property and the sensitivity condition checked
  check_fills        1. the public ghost fills at (t0, 0) and at every (t, dt) of the sequence, input ghosts poisoned with NaN
  check_single_steps 2. one godunov_unsplit(0, dt, t) at every step time of the sequence
  check_step_loop    3. K x oneStepIntegration from t0 (offsets formed on the host)
  check_run_steps    4. run_steps(K) from t0 (offsets formed on the device): whole, in pieces that begin a batch on the planted step, and
                        with tEnd inside the step after it
  check_options      5. run_steps(K) under a diagnostic option == the default run, bit for bit

Bars: the exact library and the emulation equal the oracle to the bit, ghosts included (parity_checks.assert_same on the whole array:
the rotating path defines the output's ghosts); the contracted library within parity_checks.L2_TOLERANCE per variable in specific form
(parity_checks.assert_close_specific), its dts within the relative 1e-11 of parity_checks.check_run_vs_oracle."""
import collections
import math
import os

import numpy as np

import parity_checks as pc
from conftest import ini
from ramsesgpu_amd.solver import Solver, interior

BASE = "mhd_mri_3d"
DT_RTOL = 1e-11          # the contracted library's dt against the oracle's (parity_checks.check_run_vs_oracle)
SENSITIVITY = 1e6        # the oracle's fill one row further differs by at least this many times the tolerance applied
IA = 5                   # Bx (dev_numerics.h)
INF = float("inf")


class PlantError(AssertionError):
    """the generator's own claim does not hold (the sequence lacks the plant's property, or the state cannot tell rows apart): never a pass"""


# ---- shapes: the smallest that still hold every seam of the 16 x 8 MhMain tiles (hip/tiled_mhd.h) ------------------------------------
SHAPES = {
    # nx % 16 == 0: the last face column in MhLastX; ny % 8 == 0: the y layer copied from its image
    "16x8x8": ("mesh.nx=16;mesh.ny=8;mesh.nz=8", 2),
    # partial last tiles in x and y, the y layer not copied
    "24x20x10": ("mesh.nx=24;mesh.ny=20;mesh.nz=10", 1),
    # two tile columns and three tile rows: a shifted source row lies in another tile row than its target
    "32x24x9": ("mesh.nx=32;mesh.ny=24;mesh.nz=9", 2),
    # fewer rows than a tile, nx < 16
    "8x12x6": ("mesh.nx=8;mesh.ny=12;mesh.nz=6", 1),
}
# slope types 1 and 2 only: the ghost-remap slopes exist for those alone (kernels_bc.h: shear_border_slope)

PLANTS = ("start", "last-row", "cell-crossing", "exact-cell", "late", "fast")
K_STEPS = {"fast": 14}   # 6 for all others
Case = collections.namedtuple("Case", "shape family plant")     # family: a parity_checks.stress_state family, or "initial"

STATE_CASES = [("16x8x8", "rough"), ("24x20x10", "rough"), ("32x24x9", "rough"), ("8x12x6", "rough"),
               ("16x8x8", "contrast"), ("32x24x9", "contrast"), ("24x20x10", "floor")]
# the MRI initial condition is uniform in y up to its perturbation (a wrong row would move perturbation-size numbers only): used where
# the plant needs the dt of the smooth problem -- `late` on every shape; `fast` where 14 steps can visit every row (ny = 8)
CASES = ([Case(s, f, pl) for s, f in STATE_CASES for pl in ("start", "last-row", "cell-crossing", "exact-cell")]
         + [Case(s, "initial", "late") for s in SHAPES] + [Case("16x8x8", "initial", "fast")])
GOLDEN_FAST = "mri_16x8x8_fastshear"      # the same run as CASES[-1], written by the reference binary itself
# check 5
OPTION_CASES = [Case("32x24x9", "rough", "last-row"), Case("32x24x9", "initial", "fast"), Case("16x8x8", "initial", "fast")]
OPTIONS = [("spec", 0), ("ghost_images", 0), ("step_clock", 0), ("zseg", 3)]


def case_id(c):
    return "%s-%s-%s" % (c.plant, c.shape, c.family)


def steps_of(case):
    return K_STEPS.get(case.plant, 6)


def case_ov(case):
    """the overrides of a case: the shape, its slope type, and the rotation rate (and box length) the plant needs"""
    ov, slope = SHAPES[case.shape]
    ov += ";hydro.slope_type=%.1f" % slope
    ny = int(ov.split("mesh.ny=")[1].split(";")[0])
    if case.plant in ("start", "last-row", "cell-crossing"):
        ov += ";MHD.omega0=0.3"
    elif case.plant == "exact-cell":
        # 1.5 Omega0 xlen = 0.375 and dy = 0.25 are dyadic: deltay can be an exact multiple of dy beyond a wrap of ylen = ny / 4
        ov += ";MHD.omega0=0.25;mesh.ymin=%r;mesh.ymax=%r" % (-ny / 8.0, ny / 8.0)
    elif case.plant == "late":
        ov += ";MRI.amp=0.3"                     # Omega0 as shipped
    elif case.plant == "fast":
        ov += ";MHD.omega0=1.0;MRI.amp=0.3"
    else:
        raise ValueError(case.plant)
    return ov


# ---- the shift -------------------------------------------------------------------------------------------------------------------
def shift_rate(p):
    return 1.5 * p.Omega0 * (p.dx * p.nx)


def raw_shift(p, t):
    """1.5 Omega0 xlen t, before the wrap"""
    return shift_rate(p) * t


def phase(p, t):
    """(jplus, eps_max) at time t, in the expression order of step_clock_form (xlen = dx * nx, ylen = dy * ny)"""
    xlen, ylen = p.dx * p.nx, p.dy * p.ny
    deltay = 1.5 * p.Omega0 * xlen * t
    deltay = math.fmod(deltay, ylen)
    jplus = int(deltay / p.dy)
    epsi = math.fmod(deltay, p.dy)
    return jplus, epsi / p.dy


def step_phases(p, t, dt):
    """(remap jplus at t + dt/2, ghost jplus at t + dt) of one step"""
    return phase(p, t + dt / 2)[0], phase(p, t + dt)[0]


# ---- the oracle loop ---------------------------------------------------------------------------------------------------------------
def oracle_loop(oracle, p, U, t0, K, tEnd=INF):
    """the reference's loop from t0: (ts[0 .. n], dts[0 .. n - 1], states[0 .. n]); states[0] is U with its ghosts filled at (t0, 0)"""
    F = U.copy()
    oracle.make_all_boundaries(p, F, t0, 0.0)
    ts, dts, states = [t0], [], [F]
    t = t0
    while len(dts) < K and t < tEnd:
        dt = oracle.compute_dt(p, states[-1])
        states.append(oracle.godunov_unsplit(p, states[-1].copy(), dt, t))
        t += dt
        dts.append(dt)
        ts.append(t)
    return ts, dts, states


def sensitivity(oracle, p, U, t0):
    """relative L2, in the x-ghost columns, between the oracle's ghost fill at t0 and at the time the shift is one row further"""
    A, B = U.copy(), U.copy()
    oracle.make_all_boundaries(p, A, t0, 0.0)
    oracle.make_all_boundaries(p, B, t0 + p.dy / shift_rate(p), 0.0)
    gw = p.ghostWidth
    cols = list(range(gw)) + list(range(p.nx + gw, p.nx + 2 * gw))
    return float(pc.rel_l2(B[..., cols], A[..., cols]))


def _find_step(p, ts, dts, want):
    for n in range(1, len(dts)):                         # not the first step of the batch
        if want(*step_phases(p, ts[n], dts[n])):
            return n
    return None


def _planted_sequence(oracle, p, U, K, target, want, what):
    """t0 such that the shift passes `target` between t + dt/2 and t + dt of a step n >= 1 of the oracle's loop, by fixed-point
    iteration on the oracle's own dts (the first guess uses dt0 = compute_dt of the state alone); n <= K - 3, so that the step after
    it and one more lie inside the K steps"""
    tstar = target / shift_rate(p)
    F = U.copy()
    oracle.make_all_boundaries(p, F, 0.0, 0.0)
    dt0 = oracle.compute_dt(p, F)
    n = 2
    t0 = tstar - (n + 0.75) * dt0
    for _ in range(6):
        if not t0 >= 0:
            break
        ts, dts, states = oracle_loop(oracle, p, U, t0, K)
        m = _find_step(p, ts, dts, want)
        if m is not None and 1 <= m <= K - 3:
            return t0, ts, dts, states, m
        t0 = tstar - math.fsum(dts[:n]) - 0.75 * dts[n]
    raise PlantError("%s: no t0 found whose oracle sequence has the property (last try t0 = %r)" % (what, t0))


Ref = collections.namedtuple("Ref", "case ov p U t0 ts dts states planted phases sens singles")
_REFS = collections.OrderedDict()     # the last cases' references: the checks of a case and both libraries run in a row; read-only


def reference(lib, oracle, case):
    """the oracle's run of a case with the generator's proofs (PlantError otherwise).  lib: any library (parameters, initial condition)"""
    if case in _REFS:
        return _REFS[case]
    ov = case_ov(case)
    K = steps_of(case)
    p = lib.params_from_ini(ini(BASE), ov)
    what = "%s [%s]" % (case_id(case), ov)
    assert p.shearingBoxEnabled and p.Omega0 > 0 and p.slope_type in (1, 2), what
    U = lib.init_condition(ini(BASE), ov, p) if case.family == "initial" else pc.stress_state(p, 3, case.family)
    ny, ylen = p.ny, p.dy * p.ny
    plant = case.plant
    if plant == "start":
        t0, planted = 0.0, K // 2
        j, eps = phase(p, t0 + 0.0)
        if not (j == 0 and eps == 0.0 and 1.0 - eps == 1.0):
            raise PlantError("%s: the fill at (0, 0) has jplus %d eps_max %r" % (what, j, eps))
    elif plant == "last-row":
        # the fmod(., ylen) wrap between t + dt/2 and t + dt
        seq = _planted_sequence(oracle, p, U, K, ylen, lambda r, g: r == ny - 1 and g == 0, what)
    elif plant == "cell-crossing":
        jstar = ny // 2
        seq = _planted_sequence(oracle, p, U, K, jstar * p.dy, lambda r, g: g == r + 1 and 0 < r < ny - 2, what)
    elif plant == "exact-cell":
        t0, planted = None, K // 2
        s = shift_rate(p)
        for m in (1, 2, 3):
            for j in range(1, ny - 1):
                x = m * ylen + j * p.dy
                t = x / s
                if s * t == x and math.fmod(math.fmod(x, ylen), p.dy) == 0.0 and t0 is None:
                    t0 = t
        if t0 is None:
            raise PlantError("%s: no t0 with deltay an exact multiple of dy" % what)
        j, eps = phase(p, t0)
        if not (eps == 0.0 and 0 < j < ny - 1 and raw_shift(p, t0) > ylen):
            raise PlantError("%s: at t0 = %r jplus %d eps_max %r raw shift %r" % (what, t0, j, eps, raw_shift(p, t0)))
    elif plant == "late":
        t0, planted = 600000.0, K // 2        # the shipped tend is 630000
        if not raw_shift(p, t0) / ylen >= 100:
            raise PlantError("%s: only %.1f wraps of ylen behind t0" % (what, raw_shift(p, t0) / ylen))
    else:   # fast
        t0, planted = 0.0, None
    if plant in ("last-row", "cell-crossing"):
        t0, ts, dts, states, planted = seq
    else:
        ts, dts, states = oracle_loop(oracle, p, U, t0, K)
    if len(dts) != K or not all(np.isfinite(s).all() for s in states):
        raise PlantError("%s: the oracle's run from t0 = %r is not finite" % (what, t0))
    phases = [step_phases(p, ts[n], dts[n]) for n in range(K)]
    if plant == "fast":
        wraps = int(raw_shift(p, ts[K]) / ylen)
        remap, ghost = {r for r, _ in phases}, {g for _, g in phases}
        if ny <= K:
            # every row occurs as a remap offset and as a ghost offset, ylen wrapped at least twice
            ok = remap == set(range(ny)) and ghost == set(range(ny)) and wraps >= 2
        else:
            # more rows than steps (the 24 rows of 32x24x9, where dt is half as long: the shift stays below ylen): no wrap is claimed,
            # only that every step has another remap and another ghost offset, and that the two differ within most steps
            ok = len(remap) == K and len(ghost) == K and sum(r != g for r, g in phases) >= K // 2
        if not ok:
            raise PlantError("%s: offsets (remap, ghost) %r, %d wraps of ylen" % (what, phases, wraps))
        hits = [n for n in range(1, K - 2) if phases[n][0] == ny - 1 and phases[n][1] == 0]
        planted = hits[0] if hits else K // 2
    sens = sensitivity(oracle, p, U, t0)
    print("shear phase %s: t0 = %r, offsets (remap, ghost) per step %r, planted step %d, one row further moves the x ghosts by %.3e"
          % (what, t0, phases, planted, sens))
    if not sens >= SENSITIVITY * pc.L2_TOLERANCE:
        raise PlantError("%s: the oracle's fill one row further differs by %.3e in the x-ghost columns, below %g x the tolerance %g"
                         % (what, sens, SENSITIVITY, pc.L2_TOLERANCE))
    for a in [U] + states:
        a.flags.writeable = False
    while len(_REFS) >= 3:
        _REFS.popitem(last=False)
    _REFS[case] = Ref(case, ov, p, U, t0, ts, dts, states, planted, phases, sens, [])
    return _REFS[case]


# ---- comparisons -------------------------------------------------------------------------------------------------------------------
def _record(lib, what, errs):
    """the contracted library's specific-form errors: printed (pytest -s shows them) and, when RGPU_TEST_LOG_DIR names a directory,
    appended to shear_phase_contracted.txt there"""
    line = "contracted, specific-form relative L2: %s: %s" % (what, " ".join("%s %.2e" % kv for kv in errs.items()))
    print(line)
    if "emulation" in lib.backend:
        return
    if not os.environ.get("RGPU_TEST_LOG_DIR"):
        return
    try:
        out = os.path.join(os.environ["RGPU_TEST_LOG_DIR"], "shear_phase_contracted.txt")
        os.makedirs(os.path.dirname(out), exist_ok=True)
        with open(out, "a") as f:
            f.write(line + "\n")
    except OSError:
        pass


def _compare(lib, got, ref, p, what, exact):
    if exact:
        pc.assert_same(got, ref, what)
    else:
        _record(lib, what, pc.assert_close_specific(got, ref, p, what))


def _compare_poisoned(lib, got, want, p, what, exact):
    """arrays in which some ghost cells are still NaN (a partial fill of a poisoned input): the same cells must be, the others compare"""
    nan = np.isnan(want)
    bad = int((np.isnan(got) != nan).sum())
    assert bad == 0, "%s: %d cells are NaN on one side only (an unwritten ghost, or a write where none belongs)" % (what, bad)
    g, w = np.where(nan, 0.0, got), np.where(nan, 0.0, want)
    if exact:
        pc.assert_same(g, w, what)
    else:
        rho = np.maximum(np.abs(np.where(nan[0], 1.0, want[0])), p.smallr)
        _record(lib, what, pc.assert_close_specific(g, w, p, what, rho=rho))


def _dts_equal(got, ref, what, exact):
    assert len(got) == len(ref), (what, got, ref)
    if exact:
        assert list(got) == list(ref), "%s: dt sequence %r, the oracle's %r" % (what, list(got), list(ref))
    else:
        assert all(abs(a / b - 1.0) < DT_RTOL for a, b in zip(got, ref)), "%s: dt sequence %r, the oracle's %r" % (what, list(got), list(ref))


def _time_equal(got, ref, what, exact):
    if exact:
        assert got == ref, "%s: t = %r, the oracle's %r" % (what, got, ref)
    else:
        assert abs(got - ref) <= DT_RTOL * abs(ref), "%s: t = %r, the oracle's %r" % (what, got, ref)


def poisoned(p, U):
    """U with every ghost cell NaN, except the first outer Bx face of the interior rows and planes: an evolved face value the shearing
    fill keeps (kernels_bc.h: shear_ghost_cell)"""
    gw = p.ghostWidth
    P = np.full_like(U, np.nan)
    P[:, gw:-gw, gw:-gw, gw:-gw] = U[:, gw:-gw, gw:-gw, gw:-gw]
    P[IA, gw:-gw, gw:-gw, p.nx + gw] = U[IA, gw:-gw, gw:-gw, p.nx + gw]
    return P


def _started(lib, R):
    """a context holding the oracle-filled state of t0 in both arrays, its clock at t0"""
    sv = Solver(R.p, lib)
    sv.upload(R.states[0], both=True)
    sv.nStep, sv.totalTime = 0, R.t0
    return sv


def _device_path_expected(lib):
    return not (os.environ.get("RGPU_TILED") == "0" or lib.get_option("step_clock") == 0 or lib.get_option("ghost_images") == 0)


# ---- 1. the public fills -----------------------------------------------------------------------------------------------------------
def check_fills(lib, oracle, case, exact=True):
    """rgpu_make_boundaries_shear after the y pass, rgpu_make_all_boundaries (the separate passes) and the one-launch in-plane fill
    (rgpu_step_fill_planes_pair: fill_xy_cell) against the oracle, at (t0, 0) and at every (t, dt) of the sequence; the input's ghosts
    are NaN, so an unwritten ghost shows; the kept Bx face is compared like everything else"""
    R = reference(lib, oracle, case)
    p = R.p
    gw, ks = p.ghostWidth, p.nz + 2 * p.ghostWidth
    P = poisoned(p, R.U)
    sv = Solver(p, lib)
    try:
        for t, dt in [(R.t0, 0.0)] + list(zip(R.ts[:-1], R.dts)):
            what = "%s, %s library, fill at (t, dt) = (%r, %r), ghost offset %d" % (case_id(case), lib.arithmetic, t, dt, phase(p, t + dt)[0])
            part = P.copy()
            oracle.make_boundaries(p, part, 2)
            oracle.make_boundaries_shear(p, part, t, dt)
            inner = part[:, gw:-gw]
            assert np.isfinite(inner[:, :, gw:-gw, :]).all() and np.isfinite(inner[:, :, :, gw:-gw]).all(), what   # (the oracle's own)
            full = P.copy()
            oracle.make_all_boundaries(p, full, t, dt)
            assert np.isfinite(full).all(), what
            sv.upload(P, both=False)
            sv.make_boundaries(0, 2)
            sv._chk(lib.lib.rgpu_make_boundaries_shear(sv.ctx, 0, t, dt), "make_boundaries_shear")
            _compare_poisoned(lib, sv.getDataHost(0), part, p, what + ": shear pass after the y pass", exact)
            sv.upload(P, both=False)
            sv.make_all_boundaries(0, t, dt)
            _compare(lib, sv.getDataHost(0), full, p, what + ": make_all_boundaries", exact)
            sv.upload(P, both=True)
            sv.step_fill_planes_pair(1, dt, t, (gw, ks - gw), (0, 0))       # step 1 writes U[0]
            want = P.copy()
            want[:, gw:ks - gw] = full[:, gw:ks - gw]
            _compare_poisoned(lib, sv.getDataHost(0), want, p, what + ": one-launch fill of the interior planes", exact)
    finally:
        sv.close()


# ---- 2. single steps ---------------------------------------------------------------------------------------------------------------
def check_single_steps(lib, oracle, case, exact=True):
    """one godunov_unsplit(0, dt, t) at each step time of the sequence, from the case's stress state filled by the oracle at that time
    (the plants that run from the initial condition take the rough state here: the step times are the plant's, the rows differ at O(1)),
    dt = 0.3 x the oracle's CFL dt (parity_checks.check_single_step_random); the whole output array compared"""
    R = reference(lib, oracle, case)
    p = R.p
    if not R.singles:
        S = pc.stress_state(p, 3, "rough") if case.family == "initial" else R.U
        for t in R.ts[:-1]:
            F = S.copy()
            oracle.make_all_boundaries(p, F, t, 0.0)
            dt = 0.3 * oracle.compute_dt(p, F)
            out = oracle.godunov_unsplit(p, F.copy(), dt, t)
            if not np.isfinite(out).all():
                raise PlantError("%s: the oracle's single step at t = %r is not finite" % (case_id(case), t))
            R.singles.append((t, dt, F, out))
    sv = Solver(p, lib)
    try:
        for t, dt, F, out in R.singles:
            sv.upload(F, both=True)
            sv.godunov_unsplit(0, dt, t)
            _compare(lib, sv.getDataHost(1), out, p, "%s, %s library, single step at t = %r (offsets %r)"
                     % (case_id(case), lib.arithmetic, t, step_phases(p, t, dt)), exact)
    finally:
        sv.close()


# ---- 3. the host-clock loop --------------------------------------------------------------------------------------------------------
def check_step_loop(lib, oracle, case, exact=True):
    """K x oneStepIntegration from t0 == the oracle loop: every dt, totalTime, every double (exact: after every step)"""
    R = reference(lib, oracle, case)
    K = len(R.dts)
    what = "%s, %s library, %d x oneStepIntegration from t0 = %r" % (case_id(case), lib.arithmetic, K, R.t0)
    sv = _started(lib, R)
    try:
        dts = []
        for n in range(K):
            dts.append(sv.oneStepIntegration())
            if exact:
                assert dts[-1] == R.dts[n], "%s: dt of step %d is %r, the oracle's %r" % (what, n, dts[-1], R.dts[n])
                pc.assert_same(sv.getDataHost(), R.states[n + 1], "%s: after step %d (offsets %r)" % (what, n, R.phases[n]))
        _dts_equal(dts, R.dts, what, exact)
        _time_equal(sv.totalTime, R.ts[K], what, exact)
        assert sv.nStep == K
        _compare(lib, sv.getDataHost(), R.states[K], R.p, what, exact)
    finally:
        sv.close()


# ---- 4. the device-clock batch -----------------------------------------------------------------------------------------------------
def check_run_steps(lib, oracle, case, exact=True):
    """run_steps(K) from t0 == the oracle loop (state, totalTime, dt_log; rgpu_device_time_step_ready afterwards); in two calls, the
    second beginning on the planted step; and with tEnd inside the step after the planted one -- the count and t of the oracle loop,
    then one oneStepIntegration whose dt matches"""
    R = reference(lib, oracle, case)
    p, K, n = R.p, len(R.dts), R.planted
    what = "%s, %s library, run_steps from t0 = %r" % (case_id(case), lib.arithmetic, R.t0)

    def ends_like_the_oracle(sv, m, how):
        assert sv.nStep == m, (how, sv.nStep, m)
        _time_equal(sv.totalTime, R.ts[m], how, exact)
        _compare(lib, sv.getDataHost(), R.states[m], p, how, exact)

    sv = _started(lib, R)
    try:
        assert sv.run_steps(K) == K, what
        _dts_equal(sv.dt_log, R.dts, what, exact)
        assert sv.dt == sv.dt_log[-1]
        ends_like_the_oracle(sv, K, what + ", one call of %d" % K)
        if _device_path_expected(lib):
            assert lib.lib.rgpu_device_time_step_ready(sv.ctx, sv.nStep % 2) == 1, what
    finally:
        sv.close()
    assert 1 <= n <= K - 3, (what, n)
    sv = _started(lib, R)
    try:   # a batch that begins on the planted step
        how = what + ", %d + %d steps (the second call begins on offsets %r)" % (n, K - n, R.phases[n])
        assert sv.run_steps(n) == n, how
        log = list(sv.dt_log)
        assert sv.run_steps(K - n) == K - n, how
        _dts_equal(log + list(sv.dt_log), R.dts, how, exact)
        ends_like_the_oracle(sv, K, how)
    finally:
        sv.close()
    sv = _started(lib, R)
    try:   # the loop condition t < tEnd on the device: the step after the planted one carries t past tEnd and is the last
        tEnd = R.ts[n + 1] + 0.5 * R.dts[n + 1]
        ts_ref, dts_ref, _ = oracle_loop(oracle, p, R.U, R.t0, K, tEnd)
        m = len(dts_ref)
        assert m == n + 2 and ts_ref == R.ts[:m + 1]
        how = what + ", tEnd = %r inside step %d" % (tEnd, n + 1)
        assert sv.run_steps(K, tEnd) == m, (how, sv.nStep)
        _dts_equal(sv.dt_log, dts_ref, how, exact)
        ends_like_the_oracle(sv, m, how)
        assert sv.run_steps(K, tEnd) == 0, how
        sv.oneStepIntegration()
        _dts_equal([sv.dt], [R.dts[m]], how + ", one more step", exact)
    finally:
        sv.close()


# ---- 5. diagnostic options ---------------------------------------------------------------------------------------------------------
def check_options(lib, oracle, case, option, value):
    """run_steps(K) from t0 with a diagnostic option of the library switched (read at rgpu_create) == the default run: the same bits and
    the same time steps (the default run itself is held to the oracle by check_run_steps)"""
    R = reference(lib, oracle, case)
    K = len(R.dts)
    outs = []
    for on in (False, True):
        old = lib.set_option(option, value) if on else None
        try:
            sv = _started(lib, R)
            try:
                assert sv.run_steps(K) == K
                outs.append((sv.getDataHost().copy(), sv.totalTime, list(sv.dt_log)))
            finally:
                sv.close()
        finally:
            if on:
                lib.set_option(option, old)
    assert np.array_equal(outs[0][0], outs[1][0]) and outs[0][1:] == outs[1][1:], "%s: %s = %d changes %d doubles" % (
        case_id(case), option, value, int((outs[0][0] != outs[1][0]).sum()))
    pc.assert_same(outs[0][0], R.states[K], "%s: run_steps(%d) at the default options" % (case_id(case), K))


def check_fast_equals_golden(lib, oracle):
    """the Python oracle loop of the `fast` case is the run the reference binary wrote tests/golden/<GOLDEN_FAST>.npz from: its state
    after 7 and 14 steps equals the reference's, every double -- the loop the checks above compare with is pinned to the reference"""
    from conftest import golden_cases, load_golden
    case = CASES[-1]
    assert case.plant == "fast"
    R = reference(lib, oracle, case)
    g, meta = load_golden(GOLDEN_FAST), golden_cases()[GOLDEN_FAST]
    assert meta["base"] == BASE and all(kv in meta["overrides"].split(";") for kv in R.ov.split(";") if not kv.startswith("hydro.slope_type")), (meta, R.ov)
    assert R.p.slope_type == 2
    for s in meta["steps"]:
        pc.assert_same(interior(R.states[s], R.p), g["step_%d" % s], "oracle loop of %s, step %d vs the reference" % (case_id(case), s))
    pc.assert_dt_log(R.dts, g["log_dt"], R.p, GOLDEN_FAST)
