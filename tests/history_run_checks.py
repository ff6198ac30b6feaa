"""Shared checks of rgpu_run_steps_history (tests/test_history_run_host.py on the host emulation, tests/test_history_run_gpu.py on the GPU).

The reference series of a case is a lone Solver stepped with oneStepIntegration, with rgpu_history_mri taken before every step (and
after the last): which of those rows a call must return follows from a plain-Python transcription of the contract's condition applied
to the dt sequence alone (`model`), and so do tHist and the sample steps.  A reference is computed once per (library, case, steps),
shared among the tests and never modified."""
import math

import numpy as np

from conftest import ini
from ramsesgpu_amd.solver import Solver, interior

INF = float("inf")
_REFS = {}

# (base, overrides, steps) run by both test files besides their own lists.  fastshear: the plant `fast` of tests/shear_phase_checks.py --
# omega0 = 1 moves the shearing-box shift ~0.75 cell per step, every row offset and two wraps of ylen in 14 steps; the samples are taken
# behind the same clock records the shear remap and the ghost fill read their offsets from
SHEAR_CASES = [
    ("mhd_mri_3d", "mesh.nx=16;mesh.ny=8;mesh.nz=8;MHD.omega0=1.0;MRI.amp=0.3", 14),
]


def reference(lib, base, ov, nsteps, keep_all=True):
    """{"dts": dt of step n, "ts": t before step n (n <= nsteps), "rows": history_mri before step n (n <= nsteps), "states": {n: U}}"""
    key = (lib.path, base, ov, nsteps, keep_all)
    if key in _REFS:
        return _REFS[key]
    p = lib.params_from_ini(ini(base), ov)
    U0 = lib.init_condition(ini(base), ov, p)
    sv = Solver(p, lib)
    try:
        sv.start(U0, 0)
        ts, dts, rows, states = [sv.totalTime], [], [], {}
        for n in range(nsteps + 1):
            h = sv.history_mri()
            rows.append([h[k] for k in Solver.HISTORY_NAMES])
            if keep_all or n == nsteps:
                states[n] = sv.getDataHost()
            if n == nsteps:
                break
            dts.append(sv.oneStepIntegration())
            ts.append(sv.totalTime)
        nxt = sv.oneStepIntegration()   # the dt of one more step: what a context left in a sound state computes next
    finally:
        sv.close()
    for a in states.values():
        a.setflags(write=False)
    R = {"p": p, "U0": U0, "dts": dts, "ts": ts, "rows": np.array(rows), "states": states, "dt_next": nxt}
    R["rows"].setflags(write=False)
    _REFS[key] = R
    return R


def due(t, dt, tHist, dtHist):
    """the contract's condition, in doubles, with its expressions in its order"""
    return tHist == 0 or ((t - dt <= tHist + dtHist) and (t > tHist + dtHist))


def model(R, nsteps, dtHist, tEnd=INF, n0=0, tHist=0.0):
    """the contract's loop on the dt sequence alone: (steps done, sample steps, tHist)"""
    n, done, samples = n0, 0, []
    while done < nsteps and R["ts"][n] < tEnd:
        if due(R["ts"][n], R["dts"][n - 1] if n > 0 else 0.0, tHist, dtHist):
            samples.append(n)
            tHist += dtHist
        n += 1
        done += 1
    return done, samples, tHist


def fresh(lib, R):
    sv = Solver(R["p"], lib)
    sv.start(R["U0"], 0)
    return sv


def run_pieces(sv, pieces, dtHist, tEnd=INF):
    """the calls one after the other on one solver; returns (done per call, steps, t, dt, values, dt log) concatenated"""
    dones, S, T, D, V, log = [], [], [], [], [], []
    for m in pieces:
        done, s, t, d, v = sv.run_steps_history(m, dtHist, tEnd)
        dones.append(done)
        S += list(s); T += list(t); D += list(d); V += [list(r) for r in v]; log += sv.dt_log
    return dones, np.array(S, dtype=int), np.array(T), np.array(D), np.array(V).reshape(len(S), 8), log


def check_series(lib, R, pieces, dtHist, tEnd=INF, sv=None):
    """rgpu_run_steps_history in `pieces` == the reference series: sample steps, hist_t, hist_dt, values, tHist, nStep, t, dt, the dt
    log and the state, every double.  Returns the solver's result for further checks."""
    own = sv is None
    sv = sv or fresh(lib, R)
    try:
        n0, tH0 = sv.nStep, sv.tHist
        dones, S, T, D, V, log = run_pieces(sv, pieces, dtHist, tEnd)
        n, tH, want_S, want_done = n0, tH0, [], []
        for m in pieces:
            d, s, tH = model(R, m, dtHist, tEnd, n, tH)
            n += d
            want_S += s
            want_done.append(d)
        assert dones == want_done, (dones, want_done)
        assert list(S) == want_S, (list(S), want_S)
        assert np.array_equal(T, np.array([R["ts"][k] for k in want_S]))
        assert np.array_equal(D, np.array([R["dts"][k - 1] if k > 0 else 0.0 for k in want_S]))
        want_V = R["rows"][want_S] if want_S else np.zeros((0, 8))
        assert np.array_equal(V, want_V), (V - want_V)
        assert sv.tHist == tH, (sv.tHist, tH)
        assert sv.nStep == n and sv.totalTime == R["ts"][n] and log == R["dts"][n0:n], (sv.nStep, n, sv.totalTime)
        if n > n0:
            assert sv.dt == R["dts"][n - 1]
        if n in R["states"]:
            assert np.array_equal(interior(sv.getDataHost(), R["p"]), interior(R["states"][n], R["p"]))
        return S, V
    finally:
        if own:
            sv.close()


def call_raw(lib, sv, nsteps, tEnd=INF, dtHist=1.0, null=None):
    """rgpu_run_steps_history with one of its pointers NULL (`null`: its name); returns (code, message)"""
    import ctypes as C
    m = max(nsteps, 1)
    a = {"nStep": C.c_int(sv.nStep), "t": C.c_double(sv.totalTime), "dt": C.c_double(sv.dt), "tHist": C.c_double(sv.tHist), "hist_n": C.c_int(0),
         "hist_step": (C.c_int * m)(), "hist_t": (C.c_double * m)(), "hist_dt": (C.c_double * m)(), "hist": (C.c_double * (8 * m))()}
    ref = {k: (C.byref(v) if k in ("nStep", "t", "dt", "tHist", "hist_n") else v) for k, v in a.items()}
    if null:
        ref[null] = None
    rc = lib.lib.rgpu_run_steps_history(sv.ctx, nsteps, tEnd, ref["nStep"], ref["t"], ref["dt"], None, dtHist, ref["tHist"], ref["hist_n"],
                                        ref["hist_step"], ref["hist_t"], ref["hist_dt"], ref["hist"])
    return rc, lib.lib.rgpu_last_error(sv.ctx).decode()


def fsum_anchor(p, U, got):
    """mass and the three mean-B columns of a history row against math.fsum of the interior terms times dTau.  Bound: (N + 2) 2^-53
    fsum|terms| dTau -- the worst case of ANY summation order of N terms ((N - 1) roundings, each at most 2^-53 of a partial sum that
    never exceeds fsum|terms|) plus the two roundings of the scaling; derived, not measured."""
    I = interior(U, p)
    dTau = p.dx * p.dy * p.dz / (p.xMax - p.xMin) / (p.yMax - p.yMin) / (p.zMax - p.zMin)
    N = I[0].size
    for name, comp in (("mass", 0), ("mean_Bx", 5), ("mean_By", 6), ("mean_Bz", 7)):
        terms = [float(x) for x in I[comp].ravel()]
        want = math.fsum(terms) * dTau
        bound = (N + 2) * 2.0 ** -53 * math.fsum(abs(x) for x in terms) * dTau
        g = got[Solver.HISTORY_NAMES.index(name)]
        print("anchor %s: got %.17g fsum %.17g |diff| %.3g bound %.3g" % (name, g, want, abs(g - want), bound))
        assert abs(g - want) <= bound, (name, g, want, bound)
