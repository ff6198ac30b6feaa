"""Checks of the monitors of a lone context (rgpu_state_monitor3d, rgpu_run_steps_monitored; include/rgpu.h, "monitors") shared by
tests/test_monitor3d_host.py (the test-only host emulation, not gpu) and tests/test_monitor3d_gpu.py (-m gpu).

`model(U, p)` is an independent numpy restatement of the definition in include/rgpu.h: for a 3D state the per-cell terms by the
documented expressions and, per interior plane, monitor_checks' 2D order (segments, columns, lanes, butterfly), then the ascending
sum over the planes; a 2D state goes to monitor_checks.model.  It must equal the libraries' ten doubles bit for bit."""
import math

import numpy as np

import ensemble_checks as ec
import monitor_checks as mc
from ramsesgpu_amd import _capi
from ramsesgpu_amd.solver import Solver, interior

NQ, NSUM = mc.NQ, mc.NSUM


def cell_terms(U, p):
    """the ten per-cell terms of a ghost-inclusive 3D state U[nvar][ksize][jsize][isize] over its interior: [10][nz][ny][nx]"""
    gw, nx, ny, nz = p.ghostWidth, p.nx, p.ny, p.nz
    cell = lambda v, di=0, dj=0, dk=0: U[v, gw + dk:gw + dk + nz, gw + dj:gw + dj + ny, gw + di:gw + di + nx]
    rho, E, mx, my, mz = cell(_capi.ID), cell(_capi.IP), cell(_capi.IU), cell(_capi.IV), cell(_capi.IW)
    ekin = (0.5 * ((mx * mx + my * my) + mz * mz)) / rho
    emag, divb = np.zeros_like(rho), np.zeros_like(rho)
    if p.mhdEnabled:
        bx, bx1, by, by1, bz, bz1 = cell(_capi.IA), cell(_capi.IA, di=1), cell(_capi.IB), cell(_capi.IB, dj=1), cell(_capi.IC), cell(_capi.IC, dk=1)
        bxc, byc, bzc = 0.5 * (bx + bx1), 0.5 * (by + by1), 0.5 * (bz + bz1)
        emag = 0.5 * ((bxc * bxc + byc * byc) + bzc * bzc)
        divb = np.abs(((bx1 - bx) / p.dx + (by1 - by) / p.dy) + (bz1 - bz) / p.dz)
    eint = (E - ekin) - emag
    return np.array([rho, mx, my, mz, E, ekin, emag, rho, eint, divb])


def is3d(p):
    return p.nz_global != 1


def ordered(T, op, start):
    """one quantity T[nz][ny][nx]: V[kk] by the 2D order of plane kk, then start (op) V[0] (op) V[1] .. ascending"""
    a = np.float64(start)
    for kk in range(T.shape[0]):
        a = op(a, mc.ordered(T[kk], op, start))
    return a


def model(U, p):
    if not is3d(p):
        return mc.model(U, p)
    with np.errstate(all="ignore"):
        T = cell_terms(U, p)
        out = [ordered(T[q], np.add, 0.0) for q in range(NSUM)]
        out += [ordered(T[7], np.fmin, np.inf), ordered(T[8], np.fmin, np.inf), ordered(T[9], np.fmax, 0.0)]
    return np.array(out)


def terms_of(U, p):
    with np.errstate(all="ignore"):
        return cell_terms(U, p) if is3d(p) else mc.cell_terms(U, p)


def assert_within_any_order_bound(got, U, p):
    """|S - fsum(terms)| <= N 2^-53 fsum(|terms|), the worst case of ANY summation order of N terms; the extrema equal numpy's"""
    T = terms_of(U, p)
    N = T[0].size
    for q in range(NSUM):
        terms = [float(x) for x in T[q].ravel()]
        exact, scale = math.fsum(terms), math.fsum(abs(x) for x in terms)
        assert abs(got[q] - exact) <= N * 2.0 ** -53 * scale, (_capi.MON_NAMES[q], got[q], exact, scale)
    assert got[7] == T[7].min() and got[8] == T[8].min() and got[9] == T[9].max(), (got[7:], T[7].min(), T[8].min(), T[9].max())


def assert_nan_rules(got, U, p):
    """a sum is NaN exactly when one of its terms is; the extrema are those of the terms that are numbers, +inf / +0.0 when none is"""
    T = terms_of(U, p)
    for q in range(NSUM):
        assert np.isnan(got[q]) == bool(np.isnan(T[q]).any()), (_capi.MON_NAMES[q], got[q])
    want = [np.fmin.reduce(np.append(T[7].ravel(), np.inf)), np.fmin.reduce(np.append(T[8].ravel(), np.inf)), np.fmax.reduce(np.append(T[9].ravel(), 0.0))]
    assert not np.isnan(want).any() and list(got[7:]) == [float(x) for x in want], (got[7:], want)


def initial_state(lib, base, ov, p):
    """the problem's initial condition with monitor_checks' seeded perturbation of density and momenta (the z momentum included)"""
    return ec.member_states(lib, base, ov, p, 1)[0]


# 2D shapes (nx, ny) at the seams of the summation order: a lane without a column and a short segment; exactly full lanes and one full
# segment; one column into the second round of the lanes and one row into a second segment; the same one round and one segment later
SEAM_SHAPES = [(63, 31), (64, 32), (65, 33), (130, 65)]
SEAMS = [(base, "mesh.nx=%d;mesh.ny=%d" % s) for s in SEAM_SHAPES for base in ("kelvin_helmholtz_gpu_2d", "orszag-tang")]


def check_seam_state(lib, base, ov):
    """a lone 2D context before stepping and after 3 steps: rgpu_state_monitor == the model on its download == rgpu_ensemble_monitor
    of a one-member ensemble holding that state (uploaded, so that it is the same state in either library), bit for bit"""
    from ramsesgpu_amd.ensemble import Ensemble
    p = lib.params_from_ini(ec.ini(base), ov)
    assert not is3d(p) and p.mhdEnabled == (base == "orszag-tang") and (p.mhdEnabled or p.nbVar == 4)
    sv, ens = Solver(p, lib), Ensemble(p, 1, lib)
    try:
        sv.start(initial_state(lib, base, ov, p), 0)
        for steps in (0, 3):
            if steps:
                assert sv.run_steps(steps) == steps
            got, U = sv.state_monitor(), sv.getDataHost()
            print(base, ov, "after %d steps:" % steps, dict(zip(_capi.MON_NAMES, got)))
            assert np.array_equal(got, mc.model(U, p)), (got, mc.model(U, p))
            ens.member(0).upload(U)
            one = ens.monitor()
            assert one.shape == (1, NQ) and np.array_equal(one[0], got), (one[0], got)
    finally:
        ens.close()
        sv.close()


def check_seam_nan(lib, base, ov):
    """the NaN rules on a seam shape: one NaN density in the last column of the last row (the short lane, the short segment)"""
    p = lib.params_from_ini(ec.ini(base), ov)
    U0 = initial_state(lib, base, ov, p)
    gw = p.ghostWidth
    U0[0, 0, gw + p.ny - 1, gw + p.nx - 1] = np.nan
    sv = Solver(p, lib)
    try:
        sv.upload(U0)
        got = sv.state_monitor(0)
        assert_nan_rules(got, U0, p)
        assert np.isnan(got[0]) and np.isnan(got[5]) and not np.isnan(got[1]) and not np.isnan(got[4]) and np.isfinite(got[7:]).all()
        assert np.array_equal(got, mc.model(U0, p), equal_nan=True)
    finally:
        sv.close()


_STEPPED = {}   # (library path, base, ov, end time): {"sv": a lone Solver at step n, "at": {n: (monitor, model, t)}} -- computed once, shared, left alone


def stepped_reference(lib, base, ov, p, U0, n, tEnd=None):
    """the second lone context: stepped singly (rgpu_run_steps one at a time) to step n; returns (rgpu_state_monitor[3d] there, the
    model of its download, its time).  Steps are taken in ascending n; the results are kept."""
    key = (lib.path, base, ov, tEnd)
    end = float("inf") if tEnd is None else tEnd
    ent = _STEPPED.get(key)
    if ent is None:
        sv = Solver(p, lib)
        sv.start(U0, 0)
        ent = _STEPPED[key] = {"sv": sv, "at": {}}
    sv = ent["sv"]
    while sv.nStep < n:
        assert sv.run_steps(1, end) == 1
        ent["at"][sv.nStep] = (sv.state_monitor(), model(sv.getDataHost(), p), sv.totalTime)
    return ent["at"][n]


def check_monitored_lone(lib, base, ov, nsteps, every, pieces=None, tEnd=None, expect_batch=None):
    """One lone context run for nsteps (in `pieces`) through rgpu_run_steps_monitored, one through rgpu_run_steps_log:
      * the same return values, dt_log, nStep, t, dt, checksum and state, bit for bit (sampling only reads)
      * the sample steps are the multiples of `every` among the steps that ran, mon_t the accumulated dt log
      * every sample == rgpu_state_monitor[3d] of a second lone context stepped to that step == the model on its download
      * the last sample, when it is of the final state, == the model on the monitored context's own download
      * expect_batch: None, or a function (steps that ran, device-ready flag) -> the wanted rgpu_monitor_batch_samples
    Returns (done, steps sampled, values, batch samples)."""
    p = lib.params_from_ini(ec.ini(base), ov)
    U0 = initial_state(lib, base, ov, p)
    end = float("inf") if tEnd is None else tEnd
    runs = []
    for monitored in (True, False):
        sv = Solver(p, lib)
        try:
            sv.start(U0, 0)
            done, log, steps, ts, vals = 0, [], [], [], []
            for n in (pieces or [nsteps]):
                if monitored:
                    d, s = sv.run_steps_monitored(n, every, end)
                    steps += [int(x) for x in s.step]
                    ts += [float(x) for x in s.t]
                    vals += list(s.values)
                else:
                    d = sv.run_steps(n, end)
                done += d
                log += list(sv.dt_log)
            full = sv.getDataHost()
            runs.append({"done": done, "log": log, "nStep": sv.nStep, "t": sv.totalTime, "dt": sv.dt, "checksum": sv.state_checksum(sv.nStep % 2), "full": full,
                         "ready": lib.lib.rgpu_device_time_step_ready(sv.ctx, sv.nStep % 2), "batch": lib.lib.rgpu_monitor_batch_samples(sv.ctx),
                         "steps": steps, "ts": ts, "vals": np.array(vals).reshape(len(vals), NQ)})
        finally:
            sv.close()
    a, b = runs
    assert (a["done"], a["nStep"], a["t"], a["dt"], a["checksum"], a["log"]) == (b["done"], b["nStep"], b["t"], b["dt"], b["checksum"], b["log"]), "sampling changed the run"
    assert np.array_equal(a["full"], b["full"], equal_nan=True), "sampling changed the state"
    assert b["batch"] == 0
    assert a["steps"] == [s for s in range(1, a["done"] + 1) if s % every == 0], (a["steps"], a["done"])
    assert a["ts"] == [ec.time_of(a["log"][:s]) for s in a["steps"]], "mon_t against the accumulated dt log"
    for s, v in zip(a["steps"], a["vals"]):
        mon, mod, t = stepped_reference(lib, base, ov, p, U0, s, tEnd)
        print(base, ov, "step", s, dict(zip(_capi.MON_NAMES, v)))
        assert np.array_equal(v, mon), (s, "against the monitor of a lone context stepped singly", v, mon)
        assert np.array_equal(v, mod), (s, "against the model", v, mod)
    if a["steps"] and a["steps"][-1] == a["nStep"]:
        assert np.array_equal(a["vals"][-1], model(a["full"], p)), "the last sample against the model of the downloaded state"
    if expect_batch is not None:
        assert a["batch"] == expect_batch(a["done"], a["ready"]), (a["batch"], a["done"], a["ready"])
    return a["done"], a["steps"], a["vals"], a["batch"]


def close_references():
    for ent in _STEPPED.values():
        ent["sv"].close()
    _STEPPED.clear()
