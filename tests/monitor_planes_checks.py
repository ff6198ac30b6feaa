"""Checks of the plane monitor (rgpu_state_monitor_planes, rgpu_run_steps_monitored_planes; include/rgpu.h, "plane monitors") shared
by tests/test_monitor_planes_host.py (the test-only host emulation, not gpu) and tests/test_monitor_planes_gpu.py (-m gpu).

`model(U, p)` is an independent numpy restatement of the definition in include/rgpu.h: the ten per-cell terms of the 3D monitor
(monitor3d_checks.cell_terms), the six new ones by the documented expressions, and per interior plane monitor_checks' 2D order
(segments, columns, lanes, butterfly) -- no sum over the planes.  It must equal the libraries' nz x 16 doubles bit for bit.
`fold(rows)` is the identity the header states: the rows folded ascending in kk are the ten doubles of rgpu_state_monitor3d."""
import math

import numpy as np

import ensemble_checks as ec
import monitor3d_checks as m3
import monitor_checks as mc
from ramsesgpu_amd import _capi
from ramsesgpu_amd.solver import Solver

NQ = 16
SUMS = list(range(7)) + list(range(10, 16))   # the columns that are sums; 7, 8: minima; 9: a maximum
HYDRO_ZERO = (6, 9, 10, 11, 12, 13)           # exactly +0.0 in every row of a hydro state

initial_state = m3.initial_state


def cell_terms(U, p):
    """the sixteen per-cell terms of a ghost-inclusive 3D state U[nvar][ksize][jsize][isize] over its interior: [16][nz][ny][nx]"""
    gw, nx, ny, nz = p.ghostWidth, p.nx, p.ny, p.nz
    cell = lambda v, di=0, dj=0, dk=0: U[v, gw + dk:gw + dk + nz, gw + dj:gw + dj + ny, gw + di:gw + di + nx]
    T = m3.cell_terms(U, p)
    rho, mx, my = cell(_capi.ID), cell(_capi.IU), cell(_capi.IV)
    zero = np.zeros_like(rho)
    bxc, byc, bzc, bxby = zero, zero, zero, zero
    if p.mhdEnabled:
        bxc = 0.5 * (cell(_capi.IA) + cell(_capi.IA, di=1))
        byc = 0.5 * (cell(_capi.IB) + cell(_capi.IB, dj=1))
        bzc = 0.5 * (cell(_capi.IC) + cell(_capi.IC, dk=1))
        bxby = bxc * byc
    rvxvy = (mx * my) / rho
    rho2 = rho * rho
    return np.array(list(T) + [bxc, byc, bzc, bxby, rvxvy, rho2])


def reduction(q):
    return (np.fmin, np.inf) if q in (7, 8) else (np.fmax, 0.0) if q == 9 else (np.add, 0.0)


def model(U, p):
    """[nz][16]: row kk is steps 1 - 4 of the documented order on the nx x ny cells of interior plane kk"""
    with np.errstate(all="ignore"):
        T = cell_terms(U, p)
        return np.array([[mc.ordered(T[q][kk], *reduction(q)) for q in range(NQ)] for kk in range(p.nz)])


def fold(rows):
    """the identity of include/rgpu.h: the rows folded ascending in kk from +0.0 / +inf / +0.0 with + / fmin / fmax, columns 0 - 9"""
    out = []
    with np.errstate(all="ignore"):
        for q in range(m3.NQ):
            op, start = reduction(q)
            a = np.float64(start)
            for kk in range(rows.shape[0]):
                a = op(a, rows[kk, q])
            out.append(a)
    return np.array(out)


def assert_within_any_order_bound(rows, U, p):
    """per plane: |S - fsum(terms)| <= N 2^-53 fsum(|terms|), the worst case of ANY summation order of the N = nx ny terms of the plane;
    the extrema equal numpy's"""
    T = cell_terms(U, p)
    N = p.nx * p.ny
    for kk in range(p.nz):
        for q in SUMS:
            terms = [float(x) for x in T[q][kk].ravel()]
            exact, scale = math.fsum(terms), math.fsum(abs(x) for x in terms)
            assert abs(rows[kk, q] - exact) <= N * 2.0 ** -53 * scale, (kk, _capi.MONP_NAMES[q], rows[kk, q], exact, scale)
        assert rows[kk, 7] == T[7][kk].min() and rows[kk, 8] == T[8][kk].min() and rows[kk, 9] == T[9][kk].max(), (kk, rows[kk, 7:10])


def assert_hydro_zeros(rows):
    for q in HYDRO_ZERO:
        assert (rows[:, q] == 0.0).all() and not np.signbit(rows[:, q]).any(), (_capi.MONP_NAMES[q], rows[:, q])


def check_single_samples(lib, base, ov):
    """a lone context before stepping and after 3 steps: the rows == the model, all 16 columns; folded they are Solver.state_monitor();
    every sum within the any-order bound per plane; the call changes neither the checksum nor the device-ready flag"""
    p = lib.params_from_ini(ec.ini(base), ov)
    U0 = initial_state(lib, base, ov, p)
    sv = Solver(p, lib)
    try:
        sv.start(U0, 0)
        for steps in (0, 3):
            if steps:
                assert sv.run_steps(steps) == steps
            par = sv.nStep % 2
            ready, checksum = lib.lib.rgpu_device_time_step_ready(sv.ctx, par), sv.state_checksum(par)
            rows = sv.state_monitor_planes()
            assert lib.lib.rgpu_device_time_step_ready(sv.ctx, par) == ready and sv.state_checksum(par) == checksum
            U = sv.getDataHost()
            want = model(U, p)
            print(base, ov, "after %d steps, plane 0:" % steps, dict(zip(_capi.MONP_NAMES, rows[0])))
            assert rows.shape == (p.nz, NQ) and np.isfinite(rows).all()
            assert np.array_equal(rows, want), (np.argwhere(rows != want), rows[rows != want], want[rows != want])
            assert np.array_equal(rows, sv.state_monitor_planes(par))
            assert np.array_equal(fold(rows), sv.state_monitor()), (fold(rows), sv.state_monitor())
            assert_within_any_order_bound(rows, U, p)
            if not p.mhdEnabled:
                assert_hydro_zeros(rows)
            else:
                assert (rows[:, 6] > 0.0).all() and (rows[:, [10, 11, 12, 13]] != 0.0).any()
            assert (rows[:, 15] > 0.0).all() and (rows[:, 14] != 0.0).any()
        assert sv.run_steps(2) == 2   # (the steps after a sample run as ever)
    finally:
        sv.close()


def check_nan_plane(lib, base, ov):
    """one NaN density in the last column of the last row of a middle plane: that plane's mass, ekin, rvxvy and rho2 are NaN, its extrema
    those of the cells that are numbers; every other plane's row is the row of the clean state, bit for bit; the model agrees"""
    p = lib.params_from_ini(ec.ini(base), ov)
    U0 = initial_state(lib, base, ov, p)
    gw, km = p.ghostWidth, p.nz // 2
    sv = Solver(p, lib)
    try:
        sv.upload(U0)
        clean = sv.state_monitor_planes(0)
        U1 = U0.copy()
        U1[_capi.ID, gw + km, gw + p.ny - 1, gw + p.nx - 1] = np.nan
        sv.upload(U1)
        rows = sv.state_monitor_planes(0)
    finally:
        sv.close()
    assert np.isnan(rows[km, [0, 5, 14, 15]]).all(), rows[km]
    assert not np.isnan(rows[km, [1, 2, 3, 4]]).any() and np.isfinite(rows[km, 7:10]).all(), rows[km]
    with np.errstate(all="ignore"):
        T = cell_terms(U1, p)
    assert rows[km, 7] == np.fmin.reduce(T[7][km].ravel()) and rows[km, 8] == np.fmin.reduce(T[8][km].ravel()) and rows[km, 9] == np.fmax.reduce(np.append(T[9][km].ravel(), 0.0))
    others = [kk for kk in range(p.nz) if kk != km]
    assert np.array_equal(rows[others], clean[others])
    assert np.array_equal(rows, model(U1, p), equal_nan=True)
    assert not np.isnan(clean).any() and np.array_equal(clean, model(U0, p))


_STEPPED = {}   # (library path, base, ov, end time): {"sv": a lone Solver at step n, "at": {n: (rows, model, t)}} -- computed once, shared, left alone


def stepped_reference(lib, base, ov, p, U0, n, tEnd=None):
    """the second lone context: stepped singly (rgpu_run_steps one at a time) to step n; returns (rgpu_state_monitor_planes there, the
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
        ent["at"][sv.nStep] = (sv.state_monitor_planes(), model(sv.getDataHost(), p), sv.totalTime)
    return ent["at"][n]


def close_references():
    for ent in _STEPPED.values():
        ent["sv"].close()
    _STEPPED.clear()


def batch_samples(every):
    """rgpu_monitor_planes_batch_samples of one call of `done` steps from step 0: the qualifying steps behind the first, plain step --
    on the device path, which the context must be on afterwards"""
    def want(done, ready):
        assert ready == 1, "the context does not take its time step from the device"
        return len([s for s in range(2, done + 1) if s % every == 0])
    return want


def check_monitored_planes(lib, base, ov, nsteps, every, pieces=None, tEnd=None, expect_batch=None):
    """One lone context run for nsteps (in `pieces`) through rgpu_run_steps_monitored_planes, one through rgpu_run_steps_log:
      * the same return values, dt_log, nStep, t, dt, checksum and state, bit for bit (sampling only reads)
      * the sample steps are the multiples of `every` among the steps that ran, mon_t the accumulated dt log
      * every sample == rgpu_state_monitor_planes of a second lone context stepped singly to that step == the model on its download
      * the last sample, when it is of the final state, == the model on the monitored context's own download
      * rgpu_monitor_batch_samples stays 0; expect_batch: None, or a function (steps that ran, device-ready flag) -> the wanted
        rgpu_monitor_planes_batch_samples
    Returns (done, steps sampled, values [n][nz][16], batch samples)."""
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
                    d, s = sv.run_steps_monitored_planes(n, every, end)
                    assert s.values.shape == (len(s.step), p.nz, NQ)
                    steps += [int(x) for x in s.step]
                    ts += [float(x) for x in s.t]
                    vals += list(s.values)
                else:
                    d = sv.run_steps(n, end)
                done += d
                log += list(sv.dt_log)
            runs.append({"done": done, "log": log, "nStep": sv.nStep, "t": sv.totalTime, "dt": sv.dt, "checksum": sv.state_checksum(sv.nStep % 2), "full": sv.getDataHost(),
                         "ready": lib.lib.rgpu_device_time_step_ready(sv.ctx, sv.nStep % 2), "batch": lib.lib.rgpu_monitor_planes_batch_samples(sv.ctx),
                         "other": lib.lib.rgpu_monitor_batch_samples(sv.ctx), "steps": steps, "ts": ts, "vals": np.array(vals).reshape(len(vals), p.nz, NQ)})
        finally:
            sv.close()
    a, b = runs
    assert (a["done"], a["nStep"], a["t"], a["dt"], a["checksum"], a["log"]) == (b["done"], b["nStep"], b["t"], b["dt"], b["checksum"], b["log"]), "sampling changed the run"
    assert np.array_equal(a["full"], b["full"], equal_nan=True), "sampling changed the state"
    assert b["batch"] == 0 and a["other"] == 0 and b["other"] == 0
    assert a["steps"] == [s for s in range(1, a["done"] + 1) if s % every == 0], (a["steps"], a["done"])
    assert a["ts"] == [ec.time_of(a["log"][:s]) for s in a["steps"]], "mon_t against the accumulated dt log"
    for s, v in zip(a["steps"], a["vals"]):
        rows, mod, t = stepped_reference(lib, base, ov, p, U0, s, tEnd)
        assert np.array_equal(v, rows), (s, "against the plane monitor of a lone context stepped singly", np.argwhere(v != rows))
        assert np.array_equal(v, mod), (s, "against the model", np.argwhere(v != mod))
    if a["steps"] and a["steps"][-1] == a["nStep"]:
        assert np.array_equal(a["vals"][-1], model(a["full"], p)), "the last sample against the model of the downloaded state"
    if expect_batch is not None:
        assert a["batch"] == expect_batch(a["done"], a["ready"]), (a["batch"], a["done"], a["ready"])
    return a["done"], a["steps"], a["vals"], a["batch"]


def parse_planes_file(path, nz):
    """(steps [n], times [n], values [n][nz][16]) of <prefix>_monitor_planes.txt, whose header and plane numbering are checked"""
    lines = open(path).read().splitlines()
    assert lines[0] == "# nStep totalTime k " + " ".join(_capi.MONP_NAMES)
    rows = [ln.split() for ln in lines[1:]]
    assert len(rows) % nz == 0 and all(len(r) == 3 + NQ for r in rows)
    assert [int(r[2]) for r in rows] == list(range(nz)) * (len(rows) // nz)
    steps = [int(r[0]) for r in rows[::nz]]
    assert [int(r[0]) for r in rows] == [s for s in steps for _ in range(nz)]
    ts = [float(r[1]) for r in rows[::nz]]
    assert [float(r[1]) for r in rows] == [t for t in ts for _ in range(nz)]
    return steps, ts, np.array([[float(x) for x in r[3:]] for r in rows]).reshape(len(steps), nz, NQ)
