"""Checks of the monitors (rgpu_state_monitor, rgpu_ensemble_monitor, rgpu_ensemble_run_steps_monitored; include/rgpu.h, "monitors")
shared by tests/test_monitor_host.py (the test-only host emulation, not gpu) and tests/test_monitor_gpu.py (-m gpu).

`model(U, p)` is an independent numpy restatement of the definition in include/rgpu.h: the per-cell terms by the documented expressions
(numpy evaluates every operation on its own: IEEE, no contraction) and the sums in the documented order -- segments of RGPU_MON_ROWS
rows, columns, RGPU_MON_LANES lanes, butterfly.  It must equal the libraries' ten doubles bit for bit.  `lone_series` is the other
reference: a lone Solver stepped to every sampling step, rgpu_state_monitor there."""
import math

import numpy as np

import ensemble_checks as ec
from ramsesgpu_amd import _capi
from ramsesgpu_amd.ensemble import Ensemble
from ramsesgpu_amd.solver import Solver, interior

NQ, NSUM, ROWS, LANES = 10, 7, 32, 64   # RGPU_MON_NQ, the sums among them, RGPU_MON_ROWS, RGPU_MON_LANES


def cell_terms(U, p):
    """the ten per-cell terms of a ghost-inclusive 2D state U[nvar][1][jsize][isize] over its interior: [10][ny][nx]"""
    gw, nx, ny = p.ghostWidth, p.nx, p.ny
    cell = lambda v, di=0, dj=0: U[v, 0, gw + dj:gw + dj + ny, gw + di:gw + di + nx]
    rho, E, mx, my = cell(_capi.ID), cell(_capi.IP), cell(_capi.IU), cell(_capi.IV)
    mz = cell(_capi.IW) if p.nbVar > 4 else np.zeros_like(rho)
    ekin = (0.5 * ((mx * mx + my * my) + mz * mz)) / rho
    emag, divb = np.zeros_like(rho), np.zeros_like(rho)
    if p.mhdEnabled:
        bx, bx1, by, by1, bzc = cell(_capi.IA), cell(_capi.IA, di=1), cell(_capi.IB), cell(_capi.IB, dj=1), cell(_capi.IC)
        bxc, byc = 0.5 * (bx + bx1), 0.5 * (by + by1)
        emag = 0.5 * ((bxc * bxc + byc * byc) + bzc * bzc)
        divb = np.abs((bx1 - bx) / p.dx + (by1 - by) / p.dy)
    eint = (E - ekin) - emag
    return np.array([rho, mx, my, mz, E, ekin, emag, rho, eint, divb])


def ordered(T, op, start):
    """one quantity T[ny][nx] reduced in the documented order with a = op(a, x), every accumulator starting at `start`"""
    ny, nx = T.shape
    nseg = (ny + ROWS - 1) // ROWS
    C = np.full(nx, start)
    for s in range(nseg):                                   # 2. columns: the segments in ascending order
        P = np.full(nx, start)
        for jj in range(s * ROWS, min(ny, (s + 1) * ROWS)):  # 1. a segment: its rows in ascending order
            P = op(P, T[jj])
        C = op(C, P)
    L = np.full(LANES, start)
    for i0 in range(0, nx, LANES):                          # 3. lanes: ii = l, l + LANES, ..
        n = min(LANES, nx - i0)
        L[:n] = op(L[:n], C[i0:i0 + n])
    lane = np.arange(LANES)
    off = LANES // 2
    while off:                                              # 4. butterfly
        L = op(L, L[lane ^ off])
        off //= 2
    return L[0]


def model(U, p):
    with np.errstate(all="ignore"):
        T = cell_terms(U, p)
        out = [ordered(T[q], np.add, 0.0) for q in range(NSUM)]
        out += [ordered(T[7], np.fmin, np.inf), ordered(T[8], np.fmin, np.inf), ordered(T[9], np.fmax, 0.0)]
    return np.array(out)


def assert_within_any_order_bound(got, U, p):
    """independent of the chosen order: |S - fsum(terms)| <= N 2^-53 fsum(|terms|), the worst case of ANY summation order of N
    terms; the extrema equal numpy's exactly"""
    T = cell_terms(U, p)
    N = p.nx * p.ny
    for q in range(NSUM):
        terms = [float(x) for x in T[q].ravel()]
        exact, scale = math.fsum(terms), math.fsum(abs(x) for x in terms)
        assert abs(got[q] - exact) <= N * 2.0 ** -53 * scale, (_capi.MON_NAMES[q], got[q], exact, scale)
    assert got[7] == T[7].min() and got[8] == T[8].min() and got[9] == T[9].max(), (got[7:], T[7].min(), T[8].min(), T[9].max())


def column_tolerances(U, p, rel=1e-11):
    """How far a monitor of two states that agree to the contracted library's tolerance (relative L2 <= 1e-12, tests/parity_checks.py)
    may differ, per column, with the factor 10 the dt comparisons of ensemble_checks.assert_member take: a sum moves by at most the
    relative change times the sum of |terms| (NOT times |sum|: the momentum sums cancel); a minimum by it times the largest |term|; div B
    is a difference of face fields over dx, so it moves by it times max (|Bx| / dx + |By| / dy) however small div B itself is.  The scales
    are taken from U, the member's final state (they change by a few per cent over the steps of a test)."""
    T = np.abs(cell_terms(U, p))
    tol = [rel * math.fsum(float(x) for x in T[q].ravel()) for q in range(NSUM)] + [rel * float(T[7].max()), rel * float(T[8].max())]
    gw = p.ghostWidth
    B = np.abs(U[_capi.IA, 0, gw:-gw, gw:-gw]) / p.dx + np.abs(U[_capi.IB, 0, gw:-gw, gw:-gw]) / p.dy if p.mhdEnabled else np.zeros(1)
    return np.array(tol + [rel * 2.0 * float(B.max())])


def assert_nan_rules(got, U, p):
    """what include/rgpu.h says about NaN, on a state that may hold some: a sum is NaN exactly when one of its terms is; the extrema are
    those of the terms that are numbers (np.fmin / np.fmax drop a NaN operand), +inf / +0.0 when none is"""
    with np.errstate(all="ignore"):
        T = cell_terms(U, p)
    for q in range(NSUM):
        assert np.isnan(got[q]) == bool(np.isnan(T[q]).any()), (_capi.MON_NAMES[q], got[q])
    want = [np.fmin.reduce(np.append(T[7].ravel(), np.inf)), np.fmin.reduce(np.append(T[8].ravel(), np.inf)), np.fmax.reduce(np.append(T[9].ravel(), 0.0))]
    assert not np.isnan(want).any() and list(got[7:]) == [float(x) for x in want], (got[7:], want)


def lone_series(lib, p, U0, nsteps, every, tEnd=None, pre=0):
    """a lone Solver holding U0: `pre` steps unsampled, then up to nsteps steps, rgpu_state_monitor after every step that brings nStep
    to a multiple of `every`.  Returns {"step", "t", "values", and the final "U", "nStep", "checksum", "dt_log" (all steps)}"""
    sv = Solver(p, lib)
    try:
        sv.start(U0, 0)
        log = []
        if pre:
            sv.run_steps(pre)
            log += list(sv.dt_log)
        end = float("inf") if tEnd is None else tEnd
        steps, ts, vals, left = [], [], [], nsteps
        while left > 0 and sv.totalTime < end:
            k = min(left, every - sv.nStep % every)
            did = sv.run_steps(k, end)
            log += list(sv.dt_log)
            left -= k
            if did and sv.nStep % every == 0:
                steps.append(sv.nStep)
                ts.append(sv.totalTime)
                vals.append(sv.state_monitor())
            if did < k:
                break
        return {"step": steps, "t": ts, "values": np.array(vals).reshape(len(vals), NQ), "U": interior(sv.getDataHost(), p).copy(), "nStep": sv.nStep,
                "checksum": sv.state_checksum(sv.nStep % 2), "dt_log": log}
    finally:
        sv.close()


def make(lib, ps, scan):
    return Ensemble.scan(ps, lib) if scan else Ensemble(ps[0], len(ps), lib)


def check_monitored(lib, ps, U0s, nsteps, every, tEnds=None, pieces=None, pre=None, scan=False, exact=True, skip=()):
    """One ensemble (member m: parameter set ps[m], state U0s[m], pre.get(m, 0) steps alone through its view first) run for nsteps in
    `pieces` with sampling every `every` steps and the end times tEnds[m] (None: none).  For every member not in `skip`:
      * its series == lone_series on the same library: the step numbers, the times (== the accumulated dt log) and the values
        (exact: bit for bit; the contracted library: bit for bit whenever the member's final state is the lone context's bit for bit,
        which is what its fused rounds are allowed, not promised, to be -- include/rgpu.h; else column by column within column_tolerances)
      * a sample taken at the member's final step == model(its downloaded state), bit for bit in both libraries
      * rgpu_ensemble_monitor == rgpu_state_monitor of each member, before the first step and after the run, and == the model
      * final states, dt logs and checksums == an unmonitored ensemble driven the same way
    Returns (done, stop, fused, samples) summed / concatenated over the pieces."""
    M = len(ps)
    pre = pre or {}
    ends = None if tEnds is None else [float("inf") if x is None else x for x in tEnds]
    runs = []
    for monitored in (True, False):
        ens = make(lib, ps, scan)
        try:
            ens.start(U0s)
            for m, k in pre.items():
                assert ens.member(m).run_steps(k) == k
            if monitored:
                before = ens.monitor()
                for m in range(M):
                    v = ens.member(m)
                    assert np.array_equal(before[m], v.state_monitor(), equal_nan=True), ("ensemble_monitor before the run", m)
                    if m not in skip:
                        assert np.array_equal(before[m], model(v.getDataHost(), ps[m])), ("ensemble_monitor against the model", m)
                    else:
                        assert_nan_rules(before[m], v.getDataHost(), ps[m])
            done, fused, logs = [0] * M, 0, [[] for _ in range(M)]
            series = [([], [], []) for _ in range(M)]
            for n in (pieces or [nsteps]):
                if monitored:
                    d, stop, f, smp = ens.run_steps_monitored(n, every, ends)
                    for m in range(M):
                        series[m][0].extend(int(x) for x in smp[m].step)
                        series[m][1].extend(float(x) for x in smp[m].t)
                        series[m][2].extend(smp[m].values)
                else:
                    d, stop, f = ens.run_steps(n, ends)
                fused += f
                for m in range(M):
                    done[m] += d[m]
                    logs[m] += list(ens.member(m).dt_log)
            final = [{"U": interior(ens.member(m).getDataHost(), ps[m]).copy(), "full": ens.member(m).getDataHost(), "nStep": ens.member(m).nStep,
                      "t": ens.member(m).totalTime, "checksum": ens.member(m).state_checksum(ens.member(m).nStep % 2)} for m in range(M)]
            if monitored:
                after = ens.monitor()
                for m in range(M):
                    assert np.array_equal(after[m], ens.member(m).state_monitor(), equal_nan=True), ("ensemble_monitor after the run", m)
                    if m not in skip:
                        assert np.array_equal(after[m], model(final[m]["full"], ps[m])), ("ensemble_monitor after the run against the model", m)
                    else:   # a member whose state may hold NaN: the documented NaN rules, and the model (which follows them) bit for bit
                        assert_nan_rules(after[m], final[m]["full"], ps[m])
                        assert np.array_equal(after[m], model(final[m]["full"], ps[m]), equal_nan=True), ("poisoned member against the model", m)
            runs.append((done, list(stop), fused, logs, final, series))
        finally:
            ens.close()
    (done, stop, fused, logs, final, series), (done1, stop1, fused1, logs1, final1, _) = runs
    assert done == done1 and stop == stop1 and fused == fused1, ("monitored against unmonitored", done, done1, stop, stop1, fused, fused1)
    for m in range(M):
        same = lambda a, b: np.array_equal(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), equal_nan=True)
        assert same(logs[m], logs1[m]) and same(final[m]["U"], final1[m]["U"]) and final[m]["checksum"] == final1[m]["checksum"], ("sampling changed member", m)
        assert final[m]["nStep"] == final1[m]["nStep"] and same(final[m]["t"], final1[m]["t"])
        if m in skip:
            continue
        steps, ts, vals = series[m]
        vals = np.array(vals).reshape(len(vals), NQ)
        want = lone_series(lib, ps[m], U0s[m], nsteps, every, None if tEnds is None else tEnds[m], pre.get(m, 0))
        n0 = pre.get(m, 0)
        assert steps == want["step"] == [s for s in range(n0 + 1, n0 + done[m] + 1) if s % every == 0], (m, steps, want["step"], done[m])
        all_dts = want["dt_log"][:n0] + logs[m]
        assert ts == [ec.time_of(all_dts[:s]) for s in steps], (m, "mon_t against the accumulated dt log")
        bitwise = exact or np.array_equal(final[m]["U"], want["U"])
        if exact:
            assert ts == want["t"] and np.array_equal(final[m]["U"], want["U"]) and final[m]["checksum"] == want["checksum"], (m, "against the lone context")
        if bitwise:
            assert np.array_equal(vals, want["values"]), (m, "samples against rgpu_state_monitor of a lone context", vals, want["values"])
        else:
            print("contracted library: member %d's state is not the lone context's bit for bit; samples compared column by column" % m)
            tol = column_tolerances(final[m]["full"], ps[m])
            assert (np.abs(vals - want["values"]) <= tol[None, :]).all(), (m, np.abs(vals - want["values"]).max(axis=0), tol)
        if steps and steps[-1] == final[m]["nStep"]:
            assert np.array_equal(vals[-1], model(final[m]["full"], ps[m])), (m, "the last sample against the model of the downloaded state")
    return done, stop, fused, series
