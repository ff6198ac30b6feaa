"""Checks of the ensemble of 2D boxes (rgpu_ensemble_*, ramsesgpu_amd/ensemble.py) shared by tests/test_ensemble_host.py (the test-only
host emulation, not gpu) and tests/test_ensemble_gpu.py (-m gpu): every member of an ensemble against the oracle's run of that member's
initial state and against a lone Solver on the same library."""
import numpy as np

import parity_checks as pc
from conftest import ini
from ramsesgpu_amd import _capi
from ramsesgpu_amd.ensemble import Ensemble
from ramsesgpu_amd.solver import Solver, interior

NO_END = 1e300   # "no end time" for the oracle (the libraries take HUGE_VAL / None)


def member_states(lib, base, ov, p, members, seed=7, amplitude=1e-3):
    """the problem's initial condition with a seeded perturbation of density and momenta per member (energy and the face field are
    left alone: div B stays 0, the pressure stays positive at this amplitude)"""
    U0 = lib.init_condition(ini(base), ov, p)
    out = []
    for m in range(members):
        rng = np.random.default_rng(1000 * seed + m)
        U = U0.copy()
        U[_capi.ID] *= 1.0 + amplitude * rng.uniform(-1.0, 1.0, U[_capi.ID].shape)
        for v in (_capi.IU, _capi.IV) + ((_capi.IW,) if p.nbVar > 4 else ()):
            U[v] += amplitude * rng.uniform(-1.0, 1.0, U[v].shape) * U0[_capi.ID]
        out.append(U)
    return out


_ORACLE_RUNS = {}        # the last runs asked for under a key, oldest first; at most ORACLE_MEMO_BYTES of states
ORACLE_MEMO_BYTES = 256 << 20


def oracle_run(oracle, p, U0, nsteps, tEnd=NO_END, key=None):
    """oracle.run; key != None: remembered under it (the exact and the contracted library ask for the same runs of the same seeded
    states, each far below the size from which Oracle.run keeps results itself).  The caller passes no key where the oracle was
    handed a field of its own (gravity) that the key does not name."""
    if key is None:
        return oracle.run_sequential(p, U0, nsteps, tEnd)
    k = key + (int(nsteps), float(tEnd))
    if k not in _ORACLE_RUNS:
        _ORACLE_RUNS[k] = oracle.run_sequential(p, U0, nsteps, tEnd)
        while sum(v[0].nbytes for v in _ORACLE_RUNS.values()) > ORACLE_MEMO_BYTES and len(_ORACLE_RUNS) > 1:
            _ORACLE_RUNS.pop(next(iter(_ORACLE_RUNS)))
    U, dts, t = _ORACLE_RUNS[k]
    return U.copy(), dts.copy(), t


def time_of(dts):
    """t after the steps dts, accumulated in the order of the reference's loop"""
    t = 0.0
    for d in dts:
        t += float(d)
    return t


def end_inside_step(dts, k):
    """an end time that the k-th step (1-based) of the dt list carries t past"""
    return time_of(dts[:k]) - 0.25 * float(dts[k - 1])


def lone_run(lib, p, U0, nsteps, tEnd=None, prepare=None, pieces=None):
    """a lone Solver holding U0: run_steps in the given pieces; returns what the ensemble must reproduce for that member"""
    sv = Solver(p, lib)
    try:
        if prepare:
            prepare(sv)
        sv.start(U0, 0)
        done, log = 0, []
        for n in (pieces or [nsteps]):
            done += sv.run_steps(n, float("inf") if tEnd is None else tEnd)
            log += list(sv.dt_log)
        return {"U": interior(sv.getDataHost(), p).copy(), "nStep": sv.nStep, "t": sv.totalTime, "dt": sv.dt, "dt_log": log, "done": done,
                "checksum": sv.state_checksum(sv.nStep % 2)}
    finally:
        sv.close()


BIT_EQUAL_TO_LONE = []   # contracted library: one entry per member compared with a lone context


def assert_member(view, got_done, want, what, exact=True, ref=None):
    """view: the member's Solver view after the ensemble call; want: lone_run's answer; ref: (U, dts, t) of the oracle or None"""
    p = view.p
    U = interior(view.getDataHost(), p)
    assert got_done == want["done"] and view.nStep == want["nStep"], (what, got_done, want["done"], view.nStep, want["nStep"])
    if exact:
        assert view.totalTime == want["t"] and view.dt == want["dt"], (what, view.totalTime, want["t"], view.dt, want["dt"])
        assert list(view.dt_log) == list(want["dt_log"]), (what, "dt_log")
        assert np.array_equal(U, want["U"], equal_nan=True), "%s: state differs from the lone context's" % what
        assert view.state_checksum(view.nStep % 2) == want["checksum"], (what, "checksum")
    else:
        # the contracted library: the stated tolerance; whether the bits were equal all the same is reported (BIT_EQUAL_TO_LONE)
        BIT_EQUAL_TO_LONE.append(bool(np.array_equal(U, want["U"], equal_nan=True) and list(view.dt_log) == list(want["dt_log"])))
        assert abs(view.totalTime - want["t"]) <= 1e-11 * abs(want["t"]) and abs(view.dt - want["dt"]) <= 1e-11 * abs(want["dt"]), (what, view.totalTime, want["t"])
        assert pc.rel_l2(U, want["U"]) <= pc.L2_TOLERANCE, (what, pc.rel_l2(U, want["U"]))
    if ref is None:
        return
    Uref, dts, t = ref
    assert view.nStep == len(dts), (what, view.nStep, len(dts))
    if exact:
        assert list(view.dt_log) == [float(d) for d in dts[len(dts) - len(view.dt_log):]], (what, "dt_log against the oracle")
        assert view.totalTime == time_of(dts), (what, view.totalTime, time_of(dts))
        pc.assert_same(U, interior(Uref, p), what, exact=True)
    else:
        pc.assert_same(U, interior(Uref, p), what, exact=False)
        assert np.abs(np.array(view.dt_log) / np.array(dts[len(dts) - len(view.dt_log):]) - 1.0).max() < 1e-11, (what, "dt_log against the oracle")


def check_ensemble(lib, oracle, base, ov, members, nsteps, exact=True, tEnds=None, pieces=None, prepare=None, seed=7, states=None, lone=True, keep=False):
    """One ensemble of `members` perturbed copies of the problem, run for nsteps (in `pieces`) with the end times tEnds(m, dts of the
    oracle's run of member m) -> float or None: every member == a lone Solver (when `lone`) == the oracle.  Returns (done, stop, fused
    rounds summed over the pieces[, the open ensemble and the oracle runs when keep])."""
    p = lib.params_from_ini(ini(base), ov)
    U0s = states or member_states(lib, base, ov, p, members, seed)
    key = lambda m: (base, ov, seed, m) if states is None and prepare is None else None   # (prepare: a gravity field went to the oracle too)
    full = [oracle_run(oracle, p, U0s[m], nsteps, key=key(m)) for m in range(members)]
    ends = [tEnds(m, full[m][1]) if tEnds else None for m in range(members)]
    refs = [full[m] if ends[m] is None else oracle_run(oracle, p, U0s[m], nsteps, ends[m], key=key(m)) for m in range(members)]
    ens = Ensemble(p, members, lib)
    try:
        if prepare:
            for m in range(members):
                prepare(ens.member(m))
        ens.start(U0s)
        tE = None if not tEnds else [float("inf") if e is None else e for e in ends]
        done, fused, logs = [0] * members, 0, [[] for _ in range(members)]
        for n in (pieces or [nsteps]):
            d, stop, f = ens.run_steps(n, tE)
            fused += f
            for m in range(members):
                done[m] += d[m]
                logs[m] += list(ens.member(m).dt_log)
        for m in range(members):
            v = ens.member(m)
            v.dt_log = logs[m]
            want = lone_run(lib, p, U0s[m], nsteps, None if ends[m] is None else ends[m], prepare, pieces) if lone else None
            if want is None:   # the oracle alone
                want = {"U": interior(v.getDataHost(), p), "nStep": len(refs[m][1]), "t": v.totalTime, "dt": v.dt, "dt_log": logs[m], "done": len(refs[m][1]),
                        "checksum": v.state_checksum(v.nStep % 2)}
            assert_member(v, done[m], want, "%s[%s] member %d of %d" % (base, ov, m, members), exact, refs[m])
            assert stop[m] == (1 if ends[m] is not None and v.totalTime >= ends[m] else 0), (m, stop[m], v.totalTime, ends[m])
        if keep:
            return done, stop, fused, ens, U0s, refs
        return done, stop, fused
    finally:
        if not keep:
            ens.close()
