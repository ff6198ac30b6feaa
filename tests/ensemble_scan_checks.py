"""Checks of parameter scans (rgpu_ensemble_create_scan, Ensemble.scan) shared by tests/test_ensemble_scan_host.py (the test-only host
emulation, not gpu) and tests/test_ensemble_scan_gpu.py (-m gpu): every member of a scan ensemble, created from its own parameter set,
against the oracle's run with that set and against a lone Solver created from that set on the same library."""
import ensemble_checks as ec
from conftest import ini
from ramsesgpu_amd.ensemble import Ensemble

# The parameter sets, one override string per member, in non-monotonic order so that an index mix-up shows
GAMMA = ["hydro.gamma0=1.8", "hydro.gamma0=1.3", "hydro.gamma0=1.55", "hydro.gamma0=1.4", "hydro.gamma0=1.666"]
CFL_BOX = ["hydro.cfl=0.3;mesh.xmax=1.5", "hydro.cfl=0.45", "hydro.cfl=0.2;mesh.ymax=0.8"]
ISO = ["hydro.cIso=1.1", "hydro.cIso=0.9", "hydro.cIso=1.0"]   # 2D MHD, isothermal: the generic (SPEC_NONE) kernel


def join(*ovs):
    return ";".join(o for o in ovs if o)


def scan_sets(lib, base, ov_common, member_ovs):
    """per member: (overrides, parameter set)"""
    ovs = [join(ov_common, o) for o in member_ovs]
    return ovs, [lib.params_from_ini(ini(base), o) for o in ovs]


def scan_states(lib, base, ovs, ps, seed=7, same_state=False):
    """the initial condition of member m's OWN set with the seeded perturbation of ec.member_states (same_state: every member gets
    member 0's perturbation seed -- and, where the problem's initial condition does not depend on the scanned parameter, the same state)"""
    out = []
    for m, (ov, p) in enumerate(zip(ovs, ps)):
        k = 0 if same_state else m
        out.append(ec.member_states(lib, base, ov, p, k + 1, seed)[k])
    return out


def check_scan(lib, oracle, base, ov_common, member_ovs, nsteps, exact=True, tEnds=None, same_state=False, pieces=None, seed=7, keep=False):
    """One scan ensemble, member m created from params_from_ini(base, ov_common;member_ovs[m]), run for nsteps (in `pieces`) with the
    end times tEnds(m, dts of the oracle's run of member m) -> float or None: every member == a lone Solver created from ITS set == the
    oracle's run with its set.  Returns (done, stop, fused rounds summed over the pieces[, the open ensemble, the states, the oracle's
    runs when keep])."""
    M = len(member_ovs)
    ovs, ps = scan_sets(lib, base, ov_common, member_ovs)
    U0s = scan_states(lib, base, ovs, ps, seed, same_state)
    key = lambda m: (base, ovs[m], seed, 0 if same_state else m, "scan")
    full = [ec.oracle_run(oracle, ps[m], U0s[m], nsteps, key=key(m)) for m in range(M)]
    # not vacuous (the reference side only): the parameter sets make the members' time steps differ from the first step on
    first = [float(full[m][1][0]) for m in range(M)]
    assert len(set(first)) == M, ("the parameter sets do not tell the members apart", first)
    ends = [tEnds(m, full[m][1]) if tEnds else None for m in range(M)]
    refs = [full[m] if ends[m] is None else ec.oracle_run(oracle, ps[m], U0s[m], nsteps, ends[m], key=key(m)) for m in range(M)]
    ens = Ensemble.scan(ps, lib)
    try:
        assert ens.members == M and all(ens.member(m).p is ps[m] for m in range(M))
        ens.start(U0s)
        tE = None if not tEnds else [float("inf") if e is None else e for e in ends]
        done, fused, logs = [0] * M, 0, [[] for _ in range(M)]
        for n in (pieces or [nsteps]):
            d, stop, f = ens.run_steps(n, tE)
            fused += f
            for m in range(M):
                done[m] += d[m]
                logs[m] += list(ens.member(m).dt_log)
        for m in range(M):
            v = ens.member(m)
            v.dt_log = logs[m]
            want = ec.lone_run(lib, ps[m], U0s[m], nsteps, ends[m], None, pieces)
            ec.assert_member(v, done[m], want, "scan %s[%s] member %d of %d" % (base, ovs[m], m, M), exact, refs[m])
            assert stop[m] == (1 if ends[m] is not None and v.totalTime >= ends[m] else 0), (m, stop[m], v.totalTime, ends[m])
        if keep:
            return done, stop, fused, ens, U0s, refs
        return done, stop, fused
    finally:
        if not keep:
            ens.close()
