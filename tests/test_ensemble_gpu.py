"""The ensemble of 2D boxes (rgpu_ensemble_*, csrc/hip/ensemble2d.h) on the GPU, both libraries: every member of an ensemble stepped by
one step launch and one clock launch per round == a lone context holding that member's state == the oracle -- bit for bit through
librgpu.so (every double, rgpu_state_checksum, the dt sequence), at the project's tolerance (relative L2 <= 1e-12) through
librgpu_fast.so.  Covered configurations go through the fused launch (fused_steps says so), uncovered ones, first steps and mixed
states member by member through the same API."""
import ctypes as C
import os

import numpy as np
import pytest

import ensemble_checks as ec
import parity_checks as pc
from conftest import ini
from ramsesgpu_amd.ensemble import Ensemble
from ramsesgpu_amd.solver import Solver, interior

pytestmark = pytest.mark.gpu

MIXED_FACES = "mesh.boundary_xmin=1;mesh.boundary_ymax=1;mesh.boundary_xmax=2;mesh.boundary_ymin=3;mesh.boundary_ymax=3"   # as RUN_STEPS_CASES
# problem, a size that splits unevenly over the tiles (hydro: 14 x 14 owned cells, MHD: 15 x 7), extra overrides
COVERED = [
    ("orszag-tang", "mesh.nx=53;mesh.ny=45", ""),                 # 2D MHD, periodic
    ("kelvin_helmholtz_gpu_2d", "mesh.nx=50;mesh.ny=37", ""),     # 2D hydro, periodic
    ("hydro_sod2d", "mesh.nx=70;mesh.ny=50", ""),                 # 2D hydro, outflow faces
    ("blast2d", "mesh.nx=37;mesh.ny=29", MIXED_FACES),            # 2D hydro, reflecting / outflow / periodic faces mixed
]
SIZE_128 = "mesh.nx=128;mesh.ny=128"


@pytest.fixture(params=["exact", "contracted"])
def lib(request, gpu_lib, gpu_contracted_lib):
    return gpu_lib if request.param == "exact" else gpu_contracted_lib


def exact(lib):
    return lib.arithmetic == "exact"


def fused_expected(lib):
    """the condition of tests/test_gpu_parity.py (test_run_steps_equals_the_reference_loop) for "the device-clock path runs\""""
    return not (os.environ.get("RGPU_TILED") == "0" or lib.get_option("step_clock") == 0 or lib.get_option("ghost_images") == 0)


def overrides(size, extra):
    return size + (";" + extra if extra else "")


@pytest.mark.parametrize("members", [1, 5, 64])
@pytest.mark.parametrize("size", ["uneven", "128"])
@pytest.mark.parametrize("base,uneven,extra", COVERED, ids=[c[0] for c in COVERED])
def test_covered_cases(base, uneven, extra, size, members, lib, oracle):
    n = 10
    ov = overrides(uneven if size == "uneven" else SIZE_128, extra)
    done, stop, fused = ec.check_ensemble(lib, oracle, base, ov, members, n, exact=exact(lib))
    assert done == [n] * members and stop == [0] * members
    if fused_expected(lib):
        assert fused == n - 1   # the first step of a run is the plain one


def test_more_steps_than_one_clock_batch(lib, oracle):
    """300 steps of a 48 x 40 box, 5 members: more rounds than one batch of device clock records (RGPU_CLOCK_BATCH = 256)"""
    n = 300
    done, stop, fused = ec.check_ensemble(lib, oracle, "orszag-tang", "mesh.nx=48;mesh.ny=40", 5, n, exact=exact(lib))
    assert done == [n] * 5
    if fused_expected(lib):
        assert fused == n - 1


STOPPING = [("orszag-tang", "mesh.nx=53;mesh.ny=45"), ("hydro_sod2d", "mesh.nx=70;mesh.ny=50")]


@pytest.mark.parametrize("base,ov", STOPPING, ids=[c[0] for c in STOPPING])
def test_members_stopping_at_different_steps(base, ov, lib, oracle):
    n, cuts = 12, {1: 4, 2: 7, 3: 5}   # member: the step that carries its t past its end time
    ends = lambda m, dts: ec.end_inside_step(dts, cuts[m]) if m in cuts else None
    done, stop, fused = ec.check_ensemble(lib, oracle, base, ov, 5, n, exact=exact(lib), tEnds=ends)
    assert done == [cuts.get(m, n) for m in range(5)] and stop == [1 if m in cuts else 0 for m in range(5)]
    if fused_expected(lib):
        assert fused == n - 1
    # split as 3 + the rest: the second call starts on states the fused kernels left
    done, stop, fused = ec.check_ensemble(lib, oracle, base, ov, 5, n, exact=exact(lib), pieces=[3, n - 3])
    if fused_expected(lib):
        assert fused == (3 - 1) + (n - 3)


@pytest.mark.parametrize("base,ov", STOPPING, ids=[c[0] for c in STOPPING])
def test_second_call_with_a_later_end_and_mixed_parity(base, ov, lib, oracle):
    """members stopped after 3 and 4 of 8 steps go on in a second call without an end: the running members then differ in step
    parity -- whatever path the call takes, every member equals the oracle and a lone context driven the same way"""
    p = lib.params_from_ini(ini(base), ov)
    M, n1, n2, cuts = 4, 8, 6, {1: 3, 2: 4}
    U0s = ec.member_states(lib, base, ov, p, M)
    full = [ec.oracle_run(oracle, p, U0s[m], n1, key=(base, ov, 7, m)) for m in range(M)]
    ends = [ec.end_inside_step(full[m][1], cuts[m]) if m in cuts else float("inf") for m in range(M)]
    ens = Ensemble(p, M, lib)
    try:
        ens.start(U0s)
        done, stop, _ = ens.run_steps(n1, ends)
        assert done == [cuts.get(m, n1) for m in range(M)] and stop == [1 if m in cuts else 0 for m in range(M)]
        logs = [list(ens.member(m).dt_log) for m in range(M)]
        done2, stop2, _ = ens.run_steps(n2, None)
        assert done2 == [n2] * M and stop2 == [0] * M
        for m in range(M):
            v = ens.member(m)
            v.dt_log = logs[m] + list(v.dt_log)
            sv = Solver(p, lib)
            try:
                sv.start(U0s[m], 0)
                d1 = sv.run_steps(n1, ends[m])
                log = list(sv.dt_log)
                d2 = sv.run_steps(n2)
                want = {"U": interior(sv.getDataHost(), p).copy(), "nStep": sv.nStep, "t": sv.totalTime, "dt": sv.dt, "dt_log": log + list(sv.dt_log), "done": d1 + d2,
                        "checksum": sv.state_checksum(sv.nStep % 2)}
            finally:
                sv.close()
            ref = ec.oracle_run(oracle, p, U0s[m], cuts.get(m, n1) + n2, key=(base, ov, 7, m))
            ec.assert_member(v, done[m] + done2[m], want, "%s member %d" % (base, m), exact(lib), ref)
    finally:
        ens.close()


UNCOVERED = [
    ("mhd_BrioWu", "mesh.nx=128;mesh.ny=8"),               # 2D MHD with Neumann faces: no ghost images, the plain loop
    ("rayleigh_taylor_gpu_2d", "mesh.nx=40;mesh.ny=120"),  # gravity: (0.5 dt) g is a kernel argument
    ("jet2d_cpu", "mesh.nx=40;mesh.ny=120"),               # jet inflow: a ghost fill every step
    ("kelvin_helmholtz_gpu_2d", "mesh.nx=50;mesh.ny=37;hydro.nu=0.01"),   # viscous / resistive stage behind the step: no device clock
    ("orszag-tang", "mesh.nx=53;mesh.ny=45;MHD.eta=0.02"),                # (csrc/api/entry_clock.h)
]


@pytest.mark.parametrize("base,ov", UNCOVERED, ids=[c[0] for c in UNCOVERED])
def test_uncovered_configurations_take_the_fallback(base, ov, lib, oracle):
    p = lib.params_from_ini(ini(base), ov)
    G = pc.attach_gravity(lib, base, ov, p, oracle=oracle)   # the oracle's field; each member gets its own copy below
    prepare = (lambda sv: sv.set_gravity_field(G)) if G is not None else None
    try:
        done, stop, fused = ec.check_ensemble(lib, oracle, base, ov, 3, 8, exact=exact(lib), prepare=prepare)
        assert done == [8] * 3 and stop == [0] * 3 and fused == 0
    finally:
        oracle.set_gravity_field(None)


def _lone_log(lib, p, U0, nsteps):
    """rgpu_run_steps_log on a lone context, whatever it returns: (rc, nStep, t, dt, dt_log[:steps done], state)"""
    sv = Solver(p, lib)
    try:
        sv.upload(U0, both=False)
        sv.make_all_boundaries(0, 0.0, 0.0)
        sv.upload(sv.getDataHost(0), both=True)
        n, t, d = C.c_int(0), C.c_double(0.0), C.c_double(0.0)
        log = (C.c_double * nsteps)()
        rc = lib.lib.rgpu_run_steps_log(sv.ctx, nsteps, float("inf"), C.byref(n), C.byref(t), C.byref(d), log)
        return rc, n.value, t.value, d.value, [log[i] for i in range(n.value)], interior(sv.getDataHost(n.value), p).copy()
    finally:
        sv.close()


@pytest.mark.parametrize("base,ov", STOPPING, ids=[c[0] for c in STOPPING])
def test_one_member_poisoned(base, ov, lib, oracle):
    """a NaN density in one interior cell of one member (arithmetic, not a fault): that member's outcome is what rgpu_run_steps_log
    reports for a lone context with that state; every other member still equals the oracle"""
    p = lib.params_from_ini(ini(base), ov)
    M, n, bad = 4, 8, 2
    U0s = ec.member_states(lib, base, ov, p, M)
    gw = p.ghostWidth
    U0s[bad][0, 0, gw + p.ny // 2, gw + p.nx // 3] = np.nan
    rc, nS, t, d, log, U = _lone_log(lib, p, U0s[bad], n)
    ens = Ensemble(p, M, lib)
    try:
        ens.start(U0s)
        done, stop, fused = ens.run_steps(n, None)
        v = ens.member(bad)
        same = lambda a, b: np.array_equal(np.array(a, dtype=np.float64), np.array(b, dtype=np.float64), equal_nan=True)
        print("poisoned member of %s: lone rc %d, %d steps; ensemble done %d stop %d" % (base, rc, nS, done[bad], stop[bad]))
        assert done[bad] == nS and v.nStep == nS and (stop[bad] in (2, 3)) == (rc < 0), (done, stop, rc, nS)
        got = interior(v.getDataHost(), p)
        if exact(lib):
            assert same([v.totalTime, v.dt], [t, d]) and same(v.dt_log, log) and same(got, U)
        else:
            # the contracted library, at the project's tolerance: the same cells are numbers, and those agree; so do t, dt and the dt log
            # (numbers within 1e-11 relative, anything else -- inf, NaN -- alike)
            ok = np.isfinite(U)
            assert np.array_equal(ok, np.isfinite(got)) and same(got[~ok], U[~ok])
            assert pc.rel_l2(got[ok], U[ok]) <= pc.L2_TOLERANCE, pc.rel_l2(got[ok], U[ok])
            a, b = np.array([v.totalTime, v.dt] + list(v.dt_log)), np.array([t, d] + list(log))
            fin = np.isfinite(b)
            assert np.array_equal(fin, np.isfinite(a)) and same(a[~fin], b[~fin]) and np.all(np.abs(a[fin] - b[fin]) <= 1e-11 * np.abs(b[fin]))
        # what the poison does is arithmetic and is pinned by the lone context, not assumed: either the member's time step breaks down
        # (stop 2 / 3, the lone call fails) or the NaN spreads through its state while its finite cells keep the CFL maximum
        assert (stop[bad] in (2, 3)) or not np.isfinite(got).all(), "the poisoned member shows no trace of its NaN"
        for m in range(M):
            if m == bad:
                continue
            w = ens.member(m)
            ref = ec.oracle_run(oracle, p, U0s[m], n, key=(base, ov, 7, m))
            assert done[m] == n and stop[m] == 0 and w.nStep == n
            pc.assert_same(interior(w.getDataHost(), p), interior(ref[0], p), "%s member %d beside a poisoned one" % (base, m), exact=exact(lib))
            if exact(lib):
                assert w.dt_log == [float(x) for x in ref[1]]
    finally:
        ens.close()


AFTERWARDS = [("orszag-tang", "mesh.nx=53;mesh.ny=45"), ("blast2d", "mesh.nx=37;mesh.ny=29;" + MIXED_FACES), ("jet2d_cpu", "mesh.nx=40;mesh.ny=120")]


@pytest.mark.parametrize("base,ov", AFTERWARDS, ids=[c[0] for c in AFTERWARDS])
def test_member_contexts_afterwards(base, ov, lib, oracle):
    """after an ensemble call a member context is in the state the single-context loop would have left: rgpu_device_time_step_ready
    answers as for a lone context, and a lone run_steps on one member continues to the oracle's state"""
    n, more = 6, 5
    done, stop, fused, ens, U0s, refs = ec.check_ensemble(lib, oracle, base, ov, 3, n, exact=exact(lib), keep=True)
    try:
        p = ens.p
        sv = Solver(p, lib)
        try:
            sv.start(U0s[1], 0)
            sv.run_steps(n)
            ready = lib.lib.rgpu_device_time_step_ready(sv.ctx, sv.nStep % 2)
        finally:
            sv.close()
        for m in range(3):
            v = ens.member(m)
            assert lib.lib.rgpu_device_time_step_ready(v.ctx, v.nStep % 2) == ready
        v = ens.member(1)
        assert v.run_steps(more) == more
        ref = ec.oracle_run(oracle, p, U0s[1], n + more, key=(base, ov, 7, 1))
        assert v.nStep == n + more
        pc.assert_same(interior(v.getDataHost(), p), interior(ref[0], p), "%s member 1 alone after the ensemble call" % base, exact=exact(lib))
        if exact(lib):
            assert v.dt_log == [float(x) for x in ref[1][n:]] and v.totalTime == ec.time_of(ref[1])
        # and the others are untouched by that
        pc.assert_same(interior(ens.member(0).getDataHost(), p), interior(refs[0][0], p), "%s member 0" % base, exact=exact(lib))
    finally:
        ens.close()


def test_contracted_library_bit_equality_is_reported(gpu_contracted_lib, oracle):
    """librgpu_fast.so: the ensemble kernels run the single-box body, so the members are expected to equal a lone context bit for bit
    although only the tolerance is promised; this prints what was observed over the members compared in this process"""
    ec.check_ensemble(gpu_contracted_lib, oracle, "orszag-tang", "mesh.nx=53;mesh.ny=45", 5, 10, exact=False)
    seen = ec.BIT_EQUAL_TO_LONE
    print("contracted library: %d of %d members compared with a lone context were bit-equal to it" % (sum(seen), len(seen)))
    assert seen
