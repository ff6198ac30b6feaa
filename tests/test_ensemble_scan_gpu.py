"""Parameter scans (rgpu_ensemble_create_scan, csrc/hip/ensemble_scan.h) on the GPU, both libraries: every member of a scan ensemble --
its constants read from the per-member table by one step launch and one clock launch per round -- == a lone context created from that
member's parameter set == the oracle's run with that set: bit for bit through librgpu.so, at the project's tolerance (relative L2 <=
1e-12) through librgpu_fast.so.  Sizes as tests/test_ensemble_gpu.py: no tile count divides them (hydro tiles own 14 x 14 cells, MHD
tiles 15 x 7).  All three parameter sets (ensemble_scan_checks.py) were run on the host emulation and the oracle for 10 steps first:
every dt is finite with the values the sets were specified with, none had to be moved."""
import numpy as np
import pytest

import ensemble_checks as ec
import ensemble_scan_checks as sc
import parity_checks as pc
from conftest import ini
from ramsesgpu_amd.ensemble import Ensemble
from ramsesgpu_amd.solver import Solver, interior
from test_ensemble_gpu import MIXED_FACES, exact, fused_expected

pytestmark = pytest.mark.gpu

OT, KH, BLAST, SOD = "orszag-tang", "kelvin_helmholtz_gpu_2d", "blast2d", "hydro_sod2d"
OT_SIZE, KH_SIZE, BLAST_SIZE, SOD_SIZE = "mesh.nx=53;mesh.ny=45", "mesh.nx=50;mesh.ny=37", "mesh.nx=37;mesh.ny=29;" + MIXED_FACES, "mesh.nx=70;mesh.ny=50"
# What tests/test_ensemble_scan_resources.py declares for mhd2d_scan_kernel<0> (the generic 2D MHD kernel, at the scalar-register limit):
# it places like mhd2d_ensemble_kernel<0>, so no retreat was taken and an isothermal scan runs fused
ISO_SCAN_IS_FUSED = True


@pytest.fixture(params=["exact", "contracted"])
def lib(request, gpu_lib, gpu_contracted_lib):
    return gpu_lib if request.param == "exact" else gpu_contracted_lib


SCANS = [
    ("gamma", OT, OT_SIZE, sc.GAMMA), ("gamma", KH, KH_SIZE, sc.GAMMA), ("gamma", BLAST, BLAST_SIZE, sc.GAMMA),
    ("cfl_box", OT, OT_SIZE, sc.CFL_BOX), ("cfl_box", SOD, SOD_SIZE, sc.CFL_BOX),
]


@pytest.mark.parametrize("name,base,size,sets", SCANS, ids=["%s-%s" % (c[0], c[1]) for c in SCANS])
def test_scan_members_equal_lone_contexts_and_the_oracle(name, base, size, sets, lib, oracle):
    n = 10
    done, stop, fused = sc.check_scan(lib, oracle, base, size, sets, n, exact=exact(lib))
    assert done == [n] * len(sets) and stop == [0] * len(sets)
    if fused_expected(lib):
        assert fused == n - 1   # the first step of a run is the plain one


def test_isothermal_scan_through_the_generic_mhd_kernel(lib, oracle):
    """cIso differs from member to member: SPEC_NONE, the 2D MHD kernel at the scalar-register limit"""
    n = 10
    done, stop, fused = sc.check_scan(lib, oracle, OT, OT_SIZE, sc.ISO, n, exact=exact(lib))
    assert done == [n] * 3 and stop == [0] * 3
    if ISO_SCAN_IS_FUSED:
        if fused_expected(lib):
            assert fused == n - 1
    else:
        assert fused == 0


@pytest.mark.parametrize("base,size", [(OT, OT_SIZE), (KH, KH_SIZE)], ids=[OT, KH])
def test_identical_states_differing_gamma_only(base, size, lib, oracle):
    """every member starts from the same perturbation; only gamma0 differs.  A launch that handed every member one parameter set would
    leave the members equal -- and fail against the oracle's runs, whose time steps differ from the first (check_scan asserts that)"""
    n = 10
    done, stop, fused = sc.check_scan(lib, oracle, base, size, sc.GAMMA, n, exact=exact(lib), same_state=True)
    assert done == [n] * 5
    if fused_expected(lib):
        assert fused == n - 1


@pytest.mark.parametrize("base,size", [(OT, OT_SIZE), (SOD, SOD_SIZE)], ids=[OT, SOD])
def test_scan_members_stopping_at_different_steps(base, size, lib, oracle):
    n, cuts = 12, {1: 4, 2: 7, 3: 5}   # member: the step that carries its t past its end time; the table stays indexed by member
    ends = lambda m, dts: ec.end_inside_step(dts, cuts[m]) if m in cuts else None
    done, stop, fused = sc.check_scan(lib, oracle, base, size, sc.GAMMA, n, exact=exact(lib), tEnds=ends)
    assert done == [cuts.get(m, n) for m in range(5)] and stop == [1 if m in cuts else 0 for m in range(5)]
    if fused_expected(lib):
        assert fused == n - 1
    # split as 3 + the rest: the second call starts on states the fused kernels left
    done, stop, fused = sc.check_scan(lib, oracle, base, size, sc.GAMMA, n, exact=exact(lib), pieces=[3, n - 3])
    if fused_expected(lib):
        assert fused == (3 - 1) + (n - 3)


def test_scan_more_steps_than_one_clock_batch(lib, oracle):
    """300 steps of a 48 x 40 box: more rounds than one batch of device clock records (RGPU_CLOCK_BATCH = 256)"""
    n = 300
    done, stop, fused = sc.check_scan(lib, oracle, OT, "mesh.nx=48;mesh.ny=40", sc.GAMMA, n, exact=exact(lib))
    assert done == [n] * 5
    if fused_expected(lib):
        assert fused == n - 1


def _uniform_run(lib, p, U0s, n):
    ens = Ensemble(p, len(U0s), lib)
    try:
        ens.start(U0s)
        done, stop, fused = ens.run_steps(n)
        out = []
        for m in range(len(U0s)):
            v = ens.member(m)
            out.append({"U": interior(v.getDataHost(), p).copy(), "nStep": v.nStep, "t": v.totalTime, "dt": v.dt, "dt_log": list(v.dt_log),
                        "checksum": v.state_checksum(v.nStep % 2)})
        return done, stop, fused, out
    finally:
        ens.close()


@pytest.mark.parametrize("base,size", [(OT, OT_SIZE), (BLAST, BLAST_SIZE)], ids=[OT, BLAST])
def test_option_member_params_on_a_uniform_ensemble(base, size, lib, oracle):
    """option member_params = 1: a plain Ensemble(p, 5) through the table path == the same run through the by-value path"""
    n, M = 10, 5
    p = lib.params_from_ini(ini(base), size)
    U0s = ec.member_states(lib, base, size, p, M)
    assert lib.get_option("member_params") == 0
    d0, s0, f0, by_value = _uniform_run(lib, p, U0s, n)
    old = lib.set_option("member_params", 1)
    try:
        d1, s1, f1, by_table = _uniform_run(lib, p, U0s, n)
    finally:
        lib.set_option("member_params", old)
    assert (d0, s0, f0) == (d1, s1, f1)
    if fused_expected(lib):
        assert f1 == n - 1
    for m in range(M):
        a, b = by_value[m], by_table[m]
        assert a["nStep"] == b["nStep"] == n
        if exact(lib):
            assert (a["t"], a["dt"], a["dt_log"], a["checksum"]) == (b["t"], b["dt"], b["dt_log"], b["checksum"]), m
            assert np.array_equal(a["U"], b["U"]), m
        else:
            assert abs(a["t"] - b["t"]) <= 1e-11 * abs(a["t"]) and pc.rel_l2(b["U"], a["U"]) <= pc.L2_TOLERANCE, (m, pc.rel_l2(b["U"], a["U"]))
        ref = ec.oracle_run(oracle, p, U0s[m], n, key=(base, size, 7, m))
        pc.assert_same(b["U"], interior(ref[0], p), "%s member %d through the table" % (base, m), exact=exact(lib))


@pytest.mark.parametrize("base,size", [(OT, OT_SIZE), (BLAST, BLAST_SIZE)], ids=[OT, BLAST])
def test_scan_member_contexts_afterwards(base, size, lib, oracle):
    """after a scan call a member context is in the state the single-context loop would have left a lone context of ITS set in:
    rgpu_device_time_step_ready answers alike, and run_steps on member 1 alone continues to the oracle's state"""
    n, more = 6, 5
    done, stop, fused, ens, U0s, refs = sc.check_scan(lib, oracle, base, size, sc.GAMMA, n, exact=exact(lib), keep=True)
    try:
        ovs, ps = sc.scan_sets(lib, base, size, sc.GAMMA)
        for m in range(len(ps)):
            sv = Solver(ps[m], lib)
            try:
                sv.start(U0s[m], 0)
                sv.run_steps(n)
                ready = lib.lib.rgpu_device_time_step_ready(sv.ctx, sv.nStep % 2)
            finally:
                sv.close()
            v = ens.member(m)
            assert lib.lib.rgpu_device_time_step_ready(v.ctx, v.nStep % 2) == ready, m
        v, p1 = ens.member(1), ps[1]
        assert v.run_steps(more) == more and v.nStep == n + more
        ref = ec.oracle_run(oracle, p1, U0s[1], n + more, key=(base, ovs[1], 7, 1, "scan"))
        pc.assert_same(interior(v.getDataHost(), p1), interior(ref[0], p1), "%s member 1 alone after the scan call" % base, exact=exact(lib))
        if exact(lib):
            assert v.dt_log == [float(x) for x in ref[1][n:]] and v.totalTime == ec.time_of(ref[1])
        pc.assert_same(interior(ens.member(0).getDataHost(), ps[0]), interior(refs[0][0], ps[0]), "%s member 0" % base, exact=exact(lib))   # untouched by that
    finally:
        ens.close()
