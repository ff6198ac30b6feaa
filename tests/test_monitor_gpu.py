"""The monitors (include/rgpu.h, "monitors"; csrc/hip/ensemble_monitor.h) on the GPU, both libraries: samples taken by the monitor
kernels inside the batches of fused rounds == rgpu_state_monitor of a lone context after the same number of steps == the numpy model
of the documented definition on the downloaded state (tests/monitor_checks.py), bit for bit; sampling changes no state, dt sequence or
checksum; members with different step counts, end times, a poisoned neighbour, per-member dx of a parameter scan, and the
member-by-member fallback."""
import numpy as np
import pytest

import ensemble_checks as ec
import ensemble_scan_checks as sc
import monitor_checks as mc
from conftest import ini
from ramsesgpu_amd.solver import Solver
from test_ensemble_gpu import exact, fused_expected

pytestmark = pytest.mark.gpu

OT, KH = "orszag-tang", "kelvin_helmholtz_gpu_2d"
OT_SIZE, KH_SIZE = "mesh.nx=40;mesh.ny=24", "mesh.nx=72;mesh.ny=20"   # no tile count divides them; 72 columns: more than one wavefront of lanes
N = 10


@pytest.fixture(params=["exact", "contracted"])
def lib(request, gpu_lib, gpu_contracted_lib):
    return gpu_lib if request.param == "exact" else gpu_contracted_lib


def setup(lib, base, ov, members):
    p = lib.params_from_ini(ini(base), ov)
    return p, ec.member_states(lib, base, ov, p, members)


@pytest.mark.parametrize("base,ov", [(OT, "mesh.nx=24;mesh.ny=40"), (KH, KH_SIZE)], ids=[OT, KH])
def test_state_monitor_equals_the_model(base, ov, lib):
    """the kernels of a lone context on the device: after 0 and 3 steps, bit for bit the numpy model in both libraries"""
    p, (U0,) = setup(lib, base, ov, 1)
    sv = Solver(p, lib)
    try:
        sv.start(U0, 0)
        for steps in (0, 3):
            if steps:
                assert sv.run_steps(steps) == steps
            par = sv.nStep % 2
            ready, checksum = lib.lib.rgpu_device_time_step_ready(sv.ctx, par), sv.state_checksum(par)
            got, U = sv.state_monitor(), sv.getDataHost()
            assert np.array_equal(got, mc.model(U, p)), (got, mc.model(U, p))
            mc.assert_within_any_order_bound(got, U, p)
            assert lib.lib.rgpu_device_time_step_ready(sv.ctx, par) == ready and sv.state_checksum(par) == checksum
    finally:
        sv.close()


@pytest.mark.parametrize("every", [1, 3])
@pytest.mark.parametrize("base,ov,members", [(OT, OT_SIZE, 5), (KH, KH_SIZE, 3)], ids=[OT, KH])
def test_fused_rounds_are_sampled_on_the_device(base, ov, members, every, lib):
    p, U0s = setup(lib, base, ov, members)
    done, stop, fused, series = mc.check_monitored(lib, [p] * members, U0s, N, every, exact=exact(lib))
    assert done == [N] * members and stop == [0] * members
    assert [s[0] for s in series] == [[n for n in range(1, N + 1) if n % every == 0]] * members
    if fused_expected(lib):
        assert fused == N - 1   # the first step of a run is the plain one: its sample (every == 1) comes from the monitor of the member's context


def test_members_with_different_step_counts(lib):
    """member 1 has taken 2 steps alone before the call (same parity, another nStep): the batch stays fused and every member is sampled
    at ITS multiples of 3 -- member 1 after rounds 1, 4, 7, 10 of the call, the others after rounds 3, 6, 9"""
    p, U0s = setup(lib, OT, OT_SIZE, 3)
    done, stop, fused, series = mc.check_monitored(lib, [p] * 3, U0s, N, 3, pre={1: 2}, exact=exact(lib))
    assert done == [N] * 3 and [s[0] for s in series] == [[3, 6, 9], [3, 6, 9, 12], [3, 6, 9]]
    if fused_expected(lib):
        assert fused == N - 1


def test_member_reaching_its_end_inside_the_batch(lib):
    """a stopped record: member 1 stops with its 6th step, a multiple of 3 -- that step is sampled, nothing after it; member 2 with its
    5th -- no sample but the one at 3"""
    p, U0s = setup(lib, OT, OT_SIZE, 4)
    dts = [ec.lone_run(lib, p, U0s[m], N)["dt_log"] for m in (1, 2)]
    ends = [None, ec.end_inside_step(dts[0], 6), ec.end_inside_step(dts[1], 5), None]
    done, stop, fused, series = mc.check_monitored(lib, [p] * 4, U0s, N, 3, tEnds=ends, exact=exact(lib))
    assert done == [N, 6, 5, N] and stop == [0, 1, 1, 0]
    assert [s[0] for s in series] == [[3, 6, 9], [3, 6], [3], [3, 6, 9]]
    if fused_expected(lib):
        assert fused == N - 1


def test_a_poisoned_member_does_not_disturb_the_others(lib):
    """a NaN density in one interior cell of member 2 (as test_one_member_poisoned, tests/test_ensemble_gpu.py): the other members'
    series are those of lone contexts; the poisoned member's own monitor follows the documented NaN rules"""
    p, U0s = setup(lib, OT, OT_SIZE, 4)
    bad, gw = 2, p.ghostWidth
    U0s[bad][0, 0, gw + p.ny // 2, gw + p.nx // 3] = np.nan
    done, stop, fused, series = mc.check_monitored(lib, [p] * 4, U0s, 8, 1, exact=exact(lib), skip=(bad,))
    assert [done[m] for m in (0, 1, 3)] == [8] * 3 and [s[0] for m, s in enumerate(series) if m != bad] == [list(range(1, 9))] * 3
    # the poisoned member itself: check_monitored holds its monitor before and after the run to the NaN rules of include/rgpu.h (the
    # NaN cell drops out of min_rho / min_eint, which equal np.fmin over its downloaded state, and makes its sums NaN); every sample
    # it got shows the NaN in the mass
    assert all(np.isnan(v[0]) for v in series[bad][2])


def test_scan_members_take_their_own_dx(lib):
    """sc.CFL_BOX: the box length, hence dx or dy, differs from member to member: max |div B| (and every other value) of member m equals
    the lone context's created from ITS set; the series under option member_params = 1 are the same"""
    ovs, ps = sc.scan_sets(lib, OT, OT_SIZE, sc.CFL_BOX)
    assert len({(q.dx, q.dy) for q in ps}) == len(ps)
    U0s = sc.scan_states(lib, OT, ovs, ps)
    runs = []
    for option in (0, 1):
        old = lib.set_option("member_params", option)
        try:
            done, stop, fused, series = mc.check_monitored(lib, ps, U0s, N, 3, scan=True, exact=exact(lib))
        finally:
            lib.set_option("member_params", old)
        assert done == [N] * len(ps)
        if fused_expected(lib):
            assert fused == N - 1
        runs.append(series)
    for a, b in zip(*runs):
        assert a[0] == b[0] == [3, 6, 9] and a[1] == b[1] and np.array_equal(np.array(a[2]), np.array(b[2]))
        assert all(v[9] > 0.0 for v in a[2])   # not vacuous: div B is round-off, not zero, after a step


def test_uncovered_configuration_is_sampled_member_by_member(lib):
    """2D MHD with Neumann faces: no fused round; the samples come from the monitor of each member's context"""
    base, ov = "mhd_BrioWu", "mesh.nx=128;mesh.ny=8"
    p, U0s = setup(lib, base, ov, 3)
    done, stop, fused, series = mc.check_monitored(lib, [p] * 3, U0s, 6, 2, exact=exact(lib))
    assert done == [6] * 3 and fused == 0 and [s[0] for s in series] == [[2, 4, 6]] * 3
