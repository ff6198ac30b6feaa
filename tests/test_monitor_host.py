"""The monitors (include/rgpu.h, "monitors") without a GPU, on the test-only host emulation: rgpu_state_monitor against the numpy model
of the documented definition (tests/monitor_checks.py) bit for bit and against the bound that holds for any summation order; the
argument checks; and rgpu_ensemble_run_steps_monitored / rgpu_ensemble_monitor with every round member by member (the emulation has
no ensemble kernels: fused == 0) against a lone Solver and against the unmonitored call."""
import ctypes as C

import numpy as np
import pytest

import ensemble_checks as ec
import monitor_checks as mc
from conftest import ini
from ramsesgpu_amd import _capi
from ramsesgpu_amd.ensemble import Ensemble
from ramsesgpu_amd.solver import Solver

# problem, size: 40 rows = two segments of the summation order, the second one short; 72 columns = more than one wavefront of lanes
STATES = [("kelvin_helmholtz_gpu_2d", "mesh.nx=40;mesh.ny=24"), ("orszag-tang", "mesh.nx=24;mesh.ny=40"),
          ("kelvin_helmholtz_gpu_2d", "mesh.nx=72;mesh.ny=20"), ("orszag-tang", "mesh.nx=72;mesh.ny=20")]


@pytest.mark.parametrize("base,ov", STATES, ids=["%s-%s" % (b, o.replace("mesh.", "").replace(";", "-")) for b, o in STATES])
def test_state_monitor_equals_the_model(base, ov, emu_lib):
    p = emu_lib.params_from_ini(ini(base), ov)
    U0 = ec.member_states(emu_lib, base, ov, p, 1)[0]
    sv = Solver(p, emu_lib)
    try:
        sv.start(U0, 0)
        for steps in (0, 3):
            if steps:
                assert sv.run_steps(steps) == steps
            par = sv.nStep % 2
            ready, checksum, before = emu_lib.lib.rgpu_device_time_step_ready(sv.ctx, par), sv.state_checksum(par), sv.getDataHost()
            got = sv.state_monitor()
            U = sv.getDataHost()
            print(base, ov, "after %d steps:" % steps, dict(zip(_capi.MON_NAMES, got)))
            assert np.array_equal(got, mc.model(U, p)), (got, mc.model(U, p))
            mc.assert_within_any_order_bound(got, U, p)
            assert np.array_equal(got, sv.state_monitor(par))                      # explicit parity, and again: the same doubles
            if not p.mhdEnabled:
                assert got[3] == 0.0 and got[6] == 0.0 and got[9] == 0.0
            else:
                assert got[6] > 0.0
            # it reads the state only: what the context knows about its slots and ghost cells, and the state itself, are untouched
            assert emu_lib.lib.rgpu_device_time_step_ready(sv.ctx, par) == ready and sv.state_checksum(par) == checksum
            assert np.array_equal(before, U)
        assert sv.run_steps(2) == 2   # and the run goes on as the lone loop would
    finally:
        sv.close()


def test_state_monitor_does_not_change_what_follows(emu_lib):
    """three steps, a monitor call, three more == six steps"""
    base, ov = "orszag-tang", "mesh.nx=24;mesh.ny=40"
    p = emu_lib.params_from_ini(ini(base), ov)
    U0 = ec.member_states(emu_lib, base, ov, p, 1)[0]
    want = ec.lone_run(emu_lib, p, U0, 6, pieces=[3, 3])
    sv = Solver(p, emu_lib)
    try:
        sv.start(U0, 0)
        sv.run_steps(3)
        log = list(sv.dt_log)
        sv.state_monitor()
        sv.run_steps(3)
        assert log + list(sv.dt_log) == want["dt_log"] and sv.state_checksum(sv.nStep % 2) == want["checksum"]
    finally:
        sv.close()


def test_nan_cells(emu_lib):
    """one NaN density: the sums that contain the cell are NaN, the others are not, the minima are those of the remaining cells; a
    state of nothing but NaN: the sums are NaN and the extrema keep +inf, +inf, +0.0 (include/rgpu.h)"""
    for base, ov in (("orszag-tang", "mesh.nx=24;mesh.ny=40"), ("kelvin_helmholtz_gpu_2d", "mesh.nx=40;mesh.ny=24")):
        p = emu_lib.params_from_ini(ini(base), ov)
        U0 = ec.member_states(emu_lib, base, ov, p, 1)[0]
        gw = p.ghostWidth
        U0[0, 0, gw + p.ny // 2, gw + p.nx // 3] = np.nan
        sv = Solver(p, emu_lib)
        try:
            sv.upload(U0)
            got = sv.state_monitor(0)
            mc.assert_nan_rules(got, U0, p)
            assert np.isnan(got[0]) and np.isnan(got[5]) and not np.isnan(got[1]) and not np.isnan(got[4]) and np.isfinite(got[7:]).all()
            assert np.array_equal(got, mc.model(U0, p), equal_nan=True)
            sv.upload(np.full_like(U0, np.nan))
            got = sv.state_monitor(0)
            assert np.isnan(got[:7 if p.mhdEnabled else 3]).all() and list(got[7:]) == [np.inf, np.inf, 0.0], got
        finally:
            sv.close()


def test_argument_checks(emu_lib):
    L = emu_lib
    _capi.declare_ensemble_api(L.lib)
    out = (C.c_double * 10)()
    p3 = L.params_from_ini(ini("orszag-tang3d"), "mesh.nx=16;mesh.ny=16;mesh.nz=16")
    sv = Solver(p3, L)
    try:
        assert L.lib.rgpu_state_monitor(sv.ctx, 0, out) == -5 and b"2D" in L.lib.rgpu_last_error(sv.ctx)   # RGPU_EUNSUPPORTED
    finally:
        sv.close()
    p2 = L.params_from_ini(ini("orszag-tang"), "mesh.nx=16;mesh.ny=16")
    sv = Solver(p2, L)
    try:
        assert L.lib.rgpu_state_monitor(sv.ctx, 0, None) == -1                                             # RGPU_EINVAL
        assert L.lib.rgpu_state_monitor(None, 0, out) == -1
    finally:
        sv.close()
    ens = Ensemble(p2, 2, L)
    try:
        ens.start(ec.member_states(L, "orszag-tang", "mesh.nx=16;mesh.ny=16", p2, 2))
        M, n = 2, 4
        ns, ts, ds, done = (C.c_int * M)(), (C.c_double * M)(), (C.c_double * M)(), (C.c_int * M)()
        mon_n, mon_step, mon_t, mon = (C.c_int * M)(), (C.c_int * (M * 5))(), (C.c_double * (M * 5))(), (C.c_double * (M * 5 * 10))()
        call = lambda every, a, b, c, d: L.lib.rgpu_ensemble_run_steps_monitored(ens.ens, n, None, ns, ts, ds, None, done, None, None, every, a, b, c, d)
        for every in (0, -2):
            assert call(every, mon_n, mon_step, mon_t, mon) == -1 and b"every" in L.lib.rgpu_ensemble_last_error(ens.ens)
        for args in ((None, mon_step, mon_t, mon), (mon_n, None, mon_t, mon), (mon_n, mon_step, None, mon), (mon_n, mon_step, mon_t, None)):
            assert call(2, *args) == -1 and b"null pointer" in L.lib.rgpu_ensemble_last_error(ens.ens)
        assert L.lib.rgpu_ensemble_run_steps_monitored(ens.ens, n, None, None, ts, ds, None, done, None, None, 2, mon_n, mon_step, mon_t, mon) == -1
        assert L.lib.rgpu_ensemble_monitor(ens.ens, None) == -1 and L.lib.rgpu_ensemble_monitor(None, mon) == -1
        assert list(ns) == [0, 0] and ens.member(0).state_checksum(0) == ens.member(0).state_checksum(1)   # nothing ran
        assert call(2, mon_n, mon_step, mon_t, mon) == 0 and list(done) == [4, 4] and list(mon_n) == [2, 2] and list(mon_step)[:2] == [2, 4]
        assert L.lib.rgpu_ensemble_monitor_device_bytes(C.byref(p2), 0) == 0 and L.lib.rgpu_ensemble_monitor_device_bytes(C.byref(p3), 2) == 0
    finally:
        ens.close()


CASE = ("orszag-tang", "mesh.nx=24;mesh.ny=40")


@pytest.mark.parametrize("pieces", [None, [4, 6]], ids=["one-call", "pieces-4-6"])
def test_monitored_ensemble_member_by_member(pieces, emu_lib):
    base, ov = CASE
    p = emu_lib.params_from_ini(ini(base), ov)
    U0s = ec.member_states(emu_lib, base, ov, p, 3)
    done, stop, fused, series = mc.check_monitored(emu_lib, [p] * 3, U0s, 10, 3, pieces=pieces)
    assert done == [10] * 3 and stop == [0] * 3 and fused == 0
    assert [s[0] for s in series] == [[3, 6, 9]] * 3


def test_hydro_ensemble_in_pieces(emu_lib):
    base, ov = "kelvin_helmholtz_gpu_2d", "mesh.nx=40;mesh.ny=24"
    p = emu_lib.params_from_ini(ini(base), ov)
    U0s = ec.member_states(emu_lib, base, ov, p, 3)
    done, stop, fused, series = mc.check_monitored(emu_lib, [p] * 3, U0s, 10, 3, pieces=[4, 6])
    assert done == [10] * 3 and fused == 0 and [s[0] for s in series] == [[3, 6, 9]] * 3


def test_member_stopped_by_its_end_time(emu_lib):
    """member 1's t passes its end inside its 6th step, a multiple of 3: that last step is sampled; member 2's inside its 5th: it is
    not, and neither takes a sample afterwards"""
    base, ov = CASE
    p = emu_lib.params_from_ini(ini(base), ov)
    U0s = ec.member_states(emu_lib, base, ov, p, 3)
    dts = [ec.lone_run(emu_lib, p, U0s[m], 10)["dt_log"] for m in range(3)]
    ends = [None, ec.end_inside_step(dts[1], 6), ec.end_inside_step(dts[2], 5)]
    done, stop, fused, series = mc.check_monitored(emu_lib, [p] * 3, U0s, 10, 3, tEnds=ends)
    assert done == [10, 6, 5] and stop == [0, 1, 1] and fused == 0
    assert [s[0] for s in series] == [[3, 6, 9], [3, 6], [3]]
