"""A launch that fails inside a device-clock batch of a lone context (csrc/api/run_steps.h: batch_queue, batch_harvest), on the
test-only host emulation, whose rgpu_emu_fail_launch_after(k) makes the k-th plane-range launch from now fail once (tests/emu/rg_backend.h;
never on a device).  The steps queued completely in front of the failure ran: the call reports RGPU_EHIP, and nStep, t, dt, the dt
log, the samples and tHist describe exactly those steps -- against a second context stepped singly -- and the context steps on."""
import ctypes as C

import numpy as np
import pytest

import history_run_checks as hc
import monitor3d_checks as m3
from conftest import ini
from ramsesgpu_amd.solver import RgpuError, Solver, interior

CASES = [("implode3d", "mesh.nx=8;mesh.ny=8;mesh.nz=5"), ("mhd_mri_3d", "mesh.nx=8;mesh.ny=8;mesh.nz=8")]
ids = ["%s-%s" % (b, o.replace("mesh.", "").replace(";", "-")) for b, o in CASES]
LAUNCHES_PER_STEP = 4   # plane-range launches of one step of either case: the k-th fails inside step 1 + (k - 1) // 4 of the call


def after_one_step(lib, p, U0):
    sv = Solver(p, lib)
    sv.start(U0, 0)
    assert sv.run_steps(1) == 1   # the first step of a run is plain; the next call begins on the device path
    return sv


@pytest.fixture(scope="module", params=CASES, ids=ids)
def singly(request, emu_lib):
    """a context stepped singly to step 5: per step t, dt, the interior state and the monitor.  Computed once, left alone"""
    base, ov = request.param
    p = emu_lib.params_from_ini(ini(base), ov)
    U0 = m3.initial_state(emu_lib, base, ov, p)
    sv = Solver(p, emu_lib)
    at = {}
    try:
        sv.start(U0, 0)
        for n in range(1, 6):
            assert sv.run_steps(1) == 1
            at[n] = {"t": sv.totalTime, "dt": sv.dt, "U": interior(sv.getDataHost(), p), "mon": sv.state_monitor()}
    finally:
        sv.close()
    return p, U0, at


@pytest.mark.parametrize("k", range(1, 14))
def test_monitored_run_with_a_failing_launch(singly, k, emu_lib):
    p, U0, at = singly
    want_n = 1 + (k - 1) // LAUNCHES_PER_STEP   # 1, 2, 3, 4 for k in 1-4, 5-8, 9-12, 13
    sv = after_one_step(emu_lib, p, U0)
    try:
        assert emu_lib.lib.rgpu_device_time_step_ready(sv.ctx, 1) == 1
        emu_lib.lib.rgpu_emu_fail_launch_after(k)
        with pytest.raises(RgpuError) as e:
            sv.run_steps_monitored(8, 2)
        print(k, e.value)
        assert "(-4)" in str(e.value) and "queueing a device-clock step" in str(e.value)   # RGPU_EHIP
        assert sv.nStep == want_n
        ref = at[sv.nStep]
        assert sv.totalTime == ref["t"] and sv.dt == ref["dt"]
        assert np.array_equal(interior(sv.getDataHost(), p), ref["U"])
        series = sv.monitor_series
        assert list(series.step) == [s for s in range(2, sv.nStep + 1) if s % 2 == 0]
        for s, ts, v in zip(series.step, series.t, series.values):
            assert ts == at[s]["t"] and np.array_equal(v, at[s]["mon"]), (s, v, at[s]["mon"])
        assert sv.run_steps(1) == 1 and sv.nStep == want_n + 1 and sv.totalTime == at[want_n + 1]["t"]
        assert np.array_equal(interior(sv.getDataHost(), p), at[want_n + 1]["U"])
    finally:
        emu_lib.lib.rgpu_emu_fail_launch_after(0)
        sv.close()


@pytest.mark.parametrize("k,want_samples", [(1, []), (4, []), (5, [1]), (8, [1]), (9, [1, 2]), (13, [1, 2, 3])])
def test_history_run_with_a_failing_launch(k, want_samples, emu_lib):
    base, ov = CASES[1]
    L = emu_lib.lib
    R = hc.reference(emu_lib, base, ov, 5)
    sv = hc.fresh(emu_lib, R)
    try:
        assert sv.run_steps(1) == 1 and sv.tHist == 0.0
        heads0 = L.rgpu_history_batch_heads(sv.ctx)
        n, t, d, th, hn = C.c_int(sv.nStep), C.c_double(sv.totalTime), C.c_double(sv.dt), C.c_double(sv.tHist), C.c_int(0)
        log, hstep, ht, hdt, hv = (C.c_double * 8)(), (C.c_int * 8)(), (C.c_double * 8)(), (C.c_double * 8)(), (C.c_double * 64)()
        L.rgpu_emu_fail_launch_after(k)
        rc = L.rgpu_run_steps_history(sv.ctx, 8, float("inf"), C.byref(n), C.byref(t), C.byref(d), log, 0.0, C.byref(th), C.byref(hn), hstep, ht, hdt, hv)
        print(k, rc, L.rgpu_last_error(sv.ctx).decode(), "nStep", n.value, "samples", list(hstep)[:hn.value])
        assert rc == -4 and b"queueing a device-clock step" in L.rgpu_last_error(sv.ctx)   # RGPU_EHIP
        N = n.value
        assert N == 1 + (k - 1) // LAUNCHES_PER_STEP and list(hstep)[:hn.value] == want_samples == list(range(1, N))
        for i, s in enumerate(want_samples):   # the sample in front of step s: t and dt at its head, the row of the state U_s
            assert ht[i] == R["ts"][s] and hdt[i] == R["dts"][s - 1]
            assert np.array_equal(np.array(hv[8 * i:8 * i + 8]), R["rows"][s])
        _, _, want_tHist = hc.model(R, N - 1, 0.0, n0=1, tHist=0.0)
        assert th.value == want_tHist == 0.0
        assert list(log)[:N - 1] == R["dts"][1:N] and t.value == R["ts"][N] and d.value == R["dts"][N - 1]
        sv.nStep, sv.totalTime, sv.dt, sv.tHist = N, t.value, d.value, th.value
        assert np.array_equal(interior(sv.getDataHost(), R["p"]), interior(R["states"][N], R["p"]))
        # the head of the step that failed to queue was queued and is not returned: one head per step that ran, and that one
        assert L.rgpu_history_batch_heads(sv.ctx) - heads0 == N
        done, s, ts, dts, v = sv.run_steps_history(1, 0.0)   # ... and is taken again by the next call
        assert done == 1 and list(s) == [N] and ts[0] == R["ts"][N] and dts[0] == R["dts"][N - 1] and np.array_equal(v[0], R["rows"][N])
        assert sv.nStep == N + 1 and sv.totalTime == R["ts"][N + 1]
    finally:
        L.rgpu_emu_fail_launch_after(0)
        sv.close()
