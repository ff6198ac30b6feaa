"""rgpu_run_steps_history on the GPU, both libraries: the history row sampled behind the ticks of the device-clock batches
(csrc/hip/history_batch.h) == a lone context stepped singly with rgpu_history_mri in between, every double -- sample steps, times,
values, tHist, state, dt log -- where the batch runs, across batch and call boundaries, with an end time inside the batch, and where
the call falls back to the literal loop.  Helpers and the reference series: tests/history_run_checks.py."""
import os

import numpy as np
import pytest

import history_run_checks as hc

pytestmark = pytest.mark.gpu

NSTEPS = 12
CLOCKED = [
    ("mhd_mri_3d", "mesh.nx=16;mesh.ny=32;mesh.nz=16"),                    # rotating frame + shearing box, as shipped
    ("mhd_mri_3d", "mesh.nx=24;mesh.ny=32;mesh.nz=16;MHD.omega0=0.02"),    # ... with offsets that move
    ("orszag-tang3d", "mesh.nx=24;mesh.ny=20;mesh.nz=16"),                 # plain 3D MHD
    ("orszag-tang", "mesh.nx=48;mesh.ny=40"),                              # 2D MHD, all periodic: the fused step
]
FALLBACK = [
    ("orszag-tang3d", "mesh.nx=12;mesh.ny=12;mesh.nz=16;hydro.nu=0.005;MHD.eta=0.01"),   # dissipative stage: plain loop
    ("mhd_BrioWu", "mesh.nx=128;mesh.ny=8"),                                             # 2D MHD with Neumann faces: plain loop
]


@pytest.fixture(scope="module", params=["exact", "contracted"])
def lib(request, gpu_lib, gpu_contracted_lib):
    return gpu_lib if request.param == "exact" else gpu_contracted_lib


def _device_path_expected(lib):
    return not (os.environ.get("RGPU_TILED") == "0" or lib.get_option("step_clock") == 0 or lib.get_option("ghost_images") == 0)


@pytest.mark.parametrize("factor", [2.5, 0.4], ids=["dtHist2.5dt", "dtHist0.4dt"])
@pytest.mark.parametrize("case", CLOCKED, ids=["mri-shipped", "mri-omega", "orszag-tang3d", "orszag-tang2d"])
def test_device_clock_series_equals_the_lone_context(case, factor, lib):
    """12 steps; dtHist = 0.4 x the initial dt exercises the reference's quirk: a step that overshoots more than one interval ends the
    series.  After the call the context is on the device path (the means of test_run_steps_equals_the_reference_loop)."""
    R = hc.reference(lib, case[0], case[1], NSTEPS)
    sv = hc.fresh(lib, R)
    try:
        S, V = hc.check_series(lib, R, [NSTEPS], factor * R["dts"][0], sv=sv)
        assert S[0] == 0 and (len(S) >= 3 if factor > 1 else len(S) <= 3), S
        if _device_path_expected(lib):
            assert lib.lib.rgpu_device_time_step_ready(sv.ctx, sv.nStep % 2) == 1
            # ... and the heads of every step after the plain first one were queued on the device (the literal loop returns the same
            # values, so equality alone would not tell)
            assert lib.lib.rgpu_history_batch_heads(sv.ctx) == NSTEPS - 1
    finally:
        sv.close()


@pytest.mark.parametrize("base,ov,nsteps", hc.SHEAR_CASES, ids=["fastshear"])
def test_series_across_the_wrap_of_the_shearing_box(base, ov, nsteps, lib):
    """the series in one call and in two (the second batch begins after the first wrap of ylen), dtHist = 2.5 x the initial dt; every
    head after the plain first step queued on the device"""
    R = hc.reference(lib, base, ov, nsteps)
    sv = hc.fresh(lib, R)
    try:
        S1, V1 = hc.check_series(lib, R, [nsteps], 2.5 * R["dts"][0], sv=sv)
        if _device_path_expected(lib):
            assert lib.lib.rgpu_device_time_step_ready(sv.ctx, sv.nStep % 2) == 1 and lib.lib.rgpu_history_batch_heads(sv.ctx) == nsteps - 1
    finally:
        sv.close()
    S2, V2 = hc.check_series(lib, R, [6, nsteps - 6], 2.5 * R["dts"][0])
    assert len(S1) >= 4 and np.array_equal(S1, S2) and np.array_equal(V1, V2)


def test_more_than_one_batch(lib):
    """300 steps in one call (a batch holds 256): tHist and the count cross the batch boundary through the host"""
    R = hc.reference(lib, "orszag-tang", "mesh.nx=48;mesh.ny=40", 300, keep_all=False)
    S, V = hc.check_series(lib, R, [300], 7.0 * R["dts"][0])
    assert len(S) >= 20 and S.max() > 256, S


@pytest.mark.parametrize("case", [CLOCKED[1], CLOCKED[3]], ids=["mri-omega", "orszag-tang2d"])
def test_split_calls_and_tend_inside_the_batch(case, lib):
    R = hc.reference(lib, case[0], case[1], NSTEPS)
    dtHist = 2.5 * R["dts"][0]
    S1, V1 = hc.check_series(lib, R, [NSTEPS], dtHist)
    S2, V2 = hc.check_series(lib, R, [3, 9], dtHist)
    assert np.array_equal(S1, S2) and np.array_equal(V1, V2)
    cut = NSTEPS // 2
    tEnd = R["ts"][cut] - 0.25 * R["dts"][cut - 1]     # reached during step `cut` (as test_run_steps_equals_the_reference_loop cuts)
    sv = hc.fresh(lib, R)
    try:
        S, V = hc.check_series(lib, R, [NSTEPS], 0.0, tEnd, sv=sv)
        assert sv.nStep == cut and list(S) == list(range(cut))     # no sample at or after the stop
        done, s, t, d, v = sv.run_steps_history(5, 0.0, tEnd)
        assert done == 0 and len(s) == 0
        assert sv.oneStepIntegration() == R["dts"][cut]            # and the state is usable
    finally:
        sv.close()


@pytest.mark.parametrize("case", FALLBACK, ids=["dissipative3d", "briowu2d"])
def test_fallback_configurations(case, lib):
    R = hc.reference(lib, case[0], case[1], NSTEPS)
    sv = hc.fresh(lib, R)
    try:
        hc.check_series(lib, R, [NSTEPS], 2.5 * R["dts"][0], sv=sv)
        assert lib.lib.rgpu_device_time_step_ready(sv.ctx, sv.nStep % 2) == 0 and lib.lib.rgpu_history_batch_heads(sv.ctx) == 0
    finally:
        sv.close()


def test_option_history_batch_off_gives_the_same(lib):
    R = hc.reference(lib, CLOCKED[1][0], CLOCKED[1][1], NSTEPS)
    S1, V1 = hc.check_series(lib, R, [NSTEPS], 2.5 * R["dts"][0])
    assert lib.set_option("history_batch", 0) == 1
    sv = hc.fresh(lib, R)
    try:
        S0, V0 = hc.check_series(lib, R, [NSTEPS], 2.5 * R["dts"][0], sv=sv)
        assert lib.lib.rgpu_history_batch_heads(sv.ctx) == 0     # the literal loop everywhere
    finally:
        lib.set_option("history_batch", 1)
        sv.close()
    assert np.array_equal(S0, S1) and np.array_equal(V0, V1)


def test_independent_anchor(lib):
    """one sample taken inside a batch against math.fsum of the downloaded state (bound derived in history_run_checks.fsum_anchor)"""
    R = hc.reference(lib, CLOCKED[0][0], CLOCKED[0][1], NSTEPS)
    S, V = hc.check_series(lib, R, [NSTEPS], 2.5 * R["dts"][0])
    k = len(S) - 1
    assert S[k] > 1     # a sample of the batch, not of the plain first step
    hc.fsum_anchor(R["p"], R["states"][int(S[k])], V[k])


def test_bookkeeping_after_a_call(lib):
    """what the call leaves behind is what rgpu_run_steps_log leaves on a twin context; one more plain step gives the reference's dt"""
    R = hc.reference(lib, CLOCKED[0][0], CLOCKED[0][1], NSTEPS)
    a, b = hc.fresh(lib, R), hc.fresh(lib, R)
    try:
        done, s, t, d, v = a.run_steps_history(NSTEPS, 2.5 * R["dts"][0])
        assert done == NSTEPS and b.run_steps(NSTEPS) == NSTEPS
        for par in (0, 1):
            assert lib.lib.rgpu_device_time_step_ready(a.ctx, par) == lib.lib.rgpu_device_time_step_ready(b.ctx, par)
            assert a.state_checksum(par) == b.state_checksum(par)
        assert (a.nStep, a.totalTime, a.dt) == (b.nStep, b.totalTime, b.dt)
        assert a.oneStepIntegration() == R["dt_next"]
    finally:
        a.close()
        b.close()
