"""rgpu_run_steps_history on the test-only host emulation: the contract's loop, the sampling moved behind the ticks of the 3D batches
(csrc/hip/history_batch.h runs there as host loops, the record resolved at once), the refusals, the option, and the run driver's use
of it.  The reference series is a lone context stepped singly with rgpu_history_mri in between (tests/history_run_checks.py)."""
import ctypes as C

import numpy as np
import pytest

import history_run_checks as hc
from conftest import ini
from ramsesgpu_amd.solver import Solver

MRI = ("mhd_mri_3d", "mesh.nx=8;mesh.ny=12;mesh.nz=8;MHD.omega0=0.02")
OT3D = ("orszag-tang3d", "mesh.nx=8;mesh.ny=8;mesh.nz=8")
OT2D = ("orszag-tang", "mesh.nx=24;mesh.ny=20")
NSTEPS = 10


def _dt0(R):
    return R["dts"][0]


@pytest.mark.parametrize("case", [MRI, OT3D, OT2D], ids=["mri3d", "orszag-tang3d", "orszag-tang2d"])
def test_series_equals_the_lone_context(case, emu_lib):
    """10 steps, dtHist = 2.5 x the initial dt: sample steps, hist_t, hist_dt, values, final tHist, state, t and the dt log"""
    R = hc.reference(emu_lib, case[0], case[1], NSTEPS)
    S, V = hc.check_series(emu_lib, R, [NSTEPS], 2.5 * _dt0(R))
    assert len(S) >= 3 and S[0] == 0   # the series is not trivially empty: the first turn (tHist == 0) and a few crossings


@pytest.mark.parametrize("base,ov,nsteps", hc.SHEAR_CASES, ids=["fastshear"])
def test_series_across_the_wrap_of_the_shearing_box(base, ov, nsteps, emu_lib):
    """the series in one call and in two (the second batch begins after the first wrap of ylen), dtHist = 2.5 x the initial dt"""
    R = hc.reference(emu_lib, base, ov, nsteps)
    S1, V1 = hc.check_series(emu_lib, R, [nsteps], 2.5 * _dt0(R))
    S2, V2 = hc.check_series(emu_lib, R, [6, nsteps - 6], 2.5 * _dt0(R))
    assert len(S1) >= 4 and np.array_equal(S1, S2) and np.array_equal(V1, V2)


def test_3d_batches_run_on_the_emulation(emu_lib):
    """the 3D cases above do go through the batch (the emulation's device clock), so the sampling kernels are what was tested"""
    R = hc.reference(emu_lib, MRI[0], MRI[1], NSTEPS)
    sv = hc.fresh(emu_lib, R)
    try:
        sv.run_steps_history(2, 2.5 * _dt0(R))
        assert emu_lib.lib.rgpu_device_time_step_ready(sv.ctx, sv.nStep % 2) == 1
        assert emu_lib.lib.rgpu_history_batch_heads(sv.ctx) == 1   # the head of the second step (the first step of a run is plain)
    finally:
        sv.close()


@pytest.mark.parametrize("case", [MRI, OT2D], ids=["mri3d", "orszag-tang2d"])
def test_split_calls_give_the_series_of_one_call(case, emu_lib):
    R = hc.reference(emu_lib, case[0], case[1], NSTEPS)
    S1, V1 = hc.check_series(emu_lib, R, [NSTEPS], 2.5 * _dt0(R))
    S2, V2 = hc.check_series(emu_lib, R, [3, 7], 2.5 * _dt0(R))
    assert np.array_equal(S1, S2) and np.array_equal(V1, V2)


def test_dthist_zero_samples_before_every_step(emu_lib):
    R = hc.reference(emu_lib, MRI[0], MRI[1], NSTEPS)
    S, V = hc.check_series(emu_lib, R, [NSTEPS], 0.0)
    assert list(S) == list(range(NSTEPS))


def test_tend_inside_the_call(emu_lib):
    """no sample at or after the stop; a following call with the same tEnd does nothing"""
    R = hc.reference(emu_lib, MRI[0], MRI[1], NSTEPS)
    cut = NSTEPS // 2
    tEnd = R["ts"][cut] - 0.25 * R["dts"][cut - 1]   # reached during step `cut`
    sv = hc.fresh(emu_lib, R)
    try:
        S, V = hc.check_series(emu_lib, R, [NSTEPS], 0.0, tEnd, sv=sv)
        assert sv.nStep == cut and list(S) == list(range(cut))
        done, s, t, d, v = sv.run_steps_history(5, 0.0, tEnd)
        assert done == 0 and len(s) == 0 and v.shape == (0, 8) and sv.nStep == cut
    finally:
        sv.close()


def test_refusals(emu_lib):
    R = hc.reference(emu_lib, MRI[0], MRI[1], NSTEPS)
    sv = hc.fresh(emu_lib, R)
    try:
        for name in ("nStep", "t", "dt", "tHist", "hist_n", "hist_step", "hist_t", "hist_dt", "hist"):
            rc, msg = hc.call_raw(emu_lib, sv, 2, null=name)
            assert rc == -1 and "null" in msg, (name, rc, msg)          # RGPU_EINVAL
        rc, msg = hc.call_raw(emu_lib, sv, -1)
        assert rc == -1 and "negative" in msg, (rc, msg)
        rc, msg = hc.call_raw(emu_lib, sv, 2)                              # (dt_log NULL is fine)
        assert rc == 2, (rc, msg)
    finally:
        sv.close()
    p = emu_lib.params_from_ini(ini("implode3d"), "mesh.nx=8;mesh.ny=8;mesh.nz=8")
    sv = Solver(p, emu_lib)
    try:
        sv.start(emu_lib.init_condition(ini("implode3d"), "mesh.nx=8;mesh.ny=8;mesh.nz=8", p), 0)
        rc, msg = hc.call_raw(emu_lib, sv, 2)
        assert rc == -5 and "MHD" in msg, (rc, msg)                        # RGPU_EUNSUPPORTED
    finally:
        sv.close()
    ps = emu_lib.params_from_ini(ini(MRI[0]), "mesh.nx=8;mesh.ny=12;mesh.nz=8", slab=(0, 2))
    sv = Solver(ps, emu_lib)
    try:
        rc, msg = hc.call_raw(emu_lib, sv, 2)
        assert rc == -1 and "slab" in msg, (rc, msg)
    finally:
        sv.close()


def test_option_history_batch_off_gives_the_same(emu_lib):
    R = hc.reference(emu_lib, MRI[0], MRI[1], NSTEPS)
    S1, V1 = hc.check_series(emu_lib, R, [NSTEPS], 2.5 * _dt0(R))
    assert emu_lib.set_option("history_batch", 0) == 1
    try:
        S0, V0 = hc.check_series(emu_lib, R, [4, 6], 2.5 * _dt0(R))
    finally:
        emu_lib.set_option("history_batch", 1)
    assert np.array_equal(S0, S1) and np.array_equal(V0, V1)


def test_run_driver_history_file_is_the_same_both_ways(emu_lib, tmp_path):
    """rgpuh_run with [history] enabled=yes: the file written from the samples of rgpu_run_steps_history inside the batches is, byte for
    byte, the one of the literal loop (option history_batch = 0)"""
    files = []
    for opt in (1, 0):
        d = tmp_path / ("opt%d" % opt)
        d.mkdir()
        ov = "mesh.nx=8;mesh.ny=12;mesh.nz=8;history.enabled=yes;history.dtHist=80.0;run.nstepmax=12;run.noutput=1000;output.outputVtk=no;output.outputHdf5=no;output.outputDir=%s" % d
        err, mc = C.create_string_buffer(512), C.c_double(0)
        emu_lib.set_option("history_batch", opt)
        try:
            n = emu_lib.lib.rgpuh_run(ini("mhd_mri_3d").encode(), ov.encode(), C.byref(mc), err, 512)
        finally:
            emu_lib.set_option("history_batch", 1)
        assert n == 12, err.value
        files.append(open(d / "mhd_mri_3d_history.txt", "rb").read())
    rows = [ln for ln in files[0].decode().splitlines() if ln and not ln.startswith("#")]
    assert len(rows) >= 4 and files[0] == files[1]   # dtHist = 80 is about 2.5 time steps: a row every two or three steps
