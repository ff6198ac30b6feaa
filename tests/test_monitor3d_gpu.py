"""The monitors of a lone context on the GPU, both libraries: rgpu_state_monitor3d (csrc/hip/monitor3d.h) against the numpy model bit
for bit, in both forms of its column pass; rgpu_run_steps_monitored with the samples taken behind the steps of the device-clock
batches -- 3D hydro, 3D MHD, the shearing box, the fused 2D MHD step and the 2D hydro step with the folded clock -- against the
unmonitored run, a second lone context and the model; an end time inside a batch; a NaN density; and the monitor file of euler_hip.
Helpers: tests/monitor3d_checks.py."""
import os
import subprocess

import numpy as np
import pytest

import ensemble_checks as ec
import monitor3d_checks as m3
from conftest import ROOT, ini
from ramsesgpu_amd import _capi
from ramsesgpu_amd.solver import RgpuError, Solver

pytestmark = pytest.mark.gpu

STATES3D = [("implode3d", "mesh.nx=72;mesh.ny=40;mesh.nz=5"), ("orszag-tang3d", "mesh.nx=24;mesh.ny=40;mesh.nz=6"), ("mhd_mri_3d", "mesh.nx=16;mesh.ny=32;mesh.nz=8")]
BATCHED = [("implode3d", "mesh.nx=40;mesh.ny=24;mesh.nz=12"), ("orszag-tang3d", "mesh.nx=24;mesh.ny=40;mesh.nz=6"), ("mhd_mri_3d", "mesh.nx=16;mesh.ny=32;mesh.nz=8"),
           ("orszag-tang", "mesh.nx=40;mesh.ny=24"), ("kelvin_helmholtz_gpu_2d", "mesh.nx=72;mesh.ny=20")]
ids = lambda cases: ["%s-%s" % (b, o.replace("mesh.", "").replace(";", "-")) for b, o in cases]


@pytest.fixture(scope="module", params=["exact", "contracted"])
def lib(request, gpu_lib, gpu_contracted_lib):
    yield gpu_lib if request.param == "exact" else gpu_contracted_lib
    m3.close_references()


@pytest.mark.parametrize("base,ov", STATES3D, ids=ids(STATES3D))
def test_state_monitor3d_equals_the_model(base, ov, lib):
    p = lib.params_from_ini(ini(base), ov)
    U0 = m3.initial_state(lib, base, ov, p)
    sv = Solver(p, lib)
    try:
        sv.start(U0, 0)
        for steps in (0, 3):
            if steps:
                assert sv.run_steps(steps) == steps
            par = sv.nStep % 2
            ready, checksum = lib.lib.rgpu_device_time_step_ready(sv.ctx, par), sv.state_checksum(par)
            got = sv.state_monitor()
            U = sv.getDataHost()
            print(base, ov, "after %d steps:" % steps, dict(zip(_capi.MON_NAMES, got)))
            assert np.array_equal(got, m3.model(U, p)), (got, m3.model(U, p))
            m3.assert_within_any_order_bound(got, U, p)
            assert np.array_equal(got, sv.state_monitor(par))
            assert lib.lib.rgpu_device_time_step_ready(sv.ctx, par) == ready and sv.state_checksum(par) == checksum
        assert sv.run_steps(2) == 2
    finally:
        sv.close()


FOLDED = BATCHED[4]   # 2D hydro, whose clock may be folded into the step kernel: the one case that may take either path


def batch_samples(case, every, first=1):
    """rgpu_monitor_batch_samples after steps first + 1 .. done of a run whose step `first` was plain: every qualifying step among them
    was sampled on the device -- without a condition (the context must be on the device path afterwards), except for FOLDED, where
    the path is the one rgpu_device_time_step_ready reports"""
    def want(done, ready):
        assert ready == 1 or case == FOLDED, "the context does not take its time step from the device"
        return len([s for s in range(first + 1, done + 1) if s % every == 0]) if ready else 0
    return want


@pytest.mark.parametrize("every", [1, 3])
@pytest.mark.parametrize("base,ov", BATCHED, ids=ids(BATCHED))
def test_samples_inside_the_device_batches(base, ov, every, lib):
    done, steps, vals, batch = m3.check_monitored_lone(lib, base, ov, 10, every, expect_batch=batch_samples((base, ov), every))
    assert done == 10 and steps == [s for s in range(1, 11) if s % every == 0]
    assert batch == len(steps) - (1 if every == 1 else 0) or (base, ov) == FOLDED


BOUNDARY = [BATCHED[0], BATCHED[3], BATCHED[4]]


@pytest.mark.parametrize("base,ov", BOUNDARY, ids=ids(BOUNDARY))
def test_monitored_run_across_a_batch_boundary(base, ov, lib):
    """300 steps, every 7th sampled: 7 does not divide the 256 steps of a batch, so which slots of a batch hold a sample differs between
    the first batch and the second -- 3D hydro, the fused 2D MHD step, and the 2D hydro step with the folded clock, whose three slot
    arrays rotate across the boundary"""
    done, steps, vals, batch = m3.check_monitored_lone(lib, base, ov, 300, 7, expect_batch=batch_samples((base, ov), 7))
    assert done == 300 and len(steps) == 42 and steps[-1] == 294
    assert batch == 42 or (base, ov) == FOLDED


@pytest.mark.parametrize("base,ov", m3.SEAMS, ids=ids(m3.SEAMS))
def test_2d_shapes_at_the_seams_of_the_summation_order(base, ov, lib):
    """a 2D state is a volume of one plane (csrc/hip/monitor3d.h without its finish launch) at shapes where a lane, a round of the lanes
    or a segment begins or ends: against the model and the ensemble kernels, and every sample taken inside a batch against a second
    context stepped singly"""
    m3.check_seam_state(lib, base, ov)
    def want(done, ready):   # steps 2 .. 6 follow the first, plain step: on the device path, all five samples are taken inside batches
        print(base, ov, "device path after the run:", ready)
        assert ready == 1, "the context does not take its time step from the device"
        return done - 1
    done, steps, vals, batch = m3.check_monitored_lone(lib, base, ov, 6, 1, expect_batch=want)
    assert done == 6 and steps == [1, 2, 3, 4, 5, 6] and batch == 5


def test_nan_cell_on_a_seam_shape(lib):
    for base, ov in m3.SEAMS[4:6]:   # 65 x 33, hydro and MHD
        m3.check_seam_nan(lib, base, ov)


@pytest.mark.parametrize("base,ov", [BATCHED[0], BATCHED[2], BATCHED[4]], ids=ids([BATCHED[0], BATCHED[2], BATCHED[4]]))
def test_run_in_pieces(base, ov, lib):
    """[4, 6]: step 1 is plain, the second call begins on the device path -- samples 3, 6, 9 all inside batches"""
    done, steps, vals, batch = m3.check_monitored_lone(lib, base, ov, 10, 3, pieces=[4, 6], expect_batch=batch_samples((base, ov), 3))
    assert done == 10 and steps == [3, 6, 9]
    assert batch == 3 or (base, ov) == FOLDED


@pytest.mark.parametrize("base,ov", [BATCHED[0], BATCHED[1], BATCHED[3]], ids=ids([BATCHED[0], BATCHED[1], BATCHED[3]]))
def test_end_time_inside_a_batch(base, ov, lib):
    """t passes the end inside the 6th step, a multiple of 3: that last step is sampled; inside the 5th: it is not, and no sample follows.
    The sample of step 9, queued behind a step that did not run, is not counted as taken but was queued: the counter counts launches"""
    p = lib.params_from_ini(ini(base), ov)
    dts = ec.lone_run(lib, p, m3.initial_state(lib, base, ov, p), 10)["dt_log"]
    for k, want in ((6, [3, 6]), (5, [3])):
        queued = lambda done, ready: 3 if ready == 1 else -1   # steps 3, 6, 9 of the ten queued: on the device path, without a condition
        done, steps, vals, batch = m3.check_monitored_lone(lib, base, ov, 10, 3, tEnd=ec.end_inside_step(dts, k), expect_batch=queued)
        assert done == k and steps == want and batch == 3


@pytest.mark.parametrize("base,ov", [BATCHED[0], BATCHED[1]], ids=ids([BATCHED[0], BATCHED[1]]))
def test_one_nan_density(base, ov, lib):
    """arithmetic, not a fault: whether the call ends with all its steps or with a negative code (the time step stops being a number),
    *nStep counts the steps that ran, every one of them was sampled (every = 1), *mon_n counts exactly those, and the last sample is of
    the final state: its mass is NaN, its extrema are those of the cells that are numbers, the model gives its doubles"""
    p = lib.params_from_ini(ini(base), ov)
    U0 = m3.initial_state(lib, base, ov, p)
    gw = p.ghostWidth
    U0[0, gw + p.nz // 2, gw + p.ny // 2, gw + p.nx // 3] = np.nan
    sv = Solver(p, lib)
    try:
        sv.start(U0, 0)
        try:
            done, series = sv.run_steps_monitored(6, 1)
        except RgpuError as e:
            done, series = -1, sv.monitor_series
            print("the call ended with", e)
        print(base, ov, "done", done, "nStep", sv.nStep, "samples", list(series.step))
        assert done in (-1, sv.nStep) and list(series.step) == list(range(1, sv.nStep + 1)) and sv.nStep >= 2
        assert lib.lib.rgpu_monitor_batch_samples(sv.ctx) > 0   # the samples behind the first, plain step were taken inside a batch
        U = sv.getDataHost()
        last = series.values[-1]
        assert np.isnan(last[0])
        m3.assert_nan_rules(last, U, p)
        assert np.array_equal(last, m3.model(U, p), equal_nan=True)
    finally:
        sv.close()


DRIVER = [("implode3d", "mesh.nx=24;mesh.ny=24;mesh.nz=12", "implode3d"), ("orszag-tang", "mesh.nx=32;mesh.ny=32", "orszag-tang2d")]


@pytest.mark.parametrize("base,ov,prefix", DRIVER, ids=[c[0] for c in DRIVER])
def test_euler_hip_monitor_file(base, ov, prefix, gpu_lib, tmp_path):
    exe = os.path.join(ROOT, "ramsesgpu_amd", "euler_hip")
    common = ov + ";run.nstepmax=10;run.noutput=1000;output.outputVtk=no;output.outputHdf5=no;output.outputDir=%s"
    with_dir, without_dir = tmp_path / "with", tmp_path / "without"
    for d, extra in ((with_dir, ";monitor.enabled=yes;monitor.every=3"), (without_dir, "")):
        d.mkdir()
        r = subprocess.run([exe, "--param", ini(base), "--set", common % d + extra], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:]
    assert not os.path.exists(without_dir / (prefix + "_monitor.txt"))
    lines = open(with_dir / (prefix + "_monitor.txt")).read().splitlines()
    assert lines[0] == "# nStep totalTime " + " ".join(_capi.MON_NAMES)
    rows = [ln.split() for ln in lines[1:]]
    p = gpu_lib.params_from_ini(ini(base), ov)
    sv = Solver(p, gpu_lib)
    try:
        sv.start(gpu_lib.init_condition(ini(base), ov, p), 0)
        done, series = sv.run_steps_monitored(10, 3)
    finally:
        sv.close()
    assert done == 10 and [int(r[0]) for r in rows] == list(series.step) == [3, 6, 9]
    assert [float(r[1]) for r in rows] == list(series.t)
    assert np.array_equal(np.array([[float(x) for x in r[2:]] for r in rows]), series.values)
