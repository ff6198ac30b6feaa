"""The plane monitor on the GPU, both libraries (csrc/hip/monitor_profile.h): the rows against the numpy model bit for bit and folded
against rgpu_state_monitor3d at shapes on the seams of the summation order; a NaN density that stays in its plane;
rgpu_run_steps_monitored_planes with the samples taken behind the steps of the device-clock batches -- 3D hydro, 3D MHD, the
shearing box -- against the unmonitored run, a second lone context and the model; a run in pieces, an end time inside a batch, a run
across the 256-step boundary; the literal loop (gravity, the dissipative stage); the refusals; and the planes file of euler_hip.
Helpers: tests/monitor_planes_checks.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ensemble_checks as ec
import monitor_planes_checks as mp
from conftest import ROOT, ini
from ramsesgpu_amd.solver import Solver

pytestmark = pytest.mark.gpu

SEAMS = [("implode3d", "mesh.nx=65;mesh.ny=33;mesh.nz=3"), ("implode3d", "mesh.nx=63;mesh.ny=31;mesh.nz=5"), ("implode3d", "mesh.nx=130;mesh.ny=65;mesh.nz=2"),
         ("orszag-tang3d", "mesh.nx=63;mesh.ny=31;mesh.nz=4"), ("orszag-tang3d", "mesh.nx=64;mesh.ny=32;mesh.nz=3"), ("orszag-tang3d", "mesh.nx=130;mesh.ny=65;mesh.nz=3"),
         ("mhd_mri_3d", "mesh.nx=65;mesh.ny=33;mesh.nz=4")]
NAN = [SEAMS[0], SEAMS[3]]
BATCHED = [("implode3d", "mesh.nx=40;mesh.ny=24;mesh.nz=12"), ("orszag-tang3d", "mesh.nx=24;mesh.ny=40;mesh.nz=6"), ("mhd_mri_3d", "mesh.nx=16;mesh.ny=32;mesh.nz=8")]
LITERAL = [("rayleigh_taylor_gpu_3d", "mesh.nx=24;mesh.ny=16;mesh.nz=12"), ("mhd_mri_3d", "mesh.nx=16;mesh.ny=32;mesh.nz=8;hydro.nu=0.01;MHD.eta=0.01")]
ids = lambda cases: ["%s-%s" % (b, o.replace("mesh.", "").replace(";", "-")) for b, o in cases]


@pytest.fixture(scope="module", params=["exact", "contracted"])
def lib(request, gpu_lib, gpu_contracted_lib):
    yield gpu_lib if request.param == "exact" else gpu_contracted_lib
    mp.close_references()


@pytest.mark.parametrize("base,ov", SEAMS, ids=ids(SEAMS))
def test_rows_equal_the_model_and_fold_to_the_monitor(base, ov, lib):
    mp.check_single_samples(lib, base, ov)


@pytest.mark.parametrize("base,ov", NAN, ids=ids(NAN))
def test_nan_cell_stays_in_its_plane(base, ov, lib):
    mp.check_nan_plane(lib, base, ov)


@pytest.mark.parametrize("every", [1, 3])
@pytest.mark.parametrize("base,ov", BATCHED, ids=ids(BATCHED))
def test_samples_inside_the_device_batches(base, ov, every, lib):
    done, steps, vals, batch = mp.check_monitored_planes(lib, base, ov, 10, every, expect_batch=mp.batch_samples(every))
    assert done == 10 and steps == [s for s in range(1, 11) if s % every == 0]
    assert batch == len(steps) - (1 if every == 1 else 0)


@pytest.mark.parametrize("base,ov", BATCHED, ids=ids(BATCHED))
def test_run_in_pieces(base, ov, lib):
    """[4, 6]: step 1 is plain, the second call begins on the device path -- samples 3, 6, 9 all inside batches"""
    done, steps, vals, batch = mp.check_monitored_planes(lib, base, ov, 10, 3, pieces=[4, 6], expect_batch=lambda done, ready: 3 if ready == 1 else -1)
    assert done == 10 and steps == [3, 6, 9] and batch == 3


@pytest.mark.parametrize("base,ov", BATCHED, ids=ids(BATCHED))
def test_end_time_inside_a_batch(base, ov, lib):
    """t passes the end inside the 6th step, a multiple of 3: that last step is sampled; inside the 5th: it is not, and no sample follows.
    The sample of step 9, queued behind a step that did not run, is not counted as taken but was queued: the counter counts launches"""
    p = lib.params_from_ini(ini(base), ov)
    dts = ec.lone_run(lib, p, mp.initial_state(lib, base, ov, p), 10)["dt_log"]
    for k, want in ((6, [3, 6]), (5, [3])):
        queued = lambda done, ready: 3 if ready == 1 else -1   # steps 3, 6, 9 of the ten queued: on the device path, without a condition
        done, steps, vals, batch = mp.check_monitored_planes(lib, base, ov, 10, 3, tEnd=ec.end_inside_step(dts, k), expect_batch=queued)
        assert done == k and steps == want and batch == 3


def test_across_a_batch_boundary(lib):
    """300 steps, every 7th sampled: 7 does not divide the 256 steps of a batch, so the samples of the second batch sit in other slots
    of the log than those of the first"""
    base, ov = BATCHED[0]
    done, steps, vals, batch = mp.check_monitored_planes(lib, base, ov, 300, 7, expect_batch=mp.batch_samples(7))
    assert done == 300 and len(steps) == 42 and steps[-1] == 294 and batch == 42


def test_the_log_grows_with_the_cadence(lib):
    """every = 5 first (52 slots), then every = 1 on the same context (257): the second call's log is larger than the first's"""
    base, ov = BATCHED[1]
    p = lib.params_from_ini(ini(base), ov)
    U0 = mp.initial_state(lib, base, ov, p)
    sv = Solver(p, lib)
    try:
        sv.start(U0, 0)
        done, s5 = sv.run_steps_monitored_planes(5, 5)
        assert done == 5 and list(s5.step) == [5]
        done, s1 = sv.run_steps_monitored_planes(5, 1)
        assert done == 5 and list(s1.step) == [6, 7, 8, 9, 10]
        assert lib.lib.rgpu_monitor_planes_batch_samples(sv.ctx) == 1 + 5
        for s, v in zip(list(s5.step) + list(s1.step), list(s5.values) + list(s1.values)):
            assert np.array_equal(v, mp.stepped_reference(lib, base, ov, p, U0, s)[0]), s
    finally:
        sv.close()


@pytest.mark.parametrize("base,ov", LITERAL, ids=["gravity", "dissipative"])
def test_literal_path(base, ov, lib):
    """gravity and the dissipative stage take their time step from the host: the literal loop, the same series, no sample on the device"""
    def never(done, ready):
        assert ready == 0, "the context takes its time step from the device"
        return 0
    done, steps, vals, batch = mp.check_monitored_planes(lib, base, ov, 10, 3, pieces=[4, 6], expect_batch=never)
    assert done == 10 and steps == [3, 6, 9] and batch == 0


def test_refusals(lib):
    L = lib
    p2 = L.params_from_ini(ini("orszag-tang"), "mesh.nx=16;mesh.ny=16")
    p3 = L.params_from_ini(ini("orszag-tang3d"), "mesh.nx=16;mesh.ny=16;mesh.nz=8")
    out = (C.c_double * (8 * 16))()
    n, t, d, mn = C.c_int(0), C.c_double(0.0), C.c_double(0.0), C.c_int(7)
    ms, mt, mv = (C.c_int * 5)(), (C.c_double * 5)(), (C.c_double * (5 * 8 * 16))()
    full = (C.byref(n), C.byref(t), C.byref(d), C.byref(mn), ms, mt, mv)
    call = lambda ctx, nsteps, every, a, b, c_, e, f, g, h: L.lib.rgpu_run_steps_monitored_planes(ctx, nsteps, 1e300, a, b, c_, None, every, e, f, g, h)
    sv = Solver(p2, L)
    try:
        sv.start(L.init_condition(ini("orszag-tang"), "mesh.nx=16;mesh.ny=16", p2), 0)
        assert L.lib.rgpu_state_monitor_planes(sv.ctx, 0, out) == -5 and b"3D" in L.lib.rgpu_last_error(sv.ctx)   # RGPU_EUNSUPPORTED
        assert call(sv.ctx, 4, 2, *full) == -5 and b"3D" in L.lib.rgpu_last_error(sv.ctx) and mn.value == 0 and n.value == 0
    finally:
        sv.close()
    sv = Solver(p3, L)
    try:
        sv.start(L.init_condition(ini("orszag-tang3d"), "mesh.nx=16;mesh.ny=16;mesh.nz=8", p3), 0)
        assert L.lib.rgpu_state_monitor_planes(sv.ctx, 0, None) == -1
        assert call(sv.ctx, 4, 0, *full) == -1 and b"every" in L.lib.rgpu_last_error(sv.ctx)
        args = list(full)
        args[6] = None
        assert call(sv.ctx, 4, 2, *args) == -1 and b"null pointer" in L.lib.rgpu_last_error(sv.ctx)
        assert n.value == 0 and L.lib.rgpu_monitor_planes_batch_samples(sv.ctx) == 0   # nothing ran
    finally:
        sv.close()


def test_euler_hip_planes_file(gpu_lib, tmp_path):
    """[monitor] enabled=yes every=3 planes=yes: 3 x 12 rows equal to run_steps_monitored_planes; the monitor file byte for byte the one
    of a run without planes=yes; neither file when monitoring is off"""
    base, ov, prefix, nz = "implode3d", "mesh.nx=24;mesh.ny=24;mesh.nz=12", "implode3d", 12
    exe = os.path.join(ROOT, "ramsesgpu_amd", "euler_hip")
    common = ov + ";run.nstepmax=10;run.noutput=1000;output.outputVtk=no;output.outputHdf5=no;output.outputDir=%s"
    for name, extra in (("planes", ";monitor.enabled=yes;monitor.every=3;monitor.planes=yes"), ("monitor", ";monitor.enabled=yes;monitor.every=3"), ("off", ";monitor.planes=yes")):
        d = tmp_path / name
        d.mkdir()
        r = subprocess.run([exe, "--param", ini(base), "--set", common % d + extra], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:]
    assert not (tmp_path / "off" / (prefix + "_monitor.txt")).exists() and not (tmp_path / "off" / (prefix + "_monitor_planes.txt")).exists()
    assert not (tmp_path / "monitor" / (prefix + "_monitor_planes.txt")).exists()
    assert open(tmp_path / "planes" / (prefix + "_monitor.txt"), "rb").read() == open(tmp_path / "monitor" / (prefix + "_monitor.txt"), "rb").read()
    steps, ts, vals = mp.parse_planes_file(tmp_path / "planes" / (prefix + "_monitor_planes.txt"), nz)
    p = gpu_lib.params_from_ini(ini(base), ov)
    sv = Solver(p, gpu_lib)
    try:
        sv.start(gpu_lib.init_condition(ini(base), ov, p), 0)
        done, series = sv.run_steps_monitored_planes(10, 3)
    finally:
        sv.close()
    assert done == 10 and steps == list(series.step) == [3, 6, 9] and ts == list(series.t)
    assert vals.shape == (3, nz, 16) and np.array_equal(vals, series.values)
