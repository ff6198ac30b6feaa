"""The plane monitor (include/rgpu.h, "plane monitors": rgpu_state_monitor_planes, rgpu_run_steps_monitored_planes) without a GPU, on
the test-only host emulation, which runs the flat functors K_mon_prof_cols / K_mon_prof_fold: the rows against the numpy model of the
documented definition bit for bit, folded against rgpu_state_monitor3d, against the bound that holds for any summation order; the NaN
rules per plane; the monitored run inside the 3D device-clock batches (the emulation runs them, the records resolved at once) and
through the literal loop (gravity, the dissipative stage) against the unmonitored run, a second lone context and the model; the
refusals; and the planes file of the run driver.  Helpers: tests/monitor_planes_checks.py."""
import ctypes as C

import numpy as np
import pytest

import ensemble_checks as ec
import monitor_planes_checks as mp
from conftest import ini
from ramsesgpu_amd import _capi
from ramsesgpu_amd.solver import RgpuError, Solver

# shapes at the seams of the order of a row: a lane without a column and a short segment (63 x 31); exactly full lanes and one full
# segment (64 x 32); one column into the second round of the lanes and one row into a second segment (65 x 33); the same one round and
# one segment later (130 x 65); few planes, MHD with the three it needs
SEAMS = [("implode3d", "mesh.nx=65;mesh.ny=33;mesh.nz=3"), ("implode3d", "mesh.nx=63;mesh.ny=31;mesh.nz=5"), ("implode3d", "mesh.nx=130;mesh.ny=65;mesh.nz=2"),
         ("orszag-tang3d", "mesh.nx=63;mesh.ny=31;mesh.nz=4"), ("orszag-tang3d", "mesh.nx=64;mesh.ny=32;mesh.nz=3"), ("orszag-tang3d", "mesh.nx=130;mesh.ny=65;mesh.nz=3"),
         ("mhd_mri_3d", "mesh.nx=65;mesh.ny=33;mesh.nz=4")]
NAN = [SEAMS[0], SEAMS[3]]
BATCHED = [("implode3d", "mesh.nx=40;mesh.ny=24;mesh.nz=12"), ("orszag-tang3d", "mesh.nx=24;mesh.ny=40;mesh.nz=6"), ("mhd_mri_3d", "mesh.nx=16;mesh.ny=32;mesh.nz=8")]
LITERAL = [("rayleigh_taylor_gpu_3d", "mesh.nx=24;mesh.ny=16;mesh.nz=12"), ("mhd_mri_3d", "mesh.nx=16;mesh.ny=32;mesh.nz=8;hydro.nu=0.01;MHD.eta=0.01")]
ids = lambda cases: ["%s-%s" % (b, o.replace("mesh.", "").replace(";", "-")) for b, o in cases]


@pytest.fixture(scope="module", autouse=True)
def references():
    yield
    mp.close_references()


def test_names():
    assert _capi.MONP_NQ == 16 and _capi.MONP_NAMES[:10] == _capi.MON_NAMES
    assert " ".join(_capi.MONP_NAMES) == "mass mx my mz E ekin emag min_rho min_eint max_absdivb bx by bz bxby rvxvy rho2"


@pytest.mark.parametrize("base,ov", SEAMS, ids=ids(SEAMS))
def test_rows_equal_the_model_and_fold_to_the_monitor(base, ov, emu_lib):
    mp.check_single_samples(emu_lib, base, ov)


@pytest.mark.parametrize("base,ov", NAN, ids=ids(NAN))
def test_nan_cell_stays_in_its_plane(base, ov, emu_lib):
    mp.check_nan_plane(emu_lib, base, ov)


@pytest.mark.parametrize("every", [1, 3])
@pytest.mark.parametrize("base,ov", BATCHED, ids=ids(BATCHED))
def test_samples_inside_the_batches(base, ov, every, emu_lib):
    done, steps, vals, batch = mp.check_monitored_planes(emu_lib, base, ov, 10, every, expect_batch=mp.batch_samples(every))
    assert done == 10 and steps == [s for s in range(1, 11) if s % every == 0]
    assert batch == len(steps) - (1 if every == 1 else 0)


@pytest.mark.parametrize("base,ov", BATCHED, ids=ids(BATCHED))
def test_run_in_pieces(base, ov, emu_lib):
    """[4, 6]: step 1 is plain, the second call begins on the device path -- samples 3, 6, 9 all inside batches"""
    done, steps, vals, batch = mp.check_monitored_planes(emu_lib, base, ov, 10, 3, pieces=[4, 6], expect_batch=lambda done, ready: 3 if ready == 1 else -1)
    assert done == 10 and steps == [3, 6, 9] and batch == 3


@pytest.mark.parametrize("base,ov", BATCHED, ids=ids(BATCHED))
def test_end_time_inside_a_step(base, ov, emu_lib):
    """t passes the end inside the 6th step, a multiple of 3: that last step is sampled; inside the 5th: it is not, and no sample follows"""
    p = emu_lib.params_from_ini(ini(base), ov)
    dts = ec.lone_run(emu_lib, p, mp.initial_state(emu_lib, base, ov, p), 10)["dt_log"]
    for k, want in ((6, [3, 6]), (5, [3])):
        done, steps, vals, batch = mp.check_monitored_planes(emu_lib, base, ov, 10, 3, tEnd=ec.end_inside_step(dts, k))
        assert done == k and steps == want and batch > 0


def test_across_a_batch_boundary(emu_lib):
    """300 steps, every 7th sampled: 7 does not divide the 256 steps of a batch, so the samples of the second batch sit in other slots
    of the log than those of the first"""
    base, ov = BATCHED[0]
    done, steps, vals, batch = mp.check_monitored_planes(emu_lib, base, ov, 300, 7, expect_batch=mp.batch_samples(7))
    assert done == 300 and len(steps) == 42 and steps[-1] == 294 and batch == 42


def test_the_log_grows_with_the_cadence(emu_lib):
    """every = 5 first (52 slots), then every = 1 on the same context (257): the second call's log is larger than the first's"""
    base, ov = BATCHED[1]
    p = emu_lib.params_from_ini(ini(base), ov)
    U0 = mp.initial_state(emu_lib, base, ov, p)
    sv = Solver(p, emu_lib)
    try:
        sv.start(U0, 0)
        done, s5 = sv.run_steps_monitored_planes(5, 5)
        assert done == 5 and list(s5.step) == [5]
        done, s1 = sv.run_steps_monitored_planes(5, 1)
        assert done == 5 and list(s1.step) == [6, 7, 8, 9, 10]
        assert emu_lib.lib.rgpu_monitor_planes_batch_samples(sv.ctx) == 1 + 5
        for s, v in zip(list(s5.step) + list(s1.step), list(s5.values) + list(s1.values)):
            assert np.array_equal(v, mp.stepped_reference(emu_lib, base, ov, p, U0, s)[0]), s
    finally:
        sv.close()


@pytest.mark.parametrize("base,ov", LITERAL, ids=["gravity", "dissipative"])
def test_literal_path(base, ov, emu_lib):
    """gravity and the dissipative stage take their time step from the host: the literal loop, the same series, no sample on the device"""
    def never(done, ready):
        assert ready == 0, "the context takes its time step from the device"
        return 0
    done, steps, vals, batch = mp.check_monitored_planes(emu_lib, base, ov, 10, 3, pieces=[4, 6], expect_batch=never)
    assert done == 10 and steps == [3, 6, 9] and batch == 0


def test_refusals(emu_lib):
    L = emu_lib
    p2 = L.params_from_ini(ini("orszag-tang"), "mesh.nx=16;mesh.ny=16")
    p3 = L.params_from_ini(ini("orszag-tang3d"), "mesh.nx=16;mesh.ny=16;mesh.nz=8")
    ps = L.params_from_ini(ini("orszag-tang3d"), "mesh.nx=16;mesh.ny=16;mesh.nz=16", slab=(0, 2))
    out = (C.c_double * (16 * 16))()
    n, t, d, mn = C.c_int(0), C.c_double(0.0), C.c_double(0.0), C.c_int(7)
    ms, mt, mv = (C.c_int * 5)(), (C.c_double * 5)(), (C.c_double * (5 * 16 * 16))()
    full = (C.byref(n), C.byref(t), C.byref(d), C.byref(mn), ms, mt, mv)
    call = lambda ctx, nsteps, every, a, b, c_, e, f, g, h: L.lib.rgpu_run_steps_monitored_planes(ctx, nsteps, 1e300, a, b, c_, None, every, e, f, g, h)
    sv = Solver(p2, L)
    try:
        sv.start(L.init_condition(ini("orszag-tang"), "mesh.nx=16;mesh.ny=16", p2), 0)
        assert L.lib.rgpu_state_monitor_planes(sv.ctx, 0, out) == -5 and b"3D" in L.lib.rgpu_last_error(sv.ctx)   # RGPU_EUNSUPPORTED
        assert call(sv.ctx, 4, 2, *full) == -5 and b"3D" in L.lib.rgpu_last_error(sv.ctx) and mn.value == 0 and n.value == 0
        with pytest.raises(RgpuError):
            sv.state_monitor_planes()
    finally:
        sv.close()
    sv = Solver(ps, L)
    try:
        mn.value = 7
        assert L.lib.rgpu_state_monitor_planes(sv.ctx, 0, out) == -1                                               # RGPU_EINVAL
        assert call(sv.ctx, 4, 2, *full) == -1 and n.value == 0 and mn.value == 0
    finally:
        sv.close()
    sv = Solver(p3, L)
    try:
        sv.start(L.init_condition(ini("orszag-tang3d"), "mesh.nx=16;mesh.ny=16;mesh.nz=8", p3), 0)
        assert L.lib.rgpu_state_monitor_planes(sv.ctx, 0, None) == -1 and L.lib.rgpu_state_monitor_planes(None, 0, out) == -1
        for every in (0, -2):
            assert call(sv.ctx, 4, every, *full) == -1 and b"every" in L.lib.rgpu_last_error(sv.ctx)
        for hole in range(7):
            args = list(full)
            args[hole] = None
            assert call(sv.ctx, 4, 2, *args) == -1 and b"null pointer" in L.lib.rgpu_last_error(sv.ctx), hole
        assert call(sv.ctx, -1, 2, *full) == -1
        assert call(None, 4, 2, *full) == -1
        assert n.value == 0 and t.value == 0.0 and L.lib.rgpu_monitor_planes_batch_samples(sv.ctx) == 0   # nothing ran
        assert call(sv.ctx, 4, 2, *full) == 4 and n.value == 4 and mn.value == 2 and list(ms)[:2] == [2, 4]
        assert call(sv.ctx, 0, 2, *full) == 0 and mn.value == 0
    finally:
        sv.close()
    assert L.lib.rgpu_monitor_planes_batch_samples(None) == 0


def test_product_library_refuses_without_a_state(product_lib):
    """the product has no CPU fallback: on a machine without a device rgpu_create fails with RGPU_ENODEVICE and the context it returns
    holds no state, on which both entry points refuse with RGPU_EINVAL and write no sample; with a device the context is created"""
    L = product_lib
    p = L.params_from_ini(ini("implode3d"), "mesh.nx=8;mesh.ny=8;mesh.nz=8")
    ctx = C.c_void_p()
    L.lib.rgpu_create.restype = C.c_int
    rc = L.lib.rgpu_create(C.byref(p), C.byref(ctx))
    try:
        assert rc in (0, -2) and ctx.value
        if rc == -2:
            out = (C.c_double * (8 * 16))()
            n, t, d, mn = C.c_int(0), C.c_double(0.0), C.c_double(0.0), C.c_int(7)
            ms, mt, mv = (C.c_int * 3)(), (C.c_double * 3)(), (C.c_double * (3 * 8 * 16))()
            assert L.lib.rgpu_state_monitor_planes(ctx, 0, out) == -1
            assert L.lib.rgpu_run_steps_monitored_planes(ctx, 4, 1e300, C.byref(n), C.byref(t), C.byref(d), None, 2, C.byref(mn), ms, mt, mv) == -1
            assert n.value == 0 and mn.value == 0 and not any(out) and not any(mv)
    finally:
        L.lib.rgpu_destroy(ctx)


def test_run_driver_planes_file(emu_lib, tmp_path):
    """rgpuh_run with [monitor] enabled=yes every=3 planes=yes: 3 x nz rows, exactly the doubles of Solver.run_steps_monitored_planes;
    the monitor file is byte for byte the one a run without planes=yes writes; neither file appears when monitoring is off; a 2D
    run writes its monitor file and no planes file"""
    base, ov, prefix, nz = "implode3d", "mesh.nx=12;mesh.ny=12;mesh.nz=8", "implode3d", 8
    common = ov + ";run.nstepmax=10;run.noutput=1000;output.outputVtk=no;output.outputHdf5=no;output.outputDir=%s"
    for name, more in (("planes", ";monitor.enabled=yes;monitor.every=3;monitor.planes=yes"), ("monitor", ";monitor.enabled=yes;monitor.every=3"), ("off", ";monitor.planes=yes")):
        d = tmp_path / name
        d.mkdir()
        err, mc = C.create_string_buffer(512), C.c_double(0)
        assert emu_lib.lib.rgpuh_run(ini(base).encode(), (common % d + more).encode(), C.byref(mc), err, 512) == 10, err.value
    assert not (tmp_path / "off" / (prefix + "_monitor.txt")).exists() and not (tmp_path / "off" / (prefix + "_monitor_planes.txt")).exists()
    assert not (tmp_path / "monitor" / (prefix + "_monitor_planes.txt")).exists()
    assert open(tmp_path / "planes" / (prefix + "_monitor.txt"), "rb").read() == open(tmp_path / "monitor" / (prefix + "_monitor.txt"), "rb").read()
    steps, ts, vals = mp.parse_planes_file(tmp_path / "planes" / (prefix + "_monitor_planes.txt"), nz)
    p = emu_lib.params_from_ini(ini(base), ov)
    sv = Solver(p, emu_lib)
    try:
        sv.start(emu_lib.init_condition(ini(base), ov, p), 0)
        done, series = sv.run_steps_monitored_planes(10, 3)
    finally:
        sv.close()
    assert done == 10 and steps == list(series.step) == [3, 6, 9] and ts == list(series.t)
    assert vals.shape == (3, nz, 16) and np.array_equal(vals, series.values)
    d = tmp_path / "flat"
    d.mkdir()
    err, mc = C.create_string_buffer(512), C.c_double(0)
    ov2 = "mesh.nx=16;mesh.ny=16;run.nstepmax=6;run.noutput=1000;output.outputVtk=no;output.outputHdf5=no;output.outputDir=%s;monitor.enabled=yes;monitor.every=3;monitor.planes=yes" % d
    assert emu_lib.lib.rgpuh_run(ini("orszag-tang").encode(), ov2.encode(), C.byref(mc), err, 512) == 6, err.value
    assert (d / "orszag-tang2d_monitor.txt").exists() and not (d / "orszag-tang2d_monitor_planes.txt").exists()
