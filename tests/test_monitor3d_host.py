"""The monitors of a lone context (include/rgpu.h, "monitors": rgpu_state_monitor3d, rgpu_run_steps_monitored) without a GPU, on the
test-only host emulation: the 3D monitor against the numpy model of the documented definition (tests/monitor3d_checks.py) bit for bit
and against the bound that holds for any summation order, the NaN rules, the argument checks, and the monitored run -- inside the 3D
device-clock batches (the emulation runs them, the records resolved at once) and through the literal loop (2D, gravity) -- against
the unmonitored run, a second lone context and the model."""
import ctypes as C

import numpy as np
import pytest

import ensemble_checks as ec
import monitor3d_checks as m3
from conftest import ini
from ramsesgpu_amd import _capi
from ramsesgpu_amd.solver import Solver

# implode3d: 72 columns = more than one wavefront of lanes, 40 rows = two segments with the second short, an odd plane count;
# mhd_mri_3d: the shearing box, whose high faces come from ghost layers the shear fill writes
STATES3D = [("implode3d", "mesh.nx=72;mesh.ny=40;mesh.nz=5"), ("orszag-tang3d", "mesh.nx=24;mesh.ny=40;mesh.nz=6"), ("mhd_mri_3d", "mesh.nx=16;mesh.ny=32;mesh.nz=8")]
STATES2D = [("orszag-tang", "mesh.nx=24;mesh.ny=40"), ("kelvin_helmholtz_gpu_2d", "mesh.nx=40;mesh.ny=24")]
GRAVITY = ("rayleigh_taylor_gpu_3d", "mesh.nx=8;mesh.ny=8;mesh.nz=12")
ids = lambda cases: ["%s-%s" % (b, o.replace("mesh.", "").replace(";", "-")) for b, o in cases]


@pytest.fixture(scope="module", autouse=True)
def references():
    yield
    m3.close_references()


@pytest.mark.parametrize("base,ov", STATES3D, ids=ids(STATES3D))
def test_state_monitor3d_equals_the_model(base, ov, emu_lib):
    p = emu_lib.params_from_ini(ini(base), ov)
    U0 = m3.initial_state(emu_lib, base, ov, p)
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
            assert np.array_equal(got, m3.model(U, p)), (got, m3.model(U, p))
            m3.assert_within_any_order_bound(got, U, p)
            assert np.array_equal(got, sv.state_monitor(par))
            if not p.mhdEnabled:
                assert got[6] == 0.0 and got[9] == 0.0 and got[3] != 0.0   # (the perturbation moves the gas along z)
            else:
                assert got[6] > 0.0
            # it reads the state only
            assert emu_lib.lib.rgpu_device_time_step_ready(sv.ctx, par) == ready and sv.state_checksum(par) == checksum
            assert np.array_equal(before, U)
        assert sv.run_steps(2) == 2
    finally:
        sv.close()


def test_nan_cells(emu_lib):
    """one NaN density: the sums that contain the cell are NaN, the others are not, the minima are those of the remaining cells; a
    state of nothing but NaN: the sums are NaN and the extrema keep +inf, +inf, +0.0"""
    for base, ov in STATES3D[:2]:
        p = emu_lib.params_from_ini(ini(base), ov)
        U0 = m3.initial_state(emu_lib, base, ov, p)
        gw = p.ghostWidth
        U0[0, gw + p.nz // 2, gw + p.ny // 2, gw + p.nx // 3] = np.nan
        sv = Solver(p, emu_lib)
        try:
            sv.upload(U0)
            got = sv.state_monitor(0)
            m3.assert_nan_rules(got, U0, p)
            assert np.isnan(got[0]) and np.isnan(got[5]) and not np.isnan(got[1]) and not np.isnan(got[4]) and np.isfinite(got[7:]).all()
            assert np.array_equal(got, m3.model(U0, p), equal_nan=True)
            sv.upload(np.full_like(U0, np.nan))
            got = sv.state_monitor(0)
            assert np.isnan(got[:7 if p.mhdEnabled else 6]).all() and list(got[7:]) == [np.inf, np.inf, 0.0], got
        finally:
            sv.close()


def test_argument_checks(emu_lib):
    L = emu_lib
    out = (C.c_double * 10)()
    p2 = L.params_from_ini(ini("orszag-tang"), "mesh.nx=16;mesh.ny=16")
    p3 = L.params_from_ini(ini("orszag-tang3d"), "mesh.nx=16;mesh.ny=16;mesh.nz=16")
    ps = L.params_from_ini(ini("orszag-tang3d"), "mesh.nx=16;mesh.ny=16;mesh.nz=16", slab=(0, 2))
    sv = Solver(p2, L)
    try:
        assert L.lib.rgpu_state_monitor3d(sv.ctx, 0, out) == -5 and b"3D" in L.lib.rgpu_last_error(sv.ctx)   # RGPU_EUNSUPPORTED
    finally:
        sv.close()
    sv = Solver(ps, L)
    try:
        assert L.lib.rgpu_state_monitor3d(sv.ctx, 0, out) == -1                                             # RGPU_EINVAL
        n, t, d, mn = C.c_int(0), C.c_double(0.0), C.c_double(0.0), C.c_int(7)
        ms, mt, mv = (C.c_int * 5)(), (C.c_double * 5)(), (C.c_double * 50)()
        assert L.lib.rgpu_run_steps_monitored(sv.ctx, 4, 1e300, C.byref(n), C.byref(t), C.byref(d), None, 2, C.byref(mn), ms, mt, mv) == -1
        assert n.value == 0 and mn.value == 0
    finally:
        sv.close()
    for p in (p3, p2):
        sv = Solver(p, L)
        try:
            sv.start(L.init_condition(ini("orszag-tang3d" if p is p3 else "orszag-tang"), "mesh.nx=16;mesh.ny=16" + (";mesh.nz=16" if p is p3 else ""), p), 0)
            if p is p3:
                assert L.lib.rgpu_state_monitor3d(sv.ctx, 0, None) == -1 and L.lib.rgpu_state_monitor3d(None, 0, out) == -1
            n, t, d, mn = C.c_int(0), C.c_double(0.0), C.c_double(0.0), C.c_int(0)
            ms, mt, mv = (C.c_int * 5)(), (C.c_double * 5)(), (C.c_double * 50)()
            call = lambda nsteps, every, a, b, c_, e, f, g, h: L.lib.rgpu_run_steps_monitored(sv.ctx, nsteps, 1e300, a, b, c_, None, every, e, f, g, h)
            full = (C.byref(n), C.byref(t), C.byref(d), C.byref(mn), ms, mt, mv)
            for every in (0, -2):
                assert call(4, every, *full) == -1 and b"every" in L.lib.rgpu_last_error(sv.ctx)
            for hole in range(7):
                args = list(full)
                args[hole] = None
                assert call(4, 2, *args) == -1 and b"null pointer" in L.lib.rgpu_last_error(sv.ctx), hole
            assert call(-1, 2, *full) == -1
            assert L.lib.rgpu_run_steps_monitored(None, 4, 1e300, *full[:3], None, 2, *full[3:]) == -1
            assert n.value == 0 and t.value == 0.0 and sv.state_checksum(0) == sv.state_checksum(1) and L.lib.rgpu_monitor_batch_samples(sv.ctx) == 0   # nothing ran
            assert call(4, 2, *full) == 4 and n.value == 4 and mn.value == 2 and list(ms)[:2] == [2, 4]
            assert call(0, 2, *full) == 0 and mn.value == 0
        finally:
            sv.close()
    assert L.lib.rgpu_monitor_batch_samples(None) == 0


def batch_samples(every):
    """the qualifying steps after the first, plain step of a run of `done` steps, where the batches run; else none"""
    return lambda done, ready: len([s for s in range(2, done + 1) if s % every == 0]) if ready else 0


@pytest.mark.parametrize("every", [1, 3])
@pytest.mark.parametrize("base,ov", STATES3D + STATES2D, ids=ids(STATES3D + STATES2D))
def test_monitored_run(base, ov, every, emu_lib):
    three_d = (base, ov) in STATES3D
    want = [s for s in range(1, 11) if s % every == 0]
    for pieces in (None, [4, 6]):
        done, steps, vals, batch = m3.check_monitored_lone(emu_lib, base, ov, 10, every, pieces=pieces, expect_batch=batch_samples(every) if pieces is None else None)
        assert done == 10 and steps == want
        assert (batch > 0) == three_d   # the emulation runs the 3D device-clock batches; its 2D steps take their dt from the host


BOUNDARY = [("implode3d", "mesh.nx=8;mesh.ny=8;mesh.nz=5"), ("mhd_mri_3d", "mesh.nx=8;mesh.ny=8;mesh.nz=8")]


@pytest.mark.parametrize("base,ov", BOUNDARY, ids=ids(BOUNDARY))
def test_monitored_run_across_a_batch_boundary(base, ov, emu_lib):
    """300 steps, every 7th sampled: 7 does not divide the 256 steps of a batch, so which slots of a batch hold a sample differs between
    the first batch and the second"""
    done, steps, vals, batch = m3.check_monitored_lone(emu_lib, base, ov, 300, 7, expect_batch=batch_samples(7))
    assert done == 300 and len(steps) == 42 and steps[-1] == 294 and batch == 42


@pytest.mark.parametrize("base,ov", m3.SEAMS, ids=ids(m3.SEAMS))
def test_2d_shapes_at_the_seams_of_the_summation_order(base, ov, emu_lib):
    """a 2D state is a volume of one plane: the flat functors at shapes where a lane, a round of the lanes or a segment begins or ends"""
    m3.check_seam_state(emu_lib, base, ov)


def test_nan_cell_on_a_seam_shape(emu_lib):
    for base, ov in m3.SEAMS[4:6]:   # 65 x 33, hydro and MHD
        m3.check_seam_nan(emu_lib, base, ov)


def test_gravity_takes_the_literal_loop(emu_lib):
    base, ov = GRAVITY
    done, steps, vals, batch = m3.check_monitored_lone(emu_lib, base, ov, 10, 3, pieces=[4, 6])
    assert done == 10 and steps == [3, 6, 9] and batch == 0


@pytest.mark.parametrize("base,ov", [STATES3D[0], STATES3D[1], STATES2D[0]], ids=ids([STATES3D[0], STATES3D[1], STATES2D[0]]))
def test_end_time_inside_a_step(base, ov, emu_lib):
    """t passes the end inside the 6th step, a multiple of 3: that last step is sampled; inside the 5th: it is not, and no sample follows"""
    p = emu_lib.params_from_ini(ini(base), ov)
    dts = ec.lone_run(emu_lib, p, m3.initial_state(emu_lib, base, ov, p), 10)["dt_log"]
    for k, want in ((6, [3, 6]), (5, [3])):
        end = ec.end_inside_step(dts, k)
        done, steps, vals, batch = m3.check_monitored_lone(emu_lib, base, ov, 10, 3, tEnd=end)
        assert done == k and steps == want


DRIVER = [("implode3d", "mesh.nx=12;mesh.ny=12;mesh.nz=8", "implode3d", ""), ("orszag-tang", "mesh.nx=16;mesh.ny=16", "orszag-tang2d", ""),
          ("mhd_mri_3d", "mesh.nx=8;mesh.ny=12;mesh.nz=8", "mhd_mri_3d", ";history.enabled=yes;history.dtHist=80.0")]


@pytest.mark.parametrize("base,ov,prefix,extra", DRIVER, ids=["implode3d", "orszag-tang", "mri-with-history"])
def test_run_driver_monitor_file(base, ov, prefix, extra, emu_lib, tmp_path):
    """rgpuh_run with [monitor] enabled=yes every=3: the rows parse to exactly the doubles of Solver.run_steps_monitored -- through
    rgpu_run_steps_monitored, and, with a history file as well, through the direct calls; without the section no file appears"""
    common = ov + ";run.nstepmax=10;run.noutput=1000;output.outputVtk=no;output.outputHdf5=no;output.outputDir=%s" + extra
    for name, more in (("with", ";monitor.enabled=yes;monitor.every=3"), ("without", "")):
        d = tmp_path / name
        d.mkdir()
        err, mc = C.create_string_buffer(512), C.c_double(0)
        assert emu_lib.lib.rgpuh_run(ini(base).encode(), (common % d + more).encode(), C.byref(mc), err, 512) == 10, err.value
    assert not (tmp_path / "without" / (prefix + "_monitor.txt")).exists()
    lines = open(tmp_path / "with" / (prefix + "_monitor.txt")).read().splitlines()
    assert lines[0] == "# nStep totalTime " + " ".join(_capi.MON_NAMES)
    rows = [ln.split() for ln in lines[1:]]
    p = emu_lib.params_from_ini(ini(base), ov)
    sv = Solver(p, emu_lib)
    try:
        sv.start(emu_lib.init_condition(ini(base), ov, p), 0)
        done, series = sv.run_steps_monitored(10, 3)
    finally:
        sv.close()
    assert done == 10 and [int(r[0]) for r in rows] == list(series.step) == [3, 6, 9]
    assert [float(r[1]) for r in rows] == list(series.t)
    assert np.array_equal(np.array([[float(x) for x in r[2:]] for r in rows]), series.values)
    if extra:   # the history file is the one of a run without the monitor
        assert open(tmp_path / "with" / (prefix + "_history.txt"), "rb").read() == open(tmp_path / "without" / (prefix + "_history.txt"), "rb").read()
