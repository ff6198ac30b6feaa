"""The map monitor (include/rgpu.h, "map monitors": rgpu_state_maps, rgpu_run_steps_mapped) without a GPU, on the test-only host
emulation, which runs the flat functor K_mon_map: every double of slices and projections along the three axes against the numpy model
of the documented definition; the slice identity against the download; the any-order bound against rgpu_state_monitor3d; the NaN rule;
the mapped run inside the 3D device-clock batches (the emulation runs them, the records resolved at once) and through the literal
loop against the unmapped run, a second lone context and the model; the byte budget of the log; the refusals; and the files of the
run driver.  Helpers: tests/monitor_maps_checks.py."""
import ctypes as C

import numpy as np
import pytest

import ensemble_checks as ec
import monitor_maps_checks as mm
from conftest import ini
from ramsesgpu_amd import _capi
from ramsesgpu_amd.solver import RgpuError, Solver

# nx: a ragged 64-wide tile along i (63), exactly one (64), one cell into a second (65) and into a third (130); ny nz: row counts that
# do not fill a row tile of the kernel that sums along x
SEAMS = [("implode3d", "mesh.nx=65;mesh.ny=33;mesh.nz=3"), ("implode3d", "mesh.nx=63;mesh.ny=31;mesh.nz=5"),
         ("orszag-tang3d", "mesh.nx=64;mesh.ny=32;mesh.nz=3"), ("orszag-tang3d", "mesh.nx=130;mesh.ny=65;mesh.nz=3"),
         ("mhd_mri_3d", "mesh.nx=65;mesh.ny=33;mesh.nz=4")]
NAN = [SEAMS[0], SEAMS[2]]
BATCHED = [("implode3d", "mesh.nx=40;mesh.ny=24;mesh.nz=12"), ("orszag-tang3d", "mesh.nx=24;mesh.ny=40;mesh.nz=6"), ("mhd_mri_3d", "mesh.nx=16;mesh.ny=32;mesh.nz=8")]
LITERAL = [("rayleigh_taylor_gpu_3d", "mesh.nx=24;mesh.ny=16;mesh.nz=12"), ("mhd_mri_3d", "mesh.nx=16;mesh.ny=32;mesh.nz=8;hydro.nu=0.01;MHD.eta=0.01")]
ids = lambda cases: ["%s-%s" % (b, o.replace("mesh.", "").replace(";", "-")) for b, o in cases]


@pytest.fixture(scope="module", autouse=True)
def references():
    yield
    mm.close_references()


def test_names():
    assert _capi.MAP_NQ == 12 and " ".join(_capi.MAP_NAMES) == "rho mx my mz E ekin emag eint bx by bz rho2"
    assert [_capi.MONP_NAMES[c] for c in mm.COLUMNS] == ["mass", "mx", "my", "mz", "E", "ekin", "emag", "min_eint", "bx", "by", "bz", "rho2"]


@pytest.mark.parametrize("base,ov", SEAMS, ids=ids(SEAMS))
def test_maps_equal_the_model(base, ov, emu_lib):
    mm.check_seams(emu_lib, base, ov)


@pytest.mark.parametrize("base,ov", NAN, ids=ids(NAN))
def test_nan_cell_stays_in_its_pixel(base, ov, emu_lib):
    mm.check_nan_cell(emu_lib, base, ov)


@pytest.mark.parametrize("every", [1, 3])
@pytest.mark.parametrize("base,ov", BATCHED, ids=ids(BATCHED))
def test_samples_inside_the_batches(base, ov, every, emu_lib):
    done, steps, maps, batch = mm.check_mapped(emu_lib, base, ov, 10, every, expect_batch=mm.batch_samples(every))
    assert done == 10 and steps == [s for s in range(1, 11) if s % every == 0]
    assert batch == len(steps) - (1 if every == 1 else 0)


@pytest.mark.parametrize("base,ov", BATCHED, ids=ids(BATCHED))
def test_run_in_pieces(base, ov, emu_lib):
    """[4, 6]: step 1 is plain, the second call begins on the device path -- samples 3, 6, 9 all inside batches"""
    done, steps, maps, batch = mm.check_mapped(emu_lib, base, ov, 10, 3, pieces=[4, 6], expect_batch=lambda done, ready: 3 if ready == 1 else -1)
    assert done == 10 and steps == [3, 6, 9] and batch == 3


@pytest.mark.parametrize("base,ov", BATCHED, ids=ids(BATCHED))
def test_end_time_inside_a_step(base, ov, emu_lib):
    """t passes the end inside the 6th step, a multiple of 3: that last step is sampled; inside the 5th: it is not, and no sample follows"""
    p = emu_lib.params_from_ini(ini(base), ov)
    dts = ec.lone_run(emu_lib, p, mm.initial_state(emu_lib, base, ov, p), 10)["dt_log"]
    for k, want in ((6, [3, 6]), (5, [3])):
        done, steps, maps, batch = mm.check_mapped(emu_lib, base, ov, 10, 3, tEnd=ec.end_inside_step(dts, k))
        assert done == k and steps == want and batch > 0


def test_across_a_batch_boundary(emu_lib):
    """300 steps, every 7th sampled: 7 does not divide the 256 steps of a batch, so the samples of the second batch sit in other slots
    of the log than those of the first"""
    base, ov = BATCHED[0]
    done, steps, maps, batch = mm.check_mapped(emu_lib, base, ov, 300, 7, expect_batch=mm.batch_samples(7))
    assert done == 300 and len(steps) == 42 and steps[-1] == 294 and batch == 42


def test_a_small_budget_cuts_the_batches(emu_lib):
    """a log of exactly two samples, 20 steps, every 3rd sampled: the six samples of the default budget, all taken inside batches that
    were cut to two samples each; the option is restored"""
    base, ov = BATCHED[0]
    before = emu_lib.lib.rgpu_get_option(b"map_log_kib")
    assert before == 262144
    done, steps, maps, batch = mm.check_mapped(emu_lib, base, ov, 20, 3, expect_batch=mm.batch_samples(3))
    with mm.option(emu_lib, "map_log_kib", mm.sample_kib(emu_lib, base, ov, 2)):
        done2, steps2, maps2, batch2 = mm.check_mapped(emu_lib, base, ov, 20, 3, expect_batch=mm.batch_samples(3))
    assert emu_lib.lib.rgpu_get_option(b"map_log_kib") == before
    assert done == done2 == 20 and steps == steps2 == [3, 6, 9, 12, 15, 18] and batch == batch2 == 6
    for a, b in zip(maps, maps2):
        mm.assert_same_bits(a, b, "the small budget against the default one")


def test_a_budget_below_one_sample_takes_the_literal_loop(emu_lib):
    base, ov = BATCHED[0]
    with mm.option(emu_lib, "map_log_kib", mm.sample_kib(emu_lib, base, ov, 0)):
        done, steps, maps, batch = mm.check_mapped(emu_lib, base, ov, 10, 3, expect_batch=lambda done, ready: 0)
    assert done == 10 and steps == [3, 6, 9] and batch == 0


@pytest.mark.parametrize("base,ov", LITERAL, ids=["gravity", "dissipative"])
def test_literal_path(base, ov, emu_lib):
    """gravity and the dissipative stage take their time step from the host: the literal loop, the same series, no sample on the device"""
    def never(done, ready):
        assert ready == 0, "the context takes its time step from the device"
        return 0
    done, steps, maps, batch = mm.check_mapped(emu_lib, base, ov, 10, 3, pieces=[4, 6], expect_batch=never)
    assert done == 10 and steps == [3, 6, 9] and batch == 0


def test_refusals(emu_lib):
    L = emu_lib
    Spec = _capi.RgpuMapSpec
    p2 = L.params_from_ini(ini("orszag-tang"), "mesh.nx=16;mesh.ny=16")
    p3 = L.params_from_ini(ini("orszag-tang3d"), "mesh.nx=16;mesh.ny=12;mesh.nz=8")
    ps = L.params_from_ini(ini("orszag-tang3d"), "mesh.nx=16;mesh.ny=16;mesh.nz=16", slab=(0, 2))
    good = (Spec * 2)(Spec(2, 3, 4), Spec(0, 0, 16))
    W = 12 * (16 * 16 + 16 * 16)
    out = (C.c_double * W)()
    n, t, d, mn = C.c_int(0), C.c_double(0.0), C.c_double(0.0), C.c_int(7)
    ms, mt, mv = (C.c_int * 5)(), (C.c_double * 5)(), (C.c_double * (5 * W))()
    full = [C.byref(n), C.byref(t), C.byref(d), good, C.byref(mn), ms, mt, mv]

    def call(ctx, nsteps, every, nmaps, args):
        mn.value = 7
        a, b, c_, specs, e, f, g, h = args
        return L.lib.rgpu_run_steps_mapped(ctx, nsteps, 1e300, a, b, c_, None, every, nmaps, specs, e, f, g, h)
    sv = Solver(p2, L)
    try:
        sv.start(L.init_condition(ini("orszag-tang"), "mesh.nx=16;mesh.ny=16", p2), 0)
        assert L.lib.rgpu_state_maps(sv.ctx, 0, 2, good, out) == -5 and b"3D" in L.lib.rgpu_last_error(sv.ctx)   # RGPU_EUNSUPPORTED
        assert call(sv.ctx, 4, 2, 2, full) == -5 and b"3D" in L.lib.rgpu_last_error(sv.ctx) and mn.value == 0 and n.value == 0
        assert L.lib.rgpu_map_doubles(sv.ctx, C.byref(good[0])) == 0
        with pytest.raises(RgpuError):
            sv.state_maps([("z", 0, 1)])
    finally:
        sv.close()
    sv = Solver(ps, L)
    try:
        assert L.lib.rgpu_state_maps(sv.ctx, 0, 2, good, out) == -1                                               # RGPU_EINVAL
        assert call(sv.ctx, 4, 2, 2, full) == -1 and n.value == 0 and mn.value == 0
        assert L.lib.rgpu_map_doubles(sv.ctx, C.byref(good[0])) == 0
    finally:
        sv.close()
    sv = Solver(p3, L)
    try:
        sv.start(L.init_condition(ini("orszag-tang3d"), "mesh.nx=16;mesh.ny=12;mesh.nz=8", p3), 0)
        assert L.lib.rgpu_map_doubles(sv.ctx, C.byref(Spec(2, 3, 4))) == 12 * 12 * 16 and L.lib.rgpu_map_doubles(sv.ctx, C.byref(Spec(1, 0, 12))) == 12 * 8 * 16
        assert L.lib.rgpu_map_doubles(sv.ctx, C.byref(Spec(0, 0, 16))) == 12 * 8 * 12 and L.lib.rgpu_map_doubles(sv.ctx, None) == 0 and L.lib.rgpu_map_doubles(None, C.byref(good[0])) == 0
        assert L.lib.rgpu_state_maps(sv.ctx, 0, 2, good, None) == -1 and L.lib.rgpu_state_maps(sv.ctx, 0, 2, None, out) == -1 and L.lib.rgpu_state_maps(None, 0, 2, good, out) == -1
        for every in (0, -2):
            assert call(sv.ctx, 4, every, 2, full) == -1 and b"every" in L.lib.rgpu_last_error(sv.ctx) and mn.value == 0
        for hole in range(8):
            args = list(full)
            args[hole] = None
            assert call(sv.ctx, 4, 2, 2, args) == -1 and b"null pointer" in L.lib.rgpu_last_error(sv.ctx), hole
            assert mn.value == (7 if hole == 4 else 0)
        assert call(sv.ctx, -1, 2, 2, full) == -1 and mn.value == 0
        assert call(None, 4, 2, 2, full) == -1
        for nmaps in (0, -1, _capi.MAP_MAX + 1):
            assert call(sv.ctx, 4, 2, nmaps, full) == -1 and b"nmaps" in L.lib.rgpu_last_error(sv.ctx) and mn.value == 0
            assert L.lib.rgpu_state_maps(sv.ctx, 0, nmaps, good, out) == -1 and b"nmaps" in L.lib.rgpu_last_error(sv.ctx)
        # an axis outside 0 .. 2, and ranges that are not 0 <= lo < hi <= n_axis (nx = 16, ny = 12, nz = 8): the message names the map
        for bad in (Spec(-1, 0, 1), Spec(3, 0, 1), Spec(0, -1, 4), Spec(0, 4, 4), Spec(0, 5, 4), Spec(0, 0, 17), Spec(1, 0, 13), Spec(2, 0, 9), Spec(2, 8, 9)):
            for where in (0, 1):
                specs = (Spec * 2)(good[0], good[1])
                specs[where] = bad
                args = list(full)
                args[3] = specs
                assert call(sv.ctx, 4, 2, 2, args) == -1 and b"map %d:" % where in L.lib.rgpu_last_error(sv.ctx) and mn.value == 0, (bad.axis, bad.lo, bad.hi)
                assert L.lib.rgpu_state_maps(sv.ctx, 0, 2, specs, out) == -1 and b"map %d:" % where in L.lib.rgpu_last_error(sv.ctx)
            assert L.lib.rgpu_map_doubles(sv.ctx, C.byref(bad)) == 0
        assert n.value == 0 and t.value == 0.0 and L.lib.rgpu_map_batch_samples(sv.ctx) == 0 and not any(out) and not any(mv)   # nothing ran
        assert call(sv.ctx, 4, 2, 2, full) == 4 and n.value == 4 and mn.value == 2 and list(ms)[:2] == [2, 4]
        assert call(sv.ctx, 0, 2, 2, full) == 0 and mn.value == 0
    finally:
        sv.close()
    assert L.lib.rgpu_map_batch_samples(None) == 0


def test_product_library_refuses_without_a_state(product_lib):
    """the product has no CPU fallback: on a machine without a device rgpu_create fails with RGPU_ENODEVICE and the context it returns
    holds no state, on which the entry points refuse with RGPU_EINVAL and write no sample; with a device the context is created"""
    L = product_lib
    p = L.params_from_ini(ini("implode3d"), "mesh.nx=8;mesh.ny=8;mesh.nz=8")
    ctx = C.c_void_p()
    L.lib.rgpu_create.restype = C.c_int
    rc = L.lib.rgpu_create(C.byref(p), C.byref(ctx))
    try:
        assert rc in (0, -2) and ctx.value
        if rc == -2:
            spec = _capi.RgpuMapSpec(2, 0, 8)
            out = (C.c_double * (12 * 64))()
            n, t, d, mn = C.c_int(0), C.c_double(0.0), C.c_double(0.0), C.c_int(7)
            ms, mt, mv = (C.c_int * 3)(), (C.c_double * 3)(), (C.c_double * (3 * 12 * 64))()
            assert L.lib.rgpu_state_maps(ctx, 0, 1, C.byref(spec), out) == -1 and L.lib.rgpu_map_doubles(ctx, C.byref(spec)) == 0
            assert L.lib.rgpu_run_steps_mapped(ctx, 4, 1e300, C.byref(n), C.byref(t), C.byref(d), None, 2, 1, C.byref(spec), C.byref(mn), ms, mt, mv) == -1
            assert n.value == 0 and mn.value == 0 and not any(out) and not any(mv)
    finally:
        L.lib.rgpu_destroy(ctx)


def test_run_driver_map_files(emu_lib, tmp_path):
    """rgpuh_run with [maps]: the .npy files, their list, nothing with enabled=no, and the monitor file untouched by the maps; a 2D
    run writes no map file"""
    def run(overrides):
        err, mc = C.create_string_buffer(512), C.c_double(0)
        assert emu_lib.lib.rgpuh_run(ini("implode3d").encode(), overrides.encode(), C.byref(mc), err, 512) == 10, err.value
    mm.check_driver_files(emu_lib, run, tmp_path)
    d = tmp_path / "flat"
    d.mkdir()
    err, mc = C.create_string_buffer(512), C.c_double(0)
    ov2 = "mesh.nx=16;mesh.ny=16;run.nstepmax=6;run.noutput=1000;output.outputVtk=no;output.outputHdf5=no;output.outputDir=%s;maps.enabled=yes;maps.every=3;maps.map0=z:0" % d
    assert emu_lib.lib.rgpuh_run(ini("orszag-tang").encode(), ov2.encode(), C.byref(mc), err, 512) == 6, err.value
    assert not list(d.glob("*_map*"))
    bad = "mesh.nx=12;mesh.ny=12;mesh.nz=8;run.nstepmax=2;output.outputVtk=no;output.outputHdf5=no;output.outputDir=%s;maps.enabled=yes;maps.map0=z:8" % d
    assert emu_lib.lib.rgpuh_run(ini("implode3d").encode(), bad.encode(), C.byref(mc), err, 512) < 0 and b"map0" in err.value
