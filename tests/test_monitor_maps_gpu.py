"""The map monitor on the GPU, both libraries (csrc/hip/monitor_maps.h): every double of slices and projections along the three axes
against the numpy model at shapes on the seams of the kernels -- the maps along x with the direct and with the tiled kernel (option
"map_x_tiled"), which must give the same bits; the slice identity against the download; the any-order bound against
rgpu_state_monitor3d; the NaN rule; rgpu_run_steps_mapped with the samples taken behind the steps of the device-clock batches -- 3D
hydro, 3D MHD, the shearing box -- against the unmapped run and a second lone context; a run in pieces, an end time inside a batch, a
run across the 256-step boundary; the byte budget of the log; the literal loop (gravity, the dissipative stage); the refusals; and the
map files of euler_hip.  Helpers: tests/monitor_maps_checks.py."""
import ctypes as C
import os
import subprocess

import pytest

import ensemble_checks as ec
import monitor_maps_checks as mm
from conftest import ROOT, ini
from ramsesgpu_amd import _capi
from ramsesgpu_amd.solver import Solver

pytestmark = pytest.mark.gpu

# nx: a ragged 64-wide tile along i (63), exactly one (64), one cell into a second (65) and into a third (130); ny nz: row counts that
# do not fill a row tile of the kernel that sums along x
SEAMS = [("implode3d", "mesh.nx=65;mesh.ny=33;mesh.nz=3"), ("implode3d", "mesh.nx=63;mesh.ny=31;mesh.nz=5"),
         ("orszag-tang3d", "mesh.nx=64;mesh.ny=32;mesh.nz=3"), ("orszag-tang3d", "mesh.nx=130;mesh.ny=65;mesh.nz=3"),
         ("mhd_mri_3d", "mesh.nx=65;mesh.ny=33;mesh.nz=4")]
NAN = [SEAMS[0], SEAMS[2]]
BATCHED = [("implode3d", "mesh.nx=40;mesh.ny=24;mesh.nz=12"), ("orszag-tang3d", "mesh.nx=24;mesh.ny=40;mesh.nz=6"), ("mhd_mri_3d", "mesh.nx=16;mesh.ny=32;mesh.nz=8")]
LITERAL = [("rayleigh_taylor_gpu_3d", "mesh.nx=24;mesh.ny=16;mesh.nz=12"), ("mhd_mri_3d", "mesh.nx=16;mesh.ny=32;mesh.nz=8;hydro.nu=0.01;MHD.eta=0.01")]
ids = lambda cases: ["%s-%s" % (b, o.replace("mesh.", "").replace(";", "-")) for b, o in cases]


@pytest.fixture(scope="module", params=["exact", "contracted"])
def lib(request, gpu_lib, gpu_contracted_lib):
    yield gpu_lib if request.param == "exact" else gpu_contracted_lib
    mm.close_references()


def test_the_threshold_chooses_between_the_two_kernels_of_x(lib):
    """with "map_x_tiled" = -1 a thin and a thick range along x take different kernels: both equal the forced variants bit for bit"""
    base, ov = SEAMS[3]
    p = lib.params_from_ini(ini(base), ov)
    sv = Solver(p, lib)
    try:
        sv.start(mm.initial_state(lib, base, ov, p), 0)
        specs = [("x", 5, 6), ("x", 3, 11), ("x", 0, p.nx)]
        got = {}
        for variant in (-1, 0, 1):
            with mm.option(lib, "map_x_tiled", variant):
                got[variant] = sv.state_maps(specs)
        assert lib.lib.rgpu_get_option(b"map_x_tiled") == -1
        for m, spec in enumerate(specs):
            mm.assert_same_bits(got[-1][m], got[0][m], spec)
            mm.assert_same_bits(got[-1][m], got[1][m], spec)
    finally:
        sv.close()


@pytest.mark.parametrize("base,ov", SEAMS, ids=ids(SEAMS))
def test_maps_equal_the_model(base, ov, lib):
    mm.check_seams(lib, base, ov, x_variants=(0, 1))


@pytest.mark.parametrize("base,ov", NAN, ids=ids(NAN))
def test_nan_cell_stays_in_its_pixel(base, ov, lib):
    mm.check_nan_cell(lib, base, ov)


@pytest.mark.parametrize("every", [1, 3])
@pytest.mark.parametrize("base,ov", BATCHED, ids=ids(BATCHED))
def test_samples_inside_the_device_batches(base, ov, every, lib):
    done, steps, maps, batch = mm.check_mapped(lib, base, ov, 10, every, expect_batch=mm.batch_samples(every))
    assert done == 10 and steps == [s for s in range(1, 11) if s % every == 0]
    assert batch == len(steps) - (1 if every == 1 else 0)


@pytest.mark.parametrize("base,ov", BATCHED, ids=ids(BATCHED))
def test_run_in_pieces(base, ov, lib):
    """[4, 6]: step 1 is plain, the second call begins on the device path -- samples 3, 6, 9 all inside batches"""
    done, steps, maps, batch = mm.check_mapped(lib, base, ov, 10, 3, pieces=[4, 6], expect_batch=lambda done, ready: 3 if ready == 1 else -1)
    assert done == 10 and steps == [3, 6, 9] and batch == 3


@pytest.mark.parametrize("base,ov", BATCHED, ids=ids(BATCHED))
def test_end_time_inside_a_batch(base, ov, lib):
    """t passes the end inside the 6th step, a multiple of 3: that last step is sampled; inside the 5th: it is not, and no sample follows.
    The sample of step 9, queued behind a step that did not run, is not counted as taken but was queued: the counter counts launches"""
    p = lib.params_from_ini(ini(base), ov)
    dts = ec.lone_run(lib, p, mm.initial_state(lib, base, ov, p), 10)["dt_log"]
    for k, want in ((6, [3, 6]), (5, [3])):
        queued = lambda done, ready: 3 if ready == 1 else -1   # steps 3, 6, 9 of the ten queued: on the device path, without a condition
        done, steps, maps, batch = mm.check_mapped(lib, base, ov, 10, 3, tEnd=ec.end_inside_step(dts, k), expect_batch=queued)
        assert done == k and steps == want and batch == 3


def test_across_a_batch_boundary(lib):
    """300 steps, every 7th sampled: 7 does not divide the 256 steps of a batch, so the samples of the second batch sit in other slots
    of the log than those of the first"""
    base, ov = BATCHED[0]
    done, steps, maps, batch = mm.check_mapped(lib, base, ov, 300, 7, expect_batch=mm.batch_samples(7))
    assert done == 300 and len(steps) == 42 and steps[-1] == 294 and batch == 42


def test_a_small_budget_cuts_the_batches(lib):
    """a log of exactly two samples, 20 steps, every 3rd sampled: the six samples of the default budget, all taken inside batches that
    were cut to two samples each; the option is restored"""
    base, ov = BATCHED[0]
    before = lib.lib.rgpu_get_option(b"map_log_kib")
    assert before == 262144
    done, steps, maps, batch = mm.check_mapped(lib, base, ov, 20, 3, expect_batch=mm.batch_samples(3))
    with mm.option(lib, "map_log_kib", mm.sample_kib(lib, base, ov, 2)):
        done2, steps2, maps2, batch2 = mm.check_mapped(lib, base, ov, 20, 3, expect_batch=mm.batch_samples(3))
    assert lib.lib.rgpu_get_option(b"map_log_kib") == before
    assert done == done2 == 20 and steps == steps2 == [3, 6, 9, 12, 15, 18] and batch == batch2 == 6
    for a, b in zip(maps, maps2):
        mm.assert_same_bits(a, b, "the small budget against the default one")


def test_a_budget_below_one_sample_takes_the_literal_loop(lib):
    base, ov = BATCHED[0]
    with mm.option(lib, "map_log_kib", mm.sample_kib(lib, base, ov, 0)):
        done, steps, maps, batch = mm.check_mapped(lib, base, ov, 10, 3, expect_batch=lambda done, ready: 0)
    assert done == 10 and steps == [3, 6, 9] and batch == 0


@pytest.mark.parametrize("base,ov", LITERAL, ids=["gravity", "dissipative"])
def test_literal_path(base, ov, lib):
    """gravity and the dissipative stage take their time step from the host: the literal loop, the same series, no sample on the device"""
    def never(done, ready):
        assert ready == 0, "the context takes its time step from the device"
        return 0
    done, steps, maps, batch = mm.check_mapped(lib, base, ov, 10, 3, pieces=[4, 6], expect_batch=never)
    assert done == 10 and steps == [3, 6, 9] and batch == 0


def test_refusals(lib):
    L = lib
    Spec = _capi.RgpuMapSpec
    p2 = L.params_from_ini(ini("orszag-tang"), "mesh.nx=16;mesh.ny=16")
    p3 = L.params_from_ini(ini("orszag-tang3d"), "mesh.nx=16;mesh.ny=12;mesh.nz=8")
    good = (Spec * 2)(Spec(2, 3, 4), Spec(0, 0, 16))
    W = 12 * (16 * 16 + 16 * 16)
    out = (C.c_double * W)()
    n, t, d, mn = C.c_int(0), C.c_double(0.0), C.c_double(0.0), C.c_int(7)
    ms, mt, mv = (C.c_int * 5)(), (C.c_double * 5)(), (C.c_double * (5 * W))()

    def call(ctx, nsteps, every, nmaps, specs, maps=mv):
        mn.value = 7
        return L.lib.rgpu_run_steps_mapped(ctx, nsteps, 1e300, C.byref(n), C.byref(t), C.byref(d), None, every, nmaps, specs, C.byref(mn), ms, mt, maps)
    sv = Solver(p2, L)
    try:
        sv.start(L.init_condition(ini("orszag-tang"), "mesh.nx=16;mesh.ny=16", p2), 0)
        assert L.lib.rgpu_state_maps(sv.ctx, 0, 2, good, out) == -5 and b"3D" in L.lib.rgpu_last_error(sv.ctx)   # RGPU_EUNSUPPORTED
        assert call(sv.ctx, 4, 2, 2, good) == -5 and b"3D" in L.lib.rgpu_last_error(sv.ctx) and mn.value == 0 and n.value == 0
    finally:
        sv.close()
    sv = Solver(p3, L)
    try:
        sv.start(L.init_condition(ini("orszag-tang3d"), "mesh.nx=16;mesh.ny=12;mesh.nz=8", p3), 0)
        assert L.lib.rgpu_state_maps(sv.ctx, 0, 2, good, None) == -1
        assert call(sv.ctx, 4, 0, 2, good) == -1 and b"every" in L.lib.rgpu_last_error(sv.ctx) and mn.value == 0
        assert call(sv.ctx, 4, 2, 2, good, None) == -1 and b"null pointer" in L.lib.rgpu_last_error(sv.ctx) and mn.value == 0
        assert call(sv.ctx, -1, 2, 2, good) == -1 and call(sv.ctx, 4, 2, 0, good) == -1 and call(sv.ctx, 4, 2, _capi.MAP_MAX + 1, good) == -1
        for bad in (Spec(3, 0, 1), Spec(0, 4, 4), Spec(0, 0, 17), Spec(2, 8, 9)):
            specs = (Spec * 2)(good[0], bad)
            assert call(sv.ctx, 4, 2, 2, specs) == -1 and b"map 1:" in L.lib.rgpu_last_error(sv.ctx) and mn.value == 0
            assert L.lib.rgpu_state_maps(sv.ctx, 0, 2, specs, out) == -1 and L.lib.rgpu_map_doubles(sv.ctx, C.byref(bad)) == 0
        assert n.value == 0 and L.lib.rgpu_map_batch_samples(sv.ctx) == 0 and not any(out)   # nothing ran
    finally:
        sv.close()


def test_euler_hip_map_files(gpu_lib, tmp_path):
    """[maps] enabled=yes every=3 map0=z:6 map1=x:all: the .npy files equal run_steps_mapped and are listed; nothing with enabled=no;
    the monitor file byte for byte the one of a run without [maps]"""
    exe = os.path.join(ROOT, "ramsesgpu_amd", "euler_hip")

    def run(overrides):
        r = subprocess.run([exe, "--param", ini("implode3d"), "--set", overrides], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:]
    mm.check_driver_files(gpu_lib, run, tmp_path)
