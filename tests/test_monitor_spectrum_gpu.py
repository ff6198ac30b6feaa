"""The spectrum monitor on the GPU, both libraries (csrc/hip/monitor_spectrum.h): white noise against numpy.fft.fftn within the
backward-error bound of tests/monitor_spectrum_checks.py, every shell, on shapes at the seams of the kernels -- 4 x 4 x 4, the least box;
8 x 16 x 32 and 64 x 32 x 16, several lines per wave and tiles narrower than the widest; 128 x 8 x 4, 4 x 128 x 8 and 8 x 4 x 128, more
than one butterfly per thread and turn on each axis in turn; 1024 x 4 x 4, 4 x 1024 x 4 and 4 x 4 x 1024, the longest line on each
axis; a repeat call, specs together against specs alone, every value of option "spectrum_tile_y", bit for bit; M of the two libraries
word for word; and samples taken inside the device-clock batches against the direct call on a second context, bit for bit."""
import numpy as np
import pytest

import monitor_spectrum_checks as ms
from ramsesgpu_amd.solver import Solver

pytestmark = pytest.mark.gpu

SEAMS = ["mesh.nx=4;mesh.ny=4;mesh.nz=4", "mesh.nx=8;mesh.ny=16;mesh.nz=32", "mesh.nx=64;mesh.ny=32;mesh.nz=16",
         "mesh.nx=128;mesh.ny=8;mesh.nz=4", "mesh.nx=4;mesh.ny=128;mesh.nz=8", "mesh.nx=8;mesh.ny=4;mesh.nz=128",
         "mesh.nx=1024;mesh.ny=4;mesh.nz=4", "mesh.nx=4;mesh.ny=1024;mesh.nz=4", "mesh.nx=4;mesh.ny=4;mesh.nz=1024"]
BATCHED = [("mhd_mri_3d", "mesh.nx=16;mesh.ny=32;mesh.nz=8"), ("orszag-tang3d", "mesh.nx=32;mesh.ny=32;mesh.nz=16")]
ids = lambda cases: [o.replace("mesh.", "").replace(";", "-") for o in cases]


@pytest.fixture(scope="module", params=["exact", "contracted"])
def lib(request, gpu_lib, gpu_contracted_lib):
    yield gpu_lib if request.param == "exact" else gpu_contracted_lib
    ms.close_references()
    print("largest normalised error per library:", ms.LARGEST)


@pytest.mark.parametrize("ov", SEAMS, ids=ids(SEAMS))
def test_white_noise_against_the_model(ov, lib):
    """MHD: every channel is noise; every channel set x every weight; Parseval; together against alone; a repeat call"""
    ms.check_noise(lib, "orszag-tang3d", ov)


def test_hydro_state_has_no_magnetic_power(lib):
    ms.check_noise(lib, "implode3d", SEAMS[1])


@pytest.mark.parametrize("ov", [SEAMS[1], SEAMS[2]], ids=ids([SEAMS[1], SEAMS[2]]))
def test_plane_waves_land_in_their_shells(ov, lib):
    ms.check_plane_waves(lib, "orszag-tang3d", ov)


@pytest.mark.parametrize("ov", [SEAMS[2], SEAMS[4], SEAMS[7]], ids=ids([SEAMS[2], SEAMS[4], SEAMS[7]]))
def test_every_width_of_the_y_tile_gives_the_same_doubles(ov, lib):
    """spectrum_tile_y in {0 .. 6, -1}: one, two, ... 64 adjacent x per tile of the y pass, clamped to what the box and the tile hold:
    the same doubles as the automatic choice; the option is restored"""
    p, U = ms.random_state(lib, "orszag-tang3d", ov)
    specs = [("w", (1, 1, 1)), ("b", (4, 1, 4)), (("rho",), (0, 1, 0))]
    sv = Solver(p, lib)
    try:
        sv.upload(U)
        want = sv.state_spectra(specs, 0)
        for logw in (0, 1, 2, 3, 4, 5, 6, -1):
            with ms.option(lib, "spectrum_tile_y", logw):
                for (P, M), (wP, wM) in zip(sv.state_spectra(specs, 0), want):
                    ms.assert_same_bits(P, wP, (ov, logw))
                    ms.assert_same_bits(M, wM, (ov, logw, "modes"))
        assert lib.lib.rgpu_get_option(b"spectrum_tile_y") == -1
    finally:
        sv.close()


def test_the_two_libraries_count_the_same_modes(gpu_lib, gpu_contracted_lib):
    """M word for word, and P of one state within twice the bound of one another (each is within the bound of the model)"""
    got = []
    for lib in (gpu_lib, gpu_contracted_lib):
        p, U = ms.random_state(lib, "orszag-tang3d", SEAMS[2])
        sv = Solver(p, lib)
        try:
            sv.upload(U)
            got.append(sv.state_spectra([(ms.NAMES, w) for w in ms.WEIGHTS], 0))
        finally:
            sv.close()
    for (P, M), (P2, M2) in zip(*got):
        assert np.array_equal(M, M2) and M.dtype == np.float64
        tot = float(P.sum())
        assert np.all(np.abs(P - P2) <= 2.0 * (ms.E * (P + 2.0 * np.sqrt(P * tot)) + ms.E * ms.E * tot))


@pytest.mark.parametrize("base,ov", BATCHED, ids=ids([o for _, o in BATCHED]))
def test_samples_inside_the_device_batches(base, ov, lib):
    """10 steps, every 3rd sampled: steps 3, 6, 9 inside device-clock batches, each bit for bit the direct call on a second context"""
    done, steps, batch = ms.check_run(lib, base, ov, 10, 3, expect_batch=ms.batch_samples(3))
    assert done == 10 and steps == [3, 6, 9] and batch == 3


def test_refusals(lib):
    ms.check_refusals(lib, ms.ec.ini, slab=False)
