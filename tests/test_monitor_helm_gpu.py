"""The Helmholtz spectra on the GPU, both libraries (csrc/hip/monitor_helm.h): white noise against the numpy model of
tests/monitor_helm_checks.py within the backward-error gate, every shell of both parts, with the identities of the header, on shapes at
the seams of the kernels -- 4 x 4 x 4, the least box; 8 x 16 x 32, where the columns of a tile are cut into parts (S = 19 with weights
(1, 1, 1)); 64 x 32 x 16 with weights (64, 64, 64), S = 2347, several shells per thread; 4 x 4 x 1024, 4 x 1024 x 4 and 1024 x 4 x 4,
the longest line on each axis; pure fields and plane waves; a repeat call, specs together against specs alone, every value of option
"spectrum_tile_y", bit for bit; M of the two libraries word for word; samples taken inside the device-clock batches against the direct
call on a second context, bit for bit; and driven turbulence."""
import numpy as np
import pytest

import monitor_helm_checks as mh
import monitor_spectrum_checks as ms
from ramsesgpu_amd.solver import Solver

pytestmark = pytest.mark.gpu

SEAMS = ["mesh.nx=4;mesh.ny=4;mesh.nz=4", "mesh.nx=8;mesh.ny=16;mesh.nz=32", "mesh.nx=4;mesh.ny=4;mesh.nz=1024", "mesh.nx=4;mesh.ny=1024;mesh.nz=4", "mesh.nx=1024;mesh.ny=4;mesh.nz=4"]
MANY = "mesh.nx=64;mesh.ny=32;mesh.nz=16"
BATCHED = [("mhd_mri_3d", "mesh.nx=16;mesh.ny=32;mesh.nz=8"), ("orszag-tang3d", "mesh.nx=32;mesh.ny=32;mesh.nz=16")]
LITERAL = ("mhd_mri_3d", "mesh.nx=16;mesh.ny=32;mesh.nz=8;hydro.nu=0.01;MHD.eta=0.01")
ids = lambda cases: [o.replace("mesh.", "").replace(";", "-") for o in cases]


@pytest.fixture(scope="module", params=["exact", "contracted"])
def lib(request, gpu_lib, gpu_contracted_lib):
    yield gpu_lib if request.param == "exact" else gpu_contracted_lib
    mh.close_references()
    print("largest normalised error per library:", mh.LARGEST)


@pytest.mark.parametrize("ov", SEAMS, ids=ids(SEAMS))
def test_white_noise_against_the_model(ov, lib):
    """MHD: all four fields x the three weight sets; Parseval; the sum against rgpu_state_spectra; together against alone; a repeat call"""
    # (4 x 1024 x 4 with weights (3, 5, 7): 1024 tiles and 2561 shells.  The flux array has room for the partials of 308 workgroups of
    # the binning pass, not of 1024, so each walks three or four tiles: helm_bin_groups)
    mh.check_noise(lib, "orszag-tang3d", ov)


def test_more_shells_than_threads(lib):
    """64 x 32 x 16 with weights (64, 64, 64): S = 2347, a thread owns several shells"""
    assert ms.check_shell_rule((64, 32, 16), (64, 64, 64))[0] == 2347
    mh.check_noise(lib, "orszag-tang3d", MANY, weight_sets=[(64, 64, 64), (3, 5, 7)])


def test_hydro_state_has_no_magnetic_power(lib):
    mh.check_noise(lib, "implode3d", SEAMS[1])


@pytest.mark.parametrize("ov", ["mesh.nx=32;mesh.ny=16;mesh.nz=8", "mesh.nx=16;mesh.ny=32;mesh.nz=64", SEAMS[0]], ids=ids(["mesh.nx=32;mesh.ny=16;mesh.nz=8", "mesh.nx=16;mesh.ny=32;mesh.nz=64", SEAMS[0]]))
def test_pure_fields_keep_their_small_part(ov, lib):
    mh.check_pure_fields(lib, "orszag-tang3d", ov)


@pytest.mark.parametrize("ov", [SEAMS[1], MANY], ids=ids([SEAMS[1], MANY]))
def test_plane_waves_split_as_their_direction_says(ov, lib):
    mh.check_plane_waves(lib, "orszag-tang3d", ov)


@pytest.mark.parametrize("ov", [MANY, SEAMS[3]], ids=ids([MANY, SEAMS[3]]))
def test_every_width_of_the_y_tile_gives_the_same_doubles(ov, lib):
    """spectrum_tile_y in {0, 3, 6, -1}: the same doubles as the automatic choice; the option is restored"""
    p, U = ms.random_state(lib, "orszag-tang3d", ov)
    specs = [("w", (1, 1, 1)), ("b", (4, 1, 4)), ("v", (3, 5, 7))]
    sv = Solver(p, lib)
    try:
        sv.upload(U)
        want = sv.state_helm_spectra(specs, 0)
        for logw in (0, 3, 6, -1):
            with ms.option(lib, "spectrum_tile_y", logw):
                for got, w in zip(sv.state_helm_spectra(specs, 0), want):
                    for a, b in zip(got, w):
                        ms.assert_same_bits(a, b, (ov, logw))
        assert lib.lib.rgpu_get_option(b"spectrum_tile_y") == -1
    finally:
        sv.close()


def test_the_two_libraries_count_the_same_modes(gpu_lib, gpu_contracted_lib):
    """M word for word, and the parts of one state within twice the bound of one another (each is within the bound of the model)"""
    got = []
    for lib in (gpu_lib, gpu_contracted_lib):
        p, U = ms.random_state(lib, "orszag-tang3d", MANY)
        sv = Solver(p, lib)
        try:
            sv.upload(U)
            got.append(sv.state_helm_spectra([("w", w) for w in mh.WEIGHTS], 0))
        finally:
            sv.close()
    for (A, B, M), (A2, B2, M2) in zip(*got):
        assert np.array_equal(M, M2) and M.dtype == np.float64
        tot = float(A.sum() + B.sum())
        for P, P2 in ((A, A2), (B, B2)):
            assert np.all(np.abs(P - P2) <= 2.0 * (mh.E * (P + 2.0 * np.sqrt(P * tot)) + mh.E * mh.E * tot))


@pytest.mark.parametrize("base,ov", BATCHED, ids=ids([o for _, o in BATCHED]))
def test_samples_inside_the_device_batches(base, ov, lib):
    """10 steps, every 3rd sampled: steps 3, 6, 9 inside device-clock batches, each bit for bit the direct call on a second context"""
    done, steps, batch, _ = mh.check_run(lib, base, ov, 10, 3, expect_batch=ms.batch_samples(3))
    assert done == 10 and steps == [3, 6, 9] and batch == 3


def test_literal_path_and_a_cut_run(lib):
    done, steps, batch, _ = mh.check_run(lib, LITERAL[0], LITERAL[1], 10, 3)
    assert done == 10 and steps == [3, 6, 9] and batch == 0
    mh.check_cut_run(lib, *BATCHED[0])


def test_driven_turbulence_splits_by_ksi(lib):
    mh.check_driven(lib)


def test_refusals(lib):
    mh.check_refusals(lib, ms.ec.ini, slab=False)
