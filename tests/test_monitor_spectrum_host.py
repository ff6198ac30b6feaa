"""The spectrum monitor (include/rgpu.h, "spectrum monitors": rgpu_state_spectra, rgpu_run_steps_spectra) without a GPU, on the
test-only host emulation, which runs the flat functors K_mon_spectrum_x / _line / _bin: the integer shell rule and the mode counts
against numpy; white noise and single plane waves uploaded into an MHD and a hydro context against numpy.fft.fftn within the
backward-error bound of tests/monitor_spectrum_checks.py, every shell of every case; Parseval; odd and even channel counts; specs
together against specs alone, bit for bit; the sampled run inside the 3D device-clock batches (the emulation runs them, the records
resolved at once) and through the literal loop against the plain run and a second lone context, bit for bit; the refusals; and the
files of the run driver."""
import ctypes as C

import numpy as np
import pytest

import ensemble_checks as ec
import monitor_spectrum_checks as ms
from conftest import ini
from ramsesgpu_amd import _capi
from ramsesgpu_amd.solver import spectrum_shells, spectrum_spec

CRAFTED = [("orszag-tang3d", "mesh.nx=8;mesh.ny=16;mesh.nz=32"), ("orszag-tang3d", "mesh.nx=64;mesh.ny=32;mesh.nz=16"),
           ("implode3d", "mesh.nx=8;mesh.ny=16;mesh.nz=32"), ("implode3d", "mesh.nx=64;mesh.ny=32;mesh.nz=16")]
# the shapes of tests/test_monitor_pdf_host.py brought to powers of two: 40 x 24 x 12 -> 32 x 32 x 16, 24 x 40 x 6 -> 32 x 32 x 8 (the
# MRI box is one already); 24 x 16 x 12 -> 16 x 16 x 16
BATCHED = [("implode3d", "mesh.nx=32;mesh.ny=32;mesh.nz=16"), ("orszag-tang3d", "mesh.nx=32;mesh.ny=32;mesh.nz=8"), ("mhd_mri_3d", "mesh.nx=16;mesh.ny=32;mesh.nz=8")]
LITERAL = [("rayleigh_taylor_gpu_3d", "mesh.nx=16;mesh.ny=16;mesh.nz=16"), ("mhd_mri_3d", "mesh.nx=16;mesh.ny=32;mesh.nz=8;hydro.nu=0.01;MHD.eta=0.01")]
ids = lambda cases: ["%s-%s" % (b, o.replace("mesh.", "").replace(";", "-")) for b, o in cases]


@pytest.fixture(scope="module", autouse=True)
def references():
    yield
    ms.close_references()
    print("largest normalised error per library:", ms.LARGEST)


def test_names_and_constants(emu_lib):
    assert _capi.SPECTRUM_NQ == 13 and " ".join(_capi.SPECTRUM_NAMES) == "rho mx my mz vx vy vz wx wy wz bx by bz"
    assert (_capi.SPECTRUM_MAX, _capi.SPECTRUM_MAX_SHELLS, _capi.SPECTRUM_MAX_WEIGHT) == (4, 4096, 64)
    assert C.sizeof(_capi.RgpuSpectrumSpec) == 16
    assert emu_lib.lib.rgpu_get_option(b"spectrum_tile_y") == -1
    s = spectrum_spec(("w", (4, 1, 4)))
    assert (s.channels, s.wx, s.wy, s.wz) == (0b1110000000, 4, 1, 4)
    assert spectrum_spec((("rho", "b", "vx"), (1, 0, 0))).channels == 0b1110000010001 and spectrum_spec(("m", (1, 1, 1))).channels == 0b1110
    assert [_capi.MONP_NAMES[c] for c in (0, 1, 2, 3, 10, 11, 12)] == ["mass", "mx", "my", "mz", "bx", "by", "bz"]


def test_shell_rule_and_mode_counts():
    """the integer rule against floor(sqrt(q) + 0.5) and M against numpy.bincount, on every shape and weight the suite uses"""
    ms.check_shell_edges()
    for shape in ((8, 16, 32), (64, 32, 16), (4, 4, 4), (128, 8, 4), (4, 128, 8), (8, 4, 128), (1024, 4, 4), (4, 1024, 4), (4, 4, 1024), (32, 32, 16), (16, 32, 8)):
        for weights in ms.WEIGHTS + [(1, 0, 0), (64, 64, 64) if max(shape) <= 64 else (1, 2, 3)]:
            S, M = ms.check_shell_rule(shape, weights)
            assert S <= _capi.SPECTRUM_MAX_SHELLS
    S, M = spectrum_shells((8, 16, 32), (0, 1, 0))
    assert S == 9 and list(M) == [256, 512, 512, 512, 512, 512, 512, 512, 256]


@pytest.mark.parametrize("base,ov", CRAFTED, ids=ids(CRAFTED))
def test_white_noise_against_the_model(base, ov, emu_lib):
    ms.check_noise(emu_lib, base, ov)


@pytest.mark.parametrize("base,ov", CRAFTED, ids=ids(CRAFTED))
def test_plane_waves_land_in_their_shells(base, ov, emu_lib):
    ms.check_plane_waves(emu_lib, base, ov)


def test_mode_counts_are_the_rule(emu_lib):
    """M of the library == numpy.bincount of the integer rule, word for word, for weights the other tests do not use"""
    base, ov = CRAFTED[0]
    p, U = ms.random_state(emu_lib, base, ov)
    from ramsesgpu_amd.solver import Solver
    sv = Solver(p, emu_lib)
    try:
        sv.upload(U)
        for weights in ((1, 0, 0), (0, 0, 1), (3, 5, 7), (64, 64, 64), (1, 2, 0)):
            S, M = ms.check_shell_rule(ms.shape_of(p), weights)
            P, got = sv.state_spectra([(("rho",), weights)], 0)[0]
            assert got.dtype == np.float64 and np.array_equal(got, M.astype(np.float64)), weights
    finally:
        sv.close()


@pytest.mark.parametrize("every", [1, 3])
@pytest.mark.parametrize("base,ov", BATCHED, ids=ids(BATCHED))
def test_samples_inside_the_batches(base, ov, every, emu_lib):
    done, steps, batch = ms.check_run(emu_lib, base, ov, 10, every, expect_batch=ms.batch_samples(every))
    assert done == 10 and steps == [s for s in range(1, 11) if s % every == 0]
    assert batch == len(steps) - (1 if every == 1 else 0)


@pytest.mark.parametrize("every", [1, 3])
@pytest.mark.parametrize("base,ov", LITERAL, ids=["gravity", "dissipative"])
def test_literal_path(base, ov, every, emu_lib):
    """gravity and the dissipative stage take their time step from the host: the literal loop, the same series, no sample on the device"""
    def never(done, ready):
        assert ready == 0, "the context takes its time step from the device"
        return 0
    done, steps, batch = ms.check_run(emu_lib, base, ov, 10, every, expect_batch=never)
    assert done == 10 and steps == [s for s in range(1, 11) if s % every == 0] and batch == 0


def test_end_time_inside_a_step(emu_lib):
    """t passes the end inside the 6th step, a multiple of 3: that last step is sampled; inside the 5th: it is not, and no sample follows"""
    base, ov = BATCHED[2]
    p = emu_lib.params_from_ini(ini(base), ov)
    dts = ec.lone_run(emu_lib, p, ms.initial_state(emu_lib, base, ov, p), 10)["dt_log"]
    for k, want in ((6, [3, 6]), (5, [3])):
        done, steps, batch = ms.check_run(emu_lib, base, ov, 10, 3, tEnd=ec.end_inside_step(dts, k))
        assert done == k and steps == want and batch > 0


def test_refusals(emu_lib):
    ms.check_refusals(emu_lib, ini)


def test_run_driver_spectrum_files(emu_lib, tmp_path):
    """rgpuh_run with [spectra]: the .npy files, their list, nothing with enabled=no, the monitor file untouched by the spectra, the same
    doubles where the PDFs take the batches; a 2D run and a box of 24 cells write no spectrum file and run on; a bad spec is named"""
    def run(overrides):
        err, mc = C.create_string_buffer(512), C.c_double(0)
        assert emu_lib.lib.rgpuh_run(ini("implode3d").encode(), overrides.encode(), C.byref(mc), err, 512) == 10, err.value
    ms.check_driver_files(emu_lib, run, tmp_path)
    d = tmp_path / "flat"
    d.mkdir()
    err, mc = C.create_string_buffer(512), C.c_double(0)
    tail = "run.nstepmax=6;run.noutput=1000;output.outputVtk=no;output.outputHdf5=no;output.outputDir=%s;spectra.enabled=yes;spectra.every=3;spectra.spectrum0=rho 1 1 1" % d
    assert emu_lib.lib.rgpuh_run(ini("orszag-tang").encode(), ("mesh.nx=16;mesh.ny=16;" + tail).encode(), C.byref(mc), err, 512) == 6, err.value
    assert emu_lib.lib.rgpuh_run(ini("implode3d").encode(), ("mesh.nx=24;mesh.ny=16;mesh.nz=8;" + tail).encode(), C.byref(mc), err, 512) == 6, err.value
    assert not list(d.glob("*_spectr*"))
    for text in ("rho 1 1", "nosuch 1 1 1", "rho 0 0 0", "rho 1 1 65", "rho 1 1 1 1", "rho, 1 1 1"):
        bad = "mesh.nx=16;mesh.ny=16;mesh.nz=8;run.nstepmax=2;output.outputVtk=no;output.outputHdf5=no;output.outputDir=%s;spectra.enabled=yes;spectra.spectrum0=%s" % (d, text)
        assert emu_lib.lib.rgpuh_run(ini("implode3d").encode(), bad.encode(), C.byref(mc), err, 512) < 0 and b"spectrum0" in err.value, text
