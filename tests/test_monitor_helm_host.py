"""The Helmholtz spectra (include/rgpu.h, "Helmholtz spectra": rgpu_state_helm_spectra, rgpu_run_steps_helm_spectra) without a GPU, on the
test-only host emulation, which runs the flat functors K_mon_spectrum_x / _line once per component and K_mon_helm_bin: white noise in
an MHD and a hydro context against the numpy model of tests/monitor_helm_checks.py within the backward-error gate, every shell of both
parts; the three identities of the header; purely solenoidal and purely compressive fields, whose wrong part stays below e^2 Ptot;
plane waves whose split is known in closed form; the sampled run inside the 3D device-clock batches and through the literal loop
against the plain run and a second lone context, bit for bit; a run cut in two; driven turbulence with ksi = 1 and ksi = 0; the
refusals; and the files of the run driver."""
import ctypes as C

import numpy as np
import pytest

import monitor_helm_checks as mh
from conftest import ini
from ramsesgpu_amd import _capi
from ramsesgpu_amd.solver import helm_spec

CRAFTED = [("orszag-tang3d", "mesh.nx=8;mesh.ny=16;mesh.nz=32"), ("orszag-tang3d", "mesh.nx=64;mesh.ny=32;mesh.nz=16"), ("implode3d", "mesh.nx=8;mesh.ny=16;mesh.nz=32")]
PURE = ["mesh.nx=32;mesh.ny=16;mesh.nz=8", "mesh.nx=16;mesh.ny=32;mesh.nz=64", "mesh.nx=4;mesh.ny=4;mesh.nz=4"]
BATCHED = [("mhd_mri_3d", "mesh.nx=16;mesh.ny=32;mesh.nz=8"), ("orszag-tang3d", "mesh.nx=32;mesh.ny=32;mesh.nz=16")]
LITERAL = ("mhd_mri_3d", "mesh.nx=16;mesh.ny=32;mesh.nz=8;hydro.nu=0.01;MHD.eta=0.01")
ids = lambda cases: ["%s-%s" % (b, o.replace("mesh.", "").replace(";", "-")) for b, o in cases]


@pytest.fixture(scope="module", autouse=True)
def references():
    yield
    mh.close_references()
    print("largest normalised error per library:", mh.LARGEST)


def test_names_and_constants(emu_lib):
    assert _capi.HELM_NF == 4 and " ".join(_capi.HELM_NAMES) == "m v w b" and _capi.HELM_MAX == 4
    assert C.sizeof(_capi.RgpuHelmSpec) == 16
    s = helm_spec(("w", (4, 1, 4)))
    assert (s.field, s.wx, s.wy, s.wz) == (2, 4, 1, 4) and helm_spec((3, (1, 2, 3))).field == 3
    # the triples are those of the spectrum monitor's channels
    for f, name in enumerate(_capi.HELM_NAMES):
        assert [_capi.SPECTRUM_NAMES[1 + 3 * f + a] for a in range(3)] == [name + x for x in "xyz"]


@pytest.mark.parametrize("base,ov", CRAFTED, ids=ids(CRAFTED))
def test_white_noise_against_the_model(base, ov, emu_lib):
    mh.check_noise(emu_lib, base, ov)


@pytest.mark.parametrize("ov", PURE, ids=[o.replace("mesh.", "").replace(";", "-") for o in PURE])
def test_pure_fields_keep_their_small_part(ov, emu_lib):
    mh.check_pure_fields(emu_lib, "orszag-tang3d", ov)


@pytest.mark.parametrize("base,ov", CRAFTED[:2], ids=ids(CRAFTED[:2]))
def test_plane_waves_split_as_their_direction_says(base, ov, emu_lib):
    mh.check_plane_waves(emu_lib, base, ov)


@pytest.mark.parametrize("base,ov", BATCHED, ids=ids(BATCHED))
def test_samples_inside_the_batches(base, ov, emu_lib):
    done, steps, batch, _ = mh.check_run(emu_lib, base, ov, 10, 3, expect_batch=mh.ms.batch_samples(3))
    assert done == 10 and steps == [3, 6, 9] and batch == 3


def test_literal_path(emu_lib):
    """the dissipative stage takes its time step from the host: the literal loop, the same series, no sample on the device"""
    def never(done, ready):
        assert ready == 0, "the context takes its time step from the device"
        return 0
    done, steps, batch, _ = mh.check_run(emu_lib, LITERAL[0], LITERAL[1], 10, 3, expect_batch=never)
    assert done == 10 and steps == [3, 6, 9] and batch == 0


def test_a_run_cut_in_two_gives_one_series(emu_lib):
    mh.check_cut_run(emu_lib, *BATCHED[0])


def test_driven_turbulence_splits_by_ksi(emu_lib):
    mh.check_driven(emu_lib)


def test_refusals(emu_lib):
    mh.check_refusals(emu_lib, ini)


def test_run_driver_helmholtz_files(emu_lib, tmp_path):
    """rgpuh_run with [helmholtz]: the .npy files, their list, nothing with enabled=no, the same doubles where the spectra take the
    batches; a 2D run writes no file and runs on; a bad spec is named"""
    def run(overrides):
        err, mc = C.create_string_buffer(512), C.c_double(0)
        assert emu_lib.lib.rgpuh_run(ini("implode3d").encode(), overrides.encode(), C.byref(mc), err, 512) == 10, err.value
    mh.check_driver_files(emu_lib, run, tmp_path)
    d = tmp_path / "flat"
    d.mkdir()
    err, mc = C.create_string_buffer(512), C.c_double(0)
    tail = "run.nstepmax=6;run.noutput=1000;output.outputVtk=no;output.outputHdf5=no;output.outputDir=%s;helmholtz.enabled=yes;helmholtz.every=3;helmholtz.spectrum0=m 1 1 1" % d
    assert emu_lib.lib.rgpuh_run(ini("orszag-tang").encode(), ("mesh.nx=16;mesh.ny=16;" + tail).encode(), C.byref(mc), err, 512) == 6, err.value
    assert emu_lib.lib.rgpuh_run(ini("implode3d").encode(), ("mesh.nx=24;mesh.ny=16;mesh.nz=8;" + tail).encode(), C.byref(mc), err, 512) == 6, err.value
    assert not list(d.glob("*_helmholtz*"))
    for text in ("w 1 1", "rho 1 1 1", "w 0 1 1", "w 1 1 65", "w 1 1 1 1", "wx 1 1 1"):
        bad = "mesh.nx=16;mesh.ny=16;mesh.nz=8;run.nstepmax=2;output.outputVtk=no;output.outputHdf5=no;output.outputDir=%s;helmholtz.enabled=yes;helmholtz.spectrum0=%s" % (d, text)
        assert emu_lib.lib.rgpuh_run(ini("implode3d").encode(), bad.encode(), C.byref(mc), err, 512) < 0 and b"spectrum0" in err.value, text
