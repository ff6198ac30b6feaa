"""The PDF monitor (include/rgpu.h, "PDF monitors": rgpu_state_pdfs, rgpu_run_steps_pdfs) without a GPU, on the test-only host
emulation, which runs the flat functors K_mon_pdf_zero / K_mon_pdf: every word of 1D and joint tables, linear and octave, against the
numpy model of the documented definition at the seam shapes of the map monitor; the sum and the marginal identity; a state whose
density is crafted cell by cell around every edge; the cross-checks against rgpu_state_monitor3d; the sampled run inside the 3D
device-clock batches (the emulation runs them, the records resolved at once) and through the literal loop against the plain run, a
second lone context and the model; the refusals; and the files of the run driver.  Helpers: tests/monitor_pdf_checks.py."""
import ctypes as C

import pytest

import ensemble_checks as ec
import monitor_pdf_checks as mh
from conftest import ini
from ramsesgpu_amd import _capi
from ramsesgpu_amd.solver import pdf_axis, pdf_edges

# the shapes of tests/test_monitor_maps_host.py: nx a ragged 64-lane row (63), exactly one (64), one cell into a second (65) and into a
# third (130); row counts ny nz that no number of workgroups divides evenly
SEAMS = [("implode3d", "mesh.nx=65;mesh.ny=33;mesh.nz=3"), ("implode3d", "mesh.nx=63;mesh.ny=31;mesh.nz=5"),
         ("orszag-tang3d", "mesh.nx=64;mesh.ny=32;mesh.nz=3"), ("orszag-tang3d", "mesh.nx=130;mesh.ny=65;mesh.nz=3"),
         ("mhd_mri_3d", "mesh.nx=65;mesh.ny=33;mesh.nz=4")]
BATCHED = [("implode3d", "mesh.nx=40;mesh.ny=24;mesh.nz=12"), ("orszag-tang3d", "mesh.nx=24;mesh.ny=40;mesh.nz=6"), ("mhd_mri_3d", "mesh.nx=16;mesh.ny=32;mesh.nz=8")]
LITERAL = [("rayleigh_taylor_gpu_3d", "mesh.nx=24;mesh.ny=16;mesh.nz=12"), ("mhd_mri_3d", "mesh.nx=16;mesh.ny=32;mesh.nz=8;hydro.nu=0.01;MHD.eta=0.01")]
ids = lambda cases: ["%s-%s" % (b, o.replace("mesh.", "").replace(";", "-")) for b, o in cases]


@pytest.fixture(scope="module", autouse=True)
def references():
    yield
    mh.close_references()


def test_names_and_constants(emu_lib):
    assert _capi.PDF_NQ == 13 and " ".join(_capi.PDF_NAMES) == "rho mx my mz E ekin emag eint bx by bz absdivb v2"
    assert [_capi.MONP_NAMES[c] for c in mh.COLUMNS] == ["mass", "mx", "my", "mz", "E", "ekin", "emag", "min_eint", "bx", "by", "bz", "max_absdivb"]
    assert _capi.PDF_MAX == 8 and _capi.PDF_MAX_WORDS == 16384
    assert C.sizeof(_capi.RgpuPdfAxis) == 32 and C.sizeof(_capi.RgpuPdfSpec) == 64
    for name in ("pdf_replicas", "pdf_groups"):
        assert emu_lib.lib.rgpu_get_option(name.encode()) == -1
    a = pdf_axis(("rho", "log2", -3, 3, 2))
    assert (a.channel, a.scale, a.nbins, a.sub, a.lo, a.hi) == (0, 1, 24, 2, 0.125, 8.0)
    assert list(pdf_edges(("rho", "log2", 0, 2, 1))) == [1.0, 1.5, 2.0, 3.0, 4.0] and list(pdf_edges(("mx", "lin", -1.0, 1.0, 4))) == [-1.0, -0.5, 0.0, 0.5, 1.0]


def test_octave_rule_is_a_search_in_the_edges():
    mh.check_octave_model_against_searchsorted()


@pytest.mark.parametrize("base,ov", SEAMS, ids=ids(SEAMS))
def test_tables_equal_the_model(base, ov, emu_lib):
    mh.check_seams(emu_lib, base, ov)


def test_crafted_densities_land_where_the_model_puts_them(emu_lib):
    mh.check_crafted_state(emu_lib)


@pytest.mark.parametrize("base,ov", [SEAMS[1], SEAMS[2]], ids=ids([SEAMS[1], SEAMS[2]]))
def test_against_the_monitor(base, ov, emu_lib):
    mh.check_against_the_monitor(emu_lib, base, ov)


@pytest.mark.parametrize("every", [1, 3])
@pytest.mark.parametrize("base,ov", BATCHED, ids=ids(BATCHED))
def test_samples_inside_the_batches(base, ov, every, emu_lib):
    done, steps, tables, batch = mh.check_run(emu_lib, base, ov, 10, every, expect_batch=mh.batch_samples(every))
    assert done == 10 and steps == [s for s in range(1, 11) if s % every == 0]
    assert batch == len(steps) - (1 if every == 1 else 0)


@pytest.mark.parametrize("base,ov", BATCHED, ids=ids(BATCHED))
def test_run_in_pieces(base, ov, emu_lib):
    """[4, 6]: step 1 is plain, the second call begins on the device path -- samples 3, 6, 9 all inside batches"""
    done, steps, tables, batch = mh.check_run(emu_lib, base, ov, 10, 3, pieces=[4, 6], expect_batch=lambda done, ready: 3 if ready == 1 else -1)
    assert done == 10 and steps == [3, 6, 9] and batch == 3


@pytest.mark.parametrize("base,ov", BATCHED, ids=ids(BATCHED))
def test_end_time_inside_a_step(base, ov, emu_lib):
    """t passes the end inside the 6th step, a multiple of 3: that last step is sampled; inside the 5th: it is not, and no sample follows"""
    p = emu_lib.params_from_ini(ini(base), ov)
    dts = ec.lone_run(emu_lib, p, mh.initial_state(emu_lib, base, ov, p), 10)["dt_log"]
    for k, want in ((6, [3, 6]), (5, [3])):
        done, steps, tables, batch = mh.check_run(emu_lib, base, ov, 10, 3, tEnd=ec.end_inside_step(dts, k))
        assert done == k and steps == want and batch > 0


def test_across_a_batch_boundary(emu_lib):
    """300 steps, every 7th sampled: 7 does not divide the 256 steps of a batch, so the samples of the second batch sit in other slots
    of the log than those of the first, and slots are used again"""
    base, ov = BATCHED[0]
    done, steps, tables, batch = mh.check_run(emu_lib, base, ov, 300, 7, expect_batch=mh.batch_samples(7))
    assert done == 300 and len(steps) == 42 and steps[-1] == 294 and batch == 42


@pytest.mark.parametrize("base,ov", LITERAL, ids=["gravity", "dissipative"])
def test_literal_path(base, ov, emu_lib):
    """gravity and the dissipative stage take their time step from the host: the literal loop, the same series, no sample on the device"""
    def never(done, ready):
        assert ready == 0, "the context takes its time step from the device"
        return 0
    done, steps, tables, batch = mh.check_run(emu_lib, base, ov, 10, 3, pieces=[4, 6], expect_batch=never)
    assert done == 10 and steps == [3, 6, 9] and batch == 0


def test_refusals(emu_lib):
    mh.check_refusals(emu_lib, ini)


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
        spec = _capi.RgpuPdfSpec(_capi.RgpuPdfAxis(0, 0, 5, 0, 0.0, 2.0), _capi.RgpuPdfAxis())
        assert L.lib.rgpu_pdf_words(C.byref(spec)) == 8
        if rc == -2:
            out = (C.c_ulonglong * 8)()
            n, t, d, mn = C.c_int(0), C.c_double(0.0), C.c_double(0.0), C.c_int(7)
            ms, mt, mv = (C.c_int * 3)(), (C.c_double * 3)(), (C.c_ulonglong * 24)()
            assert L.lib.rgpu_state_pdfs(ctx, 0, 1, C.byref(spec), out) == -1
            assert L.lib.rgpu_run_steps_pdfs(ctx, 4, 1e300, C.byref(n), C.byref(t), C.byref(d), None, 2, 1, C.byref(spec), C.byref(mn), ms, mt, mv) == -1
            assert n.value == 0 and mn.value == 0 and not any(out) and not any(mv)
    finally:
        L.lib.rgpu_destroy(ctx)


def test_run_driver_pdf_files(emu_lib, tmp_path):
    """rgpuh_run with [pdfs]: the .npy files, their list, nothing with enabled=no, the monitor file untouched by the PDFs, the same
    words where the maps take the batches; a 2D run writes no PDF file; a bad spec is named"""
    def run(overrides):
        err, mc = C.create_string_buffer(512), C.c_double(0)
        assert emu_lib.lib.rgpuh_run(ini("implode3d").encode(), overrides.encode(), C.byref(mc), err, 512) == 10, err.value
    mh.check_driver_files(emu_lib, run, tmp_path)
    d = tmp_path / "flat"
    d.mkdir()
    err, mc = C.create_string_buffer(512), C.c_double(0)
    ov2 = "mesh.nx=16;mesh.ny=16;run.nstepmax=6;run.noutput=1000;output.outputVtk=no;output.outputHdf5=no;output.outputDir=%s;pdfs.enabled=yes;pdfs.every=3;pdfs.pdf0=rho:lin:0:2:8" % d
    assert emu_lib.lib.rgpuh_run(ini("orszag-tang").encode(), ov2.encode(), C.byref(mc), err, 512) == 6, err.value
    assert not list(d.glob("*_pdf*"))
    for text in ("rho:log2:0:4", "rho:lin:2:1:8", "nosuch:lin:0:1:8", "rho:log2:-4:4:7", "rho:lin:0:1:8,"):
        bad = "mesh.nx=12;mesh.ny=12;mesh.nz=8;run.nstepmax=2;output.outputVtk=no;output.outputHdf5=no;output.outputDir=%s;pdfs.enabled=yes;pdfs.pdf0=%s" % (d, text)
        assert emu_lib.lib.rgpuh_run(ini("implode3d").encode(), bad.encode(), C.byref(mc), err, 512) < 0 and b"pdf0" in err.value, text
