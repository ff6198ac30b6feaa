"""The PDF monitor on the GPU, both libraries (csrc/hip/monitor_pdf.h): every word of 1D and joint tables against the numpy model at
shapes on the seams of the kernels; every forced variant of the count kernel (options "pdf_replicas", "pdf_groups"), which must give
the same words; a constant state, where every lane of every wave counts into one word; the two libraries on one state; the crafted
densities; the cross-checks against rgpu_state_monitor3d; rgpu_run_steps_pdfs with the samples taken behind the steps of the
device-clock batches -- 3D hydro, 3D MHD, the shearing box -- against the plain run and a second lone context; a run in pieces, an end
time inside a batch, a run across the 256-step boundary; the literal loop (gravity, the dissipative stage); the refusals; and the PDF
files of euler_hip.  Helpers: tests/monitor_pdf_checks.py."""
import os
import subprocess

import pytest

import ensemble_checks as ec
import monitor_pdf_checks as mh
from conftest import ROOT, ini
from ramsesgpu_amd import _capi
from ramsesgpu_amd.solver import Solver

pytestmark = pytest.mark.gpu

# nx: a ragged 64-lane row (63), exactly one (64), one cell into a second (65) and into a third (130); row counts ny nz that no number
# of workgroups divides evenly
SEAMS = [("implode3d", "mesh.nx=65;mesh.ny=33;mesh.nz=3"), ("implode3d", "mesh.nx=63;mesh.ny=31;mesh.nz=5"),
         ("orszag-tang3d", "mesh.nx=64;mesh.ny=32;mesh.nz=3"), ("orszag-tang3d", "mesh.nx=130;mesh.ny=65;mesh.nz=3"),
         ("mhd_mri_3d", "mesh.nx=65;mesh.ny=33;mesh.nz=4")]
BATCHED = [("implode3d", "mesh.nx=40;mesh.ny=24;mesh.nz=12"), ("orszag-tang3d", "mesh.nx=24;mesh.ny=40;mesh.nz=6"), ("mhd_mri_3d", "mesh.nx=16;mesh.ny=32;mesh.nz=8")]
LITERAL = [("rayleigh_taylor_gpu_3d", "mesh.nx=24;mesh.ny=16;mesh.nz=12"), ("mhd_mri_3d", "mesh.nx=16;mesh.ny=32;mesh.nz=8;hydro.nu=0.01;MHD.eta=0.01")]
ids = lambda cases: ["%s-%s" % (b, o.replace("mesh.", "").replace(";", "-")) for b, o in cases]


@pytest.fixture(scope="module", params=["exact", "contracted"])
def lib(request, gpu_lib, gpu_contracted_lib):
    yield gpu_lib if request.param == "exact" else gpu_contracted_lib
    mh.close_references()


@pytest.mark.parametrize("base,ov", SEAMS, ids=ids(SEAMS))
def test_tables_equal_the_model(base, ov, lib):
    mh.check_seams(lib, base, ov)


@pytest.mark.parametrize("base,ov", [SEAMS[3], SEAMS[4]], ids=ids([SEAMS[3], SEAMS[4]]))
def test_every_forced_variant_gives_the_same_words(base, ov, lib):
    """pdf_replicas in {1, 2, 8, -1} x pdf_groups in {1, 2, 7, -1}: the tables of every spec set equal the model (hence one another);
    the options are restored"""
    p = lib.params_from_ini(ini(base), ov)
    sv = Solver(p, lib)
    try:
        sv.start(mh.initial_state(lib, base, ov, p), 0)
        assert sv.run_steps(3) == 3
        U = sv.getDataHost()
        Ch = mh.cell_channels(U, p)
        want = {name: [mh.model(Ch, s) for s in specs] for name, specs in mh.SPEC_SETS.items()}
        for replicas in (1, 2, 8, -1):
            for groups in (1, 2, 7, -1):
                with mh.option(lib, "pdf_replicas", replicas), mh.option(lib, "pdf_groups", groups):
                    for name, specs in mh.SPEC_SETS.items():
                        for spec, g, w in zip(specs, sv.state_pdfs(specs), want[name]):
                            mh.assert_same_words(g, w, (replicas, groups, name, spec))
        assert lib.lib.rgpu_get_option(b"pdf_replicas") == -1 and lib.lib.rgpu_get_option(b"pdf_groups") == -1
    finally:
        sv.close()


@pytest.mark.parametrize("replicas", [1, -1])
def test_constant_state_counts_every_cell_into_one_word(replicas, lib):
    """130 x 65 x 3, every density 1.0, seven workgroups: every lane of every wave adds to the same word of the LDS table, and seven
    slabs feed that word through the fold.  The count is nx ny nz"""
    base, ov = SEAMS[3]
    p = lib.params_from_ini(ini(base), ov)
    U = mh.initial_state(lib, base, ov, p).copy()
    U[_capi.ID] = 1.0
    n = p.nx * p.ny * p.nz
    sv = Solver(p, lib)
    try:
        sv.upload(U)
        with mh.option(lib, "pdf_groups", 7), mh.option(lib, "pdf_replicas", replicas):
            lin, octave, joint = sv.state_pdfs([("rho", "lin", 0.0, 2.0, 4), ("rho", "log2", -2, 2, 3), (("rho", "lin", 0.0, 2.0, 4), ("rho", "log2", -2, 2, 3))], 0)
    finally:
        sv.close()
    assert int(lin[2]) == n and int(lin.sum()) == n
    assert int(octave[16]) == n and int(octave.sum()) == n
    assert int(joint[2, 16]) == n and int(joint.sum()) == n


def test_the_two_libraries_count_alike(gpu_lib, gpu_contracted_lib):
    """the same state uploaded to the exact and to the contracted library: the same words (the per-cell terms are not contracted)"""
    base, ov = SEAMS[4]
    p = gpu_lib.params_from_ini(ini(base), ov)
    sv = Solver(p, gpu_lib)
    try:
        sv.start(mh.initial_state(gpu_lib, base, ov, p), 0)
        assert sv.run_steps(3) == 3
        U = sv.getDataHost()
        a = {name: sv.state_pdfs(specs) for name, specs in mh.SPEC_SETS.items()}
    finally:
        sv.close()
    sv = Solver(gpu_contracted_lib.params_from_ini(ini(base), ov), gpu_contracted_lib)
    try:
        sv.upload(U)
        for name, specs in mh.SPEC_SETS.items():
            for spec, x, y in zip(specs, a[name], sv.state_pdfs(specs, 0)):
                mh.assert_same_words(y, x, (name, spec))
    finally:
        sv.close()


def test_crafted_densities_land_where_the_model_puts_them(lib):
    mh.check_crafted_state(lib)


@pytest.mark.parametrize("base,ov", [SEAMS[1], SEAMS[2]], ids=ids([SEAMS[1], SEAMS[2]]))
def test_against_the_monitor(base, ov, lib):
    mh.check_against_the_monitor(lib, base, ov)


@pytest.mark.parametrize("every", [1, 3])
@pytest.mark.parametrize("base,ov", BATCHED, ids=ids(BATCHED))
def test_samples_inside_the_device_batches(base, ov, every, lib):
    done, steps, tables, batch = mh.check_run(lib, base, ov, 10, every, expect_batch=mh.batch_samples(every))
    assert done == 10 and steps == [s for s in range(1, 11) if s % every == 0]
    assert batch == len(steps) - (1 if every == 1 else 0)


@pytest.mark.parametrize("base,ov", BATCHED, ids=ids(BATCHED))
def test_run_in_pieces(base, ov, lib):
    """[4, 6]: step 1 is plain, the second call begins on the device path -- samples 3, 6, 9 all inside batches"""
    done, steps, tables, batch = mh.check_run(lib, base, ov, 10, 3, pieces=[4, 6], expect_batch=lambda done, ready: 3 if ready == 1 else -1)
    assert done == 10 and steps == [3, 6, 9] and batch == 3


@pytest.mark.parametrize("base,ov", BATCHED, ids=ids(BATCHED))
def test_end_time_inside_a_batch(base, ov, lib):
    """t passes the end inside the 6th step, a multiple of 3: that last step is sampled; inside the 5th: it is not, and no sample follows.
    The sample of step 9, queued behind a step that did not run, is not counted as taken but was queued: the counter counts launches"""
    p = lib.params_from_ini(ini(base), ov)
    dts = ec.lone_run(lib, p, mh.initial_state(lib, base, ov, p), 10)["dt_log"]
    for k, want in ((6, [3, 6]), (5, [3])):
        queued = lambda done, ready: 3 if ready == 1 else -1   # steps 3, 6, 9 of the ten queued: on the device path, without a condition
        done, steps, tables, batch = mh.check_run(lib, base, ov, 10, 3, tEnd=ec.end_inside_step(dts, k), expect_batch=queued)
        assert done == k and steps == want and batch == 3


def test_across_a_batch_boundary(lib):
    """300 steps, every 7th sampled: 7 does not divide the 256 steps of a batch, so the samples of the second batch sit in other slots
    of the log than those of the first, and slots are used again without being zeroed"""
    base, ov = BATCHED[0]
    done, steps, tables, batch = mh.check_run(lib, base, ov, 300, 7, expect_batch=mh.batch_samples(7))
    assert done == 300 and len(steps) == 42 and steps[-1] == 294 and batch == 42


@pytest.mark.parametrize("base,ov", LITERAL, ids=["gravity", "dissipative"])
def test_literal_path(base, ov, lib):
    """gravity and the dissipative stage take their time step from the host: the literal loop, the same series, no sample on the device"""
    def never(done, ready):
        assert ready == 0, "the context takes its time step from the device"
        return 0
    done, steps, tables, batch = mh.check_run(lib, base, ov, 10, 3, pieces=[4, 6], expect_batch=never)
    assert done == 10 and steps == [3, 6, 9] and batch == 0


def test_refusals(lib):
    mh.check_refusals(lib, ini, slab=False)


def test_euler_hip_pdf_files(gpu_lib, tmp_path):
    """[pdfs] enabled=yes every=3 with a 1D and a joint spec: the .npy files equal run_steps_pdfs and are listed; nothing with
    enabled=no; the monitor file byte for byte the one of a run without [pdfs]"""
    exe = os.path.join(ROOT, "ramsesgpu_amd", "euler_hip")

    def run(overrides):
        r = subprocess.run([exe, "--param", ini("implode3d"), "--set", overrides], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:]
    mh.check_driver_files(gpu_lib, run, tmp_path)
