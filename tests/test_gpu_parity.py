"""Parity of the HIP path (ramsesgpu_amd/librgpu.so, gfx950) -- the tests proper.  Everything goes through the
C ABI.  Checker: the oracle (CPU restatement pinned to the reference binary) and the reference's golden fixtures.
Bar: bit-identical doubles (stated tolerance of north_star: relative L2 < 1e-12, see parity_checks.assert_same)."""
import os

import numpy as np
import pytest

import flat_path_checks as fp
import parity_checks as pc
from conftest import ROOT, golden_cases, ini
from ramsesgpu_amd.solver import Solver, interior

pytestmark = pytest.mark.gpu
GOLDEN = sorted(golden_cases())


@pytest.mark.parametrize("name", GOLDEN)
def test_golden(name, gpu_lib):
    pc.check_golden_case(gpu_lib, name)


@pytest.mark.parametrize("base,ov,nsteps", pc.ORACLE_RUNS, ids=["%s[%s]" % (b, o) for b, o, _ in pc.ORACLE_RUNS])
def test_run_vs_oracle(base, ov, nsteps, gpu_lib, oracle):
    pc.check_run_vs_oracle(gpu_lib, oracle, base, ov, nsteps)


@pytest.mark.parametrize("base,ov,mach", pc.RANDOM_STEPS, ids=["%s[%s]" % (b, o) for b, o, _ in pc.RANDOM_STEPS])
def test_single_step_on_random_state(base, ov, mach, gpu_lib, oracle):
    pc.check_single_step_random(gpu_lib, oracle, base, ov, mach=mach)


@pytest.mark.parametrize("base,ov", pc.BOUNDARY_CASES, ids=["%s[%s]" % c for c in pc.BOUNDARY_CASES])
def test_boundaries_and_dt(base, ov, gpu_lib, oracle):
    pc.check_boundaries(gpu_lib, oracle, base, ov)
    pc.check_compute_dt(gpu_lib, oracle, base, ov)


# sizes the oracle still finishes in seconds
MEDIUM = [
    ("orszag-tang", "mesh.nx=128;mesh.ny=128", 20),
    ("mhd_BrioWu", "mesh.nx=96;mesh.ny=128", 20),
    ("mhd_mri_3d", "mesh.nx=32;mesh.ny=64;mesh.nz=32", 10),
    ("orszag-tang3d", "mesh.nx=32;mesh.ny=32;mesh.nz=32", 5),
    # the last x face column in its own 2 x 32 tiles (hip/tiled_mhd.h: MhLastX): nx a multiple of 16 without a periodic image in x --
    # shearing box with a partly filled second tile of rows; open box whose y layer is not copied either (33 face rows: a tile with one row)
    ("mhd_mri_3d", "mesh.nx=48;mesh.ny=40;mesh.nz=12", 6),
    ("orszag-tang3d", "mesh.nx=32;mesh.ny=32;mesh.nz=10;mesh.boundary_xmin=2;mesh.boundary_xmax=2;mesh.boundary_ymin=2;mesh.boundary_ymax=2", 5),
    ("implode3d", "mesh.nx=48;mesh.ny=48;mesh.nz=48;hydro.riemannSolver=hllc", 10),
    ("implode3d", "mesh.nx=128;mesh.ny=128;mesh.nz=128;hydro.riemannSolver=hllc", 2),
    ("jet2d_cpu", "mesh.nx=100;mesh.ny=400", 30),
    # uniform static gravity inside the LDS-tiled hydro sweep (several tiles and z segments), both specialised solvers + generic
    ("rayleigh_taylor_gpu_3d", "mesh.nx=40;mesh.ny=36;mesh.nz=48", 6),
    ("rayleigh_taylor_gpu_3d", "mesh.nx=40;mesh.ny=36;mesh.nz=48;hydro.riemannSolver=hllc;hydro.slope_type=1", 6),
    ("rayleigh_taylor_gpu_3d", "mesh.nx=24;mesh.ny=40;mesh.nz=32;hydro.riemannSolver=hll", 6),
    ("implode3d", "mesh.nx=48;mesh.ny=40;mesh.nz=36;hydro.riemannSolver=hllc;hydro.unsplitVersion=2", 8),   # direction-wise update order
]


@pytest.mark.parametrize("base,ov,nsteps", MEDIUM, ids=["%s[%s]" % (b, o) for b, o, _ in MEDIUM])
def test_medium_sizes_vs_oracle(base, ov, nsteps, gpu_lib, oracle):
    pc.check_run_vs_oracle(gpu_lib, oracle, base, ov, nsteps)


BENCH_GEOMETRY = pc.BENCH_GEOMETRY


LONG_RUNS = [
    # hundreds of steps: the perturbation grows, limiter / solver branches diversify -- every double and every dt still equal
    ("mhd_mri_3d", "mesh.nx=24;mesh.ny=48;mesh.nz=24;MRI.amp=0.1", 400),
    ("implode3d", "mesh.nx=40;mesh.ny=40;mesh.nz=40;hydro.riemannSolver=hllc", 300),
    ("orszag-tang", "mesh.nx=96;mesh.ny=96", 400),
]


@pytest.mark.parametrize("base,ov,nsteps", LONG_RUNS, ids=["%s-%d" % (b, n) for b, _, n in LONG_RUNS])
def test_long_runs_vs_oracle(base, ov, nsteps, gpu_lib, oracle):
    pc.check_run_vs_oracle(gpu_lib, oracle, base, ov, nsteps)


@pytest.mark.parametrize("base,ov,nsteps", BENCH_GEOMETRY, ids=["%s[%s]" % (b, o) for b, o, _ in BENCH_GEOMETRY])
def test_bench_launch_geometry_vs_oracle(base, ov, nsteps, gpu_lib, oracle):
    pc.check_run_vs_oracle(gpu_lib, oracle, base, ov, nsteps)


@pytest.mark.parametrize("sub", ["0", "2048", "4096"])
@pytest.mark.parametrize("base,ov", [("mhd_mri_3d", "mesh.nx=224;mesh.ny=208;mesh.nz=16"),
                                     ("implode3d", "mesh.nx=208;mesh.ny=224;mesh.nz=8;hydro.riemannSolver=hllc"),
                                     ("mhd_mri_3d_stratified", "mesh.nx=224;mesh.ny=208;mesh.nz=16;hydro.slope_type=2.0;MRI.amp=0.3")],
                         ids=["mri-224x208x16", "implode-208x224x8", "stratified-224x208x16"])
def test_xcd_sub_band_sizes_vs_oracle(base, ov, sub, gpu_lib, oracle, monkeypatch):
    """option "xcd_sub" (read at rgpu_create, kept per context): linear order, 2048- and 4096-cell sub-bands on a >= 200^2 plane.
    The option is read by the launch_planes calls of the FLAT kernels alone (api/step_hydro.h, api/step_mhd.h, api/forcing.h).  The stratified box has a
    per-cell gravity field and runs them in any process: on it the option is exercised by default.  The first two cases run the tiled
    sweeps, which never read it, unless the process runs under RGPU_TILED=0 -- tests/flat_worker.py runs exactly these two at these three
    values in such a process, for tests/test_flat_path_gpu.py."""
    old = gpu_lib.set_option("xcd_sub", int(sub))
    try:
        if base == "mhd_mri_3d_stratified":   # the model: band of 25 workgroups of 256, cut into 4 / 2 sub-bands with idle slots
            p = gpu_lib.params_from_ini(ini(base), ov)
            nsub = fp.box_facts(p, int(sub))["b256"]["nsub"]
            assert p.gravityEnabled == 2 and nsub == {"0": None, "2048": 4, "4096": 2}[sub], nsub
            oracle = fp.OnceOracle(oracle)     # one oracle run for the three values
        pc.check_run_vs_oracle(gpu_lib, oracle, base, ov, 2)
    finally:
        gpu_lib.set_option("xcd_sub", old)


def test_orszag_tang_gate_full_size(gpu_lib, oracle):
    """BASELINE config: data/orszag-tang.ini as shipped (512^2, nstepmax=50).  Gate of north_star:
    L2 error vs euler_cpu < 1e-12 per variable; here the reference's CPU arithmetic is reproduced exactly."""
    pc.orszag_tang_gate(gpu_lib, oracle, exact=True)


def test_mri_headline_size_properties(gpu_lib):
    """BASELINE config: data/mhd_mri_3d.ini scaled to 512^3 (the bench workload).  Size-independent properties: constrained
    transport keeps div B at round-off, the shearing box conserves mass to round-off (the remapped x-border fluxes cancel), fields
    stay finite.  They hold for any consistently aliased flux or emf; tests/test_fullsize_windows.py compares a step at this size
    with the oracle, every cell."""
    pc.mri_headline_size_properties(gpu_lib)


def test_implode_bench_size_properties(gpu_lib):
    """BASELINE config: data/implode3d.ini at 256^3 with HLLC.  Reflecting walls: mass and energy are conserved to
    round-off; the initial condition is symmetric under any permutation of (x,y,z) and so must the solution be.  The oracle
    comparison of a step at this size, every cell: tests/test_fullsize_windows.py."""
    pc.implode_bench_size_properties(gpu_lib)


def test_external_state_and_stream(gpu_lib):
    """rgpu_create_external: state arrays owned by torch, work issued on torch's current stream (the slab driver's
    plumbing), same result as the self-allocating context."""
    import torch
    from slab_harness import SlabRun
    ov = "mesh.nx=16;mesh.ny=24;mesh.nz=12"
    run = SlabRun(ini("mhd_mri_3d"), ov, library=gpu_lib, device="cuda:0")
    run.init_simulation()
    dts = [run.oneStepIntegration() for _ in range(4)]
    torch.cuda.synchronize()
    got = run.local_interior().cpu().numpy()
    run.close()
    p = gpu_lib.params_from_ini(ini("mhd_mri_3d"), ov)
    sv = Solver(p, gpu_lib)
    dts_ref = sv.start(gpu_lib.init_condition(ini("mhd_mri_3d"), ov, p), 4)
    ref = interior(sv.getDataHost(), p)
    sv.close()
    assert dts == dts_ref and np.array_equal(got, ref)


SLAB1 = [
    ("mhd_mri_3d", "mesh.nx=32;mesh.ny=48;mesh.nz=40", 5),           # tiled sweep per plane range (under RGPU_TILED=0: the flat kernels' chunked two-stream schedule inside each range)
    ("orszag-tang3d", "mesh.nx=24;mesh.ny=24;mesh.nz=40", 4),
    ("orszag-tang3d", "mesh.nx=16;mesh.ny=16;mesh.nz=24;mesh.boundary_xmin=2;mesh.boundary_xmax=2;mesh.boundary_zmin=1;mesh.boundary_zmax=2", 4),
    ("implode3d", "mesh.nx=32;mesh.ny=32;mesh.nz=32;hydro.riemannSolver=hllc", 5),
    # fastshear: two wraps of ylen in 14 steps, each through a step whose remap / ghost offsets are ny - 1 / 0 (the plant `fast` of tests/shear_phase_checks.py)
    ("mhd_mri_3d", "mesh.nx=16;mesh.ny=8;mesh.nz=24;MHD.omega0=1.0;MRI.amp=0.3", 14),
]


@pytest.mark.parametrize("base,ov,nsteps", SLAB1, ids=["%s[%s]" % (b, o) for b, o, _ in SLAB1])
@pytest.mark.parametrize("overlap", [True, False], ids=["overlap", "serial"])
def test_slab_schedule_world1(base, ov, nsteps, overlap, gpu_lib, oracle):
    """SlabRun's step (boundary planes first, plane-wise ghost fill, 1/dt scanned per plane range; world 1, so the z
    faces are the physical ones) == the single-call oracle run."""
    import torch
    from slab_harness import SlabRun
    run = SlabRun(ini(base), ov, library=gpu_lib, device="cuda:0", overlap=overlap)
    run.init_simulation()
    dts = [run.oneStepIntegration() for _ in range(nsteps)]
    torch.cuda.synchronize()
    got = run.local_interior().cpu().numpy()
    p = run.p
    run.close()
    ref, dts_ref, _ = oracle.run(p, gpu_lib.init_condition(ini(base), ov, p), nsteps)
    assert np.array_equal(np.array(dts), dts_ref)
    pc.assert_same(got, interior(ref, p), "slab schedule " + base)


@pytest.mark.parametrize("base,ov", [("mhd_mri_3d", "mesh.nx=16;mesh.ny=24;mesh.nz=44"),
                                     ("implode3d", "mesh.nx=24;mesh.ny=24;mesh.nz=30"),
                                     ("mhd_mri_3d", "mesh.nx=40;mesh.ny=36;mesh.nz=40;gravity.static=yes")],
                         ids=["mri", "implode3d", "mri-gravity-field"])
def test_step_core_in_plane_pieces(base, ov, gpu_lib):
    if "gravity.static=yes" in ov:
        # per-cell gravity field: the flat 3D MHD kernels.  Of check_core_plane_pieces' pieces of ksize = 46, [8, 31) has 23 planes: the
        # chunked two-stream schedule with C = 3 on a range that does not start at plane 0 (its first prim / elec / trace planes are
        # clipped differently from the whole call's, which runs C = 5)
        p = gpu_lib.params_from_ini(ini(base), ov)
        ks = p.nz + 2 * p.ghostWidth
        assert p.gravityEnabled == 2 and ks == 46
        assert fp.chunk_facts(ks, gpu_lib.get_option("chunks"), (ks - 15) - 8)["C"] == 3 and fp.chunk_facts(ks, gpu_lib.get_option("chunks"), ks)["C"] == 5
    pc.check_core_plane_pieces(gpu_lib, base, ov)


@pytest.mark.parametrize("base,ov,nsteps", [("mhd_mri_3d", "mesh.nx=16;mesh.ny=24;mesh.nz=40", 4),
                                            ("orszag-tang3d", "mesh.nx=16;mesh.ny=16;mesh.nz=32", 3),
                                            ("implode3d", "mesh.nx=16;mesh.ny=16;mesh.nz=24;hydro.riemannSolver=hllc", 4),
                                            ("orszag-tang3d", "mesh.nx=12;mesh.ny=12;mesh.nz=24;hydro.nu=0.005;MHD.eta=0.01", 3),
                                            ("rayleigh_taylor_gpu_3d_mhd", "mesh.nx=8;mesh.ny=8;mesh.nz=32", 3)],
                         ids=["mri", "ot3d", "implode3d", "ot3d-visc-res", "rt3d-mhd-gravity"])
def test_two_slab_processes_on_one_gpu(base, ov, nsteps, gpu_lib, oracle, tmp_path):
    """world_size 2, both ranks on cuda:0 with the HIP library, ghost planes moved by gloo (RCCL needs one device per
    rank): the slab driver's overlapped schedule with a real exchange in flight == single-domain oracle."""
    import os
    import socket
    import subprocess
    import sys
    from conftest import ROOT
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    out = str(tmp_path / "result.txt")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "tests", "slab_worker.py"), base, ov, str(nsteps), out]
    env = dict(os.environ, SLAB_DEVICE="cuda:0", SLAB_OVERLAP="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    res = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=600)
    assert res.returncode == 0, res.stdout[-3000:]
    assert open(out).read().strip() == "OK", open(out).read()


@pytest.mark.parametrize("base,ov,nsteps", pc.HISTORY_CASES + [("mhd_mri_3d", "mesh.nx=64;mesh.ny=96;mesh.nz=48", 3)],
                         ids=["%s[%s]" % (b, o) for b, o, _ in pc.HISTORY_CASES] + ["mri-64x96x48"])
def test_history_diagnostics(base, ov, nsteps, gpu_lib, oracle):
    pc.check_history(gpu_lib, oracle, base, ov, nsteps)


def test_run_driver_writes_reference_history_file(gpu_lib, tmp_path):
    """rgpuh_run with [history] enabled=yes writes <prefix>_history.txt like MHDRunGodunov::start + history_mri; the
    physically meaningful columns equal the reference's file (tests/golden/mri_8x16x8_history.npz) digit for digit, the
    round-off sized ones (mean field, divB: sums that cancel to ~1e-22) stay round-off sized"""
    import ctypes as C
    from conftest import golden_cases, load_golden
    case = golden_cases()["mri_8x16x8_history"]
    H = load_golden("mri_8x16x8_history")["history"]
    ov = case["overrides"] + ";output.outputVtk=no;output.outputHdf5=no;output.outputDir=%s" % tmp_path
    err = C.create_string_buffer(512)
    mc = C.c_double(0)
    n = gpu_lib.lib.rgpuh_run(ini(case["base"]).encode(), ov.encode(), C.byref(mc), err, 512)
    assert n == 10, err.value
    rows = np.array([[float(x) for x in ln.split()] for ln in open(tmp_path / "mhd_mri_3d_history.txt") if not ln.startswith("#")])
    assert rows.shape == H.shape
    for col in (0, 1, 2, 3, 4, 5, 6):          # totalTime dt mass maxwell reynolds maxwell+reynolds magp
        assert np.allclose(rows[:, col], H[:, col], rtol=3e-6, atol=0), col
    assert np.allclose(rows[:, 8], H[:, 8], rtol=1e-4, atol=1e-18)          # mean_By: small but physical
    assert np.abs(rows[:, [7, 9, 10]]).max() <= 1e-15                        # mean_Bx, mean_Bz, divB: round-off


def test_run_driver_writes_inertial_wave_history_file(gpu_lib, tmp_path):
    """2D rotating-frame run of the shipped inertial-wave problem through the run driver: the probe rows of
    history_inertial_wave (one cell's velocity in units of cIso, 8 digits) equal the reference's file character for
    character, the missing separator between totalTime and dt included"""
    import ctypes as C
    from conftest import golden_cases, load_golden
    case = golden_cases()["inertialwave2d_16_history"]
    want = [str(x) for x in load_golden("inertialwave2d_16_history")["history_text"]]
    ov = case["overrides"] + ";output.outputVtk=no;output.outputHdf5=no;output.outputDir=%s" % tmp_path
    err = C.create_string_buffer(512)
    mc = C.c_double(0)
    n = gpu_lib.lib.rgpuh_run(ini(case["base"]).encode(), ov.encode(), C.byref(mc), err, 512)
    assert n == 8, err.value
    got = [ln.rstrip("\n") for ln in open(tmp_path / "mhd_inertialWave_2d_history.txt") if ln.strip() and not ln.startswith("#")]
    assert got == want


@pytest.mark.parametrize("base,ov", [("mhd_mri_3d", "mesh.nx=24;mesh.ny=32;mesh.nz=20;MRI.amp=0.3"),
                                     ("orszag-tang3d", "mesh.nx=24;mesh.ny=20;mesh.nz=16"),
                                     ("implode3d", "mesh.nx=24;mesh.ny=20;mesh.nz=16;hydro.riemannSolver=hllc")])
def test_launch_specialised_kernels_equal_generic_ones(base, ov, gpu_lib):
    """the launch-time specialisations (SPEC template parameter, launchers.h) only tell the optimiser what the host has
    checked: the same run with option "spec" = 0 (generic kernels) must give the same bits"""
    p = gpu_lib.params_from_ini(ini(base), ov)
    U0 = gpu_lib.init_condition(ini(base), ov, p)
    outs = []
    for spec in (1, 0):
        old = gpu_lib.set_option("spec", spec)
        sv = Solver(p, gpu_lib)
        try:
            sv.start(U0, 6)
            outs.append(sv.getDataHost().copy())
        finally:
            sv.close()
            gpu_lib.set_option("spec", old)
    assert np.array_equal(outs[0], outs[1])


OPTION_CASES = [("orszag-tang", "mesh.nx=40;mesh.ny=24"), ("kelvin_helmholtz_gpu_2d", "mesh.nx=40;mesh.ny=24"), ("implode3d", "mesh.nx=24;mesh.ny=20;mesh.nz=16;hydro.riemannSolver=hllc"),
                ("mhd_mri_3d", ""), ("orszag-tang3d", "mesh.nx=24;mesh.ny=20;mesh.nz=16")]
# ... with the viscous / resistive stage behind the step: no fused CFL scan, the 2D kernels' ghost images stale after it (a list of
# its own, so that the ids of the cases above stay what they are)
OPTION_CASES_DISSIPATIVE = [("orszag-tang", "mesh.nx=40;mesh.ny=24;MHD.eta=0.02"), ("kelvin_helmholtz_gpu_2d", "mesh.nx=40;mesh.ny=24;hydro.nu=0.01"),
                            ("orszag-tang3d", "mesh.nx=24;mesh.ny=20;mesh.nz=16;hydro.nu=0.01;MHD.eta=0.02")]


# ... and with a per-cell gravity field: the flat 3D MHD kernels, whose schedule "chunks" = 1 turns into the serial one (a list of its own again)
OPTION_CASES_GRAVITY_FIELD = [("mhd_mri_3d", "mesh.nx=40;mesh.ny=36;mesh.nz=40;gravity.static=yes")]


@pytest.mark.parametrize("option,value", [("ghost_images", 0), ("step_clock", 0), ("zseg", 5), ("spec", 0), ("chunks", 1)])
@pytest.mark.parametrize("base,ov", OPTION_CASES + OPTION_CASES_DISSIPATIVE + OPTION_CASES_GRAVITY_FIELD,
                         ids=[c[0] for c in OPTION_CASES] + [c[0] + "-dissipative" for c in OPTION_CASES_DISSIPATIVE]
                         + [c[0] + "-gravity-field" for c in OPTION_CASES_GRAVITY_FIELD])
def test_diagnostic_options_keep_the_bits(base, ov, option, value, gpu_lib):
    """every diagnostic option of the library (include/rgpu.h, "Environment and options") switches a fast path off or pins a launch
    plan: a batch of steps through rgpu_run_steps gives the same state and the same time steps either way"""
    p = gpu_lib.params_from_ini(ini(base), ov)
    U0 = gpu_lib.init_condition(ini(base), ov, p)
    outs = []
    for on in (False, True):
        old = gpu_lib.set_option(option, value) if on else None
        sv = Solver(p, gpu_lib)
        try:
            pc.attach_gravity(gpu_lib, base, ov, p, sv=sv)
            sv.upload(U0, both=False); sv.make_all_boundaries(0, 0.0, 0.0); sv.upload(sv.getDataHost(0), both=True)
            assert sv.run_steps(7) == 7
            outs.append((interior(sv.getDataHost(), p).copy(), sv.totalTime, sv.dt))
        finally:
            sv.close()
            if on:
                gpu_lib.set_option(option, old)
    assert np.array_equal(outs[0][0], outs[1][0]) and outs[0][1:] == outs[1][1:]


def test_shared_reciprocal_division_and_sqrt_are_ieee(gpu_lib):
    """rg_recip / rg_div / rg_sqrt (csrc/hip/rg_backend.h) are hand-rolled forms of the compiler's fp64 division and sqrt
    without v_div_scale / v_div_fixup.  The parity contract needs them correctly rounded for every value a simulation
    state can take: checked here against numpy's IEEE results on random operands over 2^+-400 and on edge operands
    (exact quotients, powers of two, near-ties, tiny / huge but in range); the compiler's own '/' and sqrt as well."""
    num, den = pc.arith_operands()
    quot, quot2, root, root2 = pc.selftest_arith(gpu_lib, num, den)
    want_q = num / den
    assert np.array_equal(quot2, want_q), "compiler division differs from IEEE"
    assert np.array_equal(quot, want_q), "rg_div differs from IEEE on %d operands" % int((quot != want_q).sum())
    pos = np.abs(num)
    quot, quot2, root, root2 = pc.selftest_arith(gpu_lib, pos, den)
    assert np.array_equal(root2, np.sqrt(pos)) and np.array_equal(root, np.sqrt(pos))


@pytest.mark.parametrize("smallc,iso", [(1e-7, False), (1e-100, False), (1e-7, True), (1e-101, False)], ids=["smallc1e-7", "smallc1e-100", "isothermal", "smallc-below-the-bound"])
def test_alfven_selection_against_the_reference_sequence(smallc, iso, gpu_lib):
    """the 2D HLLD edge solver run twice per sample on the device -- Alfven speeds by selection (alfven_pick / alfven_duel) and by the
    reference's own twelve roots -- on 1.2e7 random and adversarial edge states (parity_checks.alfven_samples): identical bits; both
    routes are exercised, uniform / tied states go down the reference's sequence, and below smallc = 1e-100 every wave does"""
    n = 1 << 22
    sel = ref = 0
    for seed in range(3):
        s, r, kind, route = pc.check_alfven_selftest(gpu_lib, n, 100 + seed, smallc, iso)
        sel += s; ref += r
        assert (route[kind == 2] == 1).all()      # exactly uniform states tie: their waves must take the reference's sequence
    print("alfven selftest smallc=%g: %d samples on the selection route, %d on the reference route" % (smallc, sel, ref))
    if smallc < 1e-100:
        assert sel == 0
    else:
        assert ref > 0      # (with the kinds interleaved lane by lane almost every wave holds a tied sample; the pure-selection route is
        #                     what test_alfven_selection_rough_waves below covers)


def test_alfven_selection_rough_waves(gpu_lib):
    """whole waves of rough random states: the selection route itself (no tied lane in the wave), 4e6 samples, identical bits"""
    import ctypes as C
    n = 1 << 22
    S, kind = pc.alfven_samples(n, 7)
    rough = np.ascontiguousarray(S[:, kind <= 1][:, : (int((kind <= 1).sum()) // 64) * 64])
    p = gpu_lib.params_from_ini(ini("orszag-tang3d"), "mesh.nx=8;mesh.ny=8;mesh.nz=8")
    m = rough.shape[1]
    e_sel, e_ref = np.empty(m), np.empty(m)
    route = np.empty(m, dtype=np.int32)
    f = gpu_lib.lib.rgpu_selftest_alfven
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int)]
    P = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    assert f(C.byref(p), m, P(rough), P(e_sel), P(e_ref), route.ctypes.data_as(C.POINTER(C.c_int))) == 0
    assert np.array_equal(e_sel.view(np.uint64), e_ref.view(np.uint64))
    assert (route == 0).mean() > 0.9, (route == 0).mean()      # these waves really took the selection


@pytest.mark.parametrize("base,ov,nsteps", pc.TURB_HISTORY_CASES, ids=["%s[%s]" % (b, o) for b, o, _ in pc.TURB_HISTORY_CASES])
def test_turbulence_history(base, ov, nsteps, gpu_lib, oracle):
    pc.check_history_turbulence(gpu_lib, oracle, base, ov, nsteps)


def test_run_driver_writes_turbulence_history_file(gpu_lib, tmp_path):
    """rgpuh_run on the Ornstein-Uhlenbeck MHD run with [history] enabled=yes writes <prefix>_history.txt like
    MHDRunGodunov::start + history_turbulence: same rows (same crossing times), same 20 columns; the physically meaningful
    ones equal the reference's file (tests/golden/turb_ou_mhd_12_history.npz) to the printed digits, the cancellation-noise
    ones (divB, the DFT amplitude along x) stay noise sized"""
    import ctypes as C
    from conftest import golden_cases, load_golden
    case = golden_cases()["turb_ou_mhd_12_history"]
    H = load_golden("turb_ou_mhd_12_history")["history"]
    ov = case["overrides"] + ";output.outputVtk=no;output.outputHdf5=no;output.outputDir=%s" % tmp_path
    err = C.create_string_buffer(512)
    mc = C.c_double(0)
    n = gpu_lib.lib.rgpuh_run(ini(case["base"]).encode(), ov.encode(), C.byref(mc), err, 512)
    assert n == 8, err.value
    rows = np.array([[float(x) for x in ln.split()] for ln in open(tmp_path / "turbulence_mhd_ou_history.txt") if not ln.startswith("#")])
    assert rows.shape == H.shape
    for col in (0, 1, 2, 4, 5, 7, 8, 11, 12, 13, 14, 15, 16):   # totalTime dt mass eKin eMag mean_rho mean_B mean_Bz mean_rhov(3) Ma_s Ma_alfven
        assert np.allclose(rows[:, col], H[:, col], rtol=2e-5, atol=1e-12), (col, rows[:, col], H[:, col])
    assert np.allclose(rows[:, 6], H[:, 6], rtol=1e-3, atol=1e-12)                # helicity: small but physical
    assert np.allclose(rows[:, [18, 19]], H[:, [18, 19]], rtol=1e-3, atol=1e-15)  # coef_y, coef_z: Bx picks up structure along y, z
    assert np.abs(rows[:, 3]).max() <= 1e-12                                       # divB: round-off
    assert np.abs(rows[:, 17]).max() <= 1e-18                                      # coef_x: Bx stays uniform along x to round-off


@pytest.mark.parametrize("base,ov", [("mhd_BrioWu", "mesh.nx=48;mesh.ny=32"),
                                     ("mhd_BrioWu", "mesh.nx=24;mesh.ny=16;mesh.nz=16;BrioWu.direction=0;MHD.implementationVersion=4")])
def test_public_ghost_fill_invalidates_fused_dt(base, ov, gpu_lib, oracle):
    pc.check_public_ghost_fill_invalidates_fused_dt(gpu_lib, oracle, base, ov)



@pytest.mark.parametrize("case", pc.FUSED_BOOKKEEPING, ids=[c[0] for c in pc.FUSED_BOOKKEEPING])
def test_fused_scan_and_ghost_bookkeeping(case, gpu_lib):
    """tiled kernels: which step leaves the CFL maxima of its output for the next compute_dt (phase timer of the scan), which leaves
    its ghost cells for the next step_pre (phase timer of the fill), and rgpu_inv_dt_fusable the same before and after the first step"""
    pc.check_fused_bookkeeping(gpu_lib, case)

def test_orszag_tang_large_box_properties(gpu_lib):
    """the fused 2D MHD kernel at a size the oracle does not run in seconds (2048^2: 137 x 293 tiles, the periodic ghost images
    written by the kernel itself): div B stays at round-off, mass / energy / momentum are conserved to round-off in the periodic
    box, and the flat kernels (RGPU_TILED=0 is read per process, so: a second context through the plane API is not available
    in 2D), hence
    only the properties here; bit-identity of the tiled path is pinned by the 512^2 gate and the fixtures."""
    ov = "mesh.nx=2048;mesh.ny=2048"
    p = gpu_lib.params_from_ini(ini("orszag-tang"), ov)
    U0 = gpu_lib.init_condition(ini("orszag-tang"), ov, p)
    sv = Solver(p, gpu_lib)
    try:
        sv.start(U0, 8)
        A = sv.getDataHost()
    finally:
        sv.close()
    gw = p.ghostWidth
    I0, I1 = interior(U0, p), interior(A, p)
    assert np.isfinite(A).all()
    for v in (0, 1, 2, 3):     # density, energy, x and y momentum: conserved by the flux form in a periodic box
        a, b = I1[v].sum(dtype=np.longdouble), I0[v].sum(dtype=np.longdouble)
        scale = max(abs(float(b)), float(np.abs(I0[v]).sum(dtype=np.longdouble)))
        assert abs(float(a - b)) < 1e-12 * scale, (v, float(a), float(b))
    A = A[:, 0]                # 2D: [variable, y, x] with ghosts
    bx, by = A[5], A[6]
    s = (slice(gw, -gw), slice(gw, -gw))
    div = (bx[gw:-gw, gw + 1:-gw + 1] - bx[s]) / p.dx + (by[gw + 1:-gw + 1, gw:-gw] - by[s]) / p.dy
    bscale = float(np.abs(bx[s]).max()) / min(p.dx, p.dy)
    assert float(np.abs(div).max()) < 1e-11 * bscale
    # the ghost cells the kernel wrote are the periodic images of the interior (option ghost_images = 0 / RGPU_TILED=0: the next
    # step's ghost fill does it, so the output array's ghosts are one step old)
    if gpu_lib.get_option("ghost_images") == 0 or os.environ.get("RGPU_TILED") == "0":
        return
    nx, ny = p.nx, p.ny
    assert np.array_equal(A[:, gw:-gw, :gw], A[:, gw:-gw, nx:nx + gw]) and np.array_equal(A[:, gw:-gw, nx + gw:], A[:, gw:-gw, gw:2 * gw])
    assert np.array_equal(A[:, :gw, :], A[:, ny:ny + gw, :]) and np.array_equal(A[:, ny + gw:, :], A[:, gw:2 * gw, :])


@pytest.mark.parametrize("base,ov", [("kelvin_helmholtz_gpu_2d", "mesh.nx=96;mesh.ny=64"),              # periodic x and y
                                     ("rayleigh_taylor_gpu_2d", "mesh.nx=40;mesh.ny=120"),             # periodic x, reflecting y, gravity
                                     ("hydro_sod2d", "mesh.nx=70;mesh.ny=50"),                          # outflow
                                     ("blast2d", "mesh.nx=64;mesh.ny=64;mesh.boundary_xmin=1;mesh.boundary_ymax=1;mesh.boundary_xmax=2;mesh.boundary_ymin=3;mesh.boundary_ymax=3"),
                                     ("blast2d", "mesh.nx=3;mesh.ny=5;mesh.boundary_xmin=1;mesh.boundary_xmax=1;mesh.boundary_ymin=2;mesh.boundary_ymax=2")])
def test_fused_hydro2d_ghost_images(base, ov, gpu_lib, oracle):
    """the fused 2D hydro step writes the ghost cells of its output itself (mirror / outflow / periodic images, corners = images of
    images) and the next step launches no ghost fill: after some steps the output array must equal itself after the public ghost
    fill, ghost cells included, and the interior the oracle's"""
    p = gpu_lib.params_from_ini(ini(base), ov)
    U0 = gpu_lib.init_condition(ini(base), ov, p)
    pc.attach_gravity(gpu_lib, base, ov, p, oracle=oracle)
    ref, dts_ref, _ = oracle.run(p, U0, 6)
    sv = Solver(p, gpu_lib)
    try:
        pc.attach_gravity(gpu_lib, base, ov, p, sv=sv)
        dts = sv.start(U0, 6)
        A = sv.getDataHost().copy()
        par = sv.nStep % 2
        assert np.array_equal(np.array(dts), dts_ref)
        assert np.array_equal(interior(A, p), interior(ref, p))
        if gpu_lib.get_option("ghost_images") == 0 or os.environ.get("RGPU_TILED") == "0":
            return
        sv.make_all_boundaries(par, sv.totalTime, dts[-1])
        B = sv.getDataHost(par)
        assert np.array_equal(A, B), "%d ghost cells differ from the ghost fill" % int((A != B).sum())
    finally:
        sv.close()


def test_kelvin_helmholtz_large_box_properties(gpu_lib):
    """the fused 2D hydro kernel at a size the oracle does not run in seconds (2048^2: 147 x 147 tiles, periodic ghost images written by
    the kernel itself): mass, momentum and energy are conserved to round-off by the flux form in the periodic box, and the ghost cells
    of the output are the periodic images of its interior; bit-identity of the kernel is pinned by the fixtures and oracle runs."""
    base, ov = "kelvin_helmholtz_gpu_2d", "mesh.nx=2048;mesh.ny=2048"
    p = gpu_lib.params_from_ini(ini(base), ov)
    U0 = gpu_lib.init_condition(ini(base), ov, p)
    sv = Solver(p, gpu_lib)
    try:
        sv.start(U0, 10)
        A = sv.getDataHost()
    finally:
        sv.close()
    gw = p.ghostWidth
    I0, I1 = interior(U0, p), interior(A, p)
    assert np.isfinite(A).all() and not np.array_equal(I0, I1)
    for v in range(4):
        a, b = I1[v].sum(dtype=np.longdouble), I0[v].sum(dtype=np.longdouble)
        scale = max(abs(float(b)), float(np.abs(I0[v]).sum(dtype=np.longdouble)))
        assert abs(float(a - b)) < 1e-12 * scale, (v, float(a), float(b))
    if gpu_lib.get_option("ghost_images") == 0 or os.environ.get("RGPU_TILED") == "0":
        return
    A = A[:, 0]
    nx, ny = p.nx, p.ny
    assert np.array_equal(A[:, gw:-gw, :gw], A[:, gw:-gw, nx:nx + gw]) and np.array_equal(A[:, gw:-gw, nx + gw:], A[:, gw:-gw, gw:2 * gw])
    assert np.array_equal(A[:, :gw, :], A[:, ny:ny + gw, :]) and np.array_equal(A[:, ny + gw:, :], A[:, gw:2 * gw, :])


RUN_STEPS_CASES = [
    ("orszag-tang", "mesh.nx=96;mesh.ny=80", 24, True),                        # 2D MHD, periodic box: device-side time step
    ("kelvin_helmholtz_gpu_2d", "mesh.nx=96;mesh.ny=64", 24, True),            # 2D hydro, periodic
    ("hydro_sod2d", "mesh.nx=70;mesh.ny=50", 24, True),                        # 2D hydro, outflow faces (ghost images)
    ("blast2d", "mesh.nx=64;mesh.ny=64;mesh.boundary_xmin=1;mesh.boundary_ymax=1;mesh.boundary_xmax=2;mesh.boundary_ymin=3;mesh.boundary_ymax=3", 24, True),
    ("rayleigh_taylor_gpu_2d", "mesh.nx=40;mesh.ny=120", 12, False),           # gravity: (0.5 dt) g is a kernel argument -> plain loop
    ("jet2d_cpu", "mesh.nx=40;mesh.ny=120", 12, False),                        # jet inflow: ghost fill every step -> plain loop
    ("mhd_BrioWu", "mesh.nx=128;mesh.ny=8", 12, None),                         # 2D MHD with non-periodic faces
    # 3D (round 5): the z-marching sweeps, the MHD update, the shear remap and the fused ghost fill read the record too
    ("implode3d", "mesh.nx=24;mesh.ny=24;mesh.nz=24;hydro.riemannSolver=hllc", 8, True),    # 3D hydro, reflecting walls: one sweep + ghost fill per step
    ("implode3d", "mesh.nx=20;mesh.ny=24;mesh.nz=28", 8, True),                              # ... approx solver
    ("orszag-tang3d", "mesh.nx=24;mesh.ny=20;mesh.nz=16", 8, True),                          # plain 3D MHD, periodic
    ("mhd_mri_3d", "mesh.nx=24;mesh.ny=32;mesh.nz=16;MHD.omega0=0.02", 8, True),             # rotating frame + shearing box: offsets at t + dt/2 and t + dt from the record
    ("mhd_mri_3d", "mesh.nx=16;mesh.ny=32;mesh.nz=16", 8, True),                             # ... as shipped (Omega0 = 0.001)
    ("mhd_BrioWu", "mesh.nx=32;mesh.ny=12;mesh.nz=12;BrioWu.direction=0;MHD.implementationVersion=4", 8, True),   # 3D MHD, outflow faces: the CFL scan sees unfilled ghosts
    ("rayleigh_taylor_gpu_3d_mhd", "mesh.nx=8;mesh.ny=8;mesh.nz=32", 6, False),              # gravity: plain loop
    ("orszag-tang3d", "mesh.nx=12;mesh.ny=12;mesh.nz=16;hydro.nu=0.005;MHD.eta=0.01", 6, False),   # dissipative stage: plain loop
]
# the 2D boxes of the first two lines with the dissipative stage: the plain loop, every step_pre refills the ghosts the stage left stale
# (a list of its own, so that the ids of the cases above stay what they are)
RUN_STEPS_DISSIPATIVE = [
    ("kelvin_helmholtz_gpu_2d", "mesh.nx=96;mesh.ny=64;hydro.nu=0.01", 12, False),
    ("orszag-tang", "mesh.nx=96;mesh.ny=80;MHD.eta=0.02", 12, False),
]


@pytest.mark.parametrize("base,ov,nsteps,clocked", RUN_STEPS_CASES + RUN_STEPS_DISSIPATIVE,
                         ids=[c[0] for c in RUN_STEPS_CASES] + [c[0] + "-dissipative" for c in RUN_STEPS_DISSIPATIVE])
def test_run_steps_equals_the_reference_loop(base, ov, nsteps, clocked, gpu_lib, oracle):
    """rgpu_run_steps(K) == K x oneStepIntegration == the oracle: every double of the state, nStep, t and the last dt -- where the
    time step stays on the device between the fused 2D kernels (csrc/hip/step_clock.h) and where the call falls back to the plain
    loop.  Also: in odd pieces (3 + the rest, i.e. a batch that starts in the middle of a run), and with an end time inside the batch
    (the loop condition t < tEnd is evaluated on the device: the steps behind it are no-ops)."""
    p = gpu_lib.params_from_ini(ini(base), ov)
    U0 = gpu_lib.init_condition(ini(base), ov, p)
    pc.attach_gravity(gpu_lib, base, ov, p, oracle=oracle)
    ref, dts_ref, _ = oracle.run(p, U0, nsteps)
    t_ref = 0.0
    for d in dts_ref:
        t_ref += float(d)

    def fresh():
        sv = Solver(p, gpu_lib)
        pc.attach_gravity(gpu_lib, base, ov, p, sv=sv)
        sv.start(U0, 0)
        return sv
    sv = fresh()
    try:
        assert sv.run_steps(nsteps) == nsteps
        assert sv.nStep == nsteps and sv.totalTime == t_ref and sv.dt == float(dts_ref[-1]), (sv.nStep, sv.totalTime, t_ref, sv.dt, dts_ref[-1])
        nbad = int((interior(sv.getDataHost(), p) != interior(ref, p)).sum())
        assert nbad == 0, "%d doubles differ from the oracle" % nbad
    finally:
        sv.close()
    sv = fresh()
    try:   # pieces: the first call always starts with a plain step, the second one starts on a state a fused kernel left
        assert sv.run_steps(3) == 3 and sv.run_steps(nsteps - 3) == nsteps - 3
        assert sv.nStep == nsteps and sv.totalTime == t_ref and sv.dt == float(dts_ref[-1])
        assert np.array_equal(interior(sv.getDataHost(), p), interior(ref, p))
        # one more plain step after a batch: the context's bookkeeping (CFL slots, ghost cells) is that of the single-step path
        more, dts_more, _ = oracle.run(p, U0, nsteps + 1)
        sv.oneStepIntegration()
        assert sv.dt == float(dts_more[-1]) and np.array_equal(interior(sv.getDataHost(), p), interior(more, p))
    finally:
        sv.close()
    # an end time inside the batch: the reference's loop stops after the first step that carries t to or past tEnd
    cut = nsteps // 2
    t_cut = 0.0
    for d in dts_ref[:cut]:
        t_cut += float(d)
    tEnd = t_cut - 0.25 * float(dts_ref[cut - 1])     # reached during step `cut`
    ref_cut, dts_cut, _ = oracle.run(p, U0, cut)
    sv = fresh()
    try:
        assert sv.run_steps(nsteps, tEnd) == cut, sv.nStep
        assert sv.nStep == cut and sv.totalTime == t_cut and sv.dt == float(dts_ref[cut - 1])
        assert np.array_equal(interior(sv.getDataHost(), p), interior(ref_cut, p))
        assert sv.run_steps(5, tEnd) == 0                                  # t >= tEnd: nothing to do
        sv.oneStepIntegration()                                           # and the state is usable: full CFL scan, valid ghost cells
        assert sv.dt == float(dts_ref[cut]), (sv.dt, dts_ref[cut])
    finally:
        sv.close()
    if clocked is not None and not (os.environ.get("RGPU_TILED") == "0" or gpu_lib.get_option("step_clock") == 0 or gpu_lib.get_option("ghost_images") == 0):
        # which path ran: the phase timers count launches -- a device-clock batch has no ghost fill and no stand-alone CFL scan,
        # and the timers themselves force the plain loop, so count through the dominant-kernel statistics of an untimed run instead
        sv = fresh()
        try:
            sv.run_steps(2)
            assert bool(gpu_lib.lib.rgpu_device_time_step_ready(sv.ctx, sv.nStep % 2)) == clocked
        finally:
            sv.close()


def test_run_steps_longer_than_one_clock_batch(gpu_lib, oracle):
    """more steps than one batch of device clock records (256): 300 steps of a small Orszag-Tang box in one rgpu_run_steps call == the
    oracle's 300 steps (state, t, last dt), and == 300 single steps"""
    base, ov, n = "orszag-tang", "mesh.nx=48;mesh.ny=40", 300
    p = gpu_lib.params_from_ini(ini(base), ov)
    U0 = gpu_lib.init_condition(ini(base), ov, p)
    ref, dts_ref, _ = oracle.run(p, U0, n)
    t_ref = 0.0
    for d in dts_ref:
        t_ref += float(d)
    sv = Solver(p, gpu_lib)
    try:
        sv.start(U0, 0)
        assert sv.run_steps(n) == n
        assert sv.nStep == n and sv.totalTime == t_ref and sv.dt == float(dts_ref[-1])
        assert np.array_equal(interior(sv.getDataHost(), p), interior(ref, p))
    finally:
        sv.close()


NEAR_UNIFORM = [("orszag-tang", "mesh.nx=40;mesh.ny=32"), ("orszag-tang3d", "mesh.nx=20;mesh.ny=16;mesh.nz=12"), ("mhd_mri_3d", "mesh.nx=16;mesh.ny=24;mesh.nz=12")]


@pytest.mark.parametrize("eps", [0.0, 1e-15, 3e-14, 1e-12, 3e-11, 1e-8])
@pytest.mark.parametrize("base,ov", NEAR_UNIFORM, ids=[c[0] for c in NEAR_UNIFORM])
def test_alfven_selection_near_ties(base, ov, eps, gpu_lib, oracle):
    """the Alfven-speed selection of the 2D HLLD edge solver at, inside and outside its margins (2^-40 on the star ratio, 2^-45 on
    the cross products): uniform magnetised flow + perturbations of relative size eps, one step, every double equal to the oracle's"""
    pc.check_single_step_near_uniform(gpu_lib, oracle, base, ov, eps)


@pytest.mark.parametrize("base,ov", [("implode3d", "mesh.nx=20;mesh.ny=17;mesh.nz=12"),
                                     ("implode3d", "mesh.nx=19;mesh.ny=33;mesh.nz=12;mesh.boundary_xmin=2;mesh.boundary_xmax=3;mesh.boundary_ymin=3;mesh.boundary_ymax=1"),
                                     ("orszag-tang3d", "mesh.nx=24;mesh.ny=20;mesh.nz=12;mesh.boundary_xmin=2;mesh.boundary_xmax=2;mesh.boundary_ymin=1;mesh.boundary_ymax=2"),
                                     ("mhd_mri_3d", "mesh.nx=24;mesh.ny=36;mesh.nz=12;MHD.omega0=0.05"),
                                     ("mhd_mri_3d", "mesh.nx=70;mesh.ny=130;mesh.nz=12;MHD.omega0=0.3")],
                         ids=["implode", "mixed-faces", "ot3d-open", "mri", "mri-large-shift"])
def test_one_launch_ghost_fill_equals_the_separate_passes(base, ov, gpu_lib, oracle):
    """K_fill_xy (x and y faces / shearing-box remap, corners included, two plane ranges in one launch) == the oracle's separate passes"""
    pc.check_fused_fill(gpu_lib, oracle, base, ov)
