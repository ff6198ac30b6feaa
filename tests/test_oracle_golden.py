"""The oracle (CPU restatement) against fixtures produced by THE REFERENCE ITSELF (oracle/gen_golden.py ran
oracle/_ref/euler_cpu built from /root/reference).  Bar: bit-identical doubles, dt sequence included.
This is what pins the oracle; the HIP path is then checked against the oracle and the same fixtures."""
import numpy as np
import pytest

from conftest import golden_cases, ini, load_golden
from ramsesgpu_amd.solver import interior

CASES = sorted(golden_cases().items())


@pytest.mark.parametrize("name,case", CASES, ids=[c[0] for c in CASES])
def test_oracle_reproduces_reference_bit_for_bit(name, case, oracle, product_lib):
    L = product_lib  # host entry points only: parameter file -> params, initial condition
    p = L.params_from_ini(ini(case["base"]), case["overrides"])
    g = load_golden(name)
    for s in case["steps"]:
        U0 = L.init_condition(ini(case["base"]), case["overrides"], p)
        oracle.set_gravity_field(L.init_gravity(ini(case["base"]), case["overrides"], p))   # h_gravity, where the problem has one
        oracle.set_forcing_field(L.init_forcing(ini(case["base"]), case["overrides"], p))   # h_randomForcing, likewise
        U, dts, t = oracle.run(p, U0, s)
        ref = g["step_%d" % s]
        got = interior(U, p)
        assert got.shape == ref.shape
        assert np.array_equal(got, ref), "%s step %d: %d doubles differ from the reference" % (name, s, (got != ref).sum())
        # dt log of the reference (line N carries the dt of step N-1): the MHD run class prints 12 decimals
        # (MHDRunGodunov.cpp:3955-3958), the hydro one 8
        if s >= 2 and len(g["log_dt"]) > s - 1:
            digits = 0.6e-12 if p.mhdEnabled else 0.6e-8
            np.testing.assert_allclose(dts[: s - 1], g["log_dt"][1:s], rtol=0, atol=digits * max(1.0, dts.max()))
        if s == max(case["steps"]) and np.isfinite(g["total_time"]):
            assert abs(t - float(g["total_time"])) <= 1e-11 * max(1.0, abs(t))


ROUGH_DISSIPATIVE = ["turb_mhd_10x12x14_visc_res", "turb_hydro_10x12x14_visc", "mri_8x12x10_amp_visc_res", "briowu_z_8x6x16_visc_res_open",
                     "implode3d_10x8x6_rand_visc", "kh2d_rand_20x28_visc", "ot2d_20x28_iso_visc_res", "ot2d_16x24_rot_visc_res"]


@pytest.mark.parametrize("name", ROUGH_DISSIPATIVE)
def test_rough_dissipative_fixtures_carry_a_stage_that_matters(name, product_lib):
    """the fixtures that pin the viscous / resistive stage on rough states: the explicit diffusion number
    max(nu, eta) dt / min(dx, dy, dz)^2 of every step of the reference's dt log lies in [0.02, 0.2] -- at 0.02 the stage moves the state
    by percents, up to 0.2 it amplifies no round-off -- and the reference's output is finite"""
    case = golden_cases()[name]
    p = product_lib.params_from_ini(ini(case["base"]), case["overrides"])
    g = load_golden(name)
    nsteps = max(case["steps"])
    dts = g["log_dt"]      # the initial compute_dt, then the dt of every step
    assert len(dts) >= nsteps and np.isfinite(g["step_%d" % nsteps]).all()
    h = min(p.dx, p.dy, p.dz) if p.three_d else min(p.dx, p.dy)
    D = max(p.nu, p.eta if p.mhdEnabled else 0.0) * dts / (h * h)
    print("%s: diffusion number %.3f .. %.3f" % (name, D.min(), D.max()))
    assert 0.02 <= D.min() and D.max() <= 0.2, (name, D.min(), D.max())


CORNER_FIXTURES = ["blast2d_corner_16x24_reflect", "blast2d_corner_16x24_outflow", "blast3d_corner_12x18x12_reflect", "blast3d_corner_12x18x12_outflow",
                   "fieldloop2d_corner_24x12_reflect", "fieldloop2d_corner_24x12_outflow"]


@pytest.mark.parametrize("name", CORNER_FIXTURES)
def test_corner_fixtures_carry_their_fastest_cell_in_the_outermost_layer(name, oracle, product_lib):
    """the fixtures that pin what the reference scans in its last interior layer (and when: before or after the ghost refill): in the
    oracle's state after the first step -- whose scan reproduces the second dt, the reference's log to its printed digits -- replacing
    the outermost high-side layer (i = nx - 1 or j = ny - 1 or k = nz - 1) by the low corner cell drops 1/dt to <= 0.8 of its value
    (tests/cfl_plant_checks.py: masking_ratio, MASK_CAP)"""
    import cfl_plant_checks as cp
    import parity_checks as pc
    case = golden_cases()[name]
    p = product_lib.params_from_ini(ini(case["base"]), case["overrides"])
    g = load_golden(name)
    U0 = product_lib.init_condition(ini(case["base"]), case["overrides"], p)
    U1, _, _ = oracle.run_sequential(p, U0, 1)
    _, dts, _ = oracle.run_sequential(p, U0, 2)
    assert p.cfl / oracle.compute_inv_dt(p, U1) == dts[1]
    pc.assert_dt_log(dts, g["log_dt"], p, name)
    gw = p.ghostWidth
    nz = p.nz if p.three_d else 1
    layer = [(k + gw if p.three_d else 0, j + gw, i + gw) for k in range(nz) for j in range(p.ny) for i in range(p.nx)
             if i == p.nx - 1 or j == p.ny - 1 or (p.three_d and k == nz - 1)]
    ratio = cp.masking_ratio(oracle, p, U1, layer, (gw if p.three_d else 0, gw, gw))
    print("%s: 1/dt with the outermost high-side layer masked / unmasked = %.3f" % (name, ratio))
    assert ratio <= cp.MASK_CAP, (name, ratio)


@pytest.mark.parametrize("name", ["mri_8x16x8_history", "ot3d_12_history"])
def test_oracle_history_matches_reference_history_file(name, oracle, product_lib):
    """the reference writes <prefix>_history.txt with 6 significant digits (MHDRunBase.cpp:3596-3602, 3401-3402): one
    row before every step.  The oracle's restatement of history_mri / history_default on its own (bit-identical) states
    must print the same digits."""
    from conftest import golden_cases
    case = golden_cases()[name]
    L = product_lib
    p = L.params_from_ini(ini(case["base"]), case["overrides"])
    g = load_golden(name)
    H = g["history"]
    for n in range(H.shape[0]):
        U0 = L.init_condition(ini(case["base"]), case["overrides"], p)
        U, dts, t = oracle.run(p, U0, n)
        h = oracle.history_mri(p, U)   # mass, maxwell, reynolds, magp, mean_Bx, mean_By, mean_Bz, divB
        if H.shape[1] == 11:           # totalTime dt mass maxwell reynolds maxwell+reynolds magp mean_B(3) divB
            mine = [h[0], h[1], h[2], h[1] + h[2], h[3], h[4], h[5], h[6], h[7]]
        else:                          # history_default: totalTime dt mass divB
            mine = [h[0], h[7]]
        for a, b in zip(mine, H[n, 2:]):
            assert float("%.5e" % a) == float("%.5e" % b) or abs(a - b) <= 2e-6 * abs(b), (n, a, b)


def test_oracle_turbulence_history_matches_reference_history_file(oracle, product_lib):
    """history_turbulence (MHDRunBase.cpp:3626-3810) of the Ornstein-Uhlenbeck MHD run: the reference prints a row whenever
    the time crosses the next multiple of dtHist (MHDRunGodunov.cpp:3975-3984); the oracle's restatement on its own
    (bit-identical) states prints the same 6 significant digits.  Columns that are pure cancellation noise (divB, the
    momenta means, the DFT amplitudes of an almost uniform field) are compared against the scale of their terms."""
    from conftest import golden_cases
    name = "turb_ou_mhd_12_history"
    case = golden_cases()[name]
    L = product_lib
    p = L.params_from_ini(ini(case["base"]), case["overrides"])
    H = load_golden(name)["history"]
    assert H.shape[1] == 20 and H.shape[0] >= 4
    U0 = L.init_condition(ini(case["base"]), case["overrides"], p)
    _, dts, _ = oracle.run(p, U0.copy(), 8)
    times = np.concatenate([[0.0], np.cumsum(dts)])
    for row in H:
        n = int(np.argmin(np.abs(times - row[0])))
        assert abs(times[n] - row[0]) <= 1e-5 * max(1.0, row[0])
        U, _, _ = oracle.run(p, L.init_condition(ini(case["base"]), case["overrides"], p), n)
        h = oracle.history_turbulence(p, U)
        scale = {1: 1e-4 / p.dx, 10: 1.0, 11: 1.0, 12: 1.0, 15: 1e-8, 16: 1e-8, 17: 1e-8, 4: 1e-4}   # magnitudes of the terms of the cancelling sums
        for q, (a, b) in enumerate(zip(h, row[2:])):
            if q in scale:
                assert abs(a - b) <= 1e-12 * scale[q] * p.nx * p.ny * p.nz + 6e-6 * abs(b), (n, q, a, b)   # 6 printed digits
            else:
                assert float("%.5e" % a) == float("%.5e" % b) or abs(a - b) <= 2e-6 * abs(b), (n, q, a, b)


@pytest.mark.parametrize("base,ov,nsteps,nthreads", [
    ("mhd_mri_3d", "mesh.nx=16;mesh.ny=32;mesh.nz=16", 6, 3),                  # rotating + shearing box (the headline workload)
    ("mhd_mri_3d", "mesh.nx=8;mesh.ny=12;mesh.nz=10;MHD.omega0=0.02", 4, 16),  # more threads than planes per slab
    ("orszag-tang3d", "mesh.nx=12;mesh.ny=10;mesh.nz=14", 4, 4),               # plain 3D MHD
])
def test_threaded_step_equals_sequential(base, ov, nsteps, nthreads, oracle, product_lib):
    """the all-cores CPU baseline (orc_run_mt: z-slab threads, fluxes stored, gather update in scatter order) reproduces the
    sequential restatement -- which the golden fixtures pin to the reference binary -- bit for bit, dt sequence included"""
    p = product_lib.params_from_ini(ini(base), ov)
    U0 = product_lib.init_condition(ini(base), ov, p)
    a, da, ta = oracle.run(p, U0, nsteps)
    b, db, tb = oracle.run_mt(p, U0, nsteps, nthreads)
    assert np.array_equal(da, db) and ta == tb
    assert np.array_equal(interior(a, p), interior(b, p))


@pytest.mark.parametrize("mode", [1, 2])
def test_pinned_threads_change_nothing_but_the_placement(mode, oracle, product_lib):
    """cpu_baseline_all_cores pins its threads (placement 1: all allowed CPUs in NUMA-node order, 2: the first NUMA node alone) and
    lets every z-slab be first touched by its thread: same doubles, same time steps as the unpinned and the sequential runs;
    the pinning is undone for the calling thread's process afterwards (threads are pinned one by one, never the process)"""
    import os
    base, ov, nsteps = "mhd_mri_3d", "mesh.nx=8;mesh.ny=12;mesh.nz=16;MRI.amp=0.2", 4
    p = product_lib.params_from_ini(ini(base), ov)
    U0 = product_lib.init_condition(ini(base), ov, p)
    a, da, ta = oracle.run(p, U0, nsteps)
    before = os.sched_getaffinity(0)
    ncpu = oracle.set_thread_placement(mode)
    try:
        assert 1 <= ncpu <= len(before)
        secs, used = oracle.run_mt_scan(p, U0, nsteps, [4, 2], 3)
        b, db, tb = oracle.run_mt(p, U0, nsteps, 5)
    finally:
        assert oracle.set_thread_placement(0) == 0
    assert len(secs) == nsteps and used in (4, 2)
    assert os.sched_getaffinity(0) == before
    assert np.array_equal(da, db) and ta == tb and np.array_equal(interior(a, p), interior(b, p))
