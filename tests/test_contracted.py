"""The opt-in "contracted arithmetic" variant of the product (ramsesgpu_amd/librgpu_fast.so: the same sources built with FMA
contraction, division within 18 ulp and square root within 1 ulp, see rgpu_arithmetic() in include/rgpu.h) against the reference's golden
fixtures and against the exact library: agreement to round-off -- the stated tolerance, relative L2 < 1e-12 per run
(parity_checks.L2_TOLERANCE; measured worst over the fixtures: 2e-14) -- instead of equal bits."""
import os
import subprocess
import sys

import numpy as np
import pytest

import parity_checks as pc
from conftest import ROOT, golden_cases, ini

pytestmark = pytest.mark.gpu
GOLDEN = sorted(golden_cases())


@pytest.mark.parametrize("name", GOLDEN)
def test_golden_within_tolerance(name, gpu_contracted_lib):
    pc.check_golden_case(gpu_contracted_lib, name, exact=False)


@pytest.mark.parametrize("base,ov,nsteps", [
    ("mhd_mri_3d", "mesh.nx=32;mesh.ny=64;mesh.nz=32", 20),                       # tiled MHD sweep, several tiles and segments
    ("implode3d", "mesh.nx=48;mesh.ny=48;mesh.nz=48;hydro.riemannSolver=hllc", 20),  # tiled hydro sweep
    ("orszag-tang", "mesh.nx=128;mesh.ny=128", 50),
])
def test_contracted_against_exact(base, ov, nsteps, gpu_lib, gpu_contracted_lib):
    from ramsesgpu_amd.solver import Solver, interior
    out, dts = [], []
    for lib in (gpu_lib, gpu_contracted_lib):
        p = lib.params_from_ini(ini(base), ov)
        U0 = lib.init_condition(ini(base), ov, p)
        sv = Solver(p, lib)
        try:
            dts.append(np.array(sv.start(U0, nsteps)))
            out.append(interior(sv.getDataHost(), p).copy())
        finally:
            sv.close()
    err = pc.rel_l2(out[1], out[0])
    assert np.isfinite(out[1]).all() and err < pc.L2_TOLERANCE, "%s: relative L2 %.3e" % (base, err)
    assert np.abs(dts[1] / dts[0] - 1.0).max() < 1e-11
    assert not np.array_equal(out[0], out[1]), "the contracted variant returned the exact library's bits: is it the right build?"


# The bench's launch geometry (tests/test_gpu_parity.py: BENCH_GEOMETRY -- full-width tile rows, several rounds of workgroups,
# sub-segmented last round, XCD sub-bands) for THIS build against the oracle: the same kernel sources, but compiled with the contracted
# arithmetic (RG_ARITH_FAST, -ffp-contract=fast), i.e. other code objects than the ones the exact library's geometry test covers.
BENCH_GEOMETRY = pc.BENCH_GEOMETRY


@pytest.mark.parametrize("base,ov,nsteps", BENCH_GEOMETRY, ids=["%s[%s]" % (b, o) for b, o, _ in BENCH_GEOMETRY])
def test_bench_launch_geometry_within_tolerance(base, ov, nsteps, gpu_contracted_lib, oracle):
    pc.check_run_vs_oracle(gpu_contracted_lib, oracle, base, ov, nsteps, exact=False)


def test_contracted_division_and_sqrt_stay_within_their_stated_ulps(gpu_contracted_lib):
    """the contracted build's rg_div(rg_recip) and rg_sqrt (hip/rg_backend.h, RG_ARITH_FAST) on the operands of
    test_shared_reciprocal_division_and_sqrt_are_ieee, in units in the last place of numpy's IEEE results: within the bounds that
    rg_backend.h and rgpu_arithmetic() (include/rgpu.h) state -- and not IEEE everywhere, or this is not the contracted build"""
    num, den = pc.arith_operands()
    quot, quot2, _, _ = pc.selftest_arith(gpu_contracted_lib, num, den)
    pos = np.abs(num)
    _, _, root, root2 = pc.selftest_arith(gpu_contracted_lib, pos, den)
    dq, dr = pc.ulp_distance(quot, num / den), pc.ulp_distance(root, np.sqrt(pos))
    for name, d in (("rg_div", dq), ("rg_sqrt", dr)):
        print("contracted %s: ulp distance to IEEE on %d operands:" % (name, d.size), {int(k): int(n) for k, n in zip(*np.unique(d, return_counts=True))})
    assert np.array_equal(quot2, num / den) and np.array_equal(root2, np.sqrt(pos)), "the compiler's own division / sqrt is not IEEE"
    assert dq.max() <= CONTRACTED_DIV_ULP, "rg_div: %d ulp" % int(dq.max())
    assert dr.max() <= CONTRACTED_SQRT_ULP, "rg_sqrt: %d ulp" % int(dr.max())
    assert dq.max() > 0 or dr.max() > 0, "IEEE results everywhere: is this the contracted build?"


# measured on MI355X (these operands): quotient {0: 51 %, 1: 36 %, 2: 7.4 %, 3..18: 5 %} ulp -- n * r, r after ONE Newton step on
# v_rcp_f64, whose error it squares; root: correctly rounded on every operand
CONTRACTED_DIV_ULP = 18
CONTRACTED_SQRT_ULP = 1


# ---- the gates that make the tolerance-grade number a conformant one (north_star: "Orszag-Tang L2 error vs euler_cpu < 1e-12") ----
def test_orszag_tang_gate_full_size_within_tolerance(gpu_contracted_lib, oracle):
    """data/orszag-tang.ini as shipped, 512^2 x 50 steps: relative L2 < 1e-12 per variable against the oracle"""
    errs = pc.orszag_tang_gate(gpu_contracted_lib, oracle, exact=False)
    print("Orszag-Tang 512^2 x 50, contracted arithmetic, relative L2 per variable:", {k: "%.2e" % v for k, v in errs.items()})
    assert max(errs.values()) > 0.0, "equal bits: is this the contracted build?"


def test_mri_headline_size_properties_contracted(gpu_contracted_lib):
    pc.mri_headline_size_properties(gpu_contracted_lib)


def test_implode_bench_size_properties_contracted(gpu_contracted_lib):
    pc.implode_bench_size_properties(gpu_contracted_lib)


# Long runs.  Round-off differences are perturbations of the initial value problem and grow at the rate the flow amplifies any
# perturbation (the MRI box is linearly unstable, the implosion and the vortex develop shocks and shear layers).  Measured on
# MI355X (profiles/r03_contracted_long_runs.txt): 4.7e-16 after 400 steps of the MRI box, 2.1e-15 after 300 steps of the
# implosion, 2.1e-15 after 400 steps of Orszag-Tang -- so the long runs are held to the SAME bar as the 50-step gate,
# relative L2 (all variables) < 1e-12 at every checkpoint.
LONG_RUN_TOLERANCE = pc.L2_TOLERANCE
LONG_RUNS = [
    ("mhd_mri_3d", "mesh.nx=24;mesh.ny=48;mesh.nz=24;MRI.amp=0.1", 400),
    ("implode3d", "mesh.nx=40;mesh.ny=40;mesh.nz=40;hydro.riemannSolver=hllc", 300),
    ("orszag-tang", "mesh.nx=96;mesh.ny=96", 400),
]


@pytest.mark.parametrize("base,ov,nsteps", LONG_RUNS, ids=["%s-%d" % (b, n) for b, _, n in LONG_RUNS])
def test_long_runs_within_stated_tolerance(base, ov, nsteps, gpu_contracted_lib, oracle):
    growth = pc.long_run_error_growth(gpu_contracted_lib, oracle, base, ov, nsteps, 100)
    print("long run %s, contracted arithmetic: (step, relative L2, max |dt/dt_ref - 1|) =" % base, ["(%d, %.2e, %.1e)" % g for g in growth])
    out = os.path.join(ROOT, "gpurun_out", "contracted_long_runs.txt")
    try:
        os.makedirs(os.path.dirname(out), exist_ok=True)
        with open(out, "a") as f:
            f.write("%s [%s]: %s\n" % (base, ov, " ".join("step %d L2 %.3e dt %.1e;" % g for g in growth)))
    except OSError:
        pass
    assert growth[0][1] < pc.L2_TOLERANCE, growth
    assert all(g[1] < LONG_RUN_TOLERANCE for g in growth), growth


def test_contracted_slab_driver_equals_the_single_device_run():
    """librgpu_comm_fast.so (one rank, its own z neighbour, halo planes through RCCL) against librgpu_fast.so alone: same
    arithmetic, hence the same bits.  In a subprocess: the two variants export the same symbols, a process holds one."""
    code = r'''
import os, sys
import numpy as np
sys.path.insert(0, %r)
from ramsesgpu_amd import comm as rcomm
from ramsesgpu_amd.solver import Library, Solver, interior, lib_path
L = Library(lib_path("contracted")); assert L.arithmetic == "contracted"
CL = rcomm.load_comm_library(rcomm.comm_lib_path("contracted"))
ini = os.path.join(%r, "configs", "mhd_mri_3d.ini"); ov = "mesh.nx=16;mesh.ny=32;mesh.nz=16"
run = rcomm.CommRun(ini, ov, 0, 1, rcomm.unique_id(CL), library=L, comm_library=CL)
run.init_simulation()
for _ in range(4): run.oneStepIntegration()
a = run.local_interior().copy(); run.close()
p = L.params_from_ini(ini, ov); sv = Solver(p, L); sv.start(L.init_condition(ini, ov, p), 4)
b = interior(sv.getDataHost(), p); sv.close()
assert np.array_equal(a, b), int((a != b).sum())
print("OK")
''' % (ROOT, ROOT)
    env = dict(os.environ); env.pop("RGPU_LIB", None); env.pop("RGPU_ARITH", None)
    out = subprocess.run([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=600)
    assert out.returncode == 0 and "OK" in out.stdout, out.stdout[-2000:]
