"""The fused CFL scan of the step kernels on the GPU, both libraries, with the fastest cell of the box planted where only the tiled
kernels have a mask, a seam or a slot to get wrong (tests/cfl_plant_checks.py; CPU twin: tests/test_cfl_plant_emu.py).

  shapes     STRESS_SHAPES of tests/test_stress_states.py (tile seams, MhLastX, copied periodic layers, partial last tiles) -- without
             the jet, whose inflow speed sets the time step whatever the box holds (the generator refuses it) -- plus face-type variants
             so that every step family meets periodic, reflecting and outflow faces, the shearing box and the rotating periodic box at
             its high faces, and configurations that do not fuse (the scan kernel is then what is tested)
  plants     low / high: the faces and the corner line of that side; seams: the four cells around the first tile corner, the first cell
             of the last (partial) tile; z-segment seams under the launch option zseg = 3
  slot wrap  more tiles than RG_DT_SLOTS: (blockIdx.x * waves + wave) & (RG_DT_SLOTS - 1) and the flat (idx >> 6) & 1023
  ensembles  4 members with different planted cells (per-member slot offsets and clock fold), one parameter scan
  slab       the world-1 schedule of tests/slab_harness.py from planted states, both overlap settings"""
import pytest

import cfl_plant_checks as cp
from conftest import ini
from test_ensemble_gpu import fused_expected
from test_stress_states import STRESS_SHAPES

pytestmark = pytest.mark.gpu

SHAPES = [s for s in STRESS_SHAPES if s[0] != "jet2d_cpu"] + [
    # ---- face-type variants ----
    ("orszag-tang3d", "mesh.nx=33;mesh.ny=17;mesh.nz=20;" + cp.REFLECT3),
    ("orszag-tang3d", "mesh.nx=32;mesh.ny=24;mesh.nz=14;" + cp.OUTFLOW3),
    ("mhd_mri_3d", "mesh.nx=31;mesh.ny=23;mesh.nz=26;" + cp.OPEN_Z),                  # shearing box, open z: not fused
    ("mhd_mri_3d", "mesh.nx=20;mesh.ny=18;mesh.nz=10;gravity.static=yes"),           # per-cell gravity field: flat kernels, not fused
    ("orszag-tang3d", "mesh.nx=20;mesh.ny=24;mesh.nz=10;hydro.nu=0.005"),            # not fused: viscous stage
    ("implode3d", "mesh.nx=33;mesh.ny=17;mesh.nz=30;" + cp.OUTFLOW3),
    ("implode3d", "mesh.nx=20;mesh.ny=36;mesh.nz=14;" + cp.PERIODIC3),
    ("orszag-tang", "mesh.nx=46;mesh.ny=23;" + cp.REFLECT2),                          # flat 2D MHD kernels
    ("orszag-tang", "mesh.nx=46;mesh.ny=23;" + cp.OUTFLOW2),
    ("orszag-tang", "mesh.nx=46;mesh.ny=23;MHD.eta=0.01"),                            # not fused: resistive stage
    ("implode3d", "mesh.nx=33;mesh.ny=17;mesh.nz=1;" + cp.OUTFLOW2),
    ("kelvin_helmholtz_gpu_2d", "mesh.nx=40;mesh.ny=24;hydro.nu=0.01"),              # not fused: viscous stage
    ("Keplerian_disk2d", "mesh.nx=40;mesh.ny=24"),                                    # per-cell gravity field
]
CASES = cp.grouped(SHAPES)
ZSEG_CASES = [(3, "mhd_mri_3d", "mesh.nx=31;mesh.ny=23;mesh.nz=26"),
              (3, "implode3d", "mesh.nx=33;mesh.ny=17;mesh.nz=30;hydro.riemannSolver=hllc;hydro.slope_type=2.0")]


def _lib(request, arith):
    return request.getfixturevalue("gpu_lib" if arith == "exact" else "gpu_contracted_lib")


# arith varies fastest: the exact and contracted runs of a case follow each other and share the oracle's runs
@pytest.mark.parametrize("arith", ["exact", "contracted"])
@pytest.mark.parametrize("base,ov,group", CASES, ids=cp.case_ids(CASES))
def test_planted_fastest_cell_sets_the_next_dt(base, ov, group, arith, oracle, request):
    cp.check_planted_case(_lib(request, arith), oracle, base, ov, group, exact=arith == "exact")


@pytest.mark.parametrize("arith", ["exact", "contracted"])
@pytest.mark.parametrize("base,ov", cp.WRAP_SHAPES, ids=["%s[%s]" % c for c in cp.WRAP_SHAPES])
def test_planted_cell_in_the_first_and_last_tile_of_a_box_with_more_tiles_than_slots(base, ov, arith, oracle, request):
    lib = _lib(request, arith)
    p = lib.params_from_ini(ini(base), ov)
    assert cp.wrap_tiles(p) > (512 if p.mhdEnabled else 256)
    cp.check_planted_dt(lib, oracle, base, ov, cp.wrap_plants(p), exact=arith == "exact")


@pytest.mark.parametrize("arith", ["exact", "contracted"])
@pytest.mark.parametrize("zseg,base,ov", ZSEG_CASES, ids=["zseg=%d-%s[%s]" % c for c in ZSEG_CASES])
def test_planted_cell_beside_a_z_segment_start(zseg, base, ov, arith, oracle, request):
    cp.check_planted_case(_lib(request, arith), oracle, base, ov, "seams", exact=arith == "exact", zseg=zseg)


@pytest.mark.parametrize("arith", ["exact", "contracted"])
@pytest.mark.parametrize("base,ov", cp.ENSEMBLE_SHAPES, ids=[c[0] for c in cp.ENSEMBLE_SHAPES])
def test_ensemble_members_with_different_planted_cells(base, ov, arith, oracle, request):
    lib = _lib(request, arith)
    fused = cp.check_planted_ensemble(lib, oracle, base, ov, exact=arith == "exact")
    if fused_expected(lib):
        assert fused == cp.ENSEMBLE_STEPS - 1   # the first step of a run is the plain one


@pytest.mark.parametrize("arith", ["exact", "contracted"])
def test_parameter_scan_with_different_planted_cells(arith, oracle, request):
    lib = _lib(request, arith)
    fused = cp.check_planted_scan(lib, oracle, *cp.ENSEMBLE_SHAPES[1], exact=arith == "exact")
    if fused_expected(lib):
        assert fused == cp.ENSEMBLE_STEPS - 1


@pytest.mark.parametrize("overlap", [True, False], ids=["overlap", "serial"])
@pytest.mark.parametrize("base,ov", cp.SLAB_SHAPES, ids=[c[0] for c in cp.SLAB_SHAPES])
def test_slab_schedule_from_planted_states(base, ov, overlap, gpu_lib, oracle):
    cp.check_planted_slab(gpu_lib, oracle, base, ov, overlap)
