"""The LDS-tiled step kernels (hip/tiled_mhd.h, hip/tiled_hydro.h, hip/tiled_mhd2d.h, hip/tiled_hydro2d.h) on stress states
(parity_checks.stress_state: rough, contrast, low beta, floored, piecewise-uniform) at shapes that put those states on every tile seam,
the MhLastX column, z-segment starts and partial last tiles.  One godunov_unsplit per case against the oracle: the exact library
(librgpu.so) to the bit, the contracted one (librgpu_fast.so) within the stated tolerance per variable in specific form
(parity_checks.assert_close_specific).  The emulation build runs the same families on the small RANDOM_STEPS boxes
(tests/test_kernels_emu.py), so a failure here points at the tiled code.

Tile constants the comments refer to:
  3D MHD sweep   MhMain 16 x 8 cells (face columns gw .. nx + gw, i.e. nx + 1 of them; face rows likewise ny + 1); the x / y layer
                 nx + gw / ny + gw is copied from its periodic image when nx % 16 == 0 / ny % 8 == 0 and the face is periodic; with
                 nx % 16 == 0 and no image the last face column goes to MhLastX (2 x 32); z segments of >= 8 planes (tile_grid_plan)
  3D hydro sweep 16 x 16 cells, z segments of >= 12 planes
  2D MHD step    16 x 8 problem cells per tile, 15 x 7 finished; nx + 1 by ny + 1 cells to finish (the CT layer included)
  2D hydro step  16 x 16 cells"""
import pytest

import parity_checks as pc

pytestmark = pytest.mark.gpu

OPEN_XY = ";mesh.boundary_xmin=2;mesh.boundary_xmax=2;mesh.boundary_ymin=2;mesh.boundary_ymax=2"

STRESS_SHAPES = [
    # ---- 3D MHD sweep ----
    # 34 face columns = 2 tiles + one of 2 columns, 18 face rows = 2 tiles + one of 2 rows (no periodic layer copied: 33, 17 not tile
    # multiples); 20 planes: up to 2 z segments
    ("orszag-tang3d", "mesh.nx=33;mesh.ny=17;mesh.nz=20"),
    # periodic x and y layers copied from their images (32 % 16 == 0, 24 % 8 == 0): 2 x 3 full tiles, no MhLastX
    ("orszag-tang3d", "mesh.nx=32;mesh.ny=24;mesh.nz=14"),
    # open x and y faces: no image, 32 % 16 == 0 -> the last face column in MhLastX; 33 face rows: a last tile row with one face row
    ("orszag-tang3d", "mesh.nx=32;mesh.ny=32;mesh.nz=12" + OPEN_XY),
    # shearing box: x faces have no periodic image -> MhLastX; periodic y, 40 % 8 == 0: y layer copied; the specialised kernel (spec 1)
    ("mhd_mri_3d", "mesh.nx=48;mesh.ny=40;mesh.nz=12"),
    # 26 planes: up to 3 z segments of >= 8 planes (the zseg cases below force them); 32 face columns = 2 tiles, 24 face rows = 3 tiles, nothing copied (31, 23 odd)
    ("mhd_mri_3d", "mesh.nx=31;mesh.ny=23;mesh.nz=26"),
    # rotating frame without shearing box (periodic x): Coriolis terms in the trace; 35 face columns = 2 tiles + one of 3
    ("orszag-tang3d", "mesh.nx=34;mesh.ny=18;mesh.nz=13;MHD.omega0=0.3"),
    # the LLF / HLLF EMF solvers in the sweep: partial x (21 face columns) and y (25 face rows) tiles; 18 x 10 = 16 + 2 by 8 + 2
    ("orszag-tang3d", "mesh.nx=20;mesh.ny=24;mesh.nz=10;MHD.magRiemannSolver=llf"),
    ("orszag-tang3d", "mesh.nx=17;mesh.ny=9;mesh.nz=9;MHD.magRiemannSolver=hllf;hydro.slope_type=3.0"),
    # ---- 3D hydro sweep (16 x 16 cell tiles) ----
    # 33 = 2 x 16 + 1, 17 = 16 + 1: one-cell last tiles in x and y; 30 planes: 2 z segments of >= 12
    ("implode3d", "mesh.nx=33;mesh.ny=17;mesh.nz=30;hydro.riemannSolver=hllc;hydro.slope_type=2.0"),
    # 47 = 2 x 16 + 15, 49 = 3 x 16 + 1; 25 planes: 2 z segments; the approx (iterative) solver, slope 1
    ("implode3d", "mesh.nx=47;mesh.ny=49;mesh.nz=25;hydro.riemannSolver=approx;hydro.slope_type=1.0"),
    # HLL: 20 = 16 + 4, 36 = 2 x 16 + 4
    ("implode3d", "mesh.nx=20;mesh.ny=36;mesh.nz=14;hydro.riemannSolver=hll"),
    # uniform gravity inside the sweep; 33 x 17 partial tiles, 26 planes: 2 z segments, reflecting z faces
    ("rayleigh_taylor_gpu_3d", "mesh.nx=33;mesh.ny=17;mesh.nz=26"),
    # ---- 2D MHD step (16 x 8 problem cells, 15 x 7 finished) ----
    # 47 x 24 cells to finish = 3 x 15 + 2 by 3 x 7 + 3: partial last tiles in x and y
    ("orszag-tang", "mesh.nx=46;mesh.ny=23"),
    # 45 x 21 cells to finish = 3 x 15 by 3 x 7 exactly: every tile full
    ("orszag-tang", "mesh.nx=44;mesh.ny=20"),
    # rotating frame (the 2D branch of the Coriolis trace; the step fills the output's ghosts): 37 x 30 = 2 x 15 + 7 by 4 x 7 + 2
    ("orszag-tang", "mesh.nx=36;mesh.ny=29;MHD.omega0=0.4"),
    # Neumann faces: the tiled kernel; 33 x 18 = 2 x 15 + 3 by 2 x 7 + 4
    ("mhd_BrioWu", "mesh.nx=32;mesh.ny=17"),
    # one reflecting face: the flat kernels (not tiled), so the GPU checks them on these states too
    ("mhd_BrioWu", "mesh.nx=32;mesh.ny=17;mesh.boundary_xmin=1"),
    # ---- 2D hydro step (16 x 16 cells) ----
    # 33 = 2 x 16 + 1, 17 = 16 + 1: one-cell last tiles; HLLC
    ("implode3d", "mesh.nx=33;mesh.ny=17;mesh.nz=1;hydro.riemannSolver=hllc"),
    # periodic: the step writes the output's ghost images; 40 = 2 x 16 + 8, 24 = 16 + 8
    ("kelvin_helmholtz_gpu_2d", "mesh.nx=40;mesh.ny=24"),
    # inflow faces (jet), approx solver: 36 = 2 x 16 + 4, 50 = 3 x 16 + 2
    ("jet2d_cpu", "mesh.nx=36;mesh.ny=50;jet.ijet=5;jet.offsetJet=4"),
]

STRESS_CASES = pc.stress_cases(STRESS_SHAPES)

# launch options through rgpu_set_option (read at rgpu_create), the old value restored afterwards
STRESS_OPTION_CASES = (
    [("zseg", z, "mhd_mri_3d", "mesh.nx=31;mesh.ny=23;mesh.nz=26", "contrast") for z in (1, 3, 7)]              # z-segment starts every
    + [("zseg", z, "implode3d", "mesh.nx=33;mesh.ny=17;mesh.nz=30;hydro.riemannSolver=hllc;hydro.slope_type=2.0", "contrast")   # 1 / 3 / 7
       for z in (1, 3, 7)]                                                                                       # planes
    + [("spec", 0, "mhd_mri_3d", "mesh.nx=48;mesh.ny=40;mesh.nz=12", "floor"),                                # generic kernels: the four
       ("spec", 0, "implode3d", "mesh.nx=33;mesh.ny=17;mesh.nz=30;hydro.riemannSolver=hllc;hydro.slope_type=2.0", "floor"),   # families
       ("spec", 0, "orszag-tang", "mesh.nx=46;mesh.ny=23", "floor"),
       ("spec", 0, "implode3d", "mesh.nx=33;mesh.ny=17;mesh.nz=1;hydro.riemannSolver=hllc", "floor"),
       # "xcd_sub" is read by the flat kernels' launch_planes calls alone: this context runs the tiled sweep (MhLastX of the shearing box
       # included), which ignores it, unless the process runs under RGPU_TILED=0 -- then: XCD-ordered 2048-cell sub-bands on a >= 200^2
       # plane.  The option on the device by default: tests/test_flat_path_gpu.py
       ("xcd_sub", 2048, "mhd_mri_3d", "mesh.nx=224;mesh.ny=208;mesh.nz=8", "contrast")])


def _lib(request, arith):
    return request.getfixturevalue("gpu_lib" if arith == "exact" else "gpu_contracted_lib")


def _record(arith, base, ov, family, errs):
    """print the contracted library's specific-form errors (pytest -s shows them)"""
    if errs is None:
        return
    print("contracted, specific-form relative L2: %s %s [%s]: %s" % (family, base, ov, " ".join("%s %.2e" % kv for kv in errs.items())))


# arith varies fastest: the exact and contracted runs of a case follow each other and share the oracle's step
@pytest.mark.parametrize("arith", ["exact", "contracted"])
@pytest.mark.parametrize("base,ov,family", STRESS_CASES, ids=["%s[%s]-%s" % c for c in STRESS_CASES])
def test_single_step_on_stress_state(base, ov, family, arith, oracle, request):
    lib = _lib(request, arith)
    assert family in pc.stress_families(lib.params_from_ini(pc.ini(base), ov))
    errs = pc.check_single_step_stress(lib, oracle, base, ov, family, exact=arith == "exact")
    _record(arith, base, ov, family, errs)


@pytest.mark.parametrize("arith", ["exact", "contracted"])
@pytest.mark.parametrize("option,value,base,ov,family", STRESS_OPTION_CASES, ids=["%s=%d-%s[%s]-%s" % c for c in STRESS_OPTION_CASES])
def test_stress_state_with_launch_option(option, value, base, ov, family, arith, oracle, request):
    lib = _lib(request, arith)
    old = lib.set_option(option, value)
    try:
        errs = pc.check_single_step_stress(lib, oracle, base, ov, family, exact=arith == "exact")
    finally:
        lib.set_option(option, old)
    _record(arith, base, ov + ";%s=%d" % (option, value), family, errs)


@pytest.mark.parametrize("base,ov", [("mhd_mri_3d", "mesh.nx=16;mesh.ny=24;mesh.nz=44"),
                                     ("implode3d", "mesh.nx=24;mesh.ny=24;mesh.nz=30")], ids=["mri", "implode3d"])
def test_step_core_in_plane_pieces_on_contrast_state(base, ov, gpu_lib, oracle):
    """the slab driver's plane ranges (segment starts a multi-GPU run hits) on a contrast state: pieces == whole call == oracle"""
    pc.check_core_plane_pieces(gpu_lib, base, ov, state="contrast", oracle=oracle)
