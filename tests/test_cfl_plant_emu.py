"""The fused CFL scan with the fastest cell planted on faces, corner lines and seams, on the test-only host emulation (the flat kernels:
hydro_update_cell, mhd_update2d_cell, mhd_update3d_apply and the scan kernel where a configuration does not fuse) against the oracle.
Checks and shapes: tests/cfl_plant_checks.py; GPU twin: tests/test_cfl_plant_gpu.py."""
import pytest

import cfl_plant_checks as cp
import parity_checks as pc
from conftest import ini

CASES = cp.grouped(cp.EMU_SHAPES)


@pytest.mark.parametrize("base,ov,group", CASES, ids=cp.case_ids(CASES))
def test_planted_fastest_cell_sets_the_next_dt(base, ov, group, emu_lib, oracle):
    cp.check_planted_case(emu_lib, oracle, base, ov, group)


@pytest.mark.parametrize("base,ov", cp.WRAP_SHAPES_FLAT, ids=["%s[%s]" % c for c in cp.WRAP_SHAPES_FLAT])
def test_planted_cell_in_the_first_and_last_tile_of_a_box_with_more_tiles_than_slots(base, ov, emu_lib, oracle):
    p = emu_lib.params_from_ini(ini(base), ov)
    assert (p.nx + 2 * p.ghostWidth) * (p.ny + 2 * p.ghostWidth) > 65536 or cp.wrap_tiles(p) > 512   # (the flat slot index wraps / the tiled one)
    cp.check_planted_dt(emu_lib, oracle, base, ov, cp.wrap_plants(p))


@pytest.mark.parametrize("zseg,base,ov", [(3, "orszag-tang3d", "mesh.nx=20;mesh.ny=18;mesh.nz=10"), (3, "implode3d", "mesh.nx=20;mesh.ny=18;mesh.nz=10")],
                         ids=["mhd3d", "hydro3d"])
def test_planted_cell_beside_a_z_segment_start(zseg, base, ov, emu_lib, oracle):
    """(the emulation has no z segments: the planes alone)"""
    cp.check_planted_case(emu_lib, oracle, base, ov, "seams", zseg=zseg)


@pytest.mark.parametrize("base,ov", cp.ENSEMBLE_SHAPES, ids=[c[0] for c in cp.ENSEMBLE_SHAPES])
def test_ensemble_members_with_different_planted_cells(base, ov, emu_lib, oracle):
    assert cp.check_planted_ensemble(emu_lib, oracle, base, ov) == 0   # the emulation steps member by member


def test_parameter_scan_with_different_planted_cells(emu_lib, oracle):
    cp.check_planted_scan(emu_lib, oracle, *cp.ENSEMBLE_SHAPES[1])


def test_expect_fused_agrees_with_the_bookkeeping_table(emu_lib):
    """cfl_plant_checks.expect_fused restates the rules behind the `scan` column of parity_checks.FUSED_BOOKKEEPING"""
    for name, base, ov, scan, _, _ in pc.FUSED_BOOKKEEPING:
        assert cp.expect_fused(emu_lib.params_from_ini(ini(base), ov)) == scan, name


def test_both_paths_are_taken(product_lib):
    """the shapes hold configurations that fuse and ones that do not (decided from the parameter sets alone)"""
    kinds = {cp.expect_fused(product_lib.params_from_ini(ini(b), o)) for b, o in cp.EMU_SHAPES}
    assert kinds == {True, False}
