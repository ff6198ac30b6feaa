"""The shearing box at every phase of its shift on the test-only host emulation (the flat kernels: shear_remap_cell, shear_ghost_cell,
fill_xy_cell, and the batch logic of the device-side time step with the record formed by step_clock_form) against the oracle, every
double.  Also what needs no product at all: each plant's property and the sensitivity condition from the oracle alone, and the oracle's
Python loop against the reference's own run across the wrap.  Checks and cases: tests/shear_phase_checks.py; GPU twin:
tests/test_shear_phase_gpu.py."""
import pytest

import shear_phase_checks as sp

IDS = [sp.case_id(c) for c in sp.CASES]
CHECKS = {"fills": sp.check_fills, "single-steps": sp.check_single_steps, "step-loop": sp.check_step_loop, "run-steps": sp.check_run_steps}


@pytest.mark.parametrize("case", sp.CASES + sp.OPTION_CASES[1:2], ids=IDS + [sp.case_id(c) for c in sp.OPTION_CASES[1:2]])
def test_plant_property_and_sensitivity_hold_from_the_oracle_alone(case, emu_lib, oracle):
    """(the library only reads the parameter file and writes the initial condition)"""
    R = sp.reference(emu_lib, oracle, case)
    assert len(R.dts) == sp.steps_of(case) and 1 <= R.planted <= len(R.dts) - 3
    assert R.sens >= sp.SENSITIVITY * sp.pc.L2_TOLERANCE
    if case.plant == "last-row":
        assert R.phases[R.planted] == (R.p.ny - 1, 0)


def test_every_plant_and_shape_is_listed():
    assert {c.plant for c in sp.CASES} == set(sp.PLANTS)
    assert {(c.shape, c.family) for c in sp.CASES if c.family != "initial"} == set(sp.STATE_CASES)
    assert {c.shape for c in sp.CASES if c.plant == "late"} == set(sp.SHAPES)


def test_oracle_loop_of_the_fast_case_equals_the_reference_run(emu_lib, oracle):
    sp.check_fast_equals_golden(emu_lib, oracle)


# check varies fastest: the checks of a case follow each other and share the oracle's run
@pytest.mark.parametrize("check", list(CHECKS))
@pytest.mark.parametrize("case", sp.CASES, ids=IDS)
def test_shear_phase(case, check, emu_lib, oracle):
    """(run-steps: rgpu_device_time_step_ready is 1 on the emulation too -- tests/emu/rg_tiled.h: step_clock_supported follows the option,
    and inside a batch the shear remap and the fused ghost fill take their offsets from the record as on the device)"""
    CHECKS[check](emu_lib, oracle, case)


@pytest.mark.parametrize("option,value", sp.OPTIONS, ids=["%s=%d" % o for o in sp.OPTIONS])
@pytest.mark.parametrize("case", sp.OPTION_CASES, ids=[sp.case_id(c) for c in sp.OPTION_CASES])
def test_diagnostic_options_keep_the_bits(case, option, value, emu_lib, oracle):
    sp.check_options(emu_lib, oracle, case, option, value)
