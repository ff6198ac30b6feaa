"""The shearing box at every phase of its shift on the GPU, both libraries: the tiled sweep's shear_save columns and remap, the fused
ghost fill and the device clock's offsets (hip/step_clock.h) where the row offset is at ny - 1, where the fmod(., ylen) wrap falls
between the remap time and the ghost time of one step, where a batch begins on that step, at a shift that is an exact multiple of dy, and
late in the shipped run -- on states that vary at O(1) from row to row, against the oracle: the exact library to the bit, the contracted
one within the stated tolerance (its specific-form errors are printed, and appended to $RGPU_TEST_LOG_DIR/shear_phase_contracted.txt when that is set).
Checks and cases: tests/shear_phase_checks.py; CPU twin: tests/test_shear_phase_emu.py."""
import pytest

import shear_phase_checks as sp

pytestmark = pytest.mark.gpu

IDS = [sp.case_id(c) for c in sp.CASES]
CHECKS = {"fills": sp.check_fills, "single-steps": sp.check_single_steps, "step-loop": sp.check_step_loop, "run-steps": sp.check_run_steps}


def _lib(request, arith):
    return request.getfixturevalue("gpu_lib" if arith == "exact" else "gpu_contracted_lib")


# check, then arith vary fastest: the checks of a case and both libraries follow each other and share the oracle's run
@pytest.mark.parametrize("check", list(CHECKS))
@pytest.mark.parametrize("arith", ["exact", "contracted"])
@pytest.mark.parametrize("case", sp.CASES, ids=IDS)
def test_shear_phase(case, arith, check, oracle, request):
    CHECKS[check](_lib(request, arith), oracle, case, exact=arith == "exact")


@pytest.mark.parametrize("option,value", sp.OPTIONS, ids=["%s=%d" % o for o in sp.OPTIONS])
@pytest.mark.parametrize("case", sp.OPTION_CASES, ids=[sp.case_id(c) for c in sp.OPTION_CASES])
def test_diagnostic_options_keep_the_bits(case, option, value, gpu_lib, oracle):
    sp.check_options(gpu_lib, oracle, case, option, value)
