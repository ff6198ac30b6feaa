"""The viscous / resistive stage on rough states through the TEST-ONLY host emulation of the device sources (tests/dissipative_checks.py):
the CPU twin of tests/test_dissipative_gpu.py.  Same case lists, the emulation build to the bit; the non-vacuity assertion of the rough
runs (the stage moves the state by a relative L2 >= 1e-4) is made here before anything runs on a GPU; the two properties are checked on
the oracle's own output too, against the floor alone."""
import pytest

import dissipative_checks as dc


@pytest.mark.parametrize("base,ov", dc.ROUGH_RUNS, ids=dc.ROUGH_IDS)
def test_three_steps_on_a_random_state(base, ov, emu_lib, oracle):
    dc.check_rough_run(emu_lib, oracle, base, ov)


@pytest.mark.parametrize("base,ov,state", dc.STAGE_CASES, ids=dc.STAGE_IDS)
def test_stage_alone_equals_the_oracle(base, ov, state, emu_lib, oracle):
    dc.check_stage_alone(emu_lib, oracle, base, ov, state)
    # the contracted library's bar, on a library whose doubles are equal: every error 0
    errs = dc.check_stage_alone(emu_lib, oracle, base, ov, state, exact=False)
    assert set(errs.values()) == {0.0}, errs


@pytest.mark.parametrize("base,ov,state", dc.PROPERTY_CASES, ids=dc.PROPERTY_IDS)
def test_stage_keeps_div_b_and_the_totals(base, ov, state, emu_lib, oracle):
    """the oracle's own change of div B and of the totals stays under the floor alone (64 eps x the sum of |term|): the stage is in CT and
    flux form whatever its fluxes are -- this is what no kernel-vs-oracle comparison can show; then the emulation build within the bound"""
    vals = dc.oracle_property_values(emu_lib, oracle, base, ov, state)
    assert vals
    print("oracle, %s [%s] %s: %s" % (base, ov, state, "; ".join("%s %.2e (floor %.2e)" % ((k,) + v) for k, v in vals.items())))
    assert all(change <= floor for change, floor in vals.values()), vals
    dc.check_stage_properties(emu_lib, oracle, base, ov, state)
