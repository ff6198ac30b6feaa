"""The viscous / resistive stage (csrc/kernels_dissipative.h, dissipative_nd in csrc/api/step_core.h) on the GPU, both libraries, on rough states
(tests/dissipative_checks.py; CPU twin: tests/test_dissipative_emu.py).

  three steps on one context   random state (seed 5, Mach 1), the stage behind the tile shapes of tests/test_stress_states.py; with the
                               stage the step takes another route: no fused CFL scan, stale ghost images of the 2D kernels, the stage's
                               own ghost fill (shear remap on the rotating path), and steps 2 and 3 find the scratch arrays used.
                               librgpu.so: every interior double and every dt equal to the oracle's.  librgpu_fast.so: the first step
                               through godunov_unsplit within parity_checks.assert_close_specific.
  the stage alone              rgpu_step_dissipative against orc_dissipative_stage on the same ghost-filled array at a diffusion number of
                               0.1, random and contrast states; compared over the cells the reference's loops write, the rest untouched.
  two properties               (contracted library; the exact one equals the oracle, whose own values the CPU twin checks) the resistive CT
                               update keeps the per-cell div B, the flux form keeps the totals of a fully periodic box.  Bound: 4 x the
                               oracle's own change on the same input + 64 eps x the sum of |term|.

The oracle's own values at a diffusion number of 0.1 (what the bounds are four times of; the floor in brackets), random / contrast state:
  max |change of div B| per cell   orszag-tang3d 33x17x20 V R   2.1e-14 (1.2e-12) / 5.7e-14 (3.1e-12)
                                   orszag-tang3d 32x32x12 R OPEN 2.8e-14 (1.4e-12) / 5.7e-14 (3.4e-12)
                                   orszag-tang 46x23 V R         2.8e-14 (1.3e-12) / 5.7e-14 (3.0e-12)
  |change of a total|, summed exactly: 0 for most variables (the change is below one ulp of the total); the largest
                                   orszag-tang3d 33x17x20 V R   mx 1.4e-14 (1.8e-10) / my 1.5e-11 (6.6e-8)
                                   orszag-tang 46x23 V R         0 / 0 (floors 1.7e-11 .. 6.7e-9)
                                   kelvin_helmholtz 40x24 V      mx 3.6e-15 (1.4e-11) / mx 3.6e-12 (5.4e-9)
                                   orszag-tang3d 33x17x20 V      my 1.4e-14 (1.7e-10) / mx 7.3e-12 (6.5e-8); energy 0 (6.6e-10 / 4.3e-7)
With eta > 0 the total energy is no invariant of the reference's scheme (dissipative_checks.totals_change) and is left out.

Measured on MI355X, librgpu_fast.so (specific-form relative L2 per variable, tolerance 1e-12): first step of the fourteen runs <= 3.0e-16
(mx of the 2D hydro boxes the largest); the stage alone <= 9.3e-17 in the field, <= 2.4e-17 in the energy, density and momenta equal to
the bit; the changes of div B and of the totals equal the oracle's values above to the printed digits.
"""
import pytest

import dissipative_checks as dc

pytestmark = pytest.mark.gpu


def _lib(request, arith):
    return request.getfixturevalue("gpu_lib" if arith == "exact" else "gpu_contracted_lib")


# arith varies fastest: the exact and contracted runs of a case follow each other and share the oracle's run
@pytest.mark.parametrize("arith", ["exact", "contracted"])
@pytest.mark.parametrize("base,ov", dc.ROUGH_RUNS, ids=dc.ROUGH_IDS)
def test_three_steps_on_a_random_state(base, ov, arith, oracle, request):
    errs = dc.check_rough_run(_lib(request, arith), oracle, base, ov, exact=arith == "exact")
    dc.record("%s [%s] first step, random state" % (base, ov), errs)


@pytest.mark.parametrize("arith", ["exact", "contracted"])
@pytest.mark.parametrize("base,ov,state", dc.STAGE_CASES, ids=dc.STAGE_IDS)
def test_stage_alone_equals_the_oracle(base, ov, state, arith, oracle, request):
    errs = dc.check_stage_alone(_lib(request, arith), oracle, base, ov, state, exact=arith == "exact")
    dc.record("%s [%s] stage alone, %s state" % (base, ov, state), errs)


@pytest.mark.parametrize("base,ov,state", dc.PROPERTY_CASES, ids=dc.PROPERTY_IDS)
def test_stage_keeps_div_b_and_the_totals(base, ov, state, gpu_contracted_lib, oracle):
    dc.check_stage_properties(gpu_contracted_lib, oracle, base, ov, state)
