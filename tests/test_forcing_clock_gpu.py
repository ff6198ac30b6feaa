"""Driven turbulence inside the device-clock batches of rgpu_run_steps* (option "forcing_clock"), on the device: the norm of the random
forcing and the mode step of the Ornstein-Uhlenbeck process formed by kernels that read the record, the last kick of a step carrying
the CFL scan through rg_reduce_max.  The yardstick is the literal loop of the same library (tests/forcing_clock_checks.py): bit for
bit on the exact library, within the contracted gate on the contracted one."""
import pytest

import forcing_clock_checks as fc

pytestmark = pytest.mark.gpu

PLANTS = ("first", "last", "seam-x-15", "seam-x-16", "seam-y-lo", "seam-y-hi", "z-high")
PLANT_CASES = [(case, name) for case in fc.FOUR for name in PLANTS]


@pytest.fixture(params=["exact", "contracted"])
def lib_exact(request):
    """(the library, compare bit for bit)"""
    return (request.getfixturevalue("gpu_lib"), True) if request.param == "exact" else (request.getfixturevalue("gpu_contracted_lib"), False)


def _plant_name(lib, case, name):
    if not name.startswith("seam-y"):
        return name
    sy = fc.cp.tile_shape(fc.setup(lib, case).p)[3]
    return "seam-y-%d" % (sy[0] if name.endswith("lo") else sy[1])


@pytest.mark.parametrize("case", sorted(fc.CASES))
def test_run_steps_is_the_literal_loop_and_a_batch(case, lib_exact):
    fc.check_same_run(lib_exact[0], case, exact=lib_exact[1])


@pytest.mark.parametrize("case", ["hydro", "hydro_ou", "mhd_ou", "hydro_both"])
def test_end_time_inside_a_batch_rewinds_the_generator(case, lib_exact):
    fc.check_end_time(lib_exact[0], case, exact=lib_exact[1])


def test_more_steps_than_a_batch_holds(lib_exact):
    fc.check_two_batches(lib_exact[0], exact=lib_exact[1])


@pytest.mark.parametrize("case,name", PLANT_CASES, ids=["%s-%s" % cn for cn in PLANT_CASES])
def test_the_scan_in_the_last_kick_sees_every_cell(case, name, lib_exact, oracle):
    fc.check_planted(lib_exact[0], oracle, case, _plant_name(lib_exact[0], case, name), exact=lib_exact[1])


def test_spectra_ride_along(lib_exact):
    fc.check_spectra(lib_exact[0], exact=lib_exact[1])


def test_pdfs_ride_along(lib_exact):
    fc.check_pdfs(lib_exact[0], exact=lib_exact[1])


@pytest.mark.parametrize("case", fc.FOUR)
def test_batched_steps_against_the_oracle(case, lib_exact, oracle):
    fc.check_against_oracle(lib_exact[0], oracle, case, contracted=not lib_exact[1])


@pytest.mark.parametrize("case", ["hydro", "mhd_ou"])
def test_the_external_clock_still_refuses_a_forced_context(case, gpu_lib):
    fc.check_unchanged_surfaces(gpu_lib, case)


@pytest.mark.parametrize("case,extra", [("hydro", "hydro.nu=0.001"), ("hydro_ou", "gravity.static=yes;gravity.static_field_x=0.05"), ("mhd_ou", "MHD.eta=0.0001")])
def test_viscosity_resistivity_and_gravity_keep_the_literal_loop(case, extra, gpu_lib):
    fc.check_stays_literal(gpu_lib, case, extra)
