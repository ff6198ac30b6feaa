"""Driven turbulence inside the device-clock batches of rgpu_run_steps* (option "forcing_clock"), on the CPU emulation: the forcing functors
of csrc/launchers.h (K_forcing_norm, K_ou_mode_step, the kicks that carry the CFL scan) run there as host loops, the record resolved by
value.  Every comparison is bit for bit against the literal loop of the same library (tests/forcing_clock_checks.py)."""
import ctypes as C

import numpy as np
import pytest

import forcing_clock_checks as fc
from ramsesgpu_amd.solver import interior

PLANT_CASES = [(case, name) for case in fc.FOUR for name in ("first", "last", "seam-x-15", "seam-x-16", "seam-y-lo", "seam-y-hi", "z-high")]


def _plant_name(lib, case, name):
    if not name.startswith("seam-y"):
        return name
    sy = fc.cp.tile_shape(fc.setup(lib, case).p)[3]
    return "seam-y-%d" % (sy[0] if name.endswith("lo") else sy[1])


def test_the_option_and_the_counter_exist(emu_lib):
    assert emu_lib.get_option("forcing_clock") == 1
    assert emu_lib.set_option("forcing_clock", 0) == 1 and emu_lib.get_option("forcing_clock") == 0
    assert emu_lib.set_option("forcing_clock", 1) == 0
    assert emu_lib.lib.rgpu_forcing_batch_steps(None) == 0


@pytest.mark.parametrize("case", sorted(fc.CASES))
def test_run_steps_is_the_literal_loop_and_a_batch(case, emu_lib):
    fc.check_same_run(emu_lib, case)


@pytest.mark.parametrize("case", ["hydro", "hydro_ou", "mhd_ou", "hydro_both"])
def test_end_time_inside_a_batch_rewinds_the_generator(case, emu_lib):
    fc.check_end_time(emu_lib, case)


def test_more_steps_than_a_batch_holds(emu_lib):
    fc.check_two_batches(emu_lib)


@pytest.mark.parametrize("case,name", PLANT_CASES, ids=["%s-%s" % cn for cn in PLANT_CASES])
def test_the_scan_in_the_last_kick_sees_every_cell(case, name, emu_lib, oracle):
    fc.check_planted(emu_lib, oracle, case, _plant_name(emu_lib, case, name))


def test_spectra_ride_along(emu_lib):
    fc.check_spectra(emu_lib)


def test_pdfs_ride_along(emu_lib):
    fc.check_pdfs(emu_lib)


@pytest.mark.parametrize("case", fc.FOUR)
def test_batched_steps_against_the_oracle(case, emu_lib, oracle):
    fc.check_against_oracle(emu_lib, oracle, case)


@pytest.mark.parametrize("case", ["hydro", "mhd_ou"])
def test_the_external_clock_still_refuses_a_forced_context(case, emu_lib):
    fc.check_unchanged_surfaces(emu_lib, case)


@pytest.mark.parametrize("case,extra", [("hydro", "hydro.nu=0.001"), ("hydro_ou", "hydro.nu=0.001"), ("hydro_ou", "gravity.static=yes;gravity.static_field_x=0.05"),
                                        ("mhd_ou", "MHD.eta=0.0001")])
def test_viscosity_resistivity_and_gravity_keep_the_literal_loop(case, extra, emu_lib):
    fc.check_stays_literal(emu_lib, case, extra)


def test_run_steps_history_keeps_the_literal_loop_on_a_forced_context(emu_lib):
    """the history a batch can sample is the MRI row; the turbulence runs' history stays with the literal loop, whatever the state's record says"""
    s = fc.setup(emu_lib, "mhd_ou")
    sv = fc.fresh(emu_lib, s)
    try:
        assert sv.run_steps(2) == 2 and sv.forcing_batch_steps() == 2
        done = sv.run_steps_history(3, 1e30)[0]
        assert done == 3 and sv.forcing_batch_steps() == 2 and emu_lib.lib.rgpu_history_batch_heads(sv.ctx) == 0
        got = fc.snapshot(emu_lib, sv, [])
    finally:
        sv.close()
    ref = fc.run_literal(emu_lib, s, 5)
    assert got.t == ref.t and got.checksum == ref.checksum and np.array_equal(got.ou, ref.ou)


def test_restart_carries_the_process_of_a_batch(emu_lib):
    """4 batched steps, state and rgpu_ou_forcing_get_state carried to a fresh context, 4 more == 8 steps in one run: what the batch left
    in the host's process is what a restart file needs, and set_state reaches the tables the next batch reads"""
    s = fc.setup(emu_lib, "hydro_ou")
    whole, _, done = fc.run_batched(emu_lib, s, [8])
    assert done == [8]
    first, sv, done = fc.run_batched(emu_lib, s, [4], keep=True)
    try:
        U = sv.getDataHost().copy()
    finally:
        sv.close()
    assert done == [4] and first.dts == whole.dts[:4]
    sv = fc.fresh(emu_lib, s, U0=U)
    try:
        assert sv.run_steps(1) == 1       # (a batch of the fresh process first: its tables are on the "device" when set_state comes)
        sv.start(U, 0)
        sv.totalTime = first.t
        assert emu_lib.lib.rgpu_ou_forcing_set_state(sv.ctx, first.ou.ctypes.data_as(C.POINTER(C.c_double))) == 0
        assert sv.run_steps(4) == 4 and sv.forcing_batch_steps() == 5
        assert list(sv.dt_log) == whole.dts[4:] and sv.totalTime == whole.t
        assert np.array_equal(interior(sv.getDataHost(), s.p), whole.state)
        assert np.array_equal(fc.ou_state(emu_lib, sv), whole.ou)
    finally:
        sv.close()
