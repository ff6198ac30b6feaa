"""What the forcing kernels of the device-clock batches (csrc/launchers.h, namespace monitored_run) need from the register file, in both
libraries: the compiler's kernel-resource-usage remarks of the device compile that produced the shipped libraries
(tests/test_kernel_resources.py).  They stream the state once per step: a vector register spilled to scratch would add memory traffic
per cell, and rg_reduce_max sizes its grid for eight resident workgroups of 256 threads per CU, eight waves per SIMD -- the kicks
that carry the CFL scan (31 cos, then hydro_invdt_cell / mhd_invdt_cell) must leave room for at least half of that."""
import pytest

from test_kernel_resources import pick, resources


@pytest.fixture(scope="module", params=["librgpu.so", "librgpu_fast.so"])
def lib_resources(request, product_lib, contracted_lib):
    return request.param, resources(request.param)


KERNELS = ("monitored_run::K_forcing_norm", "monitored_run::K_ou_mode_step", "monitored_run::K_add_forcing_dev", "monitored_run::K_if_running<",
           "monitored_run::K_add_forcing_scan<false>", "monitored_run::K_add_forcing_scan<true>",
           "monitored_run::K_ou_forcing_scan<false>", "monitored_run::K_ou_forcing_scan<true>")


@pytest.mark.parametrize("needle", KERNELS)
def test_forcing_kernels_do_not_spill_to_scratch(needle, lib_resources):
    name, R = lib_resources
    for k, r in pick(R, needle).items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["lds"] <= 64 and r["agprs"] == 0, (name, k, r)   # (lds: rg_reduce_max's four doubles)
        assert r["occupancy"] >= 4 and r["vgprs"] <= 128, (name, k, r)


def test_the_scan_kicks_are_launched_through_the_reduction(lib_resources):
    name, R = lib_resources
    for needle in KERNELS[4:]:
        assert all("rg_reduce_max_kernel<256" in k for k in pick(R, needle)), (name, needle)
