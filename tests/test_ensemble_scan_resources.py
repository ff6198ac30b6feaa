"""What the kernels of a parameter scan (csrc/hip/ensemble_scan.h) need from the register file and LDS, against the uniform ensemble
kernels with the same template arguments: they run the same body and differ only in where the member's constants come from (a table
in device memory instead of the kernel arguments), so a workgroup must place on a CU exactly as the uniform kernel's does -- LDS equal,
occupancy not below, spills and scratch not above -- in BOTH libraries.  Numbers: the compiler's kernel-resource-usage remarks of the
device compile that produced the shipped libraries (tests/test_kernel_resources.py).

No retreat: mhd2d_scan_kernel<0> (every solver in one kernel, at the scalar-register limit) is held to the same standard as the
others -- it stays free of scalar spills with its rotating-frame coefficients and dt in vector registers -- and a scan that needs it
runs fused (tests/test_ensemble_scan_gpu.py: ISO_SCAN_IS_FUSED)."""
import pytest

from test_ensemble_resources import assert_not_worse, template_args
from test_kernel_resources import pick, resources


@pytest.fixture(scope="module", params=["librgpu.so", "librgpu_fast.so"])
def lib_resources(request, product_lib, contracted_lib):
    return request.param, resources(request.param)


def test_scan_step_kernels_place_like_the_uniform_ensemble_kernels(lib_resources):
    name, R = lib_resources
    seen, generic_mhd = 0, 0
    for scan, uniform in (("hydro2d_scan_kernel<", "hydro2d_ensemble_kernel<"), ("mhd2d_scan_kernel<", "mhd2d_ensemble_kernel<")):
        for k, r in pick(R, scan).items():
            (k1, r1), = pick(R, uniform + template_args(k) + ">(").items()
            assert_not_worse(k, r, k1, r1)
            seen += 1
            if scan.startswith("mhd2d") and template_args(k) == "0":
                # the one instantiation the issue allowed a retreat for: stated explicitly -- none was taken
                generic_mhd += 1
                assert r["sgpr_spill"] == 0 and r["vgpr_spill"] == 0 and r["scratch"] == 0 and r["occupancy"] >= 2, (k, r)
    assert seen >= 9 and generic_mhd == 1   # 7 hydro instantiations (6 solver / slope pairs + the generic one), 2 MHD


def test_every_uniform_instantiation_has_a_scan_counterpart(lib_resources):
    """the instantiation list of a scan is the one of hydro2d_ensemble_step / mhd2d_ensemble_step"""
    name, R = lib_resources
    for scan, uniform in (("hydro2d_scan_kernel<", "hydro2d_ensemble_kernel<"), ("mhd2d_scan_kernel<", "mhd2d_ensemble_kernel<")):
        assert sorted(template_args(k) for k in pick(R, scan)) == sorted(template_args(k) for k in pick(R, uniform))


def test_scan_clock_kernel_is_the_ensemble_clock_kernel(lib_resources):
    name, R = lib_resources
    (k, r), = pick(R, "scan_clock_kernel(").items()
    (k1, r1), = pick(R, "ensemble_clock_kernel(").items()
    assert_not_worse(k, r, k1, r1)
    (k2, r2), = pick(R, "step_clock_kernel(").items()   # still exactly one of each
    assert_not_worse(k, r, k2, r2)
