"""What the ensemble kernels (csrc/hip/ensemble2d.h) need from the register file and LDS, against their single-box counterparts: they
run the same body with the member in blockIdx.y, so a workgroup must place on a CU exactly as the single-box kernel's does -- LDS equal,
occupancy not below, spills not above -- or M boxes in one launch would not be M times the single box's work per launch.  Numbers: the
compiler's kernel-resource-usage remarks of the device compile that produced the shipped libraries (tests/test_kernel_resources.py)."""
import re

import pytest

from test_kernel_resources import LDS_PER_CU, pick, resources


@pytest.fixture(scope="module", params=["librgpu.so", "librgpu_fast.so"])
def lib_resources(request, product_lib, contracted_lib):
    return request.param, resources(request.param)


def template_args(name):
    return re.search(r"\w+<([^>]*)>\(", name).group(1)


def assert_not_worse(k, r, k1, r1):
    assert r["lds"] == r1["lds"], (k, r, k1, r1)
    assert r["occupancy"] >= r1["occupancy"], (k, r, k1, r1)
    for what in ("vgpr_spill", "sgpr_spill", "scratch"):
        assert r[what] <= r1[what], (what, k, r, k1, r1)


def test_ensemble_step_kernels_place_like_their_single_box_counterparts(lib_resources):
    name, R = lib_resources
    seen = 0
    for ens, single in (("hydro2d_ensemble_kernel<", "hydro2d_step_kernel<"), ("mhd2d_ensemble_kernel<", "mhd2d_step_kernel<")):
        for k, r in pick(R, ens).items():
            (k1, r1), = pick(R, single + template_args(k) + ">(").items()
            assert_not_worse(k, r, k1, r1)
            seen += 1
    assert seen >= 9   # 7 hydro instantiations (6 solver / slope pairs + the generic one), 2 MHD


def test_ensemble_kernels_keep_the_occupancy_of_the_2d_steps(lib_resources):
    name, R = lib_resources
    for k, r in pick(R, "hydro2d_ensemble_kernel<16, 16,").items():
        generic = ", 0>" in k
        assert r["vgpr_spill"] == 0 and r["scratch"] <= (40 if generic else 0), (k, r)
        assert 3 * r["lds"] <= LDS_PER_CU and r["occupancy"] >= 3, (k, r)      # three workgroups per CU
    for k, r in pick(R, "mhd2d_ensemble_kernel<").items():
        generic = "mhd2d_ensemble_kernel<0>" in k
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["occupancy"] >= (2 if generic else 3) and 3 * r["lds"] <= LDS_PER_CU, (k, r)


def test_ensemble_clock_kernel_is_the_clock_kernel(lib_resources):
    name, R = lib_resources
    (k, r), = pick(R, "ensemble_clock_kernel(").items()
    (k1, r1), = pick(R, "step_clock_kernel(").items()
    assert_not_worse(k, r, k1, r1)
