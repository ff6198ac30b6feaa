"""What the two kernels of the plane monitor (csrc/hip/monitor_profile.h) need from the register file, in both libraries: no LDS, no
scratch, no spill, no AGPR, at least four waves per SIMD, and the numbers DESIGN 3.4.3 states.  That adding them moved no other
kernel is tests/test_monitor_resources.py::test_every_other_kernel_is_as_it_was, which accepts them by their names.  Numbers: the
kernel-resource-usage remarks of the device compile that produced the shipped libraries (tests/test_kernel_resources.py)."""
import pytest

from test_kernel_resources import pick, resources
from test_monitor_resources import raw_remarks

KERNELS = ("monitor_profile_cols_kernel(", "monitor_profile_planes_kernel(")


@pytest.fixture(scope="module", params=["librgpu.so", "librgpu_fast.so"])
def lib_resources(request, product_lib, contracted_lib):
    return request.param, resources(request.param)


def test_plane_monitor_kernels_do_not_spill(lib_resources):
    name, R = lib_resources
    for needle in KERNELS:
        (k, r), = pick(R, needle).items()
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["lds"] == 0 and r["agprs"] == 0, (k, r)
        assert r["occupancy"] >= 4 and r["vgprs"] <= 128, (k, r)   # streaming kernels: many waves in flight


# the rows of DESIGN 3.4.3, the same in both libraries: VGPRs, TotalSGPRs, occupancy (LDS, scratch, spills and AGPRs are 0 in both)
DOCUMENTED = {"monitor_profile_cols_kernel": (96, 48, 5), "monitor_profile_planes_kernel": (100, 86, 4)}


def test_plane_monitor_kernels_have_the_documented_numbers(lib_resources):
    name, _ = lib_resources
    now = raw_remarks(name)
    for needle, (vgprs, sgprs, occupancy) in DOCUMENTED.items():
        (k, r), = [(k, r) for k, r in now.items() if needle in k]
        assert (r["VGPRs"], r["TotalSGPRs"], r["Occupancy [waves/SIMD]"]) == (vgprs, sgprs, occupancy), (name, k, r)
        assert r["AGPRs"] == 0 and r["ScratchSize [bytes/lane]"] == 0 and r["LDS Size [bytes/block]"] == 0 and r["SGPRs Spill"] == 0 and r["VGPRs Spill"] == 0, (name, k, r)


def test_the_names_stay_clear_of_the_monitor_kernels(lib_resources):
    """the resource tests of the monitor pick its kernels by a piece of their names: the new names hold none of those pieces"""
    name, _ = lib_resources
    new = [k for k in raw_remarks(name) if "monitor_profile_" in k]
    assert len(new) == 2
    for k in new:
        assert not any(needle in k for needle in ("monitor_vol_cols_kernel", "monitor_plane_cols_kernel", "monitor_vol_planes_kernel", "monitor_vol_finish_kernel")), k


def test_the_flat_functors_stay_out_of_the_product(lib_resources):
    """the product runs the gfx950 kernels (RGPU_TILED_MONITOR_PROFILE, csrc/hip/rg_tiled.h); the flat K_mon_prof_* functors serve the
    host emulation and are not instantiated in it"""
    name, _ = lib_resources
    assert not [k for k in raw_remarks(name) if "K_mon_prof_" in k]
