"""What the kernels of the map monitor (csrc/hip/monitor_maps.h) need from the register file and the LDS, in both libraries: no
scratch, no spill, no AGPR; LDS in the tiled kernel of the sum along x only, little enough for two workgroups per CU; and the numbers
DESIGN 3.4.4 states.  That adding them moved no other kernel is tests/test_monitor_resources.py::test_every_other_kernel_is_as_it_was,
which accepts them by their names.  Numbers: the kernel-resource-usage remarks of the device compile that produced the shipped
libraries (tests/test_kernel_resources.py)."""
import pytest

from test_kernel_resources import pick, resources
from test_monitor_resources import raw_remarks

LDS_PER_CU = 160 * 1024


@pytest.fixture(scope="module", params=["librgpu.so", "librgpu_fast.so"])
def lib_resources(request, product_lib, contracted_lib):
    return request.param, resources(request.param)


def test_map_kernels_do_not_spill(lib_resources):
    name, R = lib_resources
    found = pick(R, "monitor_map_")
    assert len(found) == 2, sorted(found)
    for k, r in found.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["agprs"] == 0, (k, r)
        assert r["vgprs"] <= 128, (k, r)


def test_only_the_tiled_kernel_has_lds(lib_resources):
    name, R = lib_resources
    for k, r in pick(R, "monitor_map_").items():
        if "monitor_map_x_tiled_kernel(" in k:
            assert 0 < r["lds"] and 2 * r["lds"] <= LDS_PER_CU, (k, r)   # at least two workgroups share a CU
            assert r["lds"] == 12 * 8 * 65 * 8                           # MAP_NQ x MAPX_ROWS rows of MAPX_PITCH doubles
        else:
            assert r["lds"] == 0 and r["occupancy"] >= 4, (k, r)         # a streaming kernel: many waves in flight


# the rows of DESIGN 3.4.4, the same in both libraries: VGPRs, TotalSGPRs, occupancy, LDS bytes (scratch, spills and AGPRs are 0 in both)
DOCUMENTED = {"monitor_map_pixels_kernel": (74, 36, 6, 0), "monitor_map_x_tiled_kernel": (68, 67, 3, 49920)}


def test_map_kernels_have_the_documented_numbers(lib_resources):
    name, _ = lib_resources
    now = raw_remarks(name)
    for needle, (vgprs, sgprs, occupancy, lds) in DOCUMENTED.items():
        (k, r), = [(k, r) for k, r in now.items() if needle in k]
        assert (r["VGPRs"], r["TotalSGPRs"], r["Occupancy [waves/SIMD]"], r["LDS Size [bytes/block]"]) == (vgprs, sgprs, occupancy, lds), (name, k, r)
        assert r["AGPRs"] == 0 and r["ScratchSize [bytes/lane]"] == 0 and r["SGPRs Spill"] == 0 and r["VGPRs Spill"] == 0, (name, k, r)


def test_the_names_stay_clear_of_the_other_monitor_kernels(lib_resources):
    """the resource tests of the other monitors pick their kernels by a piece of their names: the new names hold none of those pieces"""
    name, _ = lib_resources
    new = [k for k in raw_remarks(name) if "monitor_map_" in k]
    assert len(new) == 2
    for k in new:
        assert not any(needle in k for needle in ("monitor_vol_", "monitor_plane_cols_", "monitor_profile_", "ensemble_monitor_")), k


def test_the_flat_functor_stays_out_of_the_product(lib_resources):
    """the product runs the gfx950 kernels (RGPU_TILED_MONITOR_MAPS, csrc/hip/rg_tiled.h); the flat K_mon_map functor serves the host
    emulation and is not instantiated in it"""
    name, _ = lib_resources
    assert not [k for k in raw_remarks(name) if "K_mon_map" in k]
