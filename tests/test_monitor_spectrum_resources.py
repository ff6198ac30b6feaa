"""What the kernels of the spectrum monitor (csrc/hip/monitor_spectrum.h) need from the register file and the LDS, in both libraries:
no scratch, no spill, no AGPR; the tile and the twiddle factors of the three pass kernels exactly their documented 147,456 bytes, one
workgroup of sixteen waves per CU of 160 KB, four waves per SIMD; 4 KB in the fold kernel; and the numbers DESIGN 3.4.6 states.
That adding them moved no other kernel is tests/test_monitor_resources.py::test_every_other_kernel_is_as_it_was, which accepts them by
their names.  Numbers: the kernel-resource-usage remarks of the device compile that produced the shipped libraries
(tests/test_kernel_resources.py)."""
import pytest

from test_kernel_resources import pick, resources
from test_monitor_resources import raw_remarks

LDS_PER_CU = 160 * 1024
TILE, TWIDDLES = 8192, 512   # complex doubles of a tile, and of the longest line's factors
LDS = 16 * (TILE + TILE // 16 + TWIDDLES)
PASSES = ["monitor_spectrum_x_kernel", "monitor_spectrum_y_kernel", "monitor_spectrum_z_kernel"]


@pytest.fixture(scope="module", params=["librgpu.so", "librgpu_fast.so"])
def lib_resources(request, product_lib, contracted_lib):
    return request.param, resources(request.param)


def test_spectrum_kernels_do_not_spill(lib_resources):
    name, R = lib_resources
    found = pick(R, "monitor_spectrum_")
    assert sorted(k.split("(")[0].split("::")[-1] for k in found) == sorted(PASSES + ["monitor_spectrum_fold_kernel"]), sorted(found)
    for k, r in found.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["agprs"] == 0, (k, r)
        assert r["vgprs"] <= 128, (k, r)   # sixteen waves of a workgroup on one CU: four per SIMD, 128 registers each


def test_the_pass_kernels_hold_a_tile_in_lds(lib_resources):
    name, R = lib_resources
    for k, r in pick(R, "monitor_spectrum_").items():
        if "monitor_spectrum_fold_kernel(" in k:
            assert r["lds"] == 2 * 16 * 16 * 8 and r["occupancy"] >= 4, (k, r)   # the fold: sixteen runs of sixteen shells, sums and counts; many waves in flight
        else:
            assert r["lds"] == LDS == 147456, (k, r)                   # the padded tile and the twiddle factors
            assert r["lds"] <= LDS_PER_CU < 2 * r["lds"], (k, r)        # the documented one workgroup per CU ...
            assert r["occupancy"] == 4, (k, r)                         # ... of sixteen waves: four per SIMD


# the rows of DESIGN 3.4.6 per library: VGPRs, TotalSGPRs, occupancy, LDS bytes (scratch, spills and AGPRs are 0 in both)
DOCUMENTED = {
    "librgpu.so": {"monitor_spectrum_x_kernel": (40, 95, 4, 147456), "monitor_spectrum_y_kernel": (26, 28, 4, 147456),
                   "monitor_spectrum_z_kernel": (64, 70, 4, 147456), "monitor_spectrum_fold_kernel": (47, 30, 8, 4096)},
    "librgpu_fast.so": {"monitor_spectrum_x_kernel": (36, 95, 4, 147456), "monitor_spectrum_y_kernel": (24, 28, 4, 147456),
                        "monitor_spectrum_z_kernel": (62, 70, 4, 147456), "monitor_spectrum_fold_kernel": (47, 30, 8, 4096)},
}


def test_spectrum_kernels_have_the_documented_numbers(lib_resources):
    name, _ = lib_resources
    now = raw_remarks(name)
    for needle, (vgprs, sgprs, occupancy, lds) in DOCUMENTED[name].items():
        (k, r), = [(k, r) for k, r in now.items() if needle in k]
        assert (r["VGPRs"], r["TotalSGPRs"], r["Occupancy [waves/SIMD]"], r["LDS Size [bytes/block]"]) == (vgprs, sgprs, occupancy, lds), (name, k, r)
        assert r["AGPRs"] == 0 and r["ScratchSize [bytes/lane]"] == 0 and r["SGPRs Spill"] == 0 and r["VGPRs Spill"] == 0, (name, k, r)


def test_the_names_stay_clear_of_the_other_monitor_kernels(lib_resources):
    """the resource tests of the other monitors pick their kernels by a piece of their names: the new names hold none of those pieces"""
    name, _ = lib_resources
    new = [k for k in raw_remarks(name) if "monitor_spectrum_" in k]
    assert len(new) == 4
    for k in new:
        assert not any(needle in k for needle in ("monitor_map_", "monitor_vol_", "monitor_plane_cols_", "monitor_profile_", "monitor_pdf_", "ensemble_monitor_")), k


def test_the_flat_functors_stay_out_of_the_product(lib_resources):
    """the product runs the gfx950 kernels (RGPU_TILED_MONITOR_SPECTRUM, csrc/hip/rg_tiled.h); the flat K_mon_spectrum functors serve the
    host emulation and are not instantiated in it"""
    name, _ = lib_resources
    assert not [k for k in raw_remarks(name) if "K_mon_spectrum" in k]
