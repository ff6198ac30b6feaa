"""What the kernels of the Helmholtz spectra (csrc/hip/monitor_helm.h) need from the register file and the LDS, in both libraries: no
scratch, no spill, no AGPR; the tile and the twiddle factors of the z and the bin kernel exactly the 147,456 bytes of the spectrum
monitor's passes, one workgroup of sixteen waves per CU of 160 KB, four waves per SIMD, at most 128 VGPRs; 6 KB in the fold kernel; and
the numbers DESIGN 3.4.8 states.  That adding them moved no other kernel is tests/test_monitor_resources.py::
test_every_other_kernel_is_as_it_was and the resource tests of the other monitors, which pass untouched.  Numbers: the
kernel-resource-usage remarks of the device compile that produced the shipped libraries (tests/test_kernel_resources.py)."""
import pytest

from test_kernel_resources import pick, resources
from test_monitor_resources import raw_remarks

LDS_PER_CU = 160 * 1024
TILE, TWIDDLES = 8192, 512   # complex doubles of a tile, and of the longest line's factors
LDS = 16 * (TILE + TILE // 16 + TWIDDLES)
KERNELS = ["monitor_helm_z_kernel", "monitor_helm_bin_kernel", "monitor_helm_fold_kernel"]


@pytest.fixture(scope="module", params=["librgpu.so", "librgpu_fast.so"])
def lib_resources(request, product_lib, contracted_lib):
    return request.param, resources(request.param)


def test_helm_kernels_do_not_spill(lib_resources):
    name, R = lib_resources
    found = pick(R, "monitor_helm_")
    assert sorted(k.split("(")[0].split("::")[-1] for k in found) == sorted(KERNELS), sorted(found)
    for k, r in found.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["agprs"] == 0, (k, r)
        assert r["vgprs"] <= 128, (k, r)   # sixteen waves of a workgroup on one CU: four per SIMD, 128 registers each


def test_the_z_and_bin_kernels_hold_a_tile_in_lds(lib_resources):
    name, R = lib_resources
    for k, r in pick(R, "monitor_helm_").items():
        if "monitor_helm_fold_kernel(" in k:
            assert r["lds"] == 3 * 16 * 16 * 8 and r["occupancy"] >= 4, (k, r)   # the fold: sixteen runs of sixteen shells, three sums; many waves in flight
        else:
            assert r["lds"] == LDS == 147456, (k, r)                   # the padded tile and the twiddle factors: (T, L) takes the slot of a complex number
            assert r["lds"] <= LDS_PER_CU < 2 * r["lds"], (k, r)        # one workgroup per CU ...
            assert r["occupancy"] == 4, (k, r)                         # ... of sixteen waves: four per SIMD


# the rows of DESIGN 3.4.8 per library: VGPRs, TotalSGPRs, occupancy, LDS bytes (scratch, spills and AGPRs are 0 in both)
DOCUMENTED = {
    "librgpu.so": {"monitor_helm_z_kernel": (26, 29, 4, 147456), "monitor_helm_bin_kernel": (86, 84, 4, 147456), "monitor_helm_fold_kernel": (66, 36, 7, 6144)},
    "librgpu_fast.so": {"monitor_helm_z_kernel": (24, 29, 4, 147456), "monitor_helm_bin_kernel": (84, 84, 4, 147456), "monitor_helm_fold_kernel": (66, 36, 7, 6144)},
}


def test_helm_kernels_have_the_documented_numbers(lib_resources):
    name, _ = lib_resources
    now = raw_remarks(name)
    for needle, (vgprs, sgprs, occupancy, lds) in DOCUMENTED[name].items():
        (k, r), = [(k, r) for k, r in now.items() if needle in k]
        assert (r["VGPRs"], r["TotalSGPRs"], r["Occupancy [waves/SIMD]"], r["LDS Size [bytes/block]"]) == (vgprs, sgprs, occupancy, lds), (name, k, r)
        assert r["AGPRs"] == 0 and r["ScratchSize [bytes/lane]"] == 0 and r["SGPRs Spill"] == 0 and r["VGPRs Spill"] == 0, (name, k, r)


def test_the_names_stay_clear_of_the_other_monitor_kernels(lib_resources):
    """the resource tests of the other monitors pick their kernels by a piece of their names: the new names hold none of those pieces"""
    name, _ = lib_resources
    new = [k for k in raw_remarks(name) if "monitor_helm_" in k]
    assert len(new) == 3
    for k in new:
        assert not any(needle in k for needle in ("monitor_spectrum_", "monitor_map_", "monitor_vol_", "monitor_plane_cols_", "monitor_profile_", "monitor_pdf_", "ensemble_monitor_")), k


def test_the_flat_functor_stays_out_of_the_product(lib_resources):
    """the product runs the gfx950 kernels (RGPU_TILED_MONITOR_HELM, csrc/hip/rg_tiled.h); the flat K_mon_helm_bin serves the host
    emulation and is not instantiated in it"""
    name, _ = lib_resources
    assert not [k for k in raw_remarks(name) if "K_mon_helm" in k]
