"""What the kernels of the PDF monitor (csrc/hip/monitor_pdf.h) need from the register file and the LDS, in both libraries: no
scratch, no spill, no AGPR; the table of counts of the count kernel exactly its documented 64 KB, two workgroups per CU; no LDS in the
fold kernel; and the numbers DESIGN 3.4.5 states.  That adding them moved no other kernel is
tests/test_monitor_resources.py::test_every_other_kernel_is_as_it_was, which accepts them by their names.  Numbers: the
kernel-resource-usage remarks of the device compile that produced the shipped libraries (tests/test_kernel_resources.py)."""
import pytest

from ramsesgpu_amd import _capi
from test_kernel_resources import pick, resources
from test_monitor_resources import raw_remarks

LDS_PER_CU = 160 * 1024


@pytest.fixture(scope="module", params=["librgpu.so", "librgpu_fast.so"])
def lib_resources(request, product_lib, contracted_lib):
    return request.param, resources(request.param)


def test_pdf_kernels_do_not_spill(lib_resources):
    name, R = lib_resources
    found = pick(R, "monitor_pdf_")
    assert len(found) == 2, sorted(found)
    assert sorted(k.split("(")[0].split("::")[-1] for k in found) == ["monitor_pdf_count_kernel", "monitor_pdf_fold_kernel"]
    for k, r in found.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["agprs"] == 0, (k, r)
        assert r["vgprs"] <= 128, (k, r)


def test_the_count_kernel_holds_the_word_budget_in_lds(lib_resources):
    name, R = lib_resources
    for k, r in pick(R, "monitor_pdf_").items():
        if "monitor_pdf_count_kernel(" in k:
            assert r["lds"] == 4 * _capi.PDF_MAX_WORDS == 65536, (k, r)   # a u32 per word of the budget
            assert 2 * r["lds"] <= LDS_PER_CU, (k, r)                     # two workgroups share a CU
        else:
            assert r["lds"] == 0 and r["occupancy"] >= 4, (k, r)          # the fold: a streaming kernel, many waves in flight


# the rows of DESIGN 3.4.5, the same in both libraries: VGPRs, TotalSGPRs, occupancy, LDS bytes (scratch, spills and AGPRs are 0 in both)
DOCUMENTED = {"monitor_pdf_count_kernel": (70, 73, 2, 65536), "monitor_pdf_fold_kernel": (26, 24, 8, 0)}


def test_pdf_kernels_have_the_documented_numbers(lib_resources):
    name, _ = lib_resources
    now = raw_remarks(name)
    for needle, (vgprs, sgprs, occupancy, lds) in DOCUMENTED.items():
        (k, r), = [(k, r) for k, r in now.items() if needle in k]
        assert (r["VGPRs"], r["TotalSGPRs"], r["Occupancy [waves/SIMD]"], r["LDS Size [bytes/block]"]) == (vgprs, sgprs, occupancy, lds), (name, k, r)
        assert r["AGPRs"] == 0 and r["ScratchSize [bytes/lane]"] == 0 and r["SGPRs Spill"] == 0 and r["VGPRs Spill"] == 0, (name, k, r)


def test_the_names_stay_clear_of_the_other_monitor_kernels(lib_resources):
    """the resource tests of the other monitors pick their kernels by a piece of their names: the new names hold none of those pieces"""
    name, _ = lib_resources
    new = [k for k in raw_remarks(name) if "monitor_pdf_" in k]
    assert len(new) == 2
    for k in new:
        assert not any(needle in k for needle in ("monitor_map_", "monitor_vol_", "monitor_plane_cols_", "monitor_profile_", "ensemble_monitor_")), k


def test_the_flat_functors_stay_out_of_the_product(lib_resources):
    """the product runs the gfx950 kernels (RGPU_TILED_MONITOR_PDF, csrc/hip/rg_tiled.h); the flat K_mon_pdf functors serve the host
    emulation and are not instantiated in it"""
    name, _ = lib_resources
    assert not [k for k in raw_remarks(name) if "K_mon_pdf" in k]
