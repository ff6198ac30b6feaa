"""What the kernels of the 3D monitor (csrc/hip/monitor3d.h) need from the register file, in both libraries: no scratch, no spill, the
pass over the state with at least four waves per SIMD, and the numbers DESIGN 3.4.2 states.  That adding them moved no other kernel is
tests/test_monitor_resources.py::test_every_other_kernel_is_as_it_was, which accepts them by their names.  Numbers: the
kernel-resource-usage remarks of the device compile that produced the shipped libraries (tests/test_kernel_resources.py)."""
import pytest

from test_kernel_resources import pick, resources
from test_monitor_resources import raw_remarks

KERNELS = ("monitor_vol_cols_kernel(", "monitor_plane_cols_kernel(", "monitor_vol_planes_kernel(", "monitor_vol_finish_kernel(")


@pytest.fixture(scope="module", params=["librgpu.so", "librgpu_fast.so"])
def lib_resources(request, product_lib, contracted_lib):
    return request.param, resources(request.param)


def test_monitor3d_kernels_do_not_spill(lib_resources):
    name, R = lib_resources
    for needle in KERNELS:
        (k, r), = pick(R, needle).items()
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["lds"] == 0 and r["agprs"] == 0, (k, r)
        assert r["occupancy"] >= 4 and r["vgprs"] <= 128, (k, r)   # streaming kernels: many waves in flight


# the rows of DESIGN 3.4.2, the same in both libraries: VGPRs, TotalSGPRs, occupancy (LDS, scratch and spills are 0 in all four)
DOCUMENTED = {"monitor_vol_cols_kernel": (72, 48, 7), "monitor_plane_cols_kernel": (62, 46, 8), "monitor_vol_planes_kernel": (64, 62, 8), "monitor_vol_finish_kernel": (126, 16, 4)}


def test_monitor3d_kernels_have_the_documented_numbers(lib_resources):
    name, _ = lib_resources
    now = raw_remarks(name)
    for needle, (vgprs, sgprs, occupancy) in DOCUMENTED.items():
        (k, r), = [(k, r) for k, r in now.items() if needle in k]
        assert (r["VGPRs"], r["TotalSGPRs"], r["Occupancy [waves/SIMD]"]) == (vgprs, sgprs, occupancy), (name, k, r)


def test_the_flat_functors_stay_out_of_the_product(lib_resources):
    """the product runs the gfx950 kernels (RGPU_TILED_MONITOR3D, csrc/hip/rg_tiled.h); the flat K_mon_vol_* functors serve the host
    emulation and are not instantiated in it"""
    name, _ = lib_resources
    assert not [k for k in raw_remarks(name) if "K_mon_vol_" in k]
