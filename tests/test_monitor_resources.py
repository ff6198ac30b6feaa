"""What the ensemble's monitor kernels (csrc/hip/ensemble_monitor.h) need from the register file,
and that adding them moved nothing else: every number the compiler reports for every kernel the libraries had before the monitors --
the step and clock kernels of the ensembles among them -- is what tests/golden/kernel_resources_before_monitors.json recorded from a
build of the commit before, in both libraries.  Numbers: the kernel-resource-usage remarks of the device compile that produced the
shipped libraries (tests/test_kernel_resources.py)."""
import json
import os
import re

import pytest

from conftest import GOLDEN
from ramsesgpu_amd import build as rb
from test_kernel_resources import pick, resources


def raw_remarks(out_name):
    """{mangled kernel name: {remark label: number}} -- every numeric line of the remarks, TotalSGPRs included"""
    out, cur = {}, None
    for line in open(rb.resources_path(out_name)):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z \[\]/]+): (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    return out


@pytest.fixture(scope="module", params=["librgpu.so", "librgpu_fast.so"])
def lib_resources(request, product_lib, contracted_lib):
    return request.param, resources(request.param)


def test_monitor_kernels_do_not_spill(lib_resources):
    name, R = lib_resources
    for needle in ("ensemble_monitor_rows_kernel(", "ensemble_monitor_fold_kernel("):
        (k, r), = pick(R, needle).items()
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["lds"] == 0, (k, r)
        assert r["occupancy"] >= 4 and r["vgprs"] <= 128 and r["agprs"] == 0, (k, r)   # streaming kernels: many waves in flight


# the rows of DESIGN 3.6.2, the same in both libraries: VGPRs, TotalSGPRs, occupancy (LDS, scratch and spills are 0 in both)
DOCUMENTED = {"ensemble_monitor_rows_kernel": (66, 44, 7), "ensemble_monitor_fold_kernel": (64, 66, 8)}


def test_monitor_kernels_have_the_documented_numbers(lib_resources):
    name, _ = lib_resources
    now = raw_remarks(name)
    for needle, (vgprs, sgprs, occupancy) in DOCUMENTED.items():
        (k, r), = [(k, r) for k, r in now.items() if needle in k]
        assert (r["VGPRs"], r["TotalSGPRs"], r["Occupancy [waves/SIMD]"]) == (vgprs, sgprs, occupancy), (name, k, r)
        assert r["AGPRs"] == 0 and r["ScratchSize [bytes/lane]"] == 0 and r["LDS Size [bytes/block]"] == 0 and r["SGPRs Spill"] == 0 and r["VGPRs Spill"] == 0, (name, k, r)


def test_every_other_kernel_is_as_it_was(lib_resources):
    name, _ = lib_resources
    before = json.load(open(os.path.join(GOLDEN, "kernel_resources_before_monitors.json")))[name]
    now = raw_remarks(name)
    assert len(before) > 150
    for k, r in before.items():
        assert k in now, "kernel %s is gone from %s" % (k, name)
        assert now[k] == r, (name, k, r, now[k])
    added = sorted(set(now) - set(before))
    assert all("monitor" in k or "K_mon_" in k or "K_hist_batch_" in k for k in added), added
