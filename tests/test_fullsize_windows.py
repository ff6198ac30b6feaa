"""The bench-size steps against the oracle, every cell (-m gpu).  The 512^3 MRI step of bench.py's headline, implode3d at 256^3 (HLLC,
bench.py --workload implode3d) and BASELINE config 5 (512 x 1024 x 512 MRI, the whole box on one device): one step inside a batch of
the bench's path, after K steps, compared with the oracle window by window (parity_checks.check_step_in_windows; the windows are pinned
to the whole-box oracle step by tests/test_zwindow_oracle.py).  The exact library must match every double; the contracted one the
specific-form relative L2 of 1e-12 per variable.  Only at these sizes do the sweep's z plans of the bench, the partial last segment of
the update and offsets past 2^31 elements and 2^32, 2^33 and 2^34 bytes occur: the check asserts that every such plane is compared."""
import json
import os
import subprocess
import sys

import pytest

import parity_checks as pc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARITHS = ["exact", "contracted"]


def _lib(request, arith):
    return request.getfixturevalue("gpu_lib" if arith == "exact" else "gpu_contracted_lib")


@pytest.mark.parametrize("arith", ARITHS)
def test_mri_512_step_in_windows(arith, request, oracle):
    """bench.py's default workload (configs/mhd_mri_3d.ini at 512^3): the 4th step of a batch of 4"""
    lib = _lib(request, arith)
    pc.check_step_in_windows(lib, oracle, "mhd_mri_3d", "mesh.nx=512;mesh.ny=512;mesh.nz=512", 3, exact=arith == "exact")


@pytest.mark.parametrize("arith", ARITHS)
def test_implode_256_step_in_windows(arith, request, oracle):
    """bench.py --workload implode3d (configs/implode3d.ini at 256^3, HLLC): the 4th step of a batch of 4, the whole box in one
    sequential oracle step (one window)"""
    lib = _lib(request, arith)
    pc.check_step_in_windows(lib, oracle, "implode3d", "mesh.nx=256;mesh.ny=256;mesh.nz=256;hydro.riemannSolver=hllc", 3,
                             exact=arith == "exact", widths=[256])


@pytest.mark.parametrize("arith", ARITHS)
def test_config5_whole_box_step_in_windows(arith, request):
    """BASELINE config 5, 512 x 1024 x 512 MRI, the whole box in one single-device context: the 3rd step of a batch of 3.  In a child
    process, which bounds the host memory of the 17.7 GB state arrays to its own life (the GPU suite's process plus this one hold the
    GPU)"""
    _lib(request, arith)   # the device answers before anything big starts
    code = r"""
import json, os, sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import parity_checks as pc
from oracle_api import Oracle
from ramsesgpu_amd.solver import Library, lib_path
L = Library(lib_path(%r))
assert L.arithmetic == %r
facts = pc.check_step_in_windows(L, Oracle(os.path.join(%r, "oracle", "liboracle.so")), "mhd_mri_3d", "mesh.nx=512;mesh.ny=1024;mesh.nz=512", 2,
                                 exact=%r)
print("FACTS " + json.dumps(facts))
""" % (ROOT, os.path.join(ROOT, "tests"), arith, arith, ROOT, arith == "exact")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    facts = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("FACTS ")][-1][6:])
    print("step in windows:", facts)
