"""bench.py's contract on the GPU box at toy sizes: a plain run prints one JSON line with the driver's keys and nothing it
would have to measure separately; --full adds `roofline`, the other build of the library and (N=1) `cpu_baseline`, for every
workload; the N>1 launch line of the driver (torch.distributed.run, one rank per GPU) exercised
with two ranks sharing the one GPU of the box: (i) through the explicitly selected test harness (RGPU_BENCH_DRIVER=python over gloo),
(ii) through the default C++ RCCL driver, which must FAIL CLEANLY there (RCCL refuses two ranks on one device; there is no
fallback), (iii) with only one device visible, where rank 1 must say so.  The C++ RCCL driver itself is covered by
tests/test_comm_driver.py."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu
KEYS = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
        "data", "config", "roofline"}


def last_json(text):
    lines = [l for l in text.splitlines() if l.startswith("{")]
    assert lines, text[-2000:]
    return json.loads(lines[-1])


@pytest.mark.parametrize("args", [["--workload", "mri", "--nx", "32", "--ny", "48", "--nz", "32"],
                                  ["--workload", "implode3d", "--size", "48"],
                                  ["--workload", "orszag-tang", "--size", "64"]], ids=["mri", "implode3d", "orszag-tang"])
def test_bench_line_single_gpu(args, gpu_lib):
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--full", "--no-cpu-baseline"] + args,
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    d = last_json(res.stdout)
    assert KEYS <= set(d) and d["n_gpus"] == 1 and d["dtype"] == "f64" and d["value"] > 0 and "workload" in d["config"]
    r = d["roofline"]
    # achieved / peak / frac are the contract's HBM figures whatever binds the kernel; the 3D MHD sweep is labelled by what does bind it
    # (fp64 vector issue) once the committed counters belong to this state of the sources, with its share of the issue slots beside
    assert r["peak"] == 8000.0 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-12 and r["hbm_frac"] == r["frac"]
    assert r["bound"] == ("valu_f64" if (args[1] == "mri" and r["valu_ceiling"] and r["valu_frac"] > r["frac"]) else "hbm")
    if r["valu_ceiling"]:
        assert r["valu_frac"] == r["valu_ceiling"]["frac"] and 0 < r["valu_frac"] < 1.0 and 0 < r["pmc_scale"] < 1.0
    # the headline is the tolerance-grade library (north_star's bar: relative L2 < 1e-12, gated by tests/test_contracted.py) and says so;
    # the bit-identical library is measured beside it the same way: a value with its own roofline
    assert d["config"]["arithmetic"] == "contracted" and "not bit-identical" in d["config"]["parity"] and "1e-12" in d["config"]["parity"]
    assert "librgpu_fast.so" in d["config"]["driver"]
    e = d["value_exact"]
    assert e["value"] > 0 and e["library"] == "librgpu.so" and e["arithmetic"] == "exact" and "bit-identical" in e["parity"]
    assert e["steps"] == d["steps"] and e["warmup"] == d["warmup"] and e["roofline"]["frac"] > 0 and e["roofline"]["avg_launch_ms"] > 0
    assert d["config"]["rccl_ranks"] is None and len(d["config"]["ranks"]) == 1 and "single device" in d["config"]["driver"]
    assert "other_workloads" not in d        # only the default headline run carries them
    # which build `value` is travels at the top level too (round-over-round comparisons: value_exact is the like-for-like number)
    assert d["value_arithmetic"] == "contracted" and d["metric_version"] == 2
    # traffic / valu_ceiling come from the committed PMC summary only when it was collected on THIS state of the kernel sources
    assert ("pmc_note" in r) == (r["traffic"] is None), r.get("pmc_note")


FULL_ONLY = {"roofline", "roofline_step", "value_exact", "value_tolerance", "cpu_baseline", "cpu_baseline_all_cores", "other_workloads"}


def test_plain_bench_line_is_the_headline_of_the_full_one(gpu_lib, tmp_path):
    """without --full the line carries the headline and its config and nothing that takes runs of its own; it times and dumps
    what the --full line times and dumps: the same fingerprint, the same arrays bit for bit"""
    box = ["--workload", "mri", "--nx", "32", "--ny", "48", "--nz", "32", "--steps", "3", "--warmup", "1"]
    lines, dumps = {}, {}
    for name, extra in (("plain", []), ("full", ["--full", "--no-cpu-baseline", "--no-second-arith"])):
        dumps[name] = str(tmp_path / name)
        res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + box + extra + ["--dump-outputs", dumps[name]],
                             stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=600)
        assert res.returncode == 0, res.stderr[-2000:]
        lines[name] = last_json(res.stdout)
    d, f = lines["plain"], lines["full"]
    assert (KEYS - {"roofline"}) <= set(d) and not (FULL_ONLY & set(d)), sorted(d)
    assert "roofline" in f and "roofline_step" in f
    for k in ("metric", "unit", "higher_is_better", "dtype", "n_gpus", "steps", "warmup", "value_arithmetic", "metric_version"):
        assert d[k] == f[k], k
    assert d["value"] > 0 and abs(d["value"] * d["ms_per_step"] / (32 * 48 * 32 * 1e-3) - 1.0) < 1e-9     # Mcell-updates/s x ms per step
    assert d["config"]["fingerprint"] == f["config"]["fingerprint"]
    assert all("phase_ms" not in r for r in d["config"]["ranks"])
    for fn in ("state.npy", "dt.npy"):
        a, b = np.load(os.path.join(dumps["plain"], fn)), np.load(os.path.join(dumps["full"], fn))
        assert a.dtype == b.dtype == np.float64 and a.shape == b.shape and np.array_equal(a, b), fn


def test_bench_line_exact_on_request(gpu_lib):
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--full", "--no-cpu-baseline", "--arith", "exact",
                          "--workload", "mri", "--nx", "32", "--ny", "48", "--nz", "32"],
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    d = last_json(res.stdout)
    assert d["config"]["arithmetic"] == "exact" and d["config"]["parity"].startswith("librgpu.so: bit-identical") and "value_exact" not in d
    t = d["value_tolerance"]
    assert t["value"] > 0 and t["library"] == "librgpu_fast.so" and t["arithmetic"] == "contracted" and t["roofline"]["frac"] > 0


def launch_two_ranks(env_extra, extra_args=()):
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1",
           "--nx", "32", "--ny", "48", "--nz", "32"] + list(extra_args)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", **env_extra)
    return subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=600)


def test_bench_two_ranks_through_the_launch_line(gpu_lib):
    """the N > 1 code path of bench.py (launch line, barriers, max over ranks, the JSON line) with the test harness selected
    EXPLICITLY -- the line says so"""
    res = launch_two_ranks(dict(RGPU_BENCH_ONE_DEVICE="1", RGPU_BENCH_BACKEND="gloo", RGPU_BENCH_DRIVER="python"))
    assert res.returncode == 0, res.stderr[-3000:]
    d = last_json(res.stdout)
    assert d["n_gpus"] == 2 and d["scaling"] == "strong" and d["value"] > 0 and "cpu_baseline" not in d
    assert "TEST HARNESS" in d["config"]["driver"] and d["config"]["rccl_ranks"] is None and len(d["config"]["ranks"]) == 2


def test_bench_fingerprint_of_two_ranks_equals_the_single_device_line(gpu_lib, gpu_contracted_lib):
    """the N > 1 bench line through the product's C++ slab driver (schedule, rgpu_comm_run_steps, fingerprint) -- with the test-only
    device-staged transport in place of RCCL's wire, two ranks on the one GPU -- carries the SAME config.fingerprint (dt-sequence hash +
    state checksum) as the N = 1 line of the same box, steps and warmup, for both arithmetics: what makes the driver's SCALE lines checkable"""
    from test_comm_device import build_dev_comm
    build_dev_comm("exact"); build_dev_comm("contracted")
    two = launch_two_ranks(dict(RGPU_BENCH_ONE_DEVICE="1", RGPU_BENCH_DRIVER="staged-test"), ["--full"])
    assert two.returncode == 0, two.stderr[-3000:]
    d2 = last_json(two.stdout)
    assert "TEST TRANSPORT" in d2["config"]["driver"] and d2["n_gpus"] == 2 and "took their time step from the device" in d2["config"]["time_loop"]
    one = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--nx", "32", "--ny", "48", "--nz", "32",
                          "--full", "--no-cpu-baseline", "--no-other-workloads"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=600)
    assert one.returncode == 0, one.stderr[-3000:]
    d1 = last_json(one.stdout)
    for key in ("dt_sha256", "state_sum_u64", "steps"):
        assert d2["config"]["fingerprint"][key] == d1["config"]["fingerprint"][key], (key, d2["config"]["fingerprint"], d1["config"]["fingerprint"])
        assert d2["value_exact"]["fingerprint"][key] == d1["value_exact"]["fingerprint"][key], (key, d2["value_exact"]["fingerprint"], d1["value_exact"]["fingerprint"])
    assert d1["config"]["fingerprint"]["state_sum_u64"] != d1["value_exact"]["fingerprint"]["state_sum_u64"]      # (two arithmetics, two states)


def test_bench_default_driver_fails_cleanly_with_two_ranks_on_one_device(gpu_lib):
    """default driver = the C++ RCCL one, no fallback: two ranks on the box's one GPU make ncclCommInitRank fail; every rank
    reports it and exits non-zero, no JSON line is printed (what a misconfigured 8-GPU launch would look like)"""
    res = launch_two_ranks(dict(RGPU_BENCH_ONE_DEVICE="1", RGPU_BENCH_BACKEND="gloo"))
    assert res.returncode != 0
    assert "C++ RCCL slab driver could not be created" in res.stderr and "no fallback" in res.stderr, res.stderr[-3000:]
    assert "ncclCommInitRank" in res.stderr, res.stderr[-3000:]
    assert not [l for l in res.stdout.splitlines() if l.startswith("{")]


def test_bench_rank_without_a_device_says_so(gpu_lib):
    """one rank <-> one device (the reference: HydroMpiParameters.cpp:196-201): with one visible GPU rank 1 has none"""
    res = launch_two_ranks(dict(HIP_VISIBLE_DEVICES="0", CUDA_VISIBLE_DEVICES="0"))
    if "only 1 device(s) are visible" not in res.stderr:
        import torch
        if torch.cuda.device_count() > 1:
            pytest.skip("the visibility mask did not take effect on this multi-GPU box")
    assert res.returncode != 0 and "rank 1 is to drive GPU 1 but only 1 device(s) are visible" in res.stderr, res.stderr[-3000:]


def test_both_slab_drivers_in_one_process(gpu_lib):
    """bench.py --gpus N > 1 measures the slabs through BOTH builds of the driver, one after the other in one process (value +
    value_exact at every N): librgpu_comm_fast.so + librgpu_fast.so, destroyed, then librgpu_comm.so + librgpu.so.  The libraries
    export the same symbols, so each pair must stay bound to itself: with one rank (its own z neighbour, real RCCL) the second,
    exact pair has to reproduce the single-device run of librgpu.so bit for bit, and the first must not."""
    code = r'''
import os, sys
import numpy as np
sys.path.insert(0, %r)
import bench
from ramsesgpu_amd.solver import Library, Solver, interior, lib_path
import torch
torch.cuda.set_device(0)
ctl = bench.Control(1, 0, 0)
ini = os.path.join(%r, "configs", "mhd_mri_3d.ini"); ov = "mesh.nx=16;mesh.ny=32;mesh.nz=16"
out = {}
for arith in ("contracted", "exact"):
    run, info, err = bench.slab_driver_run(arith, ini, ov, 0, 1, ctl)
    assert run is not None and err is None and info["ranks"] == 1, (arith, err, info)
    assert run.L.arithmetic == arith
    el = bench.timed_steps(run.oneStepIntegration, run.solver, ctl, 3, 1)
    assert el > 0
    out[arith] = run.local_interior().copy()
    run.close()
L = Library(lib_path("exact")); p = L.params_from_ini(ini, ov); sv = Solver(p, L); sv.start(L.init_condition(ini, ov, p), 4)
ref = interior(sv.getDataHost(), p); sv.close()
assert np.array_equal(out["exact"], ref), int((out["exact"] != ref).sum())
assert not np.array_equal(out["contracted"], ref)
err = float(np.sqrt(((out["contracted"] - ref) ** 2).sum() / (ref ** 2).sum()))
assert err < 1e-12, err
print("OK")
''' % (ROOT, ROOT)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"); env.pop("RGPU_LIB", None); env.pop("RGPU_ARITH", None)
    res = subprocess.run([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=600)
    assert res.returncode == 0 and "OK" in res.stdout, res.stdout[-3000:]
