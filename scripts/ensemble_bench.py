"""Whole-call rates of M equal 2D boxes on one GPU: (a) one ensemble (rgpu_ensemble_run_steps: one step launch and one clock launch per
round for all members) against (b) the same M boxes as M contexts stepped one after another with rgpu_run_steps.

    python scripts/ensemble_bench.py [--baseline-lib OLD/librgpu_fast.so] [--out profiles/ensemble_bench.json]

Mode (b) uses nothing but the API every earlier version of the library has, so this script also runs on a checkout without the ensemble
(mode (a) is then reported as missing), and --baseline-lib adds mode (b) on ANOTHER build of the library (the parent commit's) to the
same alternation: (a), (b), (b on the baseline) take turns in one process, `--repeats` windows each, every window long enough
(--window seconds, steps calibrated per mode) and ended by a device synchronise.  Numbers are cell updates per second of the WHOLE CALL
(host loop, launches, read-backs included) -- not a kernel's share of peak.  Needs a GPU: there is no fallback.

--single-box (with --baseline-lib) adds (c): ONE box stepped with rgpu_run_steps on this build and on the baseline build, taking turns,
for the 2D step kernels whose bodies the ensemble shares -- Orszag-Tang, Kelvin-Helmholtz and Rayleigh-Taylor (uniform gravity: its
instantiation of the hydro kernel is the one whose register count moved) at --single-size."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from ramsesgpu_amd.solver import Library, Solver, lib_path  # noqa: E402

WORKLOADS = {"kelvin-helmholtz": "kelvin_helmholtz_gpu_2d", "orszag-tang": "orszag-tang", "rayleigh-taylor": "rayleigh_taylor_gpu_2d"}


def ini(base):
    return os.path.join(ROOT, "configs", base + ".ini")


def member_states(lib, base, ov, p, members):
    """the initial condition with a seeded 1e-3 perturbation of density and momenta per member (tests/ensemble_checks.py)"""
    U0 = lib.init_condition(ini(base), ov, p)
    out = []
    for m in range(members):
        rng = np.random.default_rng(7000 + m)
        U = U0.copy()
        U[0] *= 1.0 + 1e-3 * rng.uniform(-1.0, 1.0, U[0].shape)
        for v in (2, 3):
            U[v] += 1e-3 * rng.uniform(-1.0, 1.0, U[v].shape) * U0[0]
        out.append(U)
    return out


class Replicas:
    """mode (b): M contexts, stepped one after another"""

    def __init__(self, lib, p, U0s):
        self.solvers = [Solver(p, lib) for _ in U0s]
        for sv, U in zip(self.solvers, U0s):
            sv.start(U, 0)

    def run(self, k):
        for sv in self.solvers:
            if sv.run_steps(k) != k:
                raise RuntimeError("replica stopped early")
        self.solvers[-1].synchronize()

    def close(self):
        for sv in self.solvers:
            sv.close()


class OneEnsemble:
    """mode (a)"""

    def __init__(self, lib, p, U0s):
        from ramsesgpu_amd.ensemble import Ensemble
        self.ens = Ensemble(p, len(U0s), lib)
        self.ens.start(U0s)
        self.fused = 0

    def run(self, k):
        done, stop, fused = self.ens.run_steps(k)
        if min(done) != k:
            raise RuntimeError("ensemble member stopped early: %s %s" % (done, stop))
        self.fused += fused
        self.ens.member(0).synchronize()

    def close(self):
        self.ens.close()


def timed(mode, k):
    t0 = time.perf_counter()
    mode.run(k)
    return time.perf_counter() - t0


def calibrate(mode, window):
    """warm-up, then the number of steps that fills `window` seconds"""
    mode.run(3)
    k = 8
    while True:
        dt = timed(mode, k)
        if dt > 0.2 * window or k >= 1 << 20:
            return max(8, int(k * 1.15 * window / dt))
        k *= 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arith", default="contracted", choices=["exact", "contracted"])
    ap.add_argument("--baseline-lib", default=None, help="another build of the library (the parent commit's): mode (b) on it joins the alternation")
    ap.add_argument("--workloads", default="kelvin-helmholtz,orszag-tang")
    ap.add_argument("--sizes", default="64,128,256,512")
    ap.add_argument("--members", default="1,8,64")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.7, help="seconds per timed window (well above 0.5)")
    ap.add_argument("--single-box", action="store_true", help="(c): one box, this build against --baseline-lib, taking turns")
    ap.add_argument("--single-size", type=int, default=512)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib = Library(lib_path(a.arith))
    base_lib = Library(a.baseline_lib) if a.baseline_lib else None
    try:
        import ramsesgpu_amd.ensemble  # noqa: F401
        have_ensemble = True
    except ImportError:
        have_ensemble = False
    rows = []
    for w in a.workloads.split(","):
        for size in (int(s) for s in a.sizes.split(",")):
            for M in (int(m) for m in a.members.split(",")):
                ov = "mesh.nx=%d;mesh.ny=%d" % (size, size)
                p = lib.params_from_ini(ini(WORKLOADS[w]), ov)
                U0s = member_states(lib, WORKLOADS[w], ov, p, M)
                modes = {}
                if have_ensemble:
                    modes["a_ensemble"] = OneEnsemble(lib, p, U0s)
                modes["b_replicas"] = Replicas(lib, p, U0s)
                if base_lib:
                    modes["b_replicas_baseline"] = Replicas(base_lib, base_lib.params_from_ini(ini(WORKLOADS[w]), ov), U0s)
                steps = {name: calibrate(mode, a.window) for name, mode in modes.items()}
                rates = {name: [] for name in modes}
                secs = {name: [] for name in modes}
                for _ in range(a.repeats):
                    for name, mode in modes.items():   # the modes take turns
                        dt = timed(mode, steps[name])
                        secs[name].append(dt)
                        rates[name].append(size * size * M * steps[name] / dt)
                row = {"workload": w, "size": size, "members": M, "arithmetic": a.arith, "what": "cell updates per second of the whole call, host clock around calls that end in a device synchronise"}
                for name in modes:
                    r = rates[name]
                    row[name] = {"median": statistics.median(r), "min": min(r), "max": max(r), "steps_per_window": steps[name], "window_s_min": min(secs[name]), "repeats": len(r)}
                if have_ensemble:
                    row["a_ensemble"]["fused_rounds"] = modes["a_ensemble"].fused
                for mode in modes.values():
                    mode.close()
                rows.append(row)
                print(json.dumps(row), flush=True)
    single = []
    if a.single_box and base_lib:
        for w in ("orszag-tang", "kelvin-helmholtz", "rayleigh-taylor"):
            size = a.single_size
            ov = "mesh.nx=%d;mesh.ny=%d" % (size, size)
            p = lib.params_from_ini(ini(WORKLOADS[w]), ov)
            U0s = [lib.init_condition(ini(WORKLOADS[w]), ov, p)]
            modes = {"this_build": Replicas(lib, p, U0s), "baseline": Replicas(base_lib, base_lib.params_from_ini(ini(WORKLOADS[w]), ov), U0s)}
            steps = {name: calibrate(mode, a.window) for name, mode in modes.items()}
            steps = {name: min(steps.values()) for name in modes}   # the same steps on both: the same stretch of the run
            rates = {name: [] for name in modes}
            for _ in range(a.repeats):
                for name, mode in modes.items():
                    rates[name].append(size * size * steps[name] / timed(mode, steps[name]))
            row = {"workload": w, "size": size, "members": 1, "arithmetic": a.arith, "what": "(c) one box, rgpu_run_steps, cell updates per second of the whole call"}
            for name in modes:
                r = rates[name]
                row[name] = {"median": statistics.median(r), "min": min(r), "max": max(r), "steps_per_window": steps[name], "repeats": len(r)}
            for mode in modes.values():
                mode.close()
            single.append(row)
            print(json.dumps(row), flush=True)
    out = {"device": "MI355X", "single_box": single, "library": os.path.basename(lib.path), "baseline_library": os.path.basename(a.baseline_lib) if a.baseline_lib else None, "rows": rows}
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
