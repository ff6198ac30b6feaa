"""Whole-call step rates of a run, 3D or 2D, that takes a monitor sample every `every` steps:

  (a) rgpu_run_steps_monitored on this build: the samples taken on the device inside the device-clock batches, one read-back per batch
  (b) plain rgpu_run_steps on ANOTHER build (--baseline-lib: the parent commit's librgpu_fast.so)
  (c) plain rgpu_run_steps on this build: against (b) it shows what the plain loop pays for the feature (nothing)
  (d) this build looping rgpu_run_steps(every) + rgpu_state_monitor[3d]: one synchronisation per sample
  (e) this build calling rgpu_state_monitor[3d] alone, again and again: cells monitored per second
  --baseline-all: (a), (d) and (e) on the other build as well, for a change that must leave every mode as fast as it was

    python scripts/monitor_bench.py [--baseline-lib OLD/librgpu_fast.so] [--out profiles/monitor3d_bench.json]

The window scheme is that of scripts/history_bench.py: the modes take turns in one process, --repeats windows each of at least --window
seconds (steps calibrated per mode, in multiples of `every`), a host clock around calls that end in a device synchronise; median
(min - max) of the windows, in cell updates per second of the WHOLE CALL.  --out FILE: the rows of this run (a --reverse run goes to a file of its own).  The
kernel-level numbers of DESIGN 3.4.2 come from scripts/monitor_kernel_probe.py.  Needs a GPU: there is no fallback."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from ensemble_bench import calibrate, ini, older_library, timed  # noqa: E402
from ramsesgpu_amd.solver import Library, Solver, lib_path  # noqa: E402

WORKLOADS = {
    "implode3d-64": ("implode3d", "mesh.nx=64;mesh.ny=64;mesh.nz=64"),
    "implode3d-256": ("implode3d", "mesh.nx=256;mesh.ny=256;mesh.nz=256"),
    "mri-64x128x64": ("mhd_mri_3d", "mesh.nx=64;mesh.ny=128;mesh.nz=64"),
    "mri-256": ("mhd_mri_3d", "mesh.nx=256;mesh.ny=256;mesh.nz=256"),
    "kh2d-512": ("kelvin_helmholtz_gpu_2d", "mesh.nx=512;mesh.ny=512"),
    "kh2d-2048": ("kelvin_helmholtz_gpu_2d", "mesh.nx=2048;mesh.ny=2048"),
    "ot2d-512": ("orszag-tang", "mesh.nx=512;mesh.ny=512"),
    "ot2d-2048": ("orszag-tang", "mesh.nx=2048;mesh.ny=2048"),
}


class Run:
    """one context of the workload; mode "a" / "c" / "d" as above ("c" on the baseline library is (b))"""

    def __init__(self, lib, base, ov, mode, every):
        self.mode, self.every = mode, every
        p = lib.params_from_ini(ini(base), ov)
        self.cells = p.nx * p.ny * p.nz
        self.sv = Solver(p, lib)
        self.sv.start(lib.init_condition(ini(base), ov, p), 0)
        self.samples = 0

    def run(self, k):
        sv = self.sv
        k = max(self.every, k - k % self.every)
        if self.mode == "a":
            done, s = sv.run_steps_monitored(k, self.every)
            self.samples += len(s.step)
        elif self.mode == "c":
            done = sv.run_steps(k)
        elif self.mode == "e":
            for _ in range(k):
                sv.state_monitor()
            self.samples += k
            done = k
        else:
            done = 0
            while done < k:
                n = min(k - done, self.every - sv.nStep % self.every)
                if sv.run_steps(n) != n:
                    break
                done += n
                if sv.nStep % self.every == 0:
                    sv.state_monitor()
                    self.samples += 1
        if done != k:
            raise RuntimeError("the run stopped early")
        sv.synchronize()

    def close(self):
        self.sv.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arith", default="contracted", choices=["exact", "contracted"])
    ap.add_argument("--baseline-lib", default=None, help="another build of the library (the parent commit's): plain rgpu_run_steps on it is mode (b)")
    ap.add_argument("--baseline-all", action="store_true", help="modes (a) and (d) on the baseline library too (it must have them)")
    ap.add_argument("--workloads", default="implode3d-64,mri-64x128x64,implode3d-256,mri-256")
    ap.add_argument("--every", type=int, default=10)
    ap.add_argument("--reverse", action="store_true", help="create the contexts of the modes in the opposite order")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.7, help="seconds per timed window (well above 0.5)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib = Library(lib_path(a.arith))
    base_lib = older_library(a.baseline_lib) if a.baseline_lib else None
    rows = []
    for w in a.workloads.split(","):
        base, ov = WORKLOADS[w]
        # (the contexts are created in this order, --reverse: in the opposite one -- where a context's arrays come to lie moves a rate
        # by a per cent or two at 256^3, as (b) against (c), the same code in two libraries, shows)
        makers = [("a_run_steps_monitored", lambda: Run(lib, base, ov, "a", a.every))]
        if base_lib:
            makers.append(("b_run_steps_baseline", lambda: Run(base_lib, base, ov, "c", a.every)))
        if base_lib and a.baseline_all:
            makers += [("a_baseline", lambda: Run(base_lib, base, ov, "a", a.every)), ("d_baseline", lambda: Run(base_lib, base, ov, "d", a.every)),
                       ("e_baseline", lambda: Run(base_lib, base, ov, "e", a.every))]
        makers += [("c_run_steps", lambda: Run(lib, base, ov, "c", a.every)), ("d_loop_state_monitor3d", lambda: Run(lib, base, ov, "d", a.every)),
                   ("e_state_monitor_alone", lambda: Run(lib, base, ov, "e", a.every))]
        modes = {name: make() for name, make in (makers[::-1] if a.reverse else makers)}
        steps = {name: max(a.every, calibrate(mode, a.window) // a.every * a.every) for name, mode in modes.items()}
        rates, secs = {name: [] for name in modes}, {name: [] for name in modes}
        for _ in range(a.repeats):
            for name, mode in modes.items():   # the modes take turns
                dt = timed(mode, steps[name])
                while dt < a.window:   # a window that came in short does not count: more steps, again
                    steps[name] = (int(1.3 * steps[name]) // a.every + 1) * a.every
                    dt = timed(mode, steps[name])
                secs[name].append(dt)
                rates[name].append(mode.cells * steps[name] / dt)
        row = {"workload": w, "overrides": ov, "arithmetic": a.arith, "every": a.every, "contexts_created": "d c b a" if a.reverse else "a b c d",
               "what": "cell updates per second of the whole call, host clock around calls that end in a device synchronise"}
        for name, mode in modes.items():
            r = rates[name]
            row[name] = {"median": statistics.median(r), "min": min(r), "max": max(r), "steps_per_window_last": steps[name], "window_s_min": min(secs[name]),
                         "us_per_step_median": 1e6 * mode.cells / statistics.median(r), "repeats": len(r), "samples": mode.samples}
        row["a_run_steps_monitored"]["batch_samples"] = int(lib.lib.rgpu_monitor_batch_samples(modes["a_run_steps_monitored"].sv.ctx))   # which path ran
        am, cm, dm = row["a_run_steps_monitored"], row["c_run_steps"], row["d_loop_state_monitor3d"]
        row["a_over_d"] = am["median"] / dm["median"]
        row["a_not_below_d_by_more_than_its_spread"] = am["median"] >= dm["median"] - (dm["max"] - dm["min"])
        if base_lib:
            bm = row["b_run_steps_baseline"]
            row["c_within_b_min_max"] = bm["min"] <= cm["median"] <= bm["max"]
            row["a_over_b"] = am["median"] / bm["median"]
            # no slower than the baseline's median by more than the baseline's own spread (max - min of its windows), mode by mode
            for name, other in (("a_run_steps_monitored", "a_baseline"), ("c_run_steps", "b_run_steps_baseline"), ("d_loop_state_monitor3d", "d_baseline"), ("e_state_monitor_alone", "e_baseline")):
                if other in row:
                    o = row[other]
                    row[name + "_over_baseline"] = row[name]["median"] / o["median"]
                    row[name + "_holds"] = row[name]["median"] >= o["median"] - (o["max"] - o["min"])
        row["a_over_c"] = am["median"] / cm["median"]
        for mode in modes.values():
            mode.close()
        rows.append(row)
        print(json.dumps(row), flush=True)
        if a.out:   # after every workload: a long run that is cut short leaves what it measured
            with open(a.out, "w") as f:
                json.dump({"device": "MI355X", "library": os.path.basename(lib.path), "baseline_library": os.path.basename(a.baseline_lib) if a.baseline_lib else None,
                           "rows": rows}, f, indent=1)
                f.write("\n")


if __name__ == "__main__":
    main()
