"""Whole-call step rates of an MHD run that records the history row at the run driver's cadence (dtHist = 10 x the initial dt):

  (a) rgpu_run_steps_history on this build: the cadence evaluated and the row formed on the device inside the device-clock batches
  (b) the per-step loop -- rgpu_one_step_integration, and rgpu_history_mri where the reference's condition holds -- which is what a run
      with [history] enabled=yes did before; on this build and, with --baseline-lib, on ANOTHER build (the parent commit's), which is
      the column the acceptance of DESIGN 3.4.1 is phrased against
  (c) rgpu_run_steps without history on this build: what the cadence costs on top of the bare batches, (a) / (c)
  --baseline-all: (a) and (c) on the other build as well, for a change that must leave every mode as fast as it was

    python scripts/history_bench.py [--baseline-lib OLD/librgpu_fast.so] [--out profiles/history_bench.json]

The window scheme is that of scripts/ensemble_bench.py: the modes take turns in one process, --repeats windows each of at least --window
seconds (steps calibrated per mode), a host clock around calls that end in a device synchronise; median (min - max) of the windows, in
cell updates per second of the WHOLE CALL.  The loop of (b) is driven from Python through ctypes (a few microseconds per call, against
steps of 40 us and more).  Needs a GPU: there is no fallback."""
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
    "mri-shipped": ("mhd_mri_3d", ""),
    "mri-128x256x128": ("mhd_mri_3d", "mesh.nx=128;mesh.ny=256;mesh.nz=128"),
    "mri-512": ("mhd_mri_3d", "mesh.nx=512;mesh.ny=512;mesh.nz=512"),
    "orszag-tang-512": ("orszag-tang", "mesh.nx=512;mesh.ny=512"),
}


def due(t, dt, tHist, dtHist):
    return tHist == 0 or ((t - dt <= tHist + dtHist) and (t > tHist + dtHist))


class Run:
    """one context of the workload; mode "a" / "b" / "c" as above"""

    def __init__(self, lib, base, ov, mode):
        self.mode = mode
        p = lib.params_from_ini(ini(base), ov)
        self.cells = p.nx * p.ny * (p.nz if p.three_d else 1)
        self.sv = Solver(p, lib)
        self.sv.start(lib.init_condition(ini(base), ov, p), 0)
        self.sv.dt = self.sv.compute_dt(0)          # the run driver's "Initial dt"
        self.dtHist = 10 * self.sv.dt
        self.samples = 0

    def run(self, k):
        sv = self.sv
        if self.mode == "a":
            done, s, t, d, v = sv.run_steps_history(k, self.dtHist)
            self.samples += len(s)
        elif self.mode == "c":
            done = sv.run_steps(k)
        else:
            for _ in range(k):
                if due(sv.totalTime, sv.dt, sv.tHist, self.dtHist):
                    sv.history_mri()
                    sv.tHist += self.dtHist
                    self.samples += 1
                sv.oneStepIntegration()
            done = k
        if done != k:
            raise RuntimeError("the run stopped early")
        sv.synchronize()

    def close(self):
        self.sv.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arith", default="contracted", choices=["exact", "contracted"])
    ap.add_argument("--baseline-lib", default=None, help="another build of the library (the parent commit's): mode (b) on it joins the alternation")
    ap.add_argument("--baseline-all", action="store_true", help="modes (a) and (c) on the baseline library too (it must have them)")
    ap.add_argument("--reverse", action="store_true", help="create the contexts of the modes in the opposite order")
    ap.add_argument("--workloads", default="mri-shipped,mri-128x256x128,orszag-tang-512,mri-512")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.7, help="seconds per timed window (well above 0.5)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib = Library(lib_path(a.arith))
    base_lib = older_library(a.baseline_lib) if a.baseline_lib else None
    rows = []
    for w in a.workloads.split(","):
        base, ov = WORKLOADS[w]
        makers = [("a_run_steps_history", lambda: Run(lib, base, ov, "a")), ("b_per_step", lambda: Run(lib, base, ov, "b"))]
        if base_lib:
            makers.append(("b_per_step_baseline", lambda: Run(base_lib, base, ov, "b")))
        if base_lib and a.baseline_all:
            makers += [("a_baseline", lambda: Run(base_lib, base, ov, "a")), ("c_baseline", lambda: Run(base_lib, base, ov, "c"))]
        makers.append(("c_run_steps", lambda: Run(lib, base, ov, "c")))
        modes = {name: make() for name, make in (makers[::-1] if a.reverse else makers)}
        steps = {name: calibrate(mode, a.window) for name, mode in modes.items()}
        rates, secs = {name: [] for name in modes}, {name: [] for name in modes}
        for _ in range(a.repeats):
            for name, mode in modes.items():   # the modes take turns
                dt = timed(mode, steps[name])
                while dt < a.window:   # a window that came in short (the calibration ran slower) does not count: more steps, again
                    steps[name] = int(1.3 * steps[name]) + 1
                    dt = timed(mode, steps[name])
                secs[name].append(dt)
                rates[name].append(mode.cells * steps[name] / dt)
        row = {"workload": w, "overrides": ov, "arithmetic": a.arith, "dtHist": "10 x the initial dt", "contexts_created": "reversed" if a.reverse else "as listed",
               "acceptance": "a_min_above_b_max: min of (a) above max of (b) on the baseline build (this build's (b) without --baseline-lib)",
               "what": "cell updates per second of the whole call, host clock around calls that end in a device synchronise"}
        for name, mode in modes.items():
            r = rates[name]
            row[name] = {"median": statistics.median(r), "min": min(r), "max": max(r), "steps_per_window_last": steps[name], "window_s_min": min(secs[name]),
                         "us_per_step_median": 1e6 * mode.cells / statistics.median(r), "repeats": len(r), "samples": mode.samples}
        if "a_run_steps_history" in row:
            ref = row.get("b_per_step_baseline", row["b_per_step"])
            row["a_over_b"] = row["a_run_steps_history"]["median"] / ref["median"]
            row["a_min_above_b_max"] = row["a_run_steps_history"]["min"] > ref["max"]
            row["a_over_c"] = row["a_run_steps_history"]["median"] / row["c_run_steps"]["median"]
        # no slower than the baseline's median by more than the baseline's own spread (max - min of its windows), mode by mode
        for name, other in (("a_run_steps_history", "a_baseline"), ("b_per_step", "b_per_step_baseline"), ("c_run_steps", "c_baseline")):
            if other in row:
                o = row[other]
                row[name + "_over_baseline"] = row[name]["median"] / o["median"]
                row[name + "_holds"] = row[name]["median"] >= o["median"] - (o["max"] - o["min"])
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
