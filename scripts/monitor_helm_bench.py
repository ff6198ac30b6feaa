"""The Helmholtz spectra measured, in the shape of scripts/monitor_spectrum_bench.py.

  --probe BOX        the kernel-level program, to be run under a kernel trace of its own, one process per box and no counters:

        rocprofv3 --kernel-trace --output-format csv -d OUT -o t -- python scripts/monitor_helm_bench.py --probe mri-512

                     after SPREAD_STEPS steps: every entry of PLAN -- the full z projection of rgpu_state_maps and the plain "w"
                     spectrum of rgpu_state_spectra, the yardsticks, then the "w" decomposition of rgpu_state_helm_spectra -- PROBE_REPS
                     times in a row: OUT/*kernel_trace.csv holds the dispatches of the monitor_map_*, monitor_spectrum_* and
                     monitor_helm_* kernels in that order
  --trace BOX=CSV .. reads those files into the "kernels" rows of --out: per entry the median time of a sample (all its dispatches, the
                     first sample left out) and of each kernel alone (per dispatch), and the ratios of the decomposition to the yardsticks
  (default)          the cost of a sample inside a run, the modes taking turns in one process, --repeats windows of at least --window
                     seconds each, a host clock around calls that end in a device synchronise; median (min - max):
                        (a) rgpu_run_steps_helm_spectra, every = 10, the spec "w"      (c) plain rgpu_run_steps
                     the extra time per sample is 10 x (a - c) per step

    python scripts/monitor_helm_bench.py [--workloads mri-512,mri-256] [--trace mri-512=OUT/t_kernel_trace.csv] --out profiles/monitor_helm_bench.json

Needs a GPU: there is no fallback."""
import argparse
import csv
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from ensemble_bench import calibrate, ini, timed  # noqa: E402
from monitor_spectrum_bench import WORKLOADS  # noqa: E402
from ramsesgpu_amd.solver import Library, Solver, lib_path  # noqa: E402

PROBE_REPS = 4
SPREAD_STEPS = 30
EVERY = 10
WEIGHTS = (1, 1, 1)
# entry -> the dispatches of one sample, in order.  The plain spectrum of three channels: two transforms of three passes, one fold.  The
# decomposition: three transforms whose x and y passes are the spectrum monitor's, the z pass of two arrays, the binning pass, the fold
PLAN = [("zmap", 1), ("spectrum_w", 7), ("helm_w", 9)]
KERNELS = ("monitor_spectrum_x_kernel", "monitor_spectrum_y_kernel", "monitor_spectrum_z_kernel", "monitor_spectrum_fold_kernel", "monitor_helm_z_kernel", "monitor_helm_bin_kernel",
           "monitor_helm_fold_kernel")


def context(lib, box):
    base, ov = WORKLOADS[box]
    p = lib.params_from_ini(ini(base), ov)
    sv = Solver(p, lib)
    sv.start(lib.init_condition(ini(base), ov, p), 0)
    return p, sv


def probe(lib, box):
    p, sv = context(lib, box)
    sv.run_steps(SPREAD_STEPS)
    for name, _ in PLAN:
        for _ in range(PROBE_REPS):
            out = sv.state_maps([("z", 0, p.nz)]) if name == "zmap" else sv.state_spectra([("w", WEIGHTS)]) if name == "spectrum_w" else sv.state_helm_spectra([("w", WEIGHTS)])
        if name == "spectrum_w":
            print(box, name, "total power:", float(out[0][0].sum()), "shells:", len(out[0][0]), flush=True)
        if name == "helm_w":
            print(box, name, "solenoidal:", float(out[0][0].sum()), "compressive:", float(out[0][1].sum()), "shells:", len(out[0][0]), flush=True)
    sv.close()


def kernel_rows(pairs):
    out = []
    for pair in pairs:
        box, path = pair.split("=", 1)
        rows = [r for r in csv.DictReader(open(path)) if any(n in r["Kernel_Name"] for n in ("monitor_spectrum_", "monitor_helm_", "monitor_map_"))]
        rows.sort(key=lambda r: int(r["Start_Timestamp"]))
        us = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3
        entries, at = {}, 0
        for name, per in PLAN:
            mine = rows[at:at + per * PROBE_REPS]
            at += per * PROBE_REPS
            assert len(mine) == per * PROBE_REPS and all(("monitor_map_" in r["Kernel_Name"]) == (name == "zmap") for r in mine), name
            samples = [sum(us(r) for r in mine[k * per:(k + 1) * per]) for k in range(1, PROBE_REPS)]
            e = {"median_us": statistics.median(samples), "min_us": min(samples), "max_us": max(samples)}
            for kernel in KERNELS:
                each = [us(r) for r in mine[per:] if kernel in r["Kernel_Name"]]
                if each:
                    e[kernel + "_us"] = statistics.median(each)
                    e[kernel + "_dispatches_per_sample"] = len(each) // (PROBE_REPS - 1)
            entries[name] = e
        assert at == len(rows), (at, len(rows))
        entries["helm_w"]["over_plain_spectrum"] = entries["helm_w"]["median_us"] / entries["spectrum_w"]["median_us"]
        entries["helm_w"]["over_z_projection"] = entries["helm_w"]["median_us"] / entries["zmap"]["median_us"]
        entries["spectrum_w"]["over_z_projection"] = entries["spectrum_w"]["median_us"] / entries["zmap"]["median_us"]
        out.append({"workload": box, "overrides": WORKLOADS[box][1], "spread_steps": SPREAD_STEPS, "weights": list(WEIGHTS),
                    "what": "kernel durations in microseconds, rocprofv3 --kernel-trace, %d samples per entry, the first left out; per-kernel times are per dispatch" % PROBE_REPS,
                    "entries": entries})
    return out


class Run:
    """one context of the workload; mode "a": rgpu_run_steps_helm_spectra, every EVERY-th step; "c": plain"""

    def __init__(self, lib, box, mode):
        self.mode = mode
        self.p, self.sv = context(lib, box)
        self.samples = 0

    def run(self, k):
        if self.mode == "a":
            done, s = self.sv.run_steps_helm_spectra(k, EVERY, [("w", WEIGHTS)])
            self.samples += len(s.step)
        else:
            done = self.sv.run_steps(k)
        if done != k:
            raise RuntimeError("the run stopped early")
        self.sv.synchronize()

    def close(self):
        self.sv.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arith", default="contracted", choices=["exact", "contracted"])
    ap.add_argument("--probe", default=None, help="run the kernel-level program of this box and exit")
    ap.add_argument("--trace", nargs="*", default=[], help="BOX=kernel_trace.csv of a --probe run under rocprofv3")
    ap.add_argument("--workloads", default="mri-512,mri-256")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.7, help="seconds per timed window (well above 0.5)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib = None if a.trace and not a.workloads else Library(lib_path(a.arith))   # (reading traces needs no device)
    if a.probe:
        return probe(lib, a.probe)
    result = {"device": "MI355X", "library": os.path.basename(lib_path(a.arith)), "kernels": kernel_rows(a.trace), "rows": []}
    for w in filter(None, a.workloads.split(",")):
        modes = {"a_run_steps_helm_spectra": Run(lib, w, "a"), "c_run_steps": Run(lib, w, "c")}
        steps = {name: calibrate(mode, a.window) for name, mode in modes.items()}
        secs = {name: [] for name in modes}
        for _ in range(a.repeats):
            for name, mode in modes.items():   # the modes take turns
                dt = timed(mode, steps[name])
                while dt < a.window:   # a window that came in short does not count: more steps, again
                    steps[name] = int(1.3 * steps[name]) + 1
                    dt = timed(mode, steps[name])
                secs[name].append(dt / steps[name])
        row = {"workload": w, "overrides": WORKLOADS[w][1], "arithmetic": a.arith, "every": EVERY, "specs": [["w", list(WEIGHTS)]],
               "what": "seconds per step of the whole call, host clock around calls that end in a device synchronise"}
        for name, mode in modes.items():
            s = secs[name]
            row[name] = {"ms_per_step_median": 1e3 * statistics.median(s), "ms_per_step_min": 1e3 * min(s), "ms_per_step_max": 1e3 * max(s), "steps_per_window_last": steps[name],
                         "repeats": len(s), "samples": mode.samples}
        row["a_run_steps_helm_spectra"]["batch_samples"] = int(lib.lib.rgpu_helm_batch_samples(modes["a_run_steps_helm_spectra"].sv.ctx))   # which path ran
        row["sample_cost_ms"] = EVERY * (row["a_run_steps_helm_spectra"]["ms_per_step_median"] - row["c_run_steps"]["ms_per_step_median"])
        row["sample_cost_over_step"] = row["sample_cost_ms"] / row["c_run_steps"]["ms_per_step_median"]
        for mode in modes.values():
            mode.close()
        result["rows"].append(row)
        print(json.dumps(row), flush=True)
    for k in result["kernels"]:
        for name, e in k["entries"].items():
            print(k["workload"], name, json.dumps(e), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
