"""The plane monitor measured, modelled on scripts/monitor_bench.py and scripts/monitor_kernel_probe.py.

  --probe BOX        the kernel-level program, to be run under a kernel trace of its own, one process per box and no counters:

        rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o t -- python scripts/monitor_planes_bench.py --probe mri-64x128x64

                     three steps, then rgpu_state_monitor_planes and rgpu_state_monitor3d ten times each: OUT/*kernel_stats.csv holds
                     the average duration of monitor_profile_cols_kernel + monitor_profile_planes_kernel (a plane sample) and of
                     monitor_vol_cols_kernel + monitor_vol_planes_kernel (the monitor's sample without its finish kernel) of the SAME run
  --stats BOX=CSV .. reads those files into the "kernels" rows of --out: the four averages, the two sums and their ratio
  (default)          the run-level overhead: cell updates per second of the whole call of
                        (a) rgpu_run_steps_monitored_planes, a sample every --every steps, taken inside the device-clock batches
                        (c) plain rgpu_run_steps
                     the modes taking turns in one process, --repeats windows of at least --window seconds each, a host clock around
                     calls that end in a device synchronise; median (min - max)

    python scripts/monitor_planes_bench.py [--workloads mri-64x128x64,implode3d-256] [--stats mri-64x128x64=OUT/t_kernel_stats.csv] --out profiles/monitor_planes_bench.json

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
from ramsesgpu_amd.solver import Library, Solver, lib_path  # noqa: E402

WORKLOADS = {
    "mri-64x128x64": ("mhd_mri_3d", "mesh.nx=64;mesh.ny=128;mesh.nz=64"),
    "implode3d-256": ("implode3d", "mesh.nx=256;mesh.ny=256;mesh.nz=256"),
    "mri-512": ("mhd_mri_3d", "mesh.nx=512;mesh.ny=512;mesh.nz=512"),
}
KERNELS = ("monitor_profile_cols_kernel", "monitor_profile_planes_kernel", "monitor_vol_cols_kernel", "monitor_vol_planes_kernel")


class Run:
    """one context of the workload; mode "a": monitored planes, "c": plain"""

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
            done, s = sv.run_steps_monitored_planes(k, self.every)
            self.samples += len(s.step)
        else:
            done = sv.run_steps(k)
        if done != k:
            raise RuntimeError("the run stopped early")
        sv.synchronize()

    def close(self):
        self.sv.close()


def probe(lib, box):
    base, ov = WORKLOADS[box]
    p = lib.params_from_ini(ini(base), ov)
    sv = Solver(p, lib)
    sv.start(lib.init_condition(ini(base), ov, p), 0)
    sv.run_steps(3)
    for _ in range(10):
        rows = sv.state_monitor_planes()
        mon = sv.state_monitor()
    print(box, "rows", rows.shape, "mass by planes", float(rows[:, 0].sum()), "by the monitor", float(mon[0]))
    sv.close()


def kernel_rows(pairs):
    out = []
    for pair in pairs:
        box, path = pair.split("=", 1)
        avg, calls = {}, {}
        for r in csv.DictReader(open(path)):
            for k in KERNELS:
                if k in r["Name"]:
                    avg[k], calls[k] = float(r["AverageNs"]) * 1e-3, int(r["Calls"])
        planes = avg["monitor_profile_cols_kernel"] + avg["monitor_profile_planes_kernel"]
        monitor = avg["monitor_vol_cols_kernel"] + avg["monitor_vol_planes_kernel"]
        out.append({"workload": box, "overrides": WORKLOADS[box][1], "what": "average kernel duration in microseconds, rocprofv3 --kernel-trace --stats, one run",
                    "average_us": avg, "calls": calls, "plane_sample_us": planes, "monitor_sample_without_finish_us": monitor, "ratio": planes / monitor})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arith", default="contracted", choices=["exact", "contracted"])
    ap.add_argument("--probe", default=None, help="run the kernel-level program of this box and exit")
    ap.add_argument("--stats", nargs="*", default=[], help="BOX=kernel_stats.csv of a --probe run under rocprofv3")
    ap.add_argument("--workloads", default="mri-64x128x64,implode3d-256")
    ap.add_argument("--every", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.7, help="seconds per timed window (well above 0.5)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib = Library(lib_path(a.arith))
    if a.probe:
        return probe(lib, a.probe)
    result = {"device": "MI355X", "library": os.path.basename(lib.path), "kernels": kernel_rows(a.stats), "rows": []}
    for w in filter(None, a.workloads.split(",")):
        base, ov = WORKLOADS[w]
        modes = {"a_run_steps_monitored_planes": Run(lib, base, ov, "a", a.every), "c_run_steps": Run(lib, base, ov, "c", a.every)}
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
        row = {"workload": w, "overrides": ov, "arithmetic": a.arith, "every": a.every,
               "what": "cell updates per second of the whole call, host clock around calls that end in a device synchronise"}
        for name, mode in modes.items():
            r = rates[name]
            row[name] = {"median": statistics.median(r), "min": min(r), "max": max(r), "steps_per_window_last": steps[name], "window_s_min": min(secs[name]),
                         "us_per_step_median": 1e6 * mode.cells / statistics.median(r), "repeats": len(r), "samples": mode.samples}
        row["a_run_steps_monitored_planes"]["batch_samples"] = int(lib.lib.rgpu_monitor_planes_batch_samples(modes["a_run_steps_monitored_planes"].sv.ctx))   # which path ran
        row["a_over_c"] = row["a_run_steps_monitored_planes"]["median"] / row["c_run_steps"]["median"]
        row["overhead_us_per_step"] = row["a_run_steps_monitored_planes"]["us_per_step_median"] - row["c_run_steps"]["us_per_step_median"]
        for mode in modes.values():
            mode.close()
        result["rows"].append(row)
        print(json.dumps(row), flush=True)
    for k in result["kernels"]:
        print(json.dumps(k), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
