"""The spectrum monitor measured, modelled on scripts/monitor_pdf_bench.py.

  --probe BOX        the kernel-level program, to be run under a kernel trace of its own, one process per box and no counters:

        rocprofv3 --kernel-trace --output-format csv -d OUT -o t -- python scripts/monitor_spectrum_bench.py --probe mri-512

                     after SPREAD_STEPS steps: every entry of probe_plan() -- a spec set with a forced "spectrum_tile_y", or the full z
                     projection of rgpu_state_maps, the family's yardstick -- PROBE_REPS times in a row: OUT/*kernel_trace.csv holds the
                     dispatches of the monitor_spectrum_* and monitor_map_* kernels in that order
  --trace BOX=CSV .. reads those files into the "kernels" rows of --out: per entry the median time of a sample (all its dispatches, the
                     first sample left out), of each pass alone (per transform), its ratio to the z projection, and the traffic model --
                     the bytes a pass must move over the time it took
  (default)          the cost of a sample inside a run, the modes taking turns in one process, --repeats windows of at least --window
                     seconds each, a host clock around calls that end in a device synchronise; median (min - max):
                        (a) rgpu_run_steps_spectra, every = 10, the spec "w"      (c) plain rgpu_run_steps
                     the extra time per sample is 10 x (a - c) per step

    python scripts/monitor_spectrum_bench.py [--workloads mri-512,mri-256] [--trace mri-512=OUT/t_kernel_trace.csv] --out profiles/monitor_spectrum_bench.json

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
    "mri-512": ("mhd_mri_3d", "mesh.nx=512;mesh.ny=512;mesh.nz=512"),
    "mri-256": ("mhd_mri_3d", "mesh.nx=256;mesh.ny=256;mesh.nz=256"),
    "mri-32": ("mhd_mri_3d", "mesh.nx=32;mesh.ny=32;mesh.nz=32"),   # (a rehearsal size)
}
PROBE_REPS = 4
SPREAD_STEPS = 30
EVERY = 10
SPEC_SETS = {"w": [("w", (1, 1, 1))], "w_b_rho": [("w", (1, 1, 1)), ("b", (1, 1, 1)), (("rho",), (1, 1, 1))]}
TRANSFORMS = {"w": 2, "w_b_rho": 5}   # three channels in two transforms; 2 + 2 + 1
FOLDS = {"w": 1, "w_b_rho": 3}
PASSES = ("monitor_spectrum_x_kernel", "monitor_spectrum_y_kernel", "monitor_spectrum_z_kernel", "monitor_spectrum_fold_kernel")
# what a pass must move per cell and transform, in bytes: x reads the density and two momenta and writes Z; y reads and writes Z; z reads Z
MODEL_BYTES = {"monitor_spectrum_x_kernel": 3 * 8 + 16, "monitor_spectrum_y_kernel": 32, "monitor_spectrum_z_kernel": 16}


def probe_plan():
    """[(set name, spectrum_tile_y)]; ("zmap", -1): the full z projection"""
    return [("zmap", -1), ("w", -1), ("w_b_rho", -1), ("w", 0), ("w", 2), ("w", 3)]


def context(lib, box):
    base, ov = WORKLOADS[box]
    p = lib.params_from_ini(ini(base), ov)
    sv = Solver(p, lib)
    sv.start(lib.init_condition(ini(base), ov, p), 0)
    return p, sv


def probe(lib, box):
    p, sv = context(lib, box)
    sv.run_steps(SPREAD_STEPS)
    for name, logw in probe_plan():
        lib.lib.rgpu_set_option(b"spectrum_tile_y", logw)
        for _ in range(PROBE_REPS):
            out = sv.state_maps([("z", 0, p.nz)]) if name == "zmap" else sv.state_spectra(SPEC_SETS[name])
        if name != "zmap":
            print(box, name, logw, "total power per spec:", [float(P.sum()) for P, M in out], "shells:", [len(P) for P, M in out], flush=True)
    lib.lib.rgpu_set_option(b"spectrum_tile_y", -1)
    sv.close()


def kernel_rows(pairs):
    out = []
    for pair in pairs:
        box, path = pair.split("=", 1)
        cells = 1
        for f in WORKLOADS[box][1].split(";"):
            cells *= int(f.split("=")[1])
        rows = [r for r in csv.DictReader(open(path)) if "monitor_spectrum_" in r["Kernel_Name"] or "monitor_map_" in r["Kernel_Name"]]
        rows.sort(key=lambda r: int(r["Start_Timestamp"]))
        us = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3
        entries, at = {}, 0
        for name, logw in probe_plan():
            per = 1 if name == "zmap" else 3 * TRANSFORMS[name] + FOLDS[name]
            mine = rows[at:at + per * PROBE_REPS]
            at += per * PROBE_REPS
            assert len(mine) == per * PROBE_REPS and all(("monitor_map_" in r["Kernel_Name"]) == (name == "zmap") for r in mine), (name, logw)
            samples = [sum(us(r) for r in mine[k * per:(k + 1) * per]) for k in range(1, PROBE_REPS)]
            e = {"median_us": statistics.median(samples), "min_us": min(samples), "max_us": max(samples)}
            if name != "zmap":
                for kernel in PASSES:
                    each = [us(r) for r in mine[per:] if kernel in r["Kernel_Name"]]
                    e[kernel + "_us"] = statistics.median(each)
                    if kernel in MODEL_BYTES:
                        e[kernel + "_model_GBps"] = MODEL_BYTES[kernel] * cells / (statistics.median(each) * 1e-6) / 1e9
                e["over_z_projection"] = e["median_us"] / entries["zmap"]["median_us"]
            entries["zmap" if name == "zmap" else "%s tile_y=%d" % (name, logw)] = e
        assert at == len(rows), (at, len(rows))
        out.append({"workload": box, "overrides": WORKLOADS[box][1], "spread_steps": SPREAD_STEPS, "spec_sets": {k: [[s[0] if isinstance(s[0], str) else list(s[0]), list(s[1])] for s in v] for k, v in SPEC_SETS.items()},
                    "what": "kernel durations in microseconds, rocprofv3 --kernel-trace, %d samples per entry, the first left out; a sample is 3 dispatches per transform and a fold per spec; "
                            "per-pass times are per dispatch; model_GBps: the bytes the pass must move per transform (x: 40 B / cell, y: 32, z: 16) over its time" % PROBE_REPS,
                    "entries": entries})
    return out


class Run:
    """one context of the workload; mode "a": rgpu_run_steps_spectra, every EVERY-th step; "c": plain"""

    def __init__(self, lib, box, mode):
        self.mode = mode
        self.p, self.sv = context(lib, box)
        self.specs = SPEC_SETS["w"]
        self.samples = 0

    def run(self, k):
        if self.mode == "a":
            done, s = self.sv.run_steps_spectra(k, EVERY, self.specs)
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
        modes = {"a_run_steps_spectra": Run(lib, w, "a"), "c_run_steps": Run(lib, w, "c")}
        steps = {name: calibrate(mode, a.window) for name, mode in modes.items()}
        secs = {name: [] for name in modes}
        for _ in range(a.repeats):
            for name, mode in modes.items():   # the modes take turns
                dt = timed(mode, steps[name])
                while dt < a.window:   # a window that came in short does not count: more steps, again
                    steps[name] = int(1.3 * steps[name]) + 1
                    dt = timed(mode, steps[name])
                secs[name].append(dt / steps[name])
        row = {"workload": w, "overrides": WORKLOADS[w][1], "arithmetic": a.arith, "every": EVERY, "specs": [["w", [1, 1, 1]]],
               "what": "seconds per step of the whole call, host clock around calls that end in a device synchronise"}
        for name, mode in modes.items():
            s = secs[name]
            row[name] = {"ms_per_step_median": 1e3 * statistics.median(s), "ms_per_step_min": 1e3 * min(s), "ms_per_step_max": 1e3 * max(s), "steps_per_window_last": steps[name],
                         "repeats": len(s), "samples": mode.samples}
        row["a_run_steps_spectra"]["batch_samples"] = int(lib.lib.rgpu_spectrum_batch_samples(modes["a_run_steps_spectra"].sv.ctx))   # which path ran
        row["sample_cost_ms"] = EVERY * (row["a_run_steps_spectra"]["ms_per_step_median"] - row["c_run_steps"]["ms_per_step_median"])
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
