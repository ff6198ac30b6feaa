"""The PDF monitor measured, modelled on scripts/monitor_maps_bench.py.

  --probe BOX        the kernel-level program, to be run under a kernel trace of its own, one process per box and no counters:

        rocprofv3 --kernel-trace --output-format csv -d OUT -o t -- python scripts/monitor_pdf_bench.py --probe mri-512

                     at step 0 and again after SPREAD_STEPS steps: every entry of probe_plan(box) -- a spec set with a forced
                     "pdf_replicas" / "pdf_groups", or the full z projection of rgpu_state_maps, the yardstick -- PROBE_REPS times in
                     a row: OUT/*kernel_trace.csv holds the dispatches of the monitor_pdf_* and monitor_map_* kernels in that order.
                     Prints, per state and spec set, how many words are not empty (what the lanes of a wave contend for)
  --trace BOX=CSV .. reads those files into the "kernels" rows of --out: per entry the median of count + fold kernel (the first
                     dispatch left out), its ratio to the z projection on the same state, and per state and spec set the fastest
                     setting
  (default)          the cost of a sample inside a run, the modes taking turns in one process, --repeats windows of at least --window
                     seconds each, a host clock around calls that end in a device synchronise; median (min - max):
                        (a) rgpu_run_steps_pdfs, every = 10, the four 1D specs      (c) plain rgpu_run_steps
                     the extra time per sample is 10 x (a - c) per step

    python scripts/monitor_pdf_bench.py [--workloads mri-512,implode3d-256] [--trace mri-512=OUT/t_kernel_trace.csv] --out profiles/monitor_pdf_bench.json

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
    "implode3d-256": ("implode3d", "mesh.nx=256;mesh.ny=256;mesh.nz=256"),
    "implode3d-48": ("implode3d", "mesh.nx=48;mesh.ny=48;mesh.nz=48"),   # (a rehearsal size)
}
PROBE_REPS = 5
SPREAD_STEPS = 30
EVERY = 10
REPLICAS = (1, 2, 4, 8, 16, 32, 64)
GROUPS = (256, 512, 1024, 2048)


def spec_sets(box):
    """one 1D spec, four 1D specs, one joint 125 x 125 spec"""
    rho = ("rho", "lin", 0.5, 1.5, 256) if box.startswith("mri") else ("rho", "lin", 0.0, 1.25, 256)
    four = [rho, ("emag", "log2", -40, 8, 2), ("v2", "log2", -40, 8, 2), ("eint", "log2", -16, 8, 3)]
    joint = (("rho", "lin", rho[2], rho[3], 122), ("eint", "log2", -30, 31, 1))
    return {"one": [rho], "four": four, "joint": [joint]}


def probe_plan(box):
    """[(set name, replicas, groups)]; ("zmap", 0, 0): the full z projection.  Replicas at the automatic grid, grids at the automatic
    replicas; the library clamps a replica count that does not fit the LDS"""
    plan = [("zmap", 0, 0)]
    for name in ("one", "four", "joint"):
        plan += [(name, r, -1) for r in ((1,) if name == "joint" else REPLICAS)] + [(name, -1, g) for g in GROUPS]
    return plan


def context(lib, box):
    base, ov = WORKLOADS[box]
    p = lib.params_from_ini(ini(base), ov)
    sv = Solver(p, lib)
    sv.start(lib.init_condition(ini(base), ov, p), 0)
    return p, sv


def probe(lib, box):
    p, sv = context(lib, box)
    sets = spec_sets(box)
    for state in ("step0", "spread"):
        if state == "spread":
            sv.run_steps(SPREAD_STEPS)
        for name, replicas, groups in probe_plan(box):
            lib.lib.rgpu_set_option(b"pdf_replicas", replicas if name != "zmap" else -1)
            lib.lib.rgpu_set_option(b"pdf_groups", groups if name != "zmap" else -1)
            for _ in range(PROBE_REPS):
                out = sv.state_maps([("z", 0, p.nz)]) if name == "zmap" else sv.state_pdfs(sets[name])
            if name != "zmap" and replicas == 1:
                print(box, state, name, "words not empty:", [int((t != 0).sum()) for t in out], "largest count:", [int(t.max()) for t in out], flush=True)
    lib.lib.rgpu_set_option(b"pdf_replicas", -1)
    lib.lib.rgpu_set_option(b"pdf_groups", -1)
    sv.close()


def kernel_rows(pairs):
    out = []
    for pair in pairs:
        box, path = pair.split("=", 1)
        rows = [r for r in csv.DictReader(open(path)) if "monitor_pdf_" in r["Kernel_Name"] or "monitor_map_" in r["Kernel_Name"]]
        rows.sort(key=lambda r: int(r["Start_Timestamp"]))
        us = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3
        entries, at = {}, 0
        for state in ("step0", "spread"):
            for name, replicas, groups in probe_plan(box):
                per = 1 if name == "zmap" else 2   # a PDF sample is two dispatches: count, fold
                mine = rows[at:at + per * PROBE_REPS]
                at += per * PROBE_REPS
                assert len(mine) == per * PROBE_REPS and all(("monitor_map_" in r["Kernel_Name"]) == (name == "zmap") for r in mine), (state, name, replicas, groups)
                samples = [sum(us(r) for r in mine[k * per:(k + 1) * per]) for k in range(1, PROBE_REPS)]
                e = {"median_us": statistics.median(samples), "min_us": min(samples), "max_us": max(samples)}
                if name != "zmap":
                    e["count_us"] = statistics.median(us(mine[k * per]) for k in range(1, PROBE_REPS))
                    e["fold_us"] = statistics.median(us(mine[k * per + 1]) for k in range(1, PROBE_REPS))
                    e["over_z_projection"] = e["median_us"] / entries["%s zmap" % state]["median_us"]
                key = "%s zmap" % state if name == "zmap" else "%s %s replicas=%d groups=%d" % (state, name, replicas, groups)
                entries[key] = e
        assert at == len(rows), (at, len(rows))
        fastest = {}
        for state in ("step0", "spread"):
            for name in ("one", "four", "joint"):
                mine = {k: e["median_us"] for k, e in entries.items() if k.startswith("%s %s " % (state, name))}
                fastest["%s %s" % (state, name)] = min(mine, key=mine.get)
        out.append({"workload": box, "overrides": WORKLOADS[box][1], "spread_steps": SPREAD_STEPS, "spec_sets": {k: [list(map(list, s)) if isinstance(s[0], tuple) else list(s) for s in v] for k, v in spec_sets(box).items()},
                    "what": "kernel durations in microseconds, rocprofv3 --kernel-trace, %d dispatches per entry, the first left out; a PDF sample is count + fold" % PROBE_REPS,
                    "entries": entries, "fastest": fastest})
    return out


class Run:
    """one context of the workload; mode "a": rgpu_run_steps_pdfs, every EVERY-th step; "c": plain"""

    def __init__(self, lib, box, mode):
        self.mode = mode
        self.p, self.sv = context(lib, box)
        self.specs = spec_sets(box)["four"]
        self.samples = 0

    def run(self, k):
        if self.mode == "a":
            done, s = self.sv.run_steps_pdfs(k, EVERY, self.specs)
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
    ap.add_argument("--workloads", default="mri-512,implode3d-256")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.7, help="seconds per timed window (well above 0.5)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib = None if a.trace and not a.workloads else Library(lib_path(a.arith))   # (reading traces needs no device)
    if a.probe:
        return probe(lib, a.probe)
    result = {"device": "MI355X", "library": os.path.basename(lib_path(a.arith)), "kernels": kernel_rows(a.trace), "rows": []}
    for w in filter(None, a.workloads.split(",")):
        modes = {"a_run_steps_pdfs": Run(lib, w, "a"), "c_run_steps": Run(lib, w, "c")}
        steps = {name: calibrate(mode, a.window) for name, mode in modes.items()}
        secs = {name: [] for name in modes}
        for _ in range(a.repeats):
            for name, mode in modes.items():   # the modes take turns
                dt = timed(mode, steps[name])
                while dt < a.window:   # a window that came in short does not count: more steps, again
                    steps[name] = int(1.3 * steps[name]) + 1
                    dt = timed(mode, steps[name])
                secs[name].append(dt / steps[name])
        row = {"workload": w, "overrides": WORKLOADS[w][1], "arithmetic": a.arith, "every": EVERY, "specs": [list(s) for s in modes["a_run_steps_pdfs"].specs],
               "what": "seconds per step of the whole call, host clock around calls that end in a device synchronise"}
        for name, mode in modes.items():
            s = secs[name]
            row[name] = {"ms_per_step_median": 1e3 * statistics.median(s), "ms_per_step_min": 1e3 * min(s), "ms_per_step_max": 1e3 * max(s), "steps_per_window_last": steps[name],
                         "repeats": len(s), "samples": mode.samples}
        row["a_run_steps_pdfs"]["batch_samples"] = int(lib.lib.rgpu_pdf_batch_samples(modes["a_run_steps_pdfs"].sv.ctx))   # which path ran
        row["sample_cost_ms"] = EVERY * (row["a_run_steps_pdfs"]["ms_per_step_median"] - row["c_run_steps"]["ms_per_step_median"])
        row["sample_cost_over_step"] = row["sample_cost_ms"] / row["c_run_steps"]["ms_per_step_median"]
        for mode in modes.values():
            mode.close()
        result["rows"].append(row)
        print(json.dumps(row), flush=True)
    for k in result["kernels"]:
        print(json.dumps({"workload": k["workload"], "fastest": k["fastest"]}), flush=True)
        for name, e in k["entries"].items():
            print(k["workload"], name, json.dumps(e), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
