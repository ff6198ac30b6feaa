"""The map monitor measured, modelled on scripts/monitor_planes_bench.py.

  --probe BOX        the kernel-level program, to be run under a kernel trace of its own, one process per box and no counters:

        rocprofv3 --kernel-trace --output-format csv -d OUT -o t -- python scripts/monitor_maps_bench.py --probe mri-512

                     three steps, then every entry of probe_plan(box) -- a spec and the kernel that takes it -- PROBE_REPS times in a
                     row through rgpu_state_maps: OUT/*kernel_trace.csv holds the dispatches of the monitor_map_* kernels in that order
  --trace BOX=CSV .. reads those files into the "kernels" rows of --out: per entry the median duration of its dispatches (the first
                     left out), the bytes the map has to read -- the variables of the state over the cells of its range, 8 bytes each
                     -- over that time, for the maps along x the ratio to the z map of the same thickness, and the thickness from
                     which the tiled kernel is the faster one
  (default)          the cost of a sample inside a run, the modes taking turns in one process, --repeats windows of at least --window
                     seconds each, a host clock around calls that end in a device synchronise; median (min - max):
                        (a) rgpu_run_steps_mapped, every = 1, the three maps z:mid y:all x:all
                        (c) plain rgpu_run_steps
                        (p) plain rgpu_run_steps on --baseline-lib, another build of the library (the parent commit's)
                     and, each --repeats times: one rgpu_download, one rgpu_state_maps of the three maps (kernels + the one read-back)

    python scripts/monitor_maps_bench.py [--workloads mri-512,implode3d-256] [--trace mri-512=OUT/t_kernel_trace.csv] --out profiles/monitor_maps_bench.json

Needs a GPU: there is no fallback."""
import argparse
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from ensemble_bench import calibrate, ini, timed  # noqa: E402
from ramsesgpu_amd import _capi  # noqa: E402
from ramsesgpu_amd.solver import Library, Solver, lib_path  # noqa: E402

WORKLOADS = {
    "mri-512": ("mhd_mri_3d", "mesh.nx=512;mesh.ny=512;mesh.nz=512"),
    "implode3d-256": ("implode3d", "mesh.nx=256;mesh.ny=256;mesh.nz=256"),
    "implode3d-48": ("implode3d", "mesh.nx=48;mesh.ny=48;mesh.nz=48"),   # (a rehearsal size)
}
PROBE_REPS = 5
THICKNESS = (1, 2, 4, 8, 16, 64)


def shape(box):
    return tuple(int(kv.split("=")[1]) for kv in WORKLOADS[box][1].split(";"))


def thicknesses(nx):
    return tuple(w for w in THICKNESS if w < nx) + (nx,)


def probe_plan(box):
    """[(name, (axis, lo, hi), map_x_tiled)]: the full maps and a middle slice on each axis, then the sum along x over 1 .. nx cells,
    every map along x with both kernels; -1: not along x"""
    nx, ny, nz = shape(box)
    plan = [("z:all", ("z", 0, nz), -1), ("y:all", ("y", 0, ny), -1), ("z:mid", ("z", nz // 2, nz // 2 + 1), -1), ("y:mid", ("y", ny // 2, ny // 2 + 1), -1)]
    for w in thicknesses(nx):
        lo = (nx - w) // 2
        plan += [("x:%d direct" % w, ("x", lo, lo + w), 0), ("x:%d tiled" % w, ("x", lo, lo + w), 1), ("z:%d" % w, ("z", (nz - min(w, nz)) // 2, (nz - min(w, nz)) // 2 + min(w, nz)), -1)]
    return plan


def three_maps(p):
    return [("z", p.nz // 2, p.nz // 2 + 1), ("y", 0, p.ny), ("x", 0, p.nx)]


def context(lib, box):
    base, ov = WORKLOADS[box]
    p = lib.params_from_ini(ini(base), ov)
    sv = Solver(p, lib)
    sv.start(lib.init_condition(ini(base), ov, p), 0)
    return p, sv


def probe(lib, box):
    p, sv = context(lib, box)
    sv.run_steps(3)
    for name, spec, variant in probe_plan(box):
        lib.lib.rgpu_set_option(b"map_x_tiled", variant)
        for _ in range(PROBE_REPS):
            m, = sv.state_maps([spec])
        print(box, name, m.shape, "rho summed over the map", float(m[0].sum()), flush=True)
    lib.lib.rgpu_set_option(b"map_x_tiled", -1)
    sv.close()


def kernel_rows(pairs, nvar):
    out = []
    for pair in pairs:
        box, path = pair.split("=", 1)
        nx, ny, nz = shape(box)
        rows = [r for r in csv.DictReader(open(path)) if "monitor_map_" in r["Kernel_Name"]]
        rows.sort(key=lambda r: int(r["Start_Timestamp"]))
        plan = probe_plan(box)
        assert len(rows) == PROBE_REPS * len(plan), (len(rows), len(plan))
        entries = {}
        for k, (name, (axis, lo, hi), variant) in enumerate(plan):
            mine = rows[k * PROBE_REPS:(k + 1) * PROBE_REPS]
            kernels = sorted(set(r["Kernel_Name"].split("(")[0].split("::")[-1] for r in mine))
            us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3 for r in mine[1:]]
            cells = (hi - lo) * {"x": ny * nz, "y": nx * nz, "z": nx * ny}[axis]
            nbytes = 8 * nvar[box] * cells
            entries[name] = {"spec": [axis, lo, hi], "kernel": kernels, "median_us": statistics.median(us), "min_us": min(us), "max_us": max(us),
                             "state_bytes": nbytes, "GB_per_s": nbytes / statistics.median(us) * 1e-3}
        crossover = None
        for w in thicknesses(nx):
            d, t, z = (entries[n % w]["median_us"] for n in ("x:%d direct", "x:%d tiled", "z:%d"))
            entries["x:%d direct" % w]["over_z_of_the_same_thickness"] = d / z
            entries["x:%d tiled" % w]["over_z_of_the_same_thickness"] = t / z
            if t < d and crossover is None:
                crossover = w
            if t >= d:
                crossover = None
        out.append({"workload": box, "overrides": WORKLOADS[box][1], "what": "kernel durations in microseconds, rocprofv3 --kernel-trace, %d dispatches per entry, the first left out" % PROBE_REPS,
                    "entries": entries, "tiled_faster_from_thickness": crossover})
    return out


class Run:
    """one context of the workload; mode "a": mapped, every step; "c": plain"""

    def __init__(self, lib, box, mode):
        self.mode = mode
        self.p, self.sv = context(lib, box)
        self.cells = self.p.nx * self.p.ny * self.p.nz
        self.specs = three_maps(self.p)
        self.samples = 0

    def run(self, k):
        sv = self.sv
        if self.mode == "a":
            done, s = sv.run_steps_mapped(k, 1, self.specs)
            self.samples += len(s.step)
        else:
            done = sv.run_steps(k)
        if done != k:
            raise RuntimeError("the run stopped early")
        sv.synchronize()

    def close(self):
        self.sv.close()


def clocked(f, repeats):
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        f()
        out.append(time.perf_counter() - t0)
    return {"median_ms": 1e3 * statistics.median(out), "min_ms": 1e3 * min(out), "max_ms": 1e3 * max(out), "repeats": repeats}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arith", default="contracted", choices=["exact", "contracted"])
    ap.add_argument("--baseline-lib", default=None, help="another build of the library (the parent commit's): plain rgpu_run_steps on it joins the alternation")
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
    nvar = {box: 8 if WORKLOADS[box][0].startswith("mhd") else 5 for box in WORKLOADS}
    result = {"device": "MI355X", "library": os.path.basename(lib_path(a.arith)), "kernels": kernel_rows(a.trace, nvar), "rows": []}
    for w in filter(None, a.workloads.split(",")):
        modes = {"a_run_steps_mapped": Run(lib, w, "a"), "c_run_steps": Run(lib, w, "c")}
        if a.baseline_lib:
            modes["p_run_steps_baseline_lib"] = Run(Library(a.baseline_lib), w, "c")
        steps = {name: calibrate(mode, a.window) for name, mode in modes.items()}
        secs = {name: [] for name in modes}
        for _ in range(a.repeats):
            for name, mode in modes.items():   # the modes take turns
                dt = timed(mode, steps[name])
                while dt < a.window:   # a window that came in short does not count: more steps, again
                    steps[name] = int(1.3 * steps[name]) + 1
                    dt = timed(mode, steps[name])
                secs[name].append(dt / steps[name])
        row = {"workload": w, "overrides": WORKLOADS[w][1], "arithmetic": a.arith, "every": 1, "maps": [list(s) for s in modes["a_run_steps_mapped"].specs],
               "what": "seconds per step of the whole call, host clock around calls that end in a device synchronise"}
        for name, mode in modes.items():
            s = secs[name]
            row[name] = {"ms_per_step_median": 1e3 * statistics.median(s), "ms_per_step_min": 1e3 * min(s), "ms_per_step_max": 1e3 * max(s), "steps_per_window_last": steps[name],
                         "repeats": len(s), "samples": mode.samples}
        A = modes["a_run_steps_mapped"]
        sample_bytes = 8 * _capi.MAP_NQ * sum(n * m for n, m in ((A.p.nx, A.p.ny), (A.p.nx, A.p.nz), (A.p.ny, A.p.nz)))
        budget = lib.lib.rgpu_get_option(b"map_log_kib") * 1024
        slots = min(256 // 1 + 1, budget // sample_bytes)
        row["a_run_steps_mapped"]["batch_samples"] = int(lib.lib.rgpu_map_batch_samples(A.sv.ctx))   # which path ran
        row["sample_cost_ms"] = row["a_run_steps_mapped"]["ms_per_step_median"] - row["c_run_steps"]["ms_per_step_median"]
        row["sample_cost_over_step"] = row["sample_cost_ms"] / row["c_run_steps"]["ms_per_step_median"]
        row["read_back"] = {"sample_bytes": sample_bytes, "log_slots": int(slots), "bytes_per_full_batch": int(slots * sample_bytes)}
        row["download"] = clocked(A.sv.getDataHost, a.repeats)
        row["state_maps_three"] = clocked(lambda: A.sv.state_maps(A.specs), a.repeats)
        row["sample_cost_over_download"] = row["sample_cost_ms"] / row["download"]["median_ms"]
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
