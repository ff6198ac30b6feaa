"""Whole-call step rates of the driven-turbulence runs, whose forcing stages ride in the device-clock batches:

  (a) rgpu_run_steps on this build, option "forcing_clock" = 1: the batches
  (c) the same with "forcing_clock" = 0: the literal loop, this build
  (b) rgpu_run_steps on ANOTHER build (--baseline-lib: the parent commit's library): the literal loop as it was
  (s) rgpu_run_steps_spectra with a spectrum of w every --every steps, "forcing_clock" = 1, and (t) the same with 0

    python scripts/forcing_bench.py [--baseline-lib OLD/librgpu_fast.so] [--out profiles/forcing_clock_bench.json]

The option is process-wide and read when a call begins: every mode sets it before its call.  The window scheme is that of
scripts/monitor_bench.py: the modes take turns in one process, --repeats windows each of at least --window seconds (steps calibrated per
mode, in multiples of --every), a host clock around calls that end in a device synchronise; median (min - max) of the windows, in cell
updates per second of the WHOLE CALL.  Conditions written into every row: (a) no slower than (b) by more than (b)'s own spread; (c)
equal to (b) within that spread.  --kernels: no timing -- a few steps of each workload both ways, for a `rocprofv3 --kernel-trace --stats`
run of its own (time per kernel of the kick that carries the scan against the kick plus the stand-alone scan).  Needs a GPU: there is
no fallback."""
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

PERT_OU = "turbulence-Ornstein-Uhlenbeck.initialDensityPerturbationAmplitude=0.1"
PERT_T = "turbulence.initialDensityPerturbationAmplitude=0.1"
WORKLOADS = {
    "hydro_ou-64": ("turbulence_hydro_ou", "mesh.nx=64;mesh.ny=64;mesh.nz=64;" + PERT_OU),
    "hydro-64": ("turbulence_hydro", "mesh.nx=64;mesh.ny=64;mesh.nz=64;" + PERT_T),
    "mhd_ou-128": ("turbulence_mhd_ou", "mesh.nx=128;mesh.ny=128;mesh.nz=128;" + PERT_OU),
    "hydro_ou-256": ("turbulence_hydro_ou", "mesh.nx=256;mesh.ny=256;mesh.nz=256;" + PERT_OU),
    "hydro-256": ("turbulence_hydro", "mesh.nx=256;mesh.ny=256;mesh.nz=256;" + PERT_T),
}


class Run:
    """one context of the workload; clock: the option "forcing_clock" of its calls (None: a library without the option);
    spectra: rgpu_run_steps_spectra with a spectrum of w every `every` steps"""

    def __init__(self, lib, base, ov, clock, every, spectra=False):
        self.lib, self.clock, self.every, self.spectra = lib, clock, every, spectra
        p = lib.params_from_ini(ini(base), ov)
        self.cells = p.nx * p.ny * p.nz
        self.sv = Solver(p, lib)
        F = lib.init_forcing(ini(base), ov, p)
        if F is not None:
            self.sv.set_forcing_field(F)
        self.sv.start(lib.init_condition(ini(base), ov, p), 0)
        self.samples = 0

    def run(self, k):
        sv = self.sv
        k = max(self.every, k - k % self.every)
        if self.clock is not None:
            self.lib.set_option("forcing_clock", self.clock)
        if self.spectra:
            done, s = sv.run_steps_spectra(k, self.every, [("w", (1, 1, 1))])
            self.samples += len(s.step)
        else:
            done = sv.run_steps(k)
        if done != k:
            raise RuntimeError("the run stopped early")
        sv.synchronize()

    def close(self):
        self.sv.close()


def kernels(lib, names, steps):
    for w in names:
        base, ov = WORKLOADS[w]
        for clock in (1, 0):
            r = Run(lib, base, ov, clock, 1)
            r.run(steps)
            print("%s forcing_clock=%d: %d steps, %d of them in batches" % (w, clock, steps, r.sv.forcing_batch_steps()), flush=True)
            r.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arith", default="contracted", choices=["exact", "contracted"])
    ap.add_argument("--baseline-lib", default=None, help="another build of the library (the parent commit's): plain rgpu_run_steps on it is mode (b)")
    ap.add_argument("--workloads", default="hydro_ou-64,hydro-64,mhd_ou-128,hydro_ou-256,hydro-256")
    ap.add_argument("--every", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.7, help="seconds per timed window (well above 0.5)")
    ap.add_argument("--kernels", type=int, default=0, help="no timing: this many steps of each workload with the option 1 and 0, for a kernel trace")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib = Library(lib_path(a.arith))
    if a.kernels:
        return kernels(lib, a.workloads.split(","), a.kernels)
    base_lib = older_library(a.baseline_lib) if a.baseline_lib else None
    rows = []
    for w in a.workloads.split(","):
        base, ov = WORKLOADS[w]
        makers = [("a_forcing_clock_1", lambda: Run(lib, base, ov, 1, a.every))]
        if base_lib:
            makers.append(("b_baseline", lambda: Run(base_lib, base, ov, None, a.every)))
        makers += [("c_forcing_clock_0", lambda: Run(lib, base, ov, 0, a.every)), ("s_spectra_forcing_clock_1", lambda: Run(lib, base, ov, 1, a.every, True)),
                   ("t_spectra_forcing_clock_0", lambda: Run(lib, base, ov, 0, a.every, True))]
        modes = {name: make() for name, make in makers}
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
                         "us_per_step_median": 1e6 * mode.cells / statistics.median(r), "repeats": len(r), "samples": mode.samples,
                         "forcing_batch_steps": mode.sv.forcing_batch_steps() if mode.clock is not None else 0}   # which path ran
        am, cm = row["a_forcing_clock_1"], row["c_forcing_clock_0"]
        row["s_spectra_forcing_clock_1"]["batch_samples"] = int(lib.lib.rgpu_spectrum_batch_samples(modes["s_spectra_forcing_clock_1"].sv.ctx))
        row["a_over_c"] = am["median"] / cm["median"]
        row["s_over_t"] = row["s_spectra_forcing_clock_1"]["median"] / row["t_spectra_forcing_clock_0"]["median"]
        if base_lib:
            bm = row["b_baseline"]
            spread = bm["max"] - bm["min"]
            row["a_over_b"] = am["median"] / bm["median"]
            row["c_over_b"] = cm["median"] / bm["median"]
            row["a_not_below_b_by_more_than_its_spread"] = am["median"] >= bm["median"] - spread
            row["c_equals_b_within_its_spread"] = abs(cm["median"] - bm["median"]) <= spread
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
