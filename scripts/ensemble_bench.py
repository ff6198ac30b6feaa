"""Whole-call rates of M equal 2D boxes on one GPU: (a) one ensemble (rgpu_ensemble_run_steps: one step launch and one clock launch per
round for all members) against (b) the same M boxes as M contexts stepped one after another with rgpu_run_steps.

    python scripts/ensemble_bench.py [--baseline-lib OLD/librgpu_fast.so] [--out profiles/ensemble_bench.json]

Mode (b) uses nothing but the API every earlier version of the library has, so this script also runs on a checkout without the ensemble
(mode (a) is then reported as missing), and --baseline-lib adds mode (b) on ANOTHER build of the library (the parent commit's) to the
same alternation: (a), (b), (b on the baseline) take turns in one process, `--repeats` windows each, every window long enough
(--window seconds, steps calibrated per mode) and ended by a device synchronise.  Numbers are cell updates per second of the WHOLE CALL
(host loop, launches, read-backs included) -- not a kernel's share of peak.  Needs a GPU: there is no fallback.

Parameter scans (rgpu_ensemble_create_scan: one parameter set per member, the members' constants read from a table on the device):
  --member-params   adds (a'): the same equal boxes as (a) with the library option member_params = 1, i.e. the uniform ensemble
                    through the table kernels -- the A/B of the table path against the by-value path; with --baseline-lib also (a) on
                    the baseline build, when that build has the ensemble
  --scan gamma0     adds (s): M boxes whose gamma0 is spread evenly over +-10 % of the ini value, as ONE scan ensemble, and (b_s):
                    the same M parameter sets as M lone contexts stepped one after another (no new API: with --baseline-lib also on
                    the baseline build, which is the column the acceptance of DESIGN 3.6.1 is phrased against)

Monitors (rgpu_ensemble_run_steps_monitored: per-member totals and extrema sampled on the device inside the batches):
  --monitor-every K adds (m): the ensemble of (a) run with sampling every K steps, and (d): what gives a user the same series through
                    the API every build with ensembles has -- rgpu_ensemble_run_steps in pieces of K steps and a download of every
                    member's state after each piece (the reduction in numpy that would follow is NOT timed); with --baseline-lib (d) and
                    (a) also on the baseline build.  The windows of (m) and (d) are whole multiples of K steps.

--single-box (with --baseline-lib) adds (c): ONE box stepped with rgpu_run_steps on this build and on the baseline build, taking turns,
for the 2D step kernels whose bodies the ensemble shares -- Orszag-Tang, Kelvin-Helmholtz and Rayleigh-Taylor (uniform gravity: its
instantiation of the hydro kernel is the one whose register count moved) at --single-size."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from ramsesgpu_amd import _capi  # noqa: E402
from ramsesgpu_amd.solver import Library, Solver, lib_path  # noqa: E402

class _Absent:
    """stands in for an entry point a library of an earlier commit does not export: the binding's declarations go through, a call raises"""

    def __init__(self, name):
        self.name, self.restype, self.argtypes = name, None, None

    def __call__(self, *args):
        raise RuntimeError("%s is not in this build of the library" % self.name)


class _OlderCDLL(ctypes.CDLL):
    def __getattr__(self, name):
        try:
            return super().__getattr__(name)
        except AttributeError:
            if not name.startswith("rgpu"):
                raise
            f = _Absent(name)
            setattr(self, name, f)
            return f


def older_library(path):
    """--baseline-lib: another build of the library, possibly of a commit whose ABI lacks entry points the binding declares"""
    L = Library.__new__(Library)
    L.path, L.lib = path, _OlderCDLL(path)
    _capi.declare_host_api(L.lib)
    _capi.declare_device_api(L.lib)
    return L


def has(lib, name):
    return not isinstance(getattr(lib.lib, name), _Absent)


WORKLOADS = {"kelvin-helmholtz": "kelvin_helmholtz_gpu_2d", "orszag-tang": "orszag-tang", "rayleigh-taylor": "rayleigh_taylor_gpu_2d"}


def ini(base):
    return os.path.join(ROOT, "configs", base + ".ini")


def member_state(lib, base, ov, p, m):
    """the initial condition with a seeded 1e-3 perturbation of density and momenta for member m (tests/ensemble_checks.py)"""
    U0 = lib.init_condition(ini(base), ov, p)
    rng = np.random.default_rng(7000 + m)
    U = U0.copy()
    U[0] *= 1.0 + 1e-3 * rng.uniform(-1.0, 1.0, U[0].shape)
    for v in (2, 3):
        U[v] += 1e-3 * rng.uniform(-1.0, 1.0, U[v].shape) * U0[0]
    return U


def member_states(lib, base, ov, p, members):
    return [member_state(lib, base, ov, p, m) for m in range(members)]


def scan_sets(lib, base, ov, key, members):
    """(s): per member (overrides, parameter set) with `key` (an ini key of section hydro, e.g. gamma0) spread evenly over +-10 % of the ini
    value, in an order that is not monotonic in the member index"""
    v0 = getattr(lib.params_from_ini(ini(base), ov), key)
    order = sorted(range(members), key=lambda m: (m * 37) % members if members > 1 else 0)
    out = []
    for m in range(members):
        v = v0 * (0.9 + 0.2 * (order[m] / (members - 1) if members > 1 else 0.5))
        o = "%s;hydro.%s=%.17g" % (ov, key, v)
        out.append((o, lib.params_from_ini(ini(base), o)))
    return out


class Replicas:
    """mode (b) / (b_s): M contexts, stepped one after another; ps: one parameter set for all, or one per context"""

    def __init__(self, lib, ps, U0s):
        if not isinstance(ps, (list, tuple)):
            ps = [ps] * len(U0s)
        self.solvers = [Solver(p, lib) for p in ps]
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
    """mode (a); member_params: (a'), the library option set around every call; ps a list: (s), a scan ensemble;
    monitor_every = K: (m), sampled every K steps; download_every = K: (d), pieces of K steps, every member downloaded after each"""

    def __init__(self, lib, ps, U0s, member_params=False, monitor_every=0, download_every=0):
        from ramsesgpu_amd.ensemble import Ensemble
        self.lib, self.member_params = lib, member_params
        self.ens = Ensemble.scan(ps, lib) if isinstance(ps, (list, tuple)) else Ensemble(ps, len(U0s), lib)
        self.ens.start(U0s)
        self.fused = 0
        self.monitor_every, self.download_every, self.samples = monitor_every, download_every, 0
        self.piece = monitor_every or download_every   # the windows of (m) and (d) are whole multiples of it
        self.host = np.empty(tuple(self.ens.p.shape)) if download_every else None

    def run(self, k):
        if self.member_params:
            old = self.lib.set_option("member_params", 1)
            try:
                done, stop, fused = self.ens.run_steps(k)
            finally:
                self.lib.set_option("member_params", old)
        elif self.monitor_every:
            done, stop, fused, smp = self.ens.run_steps_monitored(k, self.monitor_every)
            self.samples += sum(len(x.step) for x in smp)
        elif self.download_every:
            done, fused, stop = [0] * self.ens.members, 0, None
            for n in [self.download_every] * (k // self.download_every) + ([k % self.download_every] if k % self.download_every else []):
                d, stop, f = self.ens.run_steps(n)
                done, fused = [a + b for a, b in zip(done, d)], fused + f
                for m in range(self.ens.members):
                    v = self.ens.member(m)
                    v._chk(v.lib.rgpu_download(v.ctx, self.host.ctypes.data, v.nStep % 2), "download")
                    self.samples += 1
        else:
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
            k = max(8, int(k * 1.15 * window / dt))
            piece = getattr(mode, "piece", 0)
            return (k + piece - 1) // piece * piece if piece else k
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
    ap.add_argument("--member-params", action="store_true", help="(a'): the equal boxes of (a) with option member_params = 1 (the table kernels)")
    ap.add_argument("--scan", default=None, metavar="KEY", help="(s) / (b_s): M boxes with hydro.KEY (gamma0) spread over +-10 %% of the ini value")
    ap.add_argument("--monitor-every", type=int, default=0, metavar="K", help="(m) / (d): the ensemble sampled every K steps on the device / run in pieces of K steps with a download of every member")
    ap.add_argument("--no-replicas", action="store_true", help="leave out (b), the equal boxes as lone contexts (profiles/ensemble_bench.json has it)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib = Library(lib_path(a.arith))
    base_lib = older_library(a.baseline_lib) if a.baseline_lib else None
    try:
        import ramsesgpu_amd.ensemble  # noqa: F401
        have_ensemble = True
    except ImportError:
        have_ensemble = False
    have_scan = have_ensemble and hasattr(ramsesgpu_amd.ensemble.Ensemble, "scan")
    base_has_ensemble = bool(base_lib) and has(base_lib, "rgpu_ensemble_create")
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
                if not a.no_replicas:
                    modes["b_replicas"] = Replicas(lib, p, U0s)
                    if base_lib:
                        modes["b_replicas_baseline"] = Replicas(base_lib, base_lib.params_from_ini(ini(WORKLOADS[w]), ov), U0s)
                if a.member_params and have_scan:
                    modes["a_member_params"] = OneEnsemble(lib, p, U0s, member_params=True)
                    if base_has_ensemble:
                        modes["a_ensemble_baseline"] = OneEnsemble(base_lib, base_lib.params_from_ini(ini(WORKLOADS[w]), ov), U0s)
                if a.monitor_every and have_ensemble:
                    K = a.monitor_every
                    modes["m_monitored"] = OneEnsemble(lib, p, U0s, monitor_every=K)
                    modes["d_download"] = OneEnsemble(lib, p, U0s, download_every=K)
                    if base_has_ensemble:
                        pb = base_lib.params_from_ini(ini(WORKLOADS[w]), ov)
                        modes["d_download_baseline"] = OneEnsemble(base_lib, pb, U0s, download_every=K)
                        if "a_ensemble_baseline" not in modes:
                            modes["a_ensemble_baseline"] = OneEnsemble(base_lib, pb, U0s)
                if a.scan:
                    sets = scan_sets(lib, WORKLOADS[w], ov, a.scan, M)
                    Us = [member_state(lib, WORKLOADS[w], o, q, m) for m, (o, q) in enumerate(sets)]   # each set's own initial condition
                    if have_scan:
                        modes["s_scan"] = OneEnsemble(lib, [q for _, q in sets], Us)
                    modes["bs_scan_replicas"] = Replicas(lib, [q for _, q in sets], Us)
                    if base_lib:
                        modes["bs_scan_replicas_baseline"] = Replicas(base_lib, [base_lib.params_from_ini(ini(WORKLOADS[w]), o) for o, _ in sets], Us)
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
                for name, mode in modes.items():
                    if isinstance(mode, OneEnsemble):
                        row[name]["fused_rounds"] = mode.fused
                        if mode.piece:
                            row[name]["every"], row[name]["samples"] = mode.piece, mode.samples
                if a.scan:
                    row["scan"] = {"key": a.scan, "values": [getattr(q, a.scan) for _, q in sets]}
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
