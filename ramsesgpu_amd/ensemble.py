"""An ensemble of 2D boxes on one GPU (rgpu_ensemble_*, include/rgpu.h): members of one shape and one solver configuration, each with
its own state, dt sequence and end time, advanced by one step-kernel launch and one clock-kernel launch per step for all of them.
`Ensemble(p, M)`: M boxes of one parameter set; `Ensemble.scan([p_0, ..])`: a parameter scan, one set per member.
No numerics live here: `Ensemble` owns the C object, `member(m)` is a `Solver` view of one member's borrowed context."""
import ctypes as C

import numpy as np

from . import _capi
from .solver import MonitorSeries, RgpuError, Solver, load_library   # (MonitorSeries: the series of one member out of run_steps_monitored)


class _Member(Solver):
    """a Solver over a context the ensemble owns: every method of Solver works, close() leaves the context alone"""

    def __init__(self, params, library, ctx):
        self.L = library
        self.lib = library.lib
        self.p = params
        self.ctx = C.c_void_p(ctx)
        self.nStep = 0
        self.totalTime = 0.0
        self.dt = 0.0
        self.dt_log = []

    def close(self):
        self.ctx = C.c_void_p()


class Ensemble:
    def __init__(self, params, members, library=None):
        self._create(library, [params] * max(int(members), 1), int(members), scan=False)

    @classmethod
    def scan(cls, params_list, library=None):
        """a parameter scan (rgpu_ensemble_create_scan): member m is created from params_list[m].  The sets share every integer field,
        slope_type and the signs of cIso, Omega0, nu and eta (what selects code or shape); every other double may differ"""
        self = cls.__new__(cls)
        sets = list(params_list)
        self._create(library, sets, len(sets), scan=True)
        return self

    def _create(self, library, sets, members, scan):
        self.L = library or load_library()
        self.lib = _capi.declare_ensemble_api(self.L.lib)
        self.p = sets[0] if sets else None
        self.ens = C.c_void_p()
        self._sets = None
        if scan:
            self._sets = (_capi.RgpuParams * max(len(sets), 1))(*sets)   # kept: device_bytes() asks with the same array
            rc = self.lib.rgpu_ensemble_create_scan(self._sets if sets else None, members, C.byref(self.ens))
        else:
            rc = self.lib.rgpu_ensemble_create(C.byref(self.p), members, C.byref(self.ens))
        if rc:
            msg = self.lib.rgpu_ensemble_last_error(self.ens).decode() if self.ens else "?"
            self.close()
            raise RgpuError("%s failed (%d): %s" % ("rgpu_ensemble_create_scan" if scan else "rgpu_ensemble_create", rc, msg))
        self.members = self.lib.rgpu_ensemble_members(self.ens)
        self._views = [_Member(sets[m], self.L, self.lib.rgpu_ensemble_member(self.ens, m)) for m in range(self.members)]

    def close(self):
        for v in getattr(self, "_views", []):
            v.close()
        self._views = []
        if getattr(self, "ens", None):
            self.lib.rgpu_ensemble_destroy(self.ens)
            self.ens = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def member(self, m):
        """member m as a Solver (upload, getDataHost, compute_dt, state_checksum, oneStepIntegration, run_steps .. on that box alone);
        its nStep / totalTime / dt / dt_log are the ones run_steps of the ensemble keeps"""
        if not 0 <= m < self.members:
            raise IndexError("member %d of %d" % (m, self.members))
        return self._views[m]

    def device_bytes(self):
        if self._sets is not None:
            return int(self.lib.rgpu_ensemble_scan_device_bytes(self._sets, self.members))
        return int(self.lib.rgpu_ensemble_device_bytes(C.byref(self.p), self.members))

    def start(self, U0s):
        """per member what Solver.start(U0, 0) does before its time loop: upload, ghost fill, the copy to the second array"""
        assert len(U0s) == self.members, (len(U0s), self.members)
        for v, U0 in zip(self._views, U0s):
            v.start(U0, 0)

    def monitor(self):
        """rgpu_ensemble_monitor: the ten monitor quantities (_capi.MON_NAMES) of every member's current state, ndarray [members, 10]"""
        out = np.zeros((self.members, _capi.MON_NQ))
        rc = self.lib.rgpu_ensemble_monitor(self.ens, out.ctypes.data_as(_capi.c_double_p))
        if rc:
            raise RgpuError("rgpu_ensemble_monitor failed (%d): %s" % (rc, self.lib.rgpu_ensemble_last_error(self.ens).decode()))
        return out

    def monitor_device_bytes(self):
        return int(self.lib.rgpu_ensemble_monitor_device_bytes(C.byref(self.p), self.members))

    def run_steps_monitored(self, nsteps, every, tEnd=None):
        """rgpu_ensemble_run_steps_monitored: run_steps, and member m sampled on the device after each of its steps that brings its nStep
        to a multiple of `every`.  Returns (done, stop, fused_steps, samples): samples[m] is a MonitorSeries with .step [n], .t [n]
        (the member's time after that step) and .values [n, 10] (columns _capi.MON_NAMES)"""
        return self._run(nsteps, tEnd, int(every))

    def run_steps(self, nsteps, tEnd=None):
        """rgpu_ensemble_run_steps: up to nsteps steps of every member (tEnd: None, one end time for all, or one per member).
        Returns (done, stop, fused_steps): per member the steps taken and 0 or why there were fewer (1: tEnd reached, 2 / 3: its time step
        broke down), and the number of step rounds that went through the fused launch.  Every member view keeps its nStep, totalTime,
        dt and the dt_log of this call."""
        return self._run(nsteps, tEnd, None)[:3]

    def _run(self, nsteps, tEnd, every):
        M, n = self.members, int(nsteps)
        ns = (C.c_int * M)(*[v.nStep for v in self._views])
        ts = (C.c_double * M)(*[v.totalTime for v in self._views])
        ds = (C.c_double * M)(*[v.dt for v in self._views])
        ends = None
        if tEnd is not None:
            ends = (C.c_double * M)(*([float(tEnd)] * M if np.isscalar(tEnd) else [float(x) for x in tEnd]))
        log = (C.c_double * (M * max(n, 1)))()
        done, stop, fused = (C.c_int * M)(), (C.c_int * M)(), C.c_int(0)
        if every is None:
            rc = self.lib.rgpu_ensemble_run_steps(self.ens, n, ends, ns, ts, ds, log, done, stop, C.byref(fused))
            what = "rgpu_ensemble_run_steps"
        else:
            cap = max(n, 0) // max(every, 1) + 1
            mon_n, mon_step = (C.c_int * M)(), np.zeros((M, cap), dtype=np.intc)
            mon_t, mon = np.zeros((M, cap)), np.zeros((M, cap, _capi.MON_NQ))
            rc = self.lib.rgpu_ensemble_run_steps_monitored(self.ens, n, ends, ns, ts, ds, log, done, stop, C.byref(fused), every, mon_n,
                                                            mon_step.ctypes.data_as(C.POINTER(C.c_int)), mon_t.ctypes.data_as(_capi.c_double_p),
                                                            mon.ctypes.data_as(_capi.c_double_p))
            what = "rgpu_ensemble_run_steps_monitored"
        for m, v in enumerate(self._views):
            v.nStep, v.totalTime, v.dt = ns[m], ts[m], ds[m]
            v.dt_log = [log[m * n + i] for i in range(done[m])]
        if rc:
            raise RgpuError("%s failed (%d): %s" % (what, rc, self.lib.rgpu_ensemble_last_error(self.ens).decode()))
        samples = None
        if every is not None:
            samples = [MonitorSeries(mon_step[m, :mon_n[m]].astype(int), mon_t[m, :mon_n[m]].copy(), mon[m, :mon_n[m]].copy()) for m in range(M)]
        return list(done), list(stop), fused.value, samples
