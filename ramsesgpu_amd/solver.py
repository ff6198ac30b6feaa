"""Python mirror of the reference's run-class interface on top of the C ABI (include/rgpu.h).

`Solver` keeps the reference's method names and argument meaning for the path in scope
(HydroRunBase / MHDRunBase / *RunGodunov): make_all_boundaries, compute_dt(useU), godunov_unsplit(nStep, dt),
oneStepIntegration, copyGpuToCpu / getDataHost.  No numerics live here: every call goes to librgpu.so, which
fails loudly (RGPU_ENODEVICE) when there is no GPU.
"""
import collections
import ctypes as C
import os

import numpy as np

from . import _capi
from ._capi import RgpuParams

_HERE = os.path.dirname(os.path.abspath(__file__))

# the series out of run_steps_monitored (of a Solver, of one member of an Ensemble): step numbers [n], times [n], values [n, 10]
# (columns _capi.MON_NAMES); out of run_steps_monitored_planes: values [n, nz, 16] (columns _capi.MONP_NAMES)
MonitorSeries = collections.namedtuple("MonitorSeries", "step t values")
# the series out of run_steps_mapped: step numbers [n], times [n], and per spec an array [n, 12, nv, nu] (channels _capi.MAP_NAMES)
MapSeries = collections.namedtuple("MapSeries", "step t maps")
# the series out of run_steps_pdfs: step numbers [n], times [n], and per spec an array of uint64 [n, na + 3] or [n, na + 3, nb + 3]
PdfSeries = collections.namedtuple("PdfSeries", "step t pdfs")
# the series out of run_steps_spectra: step numbers [n], times [n], and per spec the power [n, S] and the mode counts [n, S]
SpectrumSeries = collections.namedtuple("SpectrumSeries", "step t power modes")
# the shorthands of a spec's channels
SPECTRUM_GROUPS = {"v": ("vx", "vy", "vz"), "w": ("wx", "wy", "wz"), "b": ("bx", "by", "bz"), "m": ("mx", "my", "mz")}


def spectrum_spec(spec):
    """a spec of a spectrum as _capi.RgpuSpectrumSpec, from one, or from (channels, (wx, wy, wz)) -- the channels one name or several of
    _capi.SPECTRUM_NAMES or of the shorthands "v", "w", "b", "m" (all three components), or the bit mask itself"""
    if isinstance(spec, _capi.RgpuSpectrumSpec):
        return spec
    channels, weights = spec
    if isinstance(channels, int):
        mask = channels
    else:
        mask = 0
        for name in ((channels,) if isinstance(channels, str) else channels):
            for ch in SPECTRUM_GROUPS.get(name, (name,)):
                mask |= 1 << _capi.SPECTRUM_NAMES.index(ch)
    wx, wy, wz = (int(w) for w in weights)
    return _capi.RgpuSpectrumSpec(mask, wx, wy, wz)


# the series out of run_steps_helm_spectra: step numbers [n], times [n], and per spec the solenoidal power, the compressive power and
# the mode counts, each [n, S]
HelmSeries = collections.namedtuple("HelmSeries", "step t solenoidal compressive modes")


def helm_spec(spec):
    """a spec of a Helmholtz spectrum as _capi.RgpuHelmSpec, from one, or from (field, (wx, wy, wz)) -- the field one of
    _capi.HELM_NAMES ("m", "v", "w", "b") or its index"""
    if isinstance(spec, _capi.RgpuHelmSpec):
        return spec
    field, weights = spec
    wx, wy, wz = (int(w) for w in weights)
    return _capi.RgpuHelmSpec(field if isinstance(field, int) else _capi.HELM_NAMES.index(field), wx, wy, wz)


def spectrum_shells(shape, weights):
    """(S, M) of the weights (wx, wy, wz) on a box of shape (nx, ny, nz), from the integer rule of include/rgpu.h ("spectrum monitors")
    without a context: the number of shells and the modes of each, numpy.int64 [S].  Shell s holds the q = (wx kx)^2 + (wy ky)^2 +
    (wz kz)^2 with s^2 - s + 1 <= q <= s^2 + s, the wave numbers folded to -n / 2 .. n / 2 - 1"""
    q1 = []
    for n, w in zip(shape, weights):
        k = np.arange(int(n), dtype=np.int64)
        q1.append((int(w) * np.minimum(k, int(n) - k)) ** 2)
    shell = lambda q: (lambda r: np.where(q <= r * r + r, r, r + 1))(_isqrt(q))
    S = int(shell(np.array([sum(int(a.max()) for a in q1)], dtype=np.int64))[0]) + 1
    M = np.zeros(S, dtype=np.int64)
    # the modes (kx, ky) by their distinct q, then one pass over kz per distinct value
    vx, cx = np.unique(q1[0], return_counts=True)
    vy, cy = np.unique(q1[1], return_counts=True)
    vz, cz = np.unique(q1[2], return_counts=True)
    flat = (vx[:, None] + vy[None, :]).ravel()
    order = np.argsort(flat, kind="stable")
    qxy, start = np.unique(flat[order], return_index=True)
    cxy = np.add.reduceat((cx[:, None] * cy[None, :]).ravel()[order], start)
    for q, c in zip(vz, cz):
        np.add.at(M, shell(qxy + q), cxy * c)
    return S, M


def _isqrt(q):
    """floor(sqrt(q)) of non-negative int64, exact: the rounded root put right in integers"""
    r = np.floor(np.sqrt(q.astype(np.float64))).astype(np.int64)
    r = np.where(r * r > q, r - 1, r)
    return np.where((r + 1) * (r + 1) <= q, r + 1, r)


def pdf_axis(axis):
    """an axis of a PDF as _capi.RgpuPdfAxis, from one, or from (channel, "lin", lo, hi, nbins) / (channel, "log2", emin, emax, sub) --
    the channel a name of _capi.PDF_NAMES or its index; "log2": octave bins on |x| from 2^emin to 2^emax, 2^sub sub-bins each"""
    if isinstance(axis, _capi.RgpuPdfAxis):
        return axis
    ch, scale, a, b, n = axis
    ch = _capi.PDF_NAMES.index(ch) if isinstance(ch, str) else int(ch)
    if scale == "lin":
        return _capi.RgpuPdfAxis(ch, 0, int(n), 0, float(a), float(b))
    if scale != "log2":
        raise ValueError('the scale of a PDF axis is "lin" or "log2"')
    return _capi.RgpuPdfAxis(ch, 1, max(int(b) - int(a), 0) << int(n), int(n), float(np.ldexp(1.0, int(a))), float(np.ldexp(1.0, int(b))))


def pdf_edges(axis):
    """the nbins + 1 edges of the bins of an axis: exact for octave bins (every edge is a double), the nominal lo + b (hi - lo) / nbins
    for linear ones (the library classifies by (x - lo) * (nbins / (hi - lo)), include/rgpu.h)"""
    a = pdf_axis(axis)
    b = np.arange(a.nbins + 1)
    if a.scale == 0:
        return a.lo + b * (a.hi - a.lo) / a.nbins
    return np.ldexp(a.lo * (1.0 + (b % (1 << a.sub)) / float(1 << a.sub)), b >> a.sub)


def lib_path(arithmetic=None):
    """in-tree location of the product library (built by __graft_entry__.build / ramsesgpu_amd/build.py).
    arithmetic: "exact" (librgpu.so: bit-identical to the reference) or "contracted" (librgpu_fast.so: FMA contraction,
    division within 18 ulp, square root within 1 ulp; agrees with the reference to round-off); default from $RGPU_ARITH, else exact."""
    if os.environ.get("RGPU_LIB"):   # an experiment build (scripts/)
        return os.environ["RGPU_LIB"]
    arithmetic = arithmetic or os.environ.get("RGPU_ARITH", "exact")
    if arithmetic not in ("exact", "contracted"):
        raise ValueError("arithmetic must be 'exact' or 'contracted', not %r" % (arithmetic,))
    return os.path.join(_HERE, "librgpu.so" if arithmetic == "exact" else "librgpu_fast.so")


class RgpuError(RuntimeError):
    pass


def _init_torch_hip_first():
    """The PyTorch-ROCm wheel bundles its own libamdhip64 (same SONAME as /opt/rocm's).  A process must end up with
    ONE HIP runtime, or torch sees "No HIP GPUs" and torch-owned device pointers (slab driver) are foreign to our
    kernels.  Whoever loads first wins, so let torch initialise HIP before librgpu.so is dlopen'ed; librgpu.so's
    DT_NEEDED libamdhip64.so.7 then resolves to the already loaded runtime.  No-op without torch / without a GPU."""
    if os.environ.get("RGPU_NO_TORCH_PRELOAD"):
        return
    try:
        import torch
        if torch.cuda.is_available():
            torch.cuda.init()
    except Exception:
        pass


class Library:
    """A loaded C-ABI library (product: librgpu.so)."""

    def __init__(self, path):
        if not os.path.exists(path):
            raise RgpuError("%s not found: build it first (python -c 'import __graft_entry__ as g; g.build()')" % path)
        self.path = path
        _init_torch_hip_first()
        self.lib = C.CDLL(path)
        _capi.declare_host_api(self.lib)
        _capi.declare_device_api(self.lib)

    @property
    def backend(self):
        return self.lib.rgpu_backend_name().decode()

    @property
    def arithmetic(self):
        """"exact" or "contracted" (see lib_path)"""
        return self.lib.rgpu_arithmetic().decode()

    def set_option(self, name, value):
        """diagnostic option of the library (include/rgpu.h, "Environment and options"); returns the previous value"""
        old = self.lib.rgpu_set_option(name.encode(), int(value))
        if old < 0 and self.lib.rgpu_get_option(name.encode()) != int(value):
            raise RgpuError("unknown option %r" % name)
        return old

    def get_option(self, name):
        return self.lib.rgpu_get_option(name.encode())

    # ---- host side: parameter file and initial condition ------------------------------------------------------
    def params_from_ini(self, ini_path, overrides="", slab=None):
        p = RgpuParams()
        err = C.create_string_buffer(512)
        ov = overrides or ""
        if slab is not None:
            ov = (ov + ";" if ov else "") + "slab.rank=%d;slab.count=%d" % slab
        rc = self.lib.rgpuh_params_from_ini(ini_path.encode(), ov.encode(), C.byref(p), err, 512)
        if rc:
            raise RgpuError("params_from_ini(%s): %s" % (ini_path, err.value.decode()))
        return p

    def run_settings(self, ini_path, overrides=""):
        n, t, o = C.c_int(), C.c_double(), C.c_int()
        err = C.create_string_buffer(512)
        rc = self.lib.rgpuh_run_settings(ini_path.encode(), (overrides or "").encode(), C.byref(n), C.byref(t), C.byref(o), err, 512)
        if rc:
            raise RgpuError(err.value.decode())
        return {"nStepmax": n.value, "tEnd": t.value, "nOutput": o.value}

    def init_condition(self, ini_path, overrides, params):
        U = np.zeros(params.shape, dtype=np.float64)
        err = C.create_string_buffer(512)
        rc = self.lib.rgpuh_init_condition(ini_path.encode(), (overrides or "").encode(), C.byref(params), U.ctypes.data, err, 512)
        if rc:
            raise RgpuError("init_condition: %s" % err.value.decode())
        return U

    def init_forcing(self, ini_path, overrides, params):
        """static driving field [3][ksize][jsize][isize] of the "turbulence" problem (params.randomForcingEnabled), else None"""
        if not int(params.randomForcingEnabled):
            return None
        F = np.zeros((3,) + tuple(params.shape[1:]), dtype=np.float64)
        err = C.create_string_buffer(512)
        rc = self.lib.rgpuh_init_forcing(ini_path.encode(), (overrides or "").encode(), C.byref(params), F.ctypes.data, err, 512)
        if rc < 0:
            raise RgpuError("init_forcing: %s" % err.value.decode())
        return F if rc == 1 else None

    def init_gravity(self, ini_path, overrides, params):
        """static gravity field [3][ksize][jsize][isize] of the problems that define one (params.gravityEnabled == 2),
        else None"""
        if int(params.gravityEnabled) != 2:
            return None
        G = np.zeros((3,) + tuple(params.shape[1:]), dtype=np.float64)
        err = C.create_string_buffer(512)
        rc = self.lib.rgpuh_init_gravity(ini_path.encode(), (overrides or "").encode(), C.byref(params), G.ctypes.data, err, 512)
        if rc < 0:
            raise RgpuError("init_gravity: %s" % err.value.decode())
        return G if rc == 1 else None


_default = None


def load_library(path=None):
    global _default
    if path is None:
        if _default is None:
            _default = Library(lib_path())
        return _default
    return Library(path)


class Solver:
    """One run object == one rgpu_ctx (one GPU / one z-slab)."""

    def __init__(self, params, library=None, external_state=None, stream=0):
        self.L = library or load_library()
        self.lib = self.L.lib
        self.p = params
        self.ctx = C.c_void_p()
        if external_state is None:
            rc = self.lib.rgpu_create(C.byref(params), C.byref(self.ctx))
        else:
            dU, dU2 = external_state
            rc = self.lib.rgpu_create_external(C.byref(params), C.c_void_p(dU), C.c_void_p(dU2), C.c_void_p(stream), C.byref(self.ctx))
        if rc:
            msg = self.lib.rgpu_last_error(self.ctx).decode() if self.ctx else "?"
            self.close()
            raise RgpuError("rgpu_create failed (%d): %s" % (rc, msg))
        self.nStep = 0
        self.totalTime = 0.0
        self.dt = 0.0
        self.tHist = 0.0

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.rgpu_destroy(self.ctx)
            self.ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, what):
        if rc:
            raise RgpuError("%s failed (%d): %s" % (what, rc, self.lib.rgpu_last_error(self.ctx).decode()))

    # ---- reference interface ----------------------------------------------------------------------------------
    def upload(self, hU, both=True):
        hU = np.ascontiguousarray(hU, dtype=np.float64)
        assert hU.shape == tuple(self.p.shape), (hU.shape, self.p.shape)
        self._chk(self.lib.rgpu_upload(self.ctx, hU.ctypes.data, int(both)), "upload")

    def getDataHost(self, nStep=None):
        """copyGpuToCpu(nStep) + getDataHost(nStep)"""
        parity = (self.nStep if nStep is None else nStep) % 2
        out = np.empty(self.p.shape, dtype=np.float64)
        self._chk(self.lib.rgpu_download(self.ctx, out.ctypes.data, parity), "download")
        return out

    def make_boundaries(self, parity, idim):
        self._chk(self.lib.rgpu_make_boundaries(self.ctx, parity, idim), "make_boundaries")

    def make_all_boundaries(self, parity=0, totalTime=0.0, dt=0.0):
        self._chk(self.lib.rgpu_make_all_boundaries(self.ctx, parity, totalTime, dt), "make_all_boundaries")

    def compute_inv_dt(self, useU=0):
        v = C.c_double()
        self._chk(self.lib.rgpu_compute_inv_dt(self.ctx, useU, C.byref(v)), "compute_inv_dt")
        return v.value

    def compute_dt(self, useU=0):
        d = self.lib.rgpu_compute_dt(self.ctx, useU)
        if d != d:
            raise RgpuError("compute_dt: " + self.lib.rgpu_last_error(self.ctx).decode())
        return d

    HISTORY_NAMES = ("mass", "maxwell", "reynolds", "magp", "mean_Bx", "mean_By", "mean_Bz", "divB")

    def set_gravity_field(self, G):
        """upload h_gravity (gravityEnabled == 2): [3][ksize][jsize][isize] doubles"""
        G = np.ascontiguousarray(G, dtype=np.float64)
        assert G.shape == (3,) + tuple(self.p.shape[1:]), G.shape
        self._chk(self.lib.rgpu_set_gravity_field(self.ctx, G.ctypes.data), "set_gravity_field")

    def set_forcing_field(self, F):
        """upload h_randomForcing (randomForcingEnabled): [3][ksize][jsize][isize] doubles"""
        F = np.ascontiguousarray(F, dtype=np.float64)
        assert F.shape == (3,) + tuple(self.p.shape[1:]), F.shape
        self._chk(self.lib.rgpu_set_forcing_field(self.ctx, F.ctypes.data), "set_forcing_field")

    def forcing_sums(self, parity):
        out = (C.c_double * 2)()
        self._chk(self.lib.rgpu_forcing_sums(self.ctx, parity, out), "forcing_sums")
        return float(out[0]), float(out[1])

    def add_forcing(self, parity, norm):
        self._chk(self.lib.rgpu_add_forcing(self.ctx, parity, float(norm)), "add_forcing")

    def read_cell(self, parity, i, j, k=0):
        """U(i, j, k, :) of one cell, ghost-inclusive local indices (the probe of history_inertial_wave)"""
        out = np.zeros(int(self.p.nbVar))
        self._chk(self.lib.rgpu_read_cell(self.ctx, parity, int(i), int(j), int(k), out.ctypes.data_as(_capi.c_double_p)), "read_cell")
        return out

    def history_mri(self, nStep=None):
        """history_mri / history_default (MHDRunBase.cpp:3311-3619) reduced on the device"""
        parity = (self.nStep if nStep is None else nStep) % 2
        out = (C.c_double * 8)()
        self._chk(self.lib.rgpu_history_mri(self.ctx, parity, out), "history_mri")
        return dict(zip(self.HISTORY_NAMES, [float(v) for v in out]))

    def state_checksum(self, parity):
        """sum mod 2^64 of the bit patterns of all interior doubles of U[parity] (rgpu_state_checksum): equal for every slab count"""
        out = C.c_ulonglong(0)
        self._chk(self.lib.rgpu_state_checksum(self.ctx, parity, C.byref(out)), "state_checksum")
        return int(out.value)

    def state_monitor(self, parity=None):
        """the ten monitor quantities of U[parity] (default: nStep % 2), columns _capi.MON_NAMES: totals of mass, momenta and energies,
        min density, min internal energy, max |div B| over the interior of the state, raw (2D: rgpu_state_monitor, 3D:
        rgpu_state_monitor3d; include/rgpu.h)"""
        out = np.zeros(_capi.MON_NQ)
        par = self.nStep % 2 if parity is None else int(parity)
        fn = self.lib.rgpu_state_monitor3d if self.p.nz_global != 1 else self.lib.rgpu_state_monitor
        self._chk(fn(self.ctx, par, out.ctypes.data_as(_capi.c_double_p)), "state_monitor")
        return out

    def run_steps_monitored(self, nsteps, every, tEnd=float("inf")):
        """run_steps with a monitor sample after every step that brings nStep to a multiple of `every` (rgpu_run_steps_monitored: inside
        the device-clock batches the samples are taken on the device, one read-back per batch).  Returns (done, MonitorSeries): the
        steps done and the samples of this call -- .step [n], .t [n] (the time after that step), .values [n, 10] (_capi.MON_NAMES)"""
        cap = max(int(nsteps), 0) // max(int(every), 1) + 1
        n, t, d, mn = C.c_int(self.nStep), C.c_double(self.totalTime), C.c_double(self.dt), C.c_int(0)
        log = (C.c_double * max(int(nsteps), 1))()
        mstep, mt, mv = np.zeros(cap, dtype=np.intc), np.zeros(cap), np.zeros((cap, _capi.MON_NQ))
        done = self.lib.rgpu_run_steps_monitored(self.ctx, int(nsteps), float(tEnd), C.byref(n), C.byref(t), C.byref(d), log, int(every), C.byref(mn),
                                                 mstep.ctypes.data_as(C.POINTER(C.c_int)), mt.ctypes.data_as(_capi.c_double_p), mv.ctypes.data_as(_capi.c_double_p))
        k = mn.value
        self.nStep, self.totalTime, self.dt = n.value, t.value, d.value   # (they describe the steps that ran, also when the call failed)
        self.monitor_series = MonitorSeries(mstep[:k].astype(int), mt[:k].copy(), mv[:k].copy())
        if done < 0:
            self._chk(done, "run_steps_monitored")
        self.dt_log = [log[i] for i in range(done)]
        return done, self.monitor_series

    def state_monitor_planes(self, parity=None):
        """the plane monitor of U[parity] (default: nStep % 2) of a 3D state: ndarray [nz, 16], one row per interior plane, columns
        _capi.MONP_NAMES -- the ten monitor quantities of the plane, then the sums of the cell-centred field, bx by, rho vx vy and
        rho^2 (rgpu_state_monitor_planes; include/rgpu.h)"""
        out = np.zeros((self.p.nz, _capi.MONP_NQ))
        par = self.nStep % 2 if parity is None else int(parity)
        self._chk(self.lib.rgpu_state_monitor_planes(self.ctx, par, out.ctypes.data_as(_capi.c_double_p)), "state_monitor_planes")
        return out

    def run_steps_monitored_planes(self, nsteps, every, tEnd=float("inf")):
        """run_steps with a plane-monitor sample after every step that brings nStep to a multiple of `every`
        (rgpu_run_steps_monitored_planes: inside the device-clock batches the samples are taken on the device, one read-back per
        batch).  Returns (done, MonitorSeries): the steps done and the samples of this call -- .step [n], .t [n] (the time after that
        step), .values [n, nz, 16] (_capi.MONP_NAMES)"""
        cap = max(int(nsteps), 0) // max(int(every), 1) + 1
        n, t, d, mn = C.c_int(self.nStep), C.c_double(self.totalTime), C.c_double(self.dt), C.c_int(0)
        log = (C.c_double * max(int(nsteps), 1))()
        mstep, mt, mv = np.zeros(cap, dtype=np.intc), np.zeros(cap), np.zeros((cap, self.p.nz, _capi.MONP_NQ))
        done = self.lib.rgpu_run_steps_monitored_planes(self.ctx, int(nsteps), float(tEnd), C.byref(n), C.byref(t), C.byref(d), log, int(every), C.byref(mn),
                                                        mstep.ctypes.data_as(C.POINTER(C.c_int)), mt.ctypes.data_as(_capi.c_double_p), mv.ctypes.data_as(_capi.c_double_p))
        k = mn.value
        self.nStep, self.totalTime, self.dt = n.value, t.value, d.value   # (they describe the steps that ran, also when the call failed)
        self.monitor_planes_series = MonitorSeries(mstep[:k].astype(int), mt[:k].copy(), mv[:k].copy())
        if done < 0:
            self._chk(done, "run_steps_monitored_planes")
        self.dt_log = [log[i] for i in range(done)]
        return done, self.monitor_planes_series

    def _map_specs(self, specs):
        """specs, each (axis, lo, hi) with the axis 0 / 1 / 2 or "x" / "y" / "z" -> (the C array, the shape [12, nv, nu] of each map)"""
        n = (self.p.nx, self.p.ny, self.p.nz)
        arr = (_capi.RgpuMapSpec * max(len(specs), 1))()
        shapes = []
        for m, (axis, lo, hi) in enumerate(specs):
            a = "xyz".index(axis) if isinstance(axis, str) else int(axis)
            arr[m].axis, arr[m].lo, arr[m].hi = a, int(lo), int(hi)
            shapes.append((_capi.MAP_NQ,) + {0: (n[2], n[1]), 1: (n[2], n[0]), 2: (n[1], n[0])}.get(a, (0, 0)))
        return arr, shapes

    def state_maps(self, specs, parity=None):
        """maps of U[parity] (default: nStep % 2) of a 3D state: a list, per spec (axis, lo, hi), of ndarrays [12, nv, nu] -- the
        channels _capi.MAP_NAMES of every pixel summed over the cells lo .. hi - 1 along the axis ("x" / "y" / "z" or 0 / 1 / 2), a
        slice where hi == lo + 1 (rgpu_state_maps; include/rgpu.h, "map monitors")"""
        arr, shapes = self._map_specs(specs)
        out = np.zeros(max(sum(int(np.prod(s)) for s in shapes), 1))
        par = self.nStep % 2 if parity is None else int(parity)
        self._chk(self.lib.rgpu_state_maps(self.ctx, par, len(specs), arr, out.ctypes.data_as(_capi.c_double_p)), "state_maps")
        cuts = np.cumsum([0] + [int(np.prod(s)) for s in shapes])
        return [out[cuts[m]:cuts[m + 1]].reshape(shapes[m]).copy() for m in range(len(specs))]

    def run_steps_mapped(self, nsteps, every, specs, tEnd=float("inf")):
        """run_steps with a sample of the maps `specs` after every step that brings nStep to a multiple of `every`
        (rgpu_run_steps_mapped: inside the device-clock batches the maps are taken on the device, one read-back per batch).  Returns
        (done, MapSeries): the steps done and the samples of this call -- .step [n], .t [n] (the time after that step), .maps a list
        per spec of [n, 12, nv, nu] (_capi.MAP_NAMES)"""
        arr, shapes = self._map_specs(specs)
        sizes = [int(np.prod(s)) for s in shapes]
        cap = max(int(nsteps), 0) // max(int(every), 1) + 1
        n, t, d, mn = C.c_int(self.nStep), C.c_double(self.totalTime), C.c_double(self.dt), C.c_int(0)
        log = (C.c_double * max(int(nsteps), 1))()
        mstep, mt, mv = np.zeros(cap, dtype=np.intc), np.zeros(cap), np.empty((cap, max(sum(sizes), 1)))   # (mv: only the samples written are read)
        done = self.lib.rgpu_run_steps_mapped(self.ctx, int(nsteps), float(tEnd), C.byref(n), C.byref(t), C.byref(d), log, int(every), len(specs), arr, C.byref(mn),
                                              mstep.ctypes.data_as(C.POINTER(C.c_int)), mt.ctypes.data_as(_capi.c_double_p), mv.ctypes.data_as(_capi.c_double_p))
        k = mn.value
        self.nStep, self.totalTime, self.dt = n.value, t.value, d.value   # (they describe the steps that ran, also when the call failed)
        cuts = np.cumsum([0] + sizes)
        self.map_series = MapSeries(mstep[:k].astype(int), mt[:k].copy(), [mv[:k, cuts[m]:cuts[m + 1]].reshape((k,) + shapes[m]).copy() for m in range(len(specs))])
        if done < 0:
            self._chk(done, "run_steps_mapped")
        self.dt_log = [log[i] for i in range(done)]
        return done, self.map_series

    def _pdf_specs(self, specs):
        """specs, each an axis (1D) or a pair of axes (joint), an axis as pdf_axis takes it -> (the C array, the shape of each table)"""
        arr = (_capi.RgpuPdfSpec * max(len(specs), 1))()
        shapes = []
        for m, spec in enumerate(specs):
            joint = isinstance(spec, (tuple, list)) and len(spec) == 2 and isinstance(spec[0], (tuple, list, _capi.RgpuPdfAxis))
            arr[m].a = pdf_axis(spec[0] if joint else spec)
            if joint:
                arr[m].b = pdf_axis(spec[1])
            shapes.append((arr[m].a.nbins + 3, arr[m].b.nbins + 3) if joint else (arr[m].a.nbins + 3,))
        return arr, shapes

    def state_pdfs(self, specs, parity=None):
        """histograms of the interior cells of U[parity] (default: nStep % 2) of a 3D state: a list, per spec, of numpy.uint64 counts
        shaped (na + 3,) -- the bins, then under, over, nan -- or (na + 3, nb + 3) for a pair of axes (rgpu_state_pdfs; include/rgpu.h,
        "PDF monitors")"""
        arr, shapes = self._pdf_specs(specs)
        out = np.zeros(max(sum(int(np.prod(s)) for s in shapes), 1), dtype=np.uint64)
        par = self.nStep % 2 if parity is None else int(parity)
        self._chk(self.lib.rgpu_state_pdfs(self.ctx, par, len(specs), arr, out.ctypes.data_as(C.POINTER(C.c_ulonglong))), "state_pdfs")
        cuts = np.cumsum([0] + [int(np.prod(s)) for s in shapes])
        return [out[cuts[m]:cuts[m + 1]].reshape(shapes[m]).copy() for m in range(len(specs))]

    def run_steps_pdfs(self, nsteps, every, specs, tEnd=float("inf")):
        """run_steps with a sample of the PDFs `specs` after every step that brings nStep to a multiple of `every` (rgpu_run_steps_pdfs:
        inside the device-clock batches the cells are counted on the device, one read-back per batch).  Returns (done, PdfSeries): the
        steps done and the samples of this call -- .step [n], .t [n] (the time after that step), .pdfs a list per spec of numpy.uint64
        [n, na + 3] or [n, na + 3, nb + 3]"""
        arr, shapes = self._pdf_specs(specs)
        sizes = [int(np.prod(s)) for s in shapes]
        cap = max(int(nsteps), 0) // max(int(every), 1) + 1
        n, t, d, mn = C.c_int(self.nStep), C.c_double(self.totalTime), C.c_double(self.dt), C.c_int(0)
        log = (C.c_double * max(int(nsteps), 1))()
        mstep, mt, mv = np.zeros(cap, dtype=np.intc), np.zeros(cap), np.zeros((cap, max(sum(sizes), 1)), dtype=np.uint64)
        done = self.lib.rgpu_run_steps_pdfs(self.ctx, int(nsteps), float(tEnd), C.byref(n), C.byref(t), C.byref(d), log, int(every), len(specs), arr, C.byref(mn),
                                            mstep.ctypes.data_as(C.POINTER(C.c_int)), mt.ctypes.data_as(_capi.c_double_p), mv.ctypes.data_as(C.POINTER(C.c_ulonglong)))
        k = mn.value
        self.nStep, self.totalTime, self.dt = n.value, t.value, d.value   # (they describe the steps that ran, also when the call failed)
        cuts = np.cumsum([0] + sizes)
        self.pdf_series = PdfSeries(mstep[:k].astype(int), mt[:k].copy(), [mv[:k, cuts[m]:cuts[m + 1]].reshape((k,) + shapes[m]).copy() for m in range(len(specs))])
        if done < 0:
            self._chk(done, "run_steps_pdfs")
        self.dt_log = [log[i] for i in range(done)]
        return done, self.pdf_series

    def _spectrum_specs(self, specs):
        """specs as spectrum_spec takes them -> (the C array, the shells of each on this context; 0 where the library refuses it)"""
        arr = (_capi.RgpuSpectrumSpec * max(len(specs), 1))()
        for m, spec in enumerate(specs):
            arr[m] = spectrum_spec(spec)
        return arr, [int(self.lib.rgpu_spectrum_shells(self.ctx, C.byref(arr[m]))) for m in range(len(specs))]

    def state_spectra(self, specs, parity=None):
        """shell-binned power spectra of U[parity] (default: nStep % 2) of a 3D state whose extents are powers of two, the box taken as
        periodic: a list, per spec, of (P, M) -- the power and the number of modes of each shell, numpy.float64 [S] (rgpu_state_spectra;
        include/rgpu.h, "spectrum monitors").  A spec is (channels, (wx, wy, wz)), see spectrum_spec"""
        arr, shells = self._spectrum_specs(specs)
        out = np.zeros(max(2 * sum(shells), 1))
        par = self.nStep % 2 if parity is None else int(parity)
        self._chk(self.lib.rgpu_state_spectra(self.ctx, par, len(specs), arr, out.ctypes.data_as(_capi.c_double_p)), "state_spectra")
        cuts = np.cumsum([0] + [2 * s for s in shells])
        return [(out[cuts[m]:cuts[m] + shells[m]].copy(), out[cuts[m] + shells[m]:cuts[m + 1]].copy()) for m in range(len(specs))]

    def run_steps_spectra(self, nsteps, every, specs, tEnd=float("inf")):
        """run_steps with a sample of the spectra `specs` after every step that brings nStep to a multiple of `every`
        (rgpu_run_steps_spectra: inside the device-clock batches the transforms run on the device, one read-back per batch).  Returns
        (done, SpectrumSeries): the steps done and the samples of this call -- .step [n], .t [n] (the time after that step), .power and
        .modes lists per spec of numpy.float64 [n, S]"""
        arr, shells = self._spectrum_specs(specs)
        cap = max(int(nsteps), 0) // max(int(every), 1) + 1
        n, t, d, mn = C.c_int(self.nStep), C.c_double(self.totalTime), C.c_double(self.dt), C.c_int(0)
        log = (C.c_double * max(int(nsteps), 1))()
        mstep, mt, mv = np.zeros(cap, dtype=np.intc), np.zeros(cap), np.zeros((cap, max(2 * sum(shells), 1)))
        done = self.lib.rgpu_run_steps_spectra(self.ctx, int(nsteps), float(tEnd), C.byref(n), C.byref(t), C.byref(d), log, int(every), len(specs), arr, C.byref(mn),
                                               mstep.ctypes.data_as(C.POINTER(C.c_int)), mt.ctypes.data_as(_capi.c_double_p), mv.ctypes.data_as(_capi.c_double_p))
        k = mn.value
        self.nStep, self.totalTime, self.dt = n.value, t.value, d.value   # (they describe the steps that ran, also when the call failed)
        cuts = np.cumsum([0] + [2 * s for s in shells])
        self.spectrum_series = SpectrumSeries(mstep[:k].astype(int), mt[:k].copy(), [mv[:k, cuts[m]:cuts[m] + shells[m]].copy() for m in range(len(specs))],
                                              [mv[:k, cuts[m] + shells[m]:cuts[m + 1]].copy() for m in range(len(specs))])
        if done < 0:
            self._chk(done, "run_steps_spectra")
        self.dt_log = [log[i] for i in range(done)]
        return done, self.spectrum_series

    def _helm_specs(self, specs):
        """specs as helm_spec takes them -> (the C array, the shells of each on this context; 0 where the library refuses it)"""
        arr = (_capi.RgpuHelmSpec * max(len(specs), 1))()
        for m, spec in enumerate(specs):
            arr[m] = helm_spec(spec)
        return arr, [int(self.lib.rgpu_helm_shells(self.ctx, C.byref(arr[m]))) for m in range(len(specs))]

    def state_helm_spectra(self, specs, parity=None):
        """Helmholtz spectra of U[parity] (default: nStep % 2) of a 3D state whose extents are powers of two, the box taken as periodic:
        a list, per spec, of (Psol, Pcomp, M) -- the solenoidal power, the compressive power and the number of modes of each shell,
        numpy.float64 [S] (rgpu_state_helm_spectra; include/rgpu.h, "Helmholtz spectra").  A spec is (field, (wx, wy, wz)), see helm_spec"""
        arr, shells = self._helm_specs(specs)
        out = np.zeros(max(3 * sum(shells), 1))
        par = self.nStep % 2 if parity is None else int(parity)
        self._chk(self.lib.rgpu_state_helm_spectra(self.ctx, par, len(specs), arr, out.ctypes.data_as(_capi.c_double_p)), "state_helm_spectra")
        cuts = np.cumsum([0] + [3 * s for s in shells])
        return [tuple(out[cuts[m] + i * shells[m]:cuts[m] + (i + 1) * shells[m]].copy() for i in range(3)) for m in range(len(specs))]

    def run_steps_helm_spectra(self, nsteps, every, specs, tEnd=float("inf")):
        """run_steps with a sample of the Helmholtz spectra `specs` after every step that brings nStep to a multiple of `every`
        (rgpu_run_steps_helm_spectra: inside the device-clock batches the transforms run on the device, one read-back per batch).
        Returns (done, HelmSeries): the steps done and the samples of this call -- .step [n], .t [n] (the time after that step),
        .solenoidal, .compressive and .modes lists per spec of numpy.float64 [n, S]"""
        arr, shells = self._helm_specs(specs)
        cap = max(int(nsteps), 0) // max(int(every), 1) + 1
        n, t, d, mn = C.c_int(self.nStep), C.c_double(self.totalTime), C.c_double(self.dt), C.c_int(0)
        log = (C.c_double * max(int(nsteps), 1))()
        mstep, mt, mv = np.zeros(cap, dtype=np.intc), np.zeros(cap), np.zeros((cap, max(3 * sum(shells), 1)))
        done = self.lib.rgpu_run_steps_helm_spectra(self.ctx, int(nsteps), float(tEnd), C.byref(n), C.byref(t), C.byref(d), log, int(every), len(specs), arr, C.byref(mn),
                                                    mstep.ctypes.data_as(C.POINTER(C.c_int)), mt.ctypes.data_as(_capi.c_double_p), mv.ctypes.data_as(_capi.c_double_p))
        k = mn.value
        self.nStep, self.totalTime, self.dt = n.value, t.value, d.value   # (they describe the steps that ran, also when the call failed)
        cuts = np.cumsum([0] + [3 * s for s in shells])
        part = lambda i: [mv[:k, cuts[m] + i * shells[m]:cuts[m] + (i + 1) * shells[m]].copy() for m in range(len(specs))]
        self.helm_series = HelmSeries(mstep[:k].astype(int), mt[:k].copy(), part(0), part(1), part(2))
        if done < 0:
            self._chk(done, "run_steps_helm_spectra")
        self.dt_log = [log[i] for i in range(done)]
        return done, self.helm_series

    def history_turbulence(self, nStep=None):
        """history_turbulence (MHDRunBase.cpp:3626-3810) reduced on the device: the 18 columns after totalTime and dt"""
        parity = (self.nStep if nStep is None else nStep) % 2
        out = (C.c_double * 18)()
        self._chk(self.lib.rgpu_history_turbulence(self.ctx, parity, out), "history_turbulence")
        return [float(v) for v in out]

    def history_columns(self, parity):
        isz = self.p.nx + 2 * self.p.ghostWidth
        cols = np.zeros((9, isz), dtype=np.float64)
        self._chk(self.lib.rgpu_history_columns(self.ctx, parity, cols.ctypes.data_as(C.POINTER(C.c_double))), "history_columns")
        return cols

    def history_reynolds(self, parity, mean_vx, mean_vy, dTau):
        isz = self.p.nx + 2 * self.p.ghostWidth
        mvx, mvy = np.ascontiguousarray(mean_vx, dtype=np.float64), np.ascontiguousarray(mean_vy, dtype=np.float64)
        col = np.zeros(isz, dtype=np.float64)
        dp = C.POINTER(C.c_double)
        self._chk(self.lib.rgpu_history_reynolds(self.ctx, parity, mvx.ctypes.data_as(dp), mvy.ctypes.data_as(dp), dTau,
                                                 col.ctypes.data_as(dp)), "history_reynolds")
        return col

    def godunov_unsplit(self, nStep, dt, totalTime=None):
        t = self.totalTime if totalTime is None else totalTime
        self._chk(self.lib.rgpu_godunov_unsplit(self.ctx, nStep, dt, t), "godunov_unsplit")

    def oneStepIntegration(self):
        n, t, d = C.c_int(self.nStep), C.c_double(self.totalTime), C.c_double(self.dt)
        self._chk(self.lib.rgpu_one_step_integration(self.ctx, C.byref(n), C.byref(t), C.byref(d)), "oneStepIntegration")
        self.nStep, self.totalTime, self.dt = n.value, t.value, d.value
        return self.dt

    def run_steps(self, nsteps, tEnd=float("inf")):
        """up to nsteps turns of the reference's time loop (rgpu_run_steps: where a step is one fused kernel the time step stays on
        the device and the batch is queued without a host round trip); returns the number of steps done"""
        n, t, d = C.c_int(self.nStep), C.c_double(self.totalTime), C.c_double(self.dt)
        log = (C.c_double * max(int(nsteps), 1))()
        done = self.lib.rgpu_run_steps_log(self.ctx, int(nsteps), float(tEnd), C.byref(n), C.byref(t), C.byref(d), log)
        self.nStep, self.totalTime, self.dt = n.value, t.value, d.value   # (they describe the steps that ran, also when the call failed)
        if done < 0:
            self._chk(done, "run_steps")
        self.dt_log = [log[i] for i in range(done)]     # the time steps of this call, in order
        return done

    def forcing_batch_steps(self):
        """how many steps of this context ran inside device-clock batches with a forcing stage queued (rgpu_forcing_batch_steps: 0 where
        every forced step took the literal loop, e.g. with option "forcing_clock" = 0)"""
        return int(self.lib.rgpu_forcing_batch_steps(self.ctx))

    def run_steps_history(self, nsteps, dtHist, tEnd=float("inf")):
        """up to nsteps turns of the reference's time loop with its history cadence inside (rgpu_run_steps_history: before a step, when
        tHist == 0 or the last step carried t past tHist + dtHist, the row of history_mri is taken and tHist += dtHist; inside the
        device-clock batches decision and row are formed on the device, one read-back per batch).  tHist lives on the solver between
        calls (start sets it to totalTime).  Returns (done, steps, t, dt, values[n, 8]): the steps done, and per sample the step number,
        the time and the dt column of the history file, and the eight values in the order of HISTORY_NAMES"""
        m = max(int(nsteps), 1)
        n, t, d, th, hn = C.c_int(self.nStep), C.c_double(self.totalTime), C.c_double(self.dt), C.c_double(self.tHist), C.c_int(0)
        log = (C.c_double * m)()
        hstep, ht, hdt, hv = np.zeros(m, dtype=np.intc), np.zeros(m), np.zeros(m), np.zeros((m, 8))
        done = self.lib.rgpu_run_steps_history(self.ctx, int(nsteps), float(tEnd), C.byref(n), C.byref(t), C.byref(d), log, float(dtHist), C.byref(th), C.byref(hn),
                                               hstep.ctypes.data_as(C.POINTER(C.c_int)), ht.ctypes.data_as(_capi.c_double_p), hdt.ctypes.data_as(_capi.c_double_p),
                                               hv.ctypes.data_as(_capi.c_double_p))
        self.nStep, self.totalTime, self.dt, self.tHist = n.value, t.value, d.value, th.value   # (also when the call failed)
        if done < 0:
            self._chk(done, "run_steps_history")
        self.dt_log = [log[i] for i in range(done)]
        k = hn.value
        return done, hstep[:k].copy(), ht[:k].copy(), hdt[:k].copy(), hv[:k].copy()

    def start(self, hU, nStepmax, tEnd=float("inf")):
        """init part + time loop of start() (MHDRunGodunov.cpp:3801-3989) without outputs; returns the dt list"""
        self.upload(hU, both=False)
        self.nStep, self.totalTime = 0, 0.0
        self.tHist = self.totalTime   # MHDRunGodunov.cpp:3916
        self.make_all_boundaries(0, 0.0, 0.0)
        # h_U.copyTo(h_U2)
        self.upload(self.getDataHost(0), both=True)
        dts = []
        while self.totalTime < tEnd and self.nStep < nStepmax:
            dts.append(self.oneStepIntegration())
        return dts

    # ---- pieces used by the slab driver -------------------------------------------------------------------------
    def step_pre(self, nStep, dt, t):
        self._chk(self.lib.rgpu_step_pre(self.ctx, nStep, dt, t), "step_pre")

    def step_core(self, nStep, dt, t):
        self._chk(self.lib.rgpu_step_core(self.ctx, nStep, dt, t), "step_core")

    def step_core_planes(self, nStep, dt, t, k_lo, k_hi):
        self._chk(self.lib.rgpu_step_core_planes(self.ctx, nStep, dt, t, k_lo, k_hi), "step_core_planes")

    def step_core_planes_split(self, nStep, dt, t, k_lo, k_hi, what):
        """what: 1 = RGPU_CORE_FLUXES, 2 = RGPU_CORE_UPDATE (include/rgpu.h)"""
        self._chk(self.lib.rgpu_step_core_planes_split(self.ctx, nStep, dt, t, k_lo, k_hi, what), "step_core_planes_split")

    def step_fill_planes(self, nStep, dt, t, k_lo, k_hi):
        self._chk(self.lib.rgpu_step_fill_planes(self.ctx, nStep, dt, t, k_lo, k_hi), "step_fill_planes")

    def step_core_planes_pair(self, nStep, dt, t, r1, r2, what):
        """two disjoint plane ranges in one call (rgpu_step_core_planes_pair): what as step_core_planes_split"""
        self._chk(self.lib.rgpu_step_core_planes_pair(self.ctx, nStep, dt, t, r1[0], r1[1], r2[0], r2[1], what), "step_core_planes_pair")

    def step_fill_planes_pair(self, nStep, dt, t, r1, r2):
        self._chk(self.lib.rgpu_step_fill_planes_pair(self.ctx, nStep, dt, t, r1[0], r1[1], r2[0], r2[1]), "step_fill_planes_pair")

    def inv_dt_accumulate(self, parity, k_lo, k_hi, reset=False):
        self._chk(self.lib.rgpu_inv_dt_accumulate(self.ctx, parity, k_lo, k_hi, int(reset)), "inv_dt_accumulate")

    def inv_dt_result(self):
        v = C.c_double(0.0)
        self._chk(self.lib.rgpu_inv_dt_result(self.ctx, C.byref(v)), "inv_dt_result")
        return v.value

    def step_dissipative(self, nStep, dt, t):
        self._chk(self.lib.rgpu_step_dissipative(self.ctx, nStep, dt, t), "step_dissipative")

    def step_post_a(self, nStep, dt, t):
        self._chk(self.lib.rgpu_step_post_a(self.ctx, nStep, dt, t), "step_post_a")

    def step_post_b(self, nStep, dt, t):
        self._chk(self.lib.rgpu_step_post_b(self.ctx, nStep, dt, t), "step_post_b")

    def synchronize(self):
        self._chk(self.lib.rgpu_synchronize(self.ctx), "synchronize")

    # ---- instrumentation ----------------------------------------------------------------------------------------
    def enable_timers(self, on=True):
        self._chk(self.lib.rgpu_enable_timers(self.ctx, int(on)), "enable_timers")

    def reset_timers(self):
        self._chk(self.lib.rgpu_reset_timers(self.ctx), "reset_timers")

    def timers(self):
        a = (C.c_double * len(_capi.T_NAMES))()
        self._chk(self.lib.rgpu_get_timers(self.ctx, a, len(_capi.T_NAMES)), "get_timers")
        return dict(zip(_capi.T_NAMES, list(a)))

    def dominant_kernel(self):
        name = C.create_string_buffer(64)
        ms, n = C.c_double(), C.c_long()
        self._chk(self.lib.rgpu_dominant_kernel(self.ctx, name, 64, C.byref(ms), C.byref(n)), "dominant_kernel")
        return name.value.decode(), ms.value, n.value


def interior(U, p):
    """strip the ghost cells of a [nvar][k][j][i] array"""
    gw = p.ghostWidth
    if p.three_d:
        return U[:, gw:-gw, gw:-gw, gw:-gw]
    return U[:, :, gw:-gw, gw:-gw]
