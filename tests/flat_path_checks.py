"""Helpers of tests/test_flat_path_gpu.py and tests/flat_worker.py: the flat per-cell kernels (kernels_hydro.h, kernels_mhd2d.h,
kernels_mhd3d.h) on the device, at shapes where the two pieces of launch machinery that belong to them alone engage --

  * the XCD-aware workgroup order of rg_launch_planes / rg_kernel_planes (csrc/hip/rg_backend.h), which every launch_planes call of
    api/step_hydro.h, api/step_mhd.h and api/forcing.h goes through: the flat hydro kernels (2D: one plane), the flat 3D MHD prim / elec / trace / Riemann
    kernels, rgpu_add_forcing and the Ornstein-Uhlenbeck kick.  (The flat 2D MHD kernels and the 3D MHD update are launched over a
    linear index range and never read "xcd_sub".)
  * the chunked two-stream schedule mhd3d_chunked (api/step_mhd.h): flat 3D MHD only.

A context takes the flat kernels when it has a per-cell gravity field (grav_on == 2) or when the process runs under RGPU_TILED=0.

The model below restates the launch arithmetic in Python, so that every case first proves what it engages (sub-band counts, live
guards, chunk counts) before it compares anything: a shape that has gone vacuous fails as a model assertion, not as a pass."""
import hashlib

import numpy as np

import parity_checks as pc
from conftest import ini
from ramsesgpu_amd.solver import Solver

K_BLOCK = 256          # api/ctx.h: kBlock, the streaming kernels
K_BLOCK_HEAVY = 64     # api/ctx.h: kBlockHeavy, the Riemann (flux) kernels
XCDS = 8
DEFAULT_XCD_SUB = 4096  # api/ctx.h: rgpu_ctx::xcd_sub
MAX_CHUNKS = 256        # api/ctx.h: rgpu_ctx::kMaxChunks


# ---- A. the model ------------------------------------------------------------------------------------------------------------
def plane_map_workgroups(plane_cells, block, sub, nplanes=1):
    """rg_launch_planes + rg_kernel_planes (or, sub == 0, rg_launch_range + rg_kernel_range) restated: for every workgroup of the grid,
    in blockIdx order, (in_band, start, stop) -- the flat cells [start, stop) relative to idx0 that its threads pass to the kernel body
    (start == stop: the guards reject the whole workgroup); in_band is None in linear order.  Returns (facts, [workgroups])."""
    n = plane_cells * nplanes
    if n == 0:
        return {"grid": 0, "linear": True}, []
    bpp = (plane_cells + block - 1) // block
    if sub == 0:
        grid = (n + block - 1) // block
        wgs = [(None, b * block, min((b + 1) * block, n)) for b in range(grid)]
        return {"bpp": bpp, "band": None, "T": None, "nsub": None, "grid": grid, "linear": True}, wgs
    band = (bpp + XCDS - 1) // XCDS
    T = sub // block if sub // block > 0 else 1
    if T > band:
        T = band
    nsub = (band + T - 1) // T
    T = (band + nsub - 1) // nsub
    grid = XCDS * nsub * nplanes * T
    wgs = []
    for b in range(grid):
        xcd, slot = b & 7, b >> 3
        per_sub = nplanes * T
        s, r = divmod(slot, per_sub)
        p, t = divmod(r, T)
        in_band = s * T + t
        off = (xcd * band + in_band) * block                      # threadIdx.x == 0
        if in_band < band and off < plane_cells:
            wgs.append((in_band, p * plane_cells + off, p * plane_cells + min(off + block, plane_cells)))
        else:
            wgs.append((in_band, 0, 0))
    return {"bpp": bpp, "band": band, "T": T, "nsub": nsub, "grid": grid, "linear": False}, wgs


def plane_map_facts(plane_cells, block, sub, nplanes=1):
    """what a launch_planes call engages: bpp (workgroups per plane), band (workgroups per XCD and plane), T (workgroups per sub-band),
    nsub, grid, grid_per_plane; whether the `in_band < band` guard and the `off < plane_cells` guard each reject at least one whole
    workgroup; how many XCDs get no cell of a plane; whether the order departs from the linear one at all"""
    f, wgs = plane_map_workgroups(plane_cells, block, sub, nplanes)
    if f["linear"]:
        f.update(grid_per_plane=f["grid"] / float(nplanes), in_band_guard_live=False, off_guard_live=False, idle_xcds=0, reordered=False)
        return f
    band = f["band"]
    f["grid_per_plane"] = f["grid"] // nplanes
    f["in_band_guard_live"] = any(ib >= band for ib, _, _ in wgs)
    f["off_guard_live"] = any(ib < band and a == b for ib, a, b in wgs)
    f["idle_xcds"] = sum(1 for x in range(XCDS) if x * band * block >= plane_cells)
    starts = [a for _, a, b in wgs if b > a]
    f["reordered"] = starts != sorted(starts)
    return f


def cover_counts(workgroups, ncells):
    """how often each of the flat cells [0, ncells) is visited by the enumerated workgroups"""
    d = np.zeros(ncells + 1, dtype=np.int64)
    for _, a, b in workgroups:
        if b > a:
            d[a] += 1
            d[b] -= 1
    return np.cumsum(d)[:ncells]


def chunk_facts(ksize, chunks_option, span, timers=False):
    """rgpu_create's nchunks (api/ctx.h) and mhd3d_core's choice of schedule (api/step_mhd.h: mhd3d_serial / mhd3d_chunked) for a flat 3D MHD update of `span` planes with what == 0
    and no device clock: {"nchunks", "serial", "C" (chunks of the two-stream schedule; 1 when serial), "cuts" (the chunk ends, relative
    to the first plane)}.  chunks_option: the option "chunks" (<= 0: the default, ksize / 8)"""
    want = chunks_option if chunks_option > 0 else ksize // 8
    want = min(want, ksize // 2, MAX_CHUNKS)
    nchunks = want if want > 1 else 1
    serial = bool(timers) or nchunks <= 1 or span < 16
    C = max(1, min((span + 7) // 8, nchunks))
    if serial:
        return {"nchunks": nchunks, "serial": True, "C": 1, "cuts": [span]}
    return {"nchunks": nchunks, "serial": False, "C": C, "cuts": [span if ci + 1 == C else span * (ci + 1) // C for ci in range(C)]}


def effective_sub(lib):
    """the sub-band size a context created now gets"""
    v = lib.get_option("xcd_sub")
    return v if v >= 0 else DEFAULT_XCD_SUB


def box_facts(p, sub, chunks_option=-1):
    """the model's facts for one whole-box step of a configuration: the plane maps of the streaming and of the flux kernels over all
    planes, and (3D MHD) the chunk schedule"""
    gw = p.ghostWidth
    plane = (p.nx + 2 * gw) * (p.ny + 2 * gw)
    ks = p.nz + 2 * gw if p.three_d else 1
    out = {"plane_cells": plane, "ksize": ks,
           "b256": plane_map_facts(plane, K_BLOCK, sub, ks), "b64": plane_map_facts(plane, K_BLOCK_HEAVY, sub, ks)}
    if p.three_d and p.mhdEnabled:
        out["chunks"] = chunk_facts(ks, chunks_option, ks)
    return out


def assert_facts(got, want, what):
    """want: {"b256.nsub": 2, "chunks.C": 5, "b64.band>=": 2, ...} against box_facts"""
    for key, v in want.items():
        ge = key.endswith(">=")
        node = got
        for part in key.rstrip(">=").split("."):
            node = node[part]
        assert (node >= v) if ge else (node == v), "%s: the model says %s = %r, the case claims %s%r" % (what, key.rstrip(">="), node, ">= " if ge else "", v)


# ---- B. the forcing probe -------------------------------------------------------------------------------------------------------
def forcing_probe_inputs(p, seed=5):
    """(U, F): rho = 1, zero momenta, constant energy; a forcing field of integers 1 .. 15 that differ per cell and component (never 0:
    every visit of a cell changes every component of it)"""
    rng = np.random.RandomState(seed)
    U = np.zeros(p.shape)
    U[0] = 1.0
    U[1] = 4.0
    F = rng.randint(1, 16, (3,) + tuple(p.shape[1:])).astype(np.float64)
    return U, F


def forcing_probe_expected(p, U, F, norm):
    """add_random_forcing on the interior in numpy (kernels_bc.h: add_forcing_cell): the energy first, from the momenta before the
    kick, then the momenta; every operation exact for forcing_probe_inputs.  Ghost cells as given."""
    gw = p.ghostWidth
    I = (slice(gw, -gw),) * 3
    out = U.copy()
    e = U[1][I].copy()
    for c in range(3):
        f = F[c][I] * norm
        e += U[2 + c][I] / U[0][I] * F[c][I] * norm + 0.5 * (f * f)
    out[1][I] = e
    for c in range(3):
        out[2 + c][I] = U[2 + c][I] + U[0][I] * F[c][I] * norm
    return out


def interior_mask(p):
    """flat [ksize * jsize * isize] mask of the interior cells of a 3D box"""
    gw = p.ghostWidth
    inside = np.zeros(tuple(p.shape[1:]), dtype=bool)
    inside[gw:-gw, gw:-gw, gw:-gw] = True
    return inside.reshape(-1)


def forcing_by_workgroups(p, U, F, norm, workgroups, idx0):
    """K_add_forcing run by an enumeration of workgroups (plane_map_workgroups over the interior planes, idx0 = gw * plane): every
    enumerated cell is forced once per visit, in place, behind the kernel's own interior guard"""
    out = U.reshape(U.shape[0], -1).copy()
    Ff = F.reshape(3, -1)
    inside = interior_mask(p)
    for _, a, b in workgroups:
        if b <= a:
            continue
        idx = np.arange(idx0 + a, idx0 + b)
        idx = idx[inside[idx]]
        e = out[1, idx]
        for c in range(3):
            f = Ff[c, idx] * norm
            e = e + (out[2 + c, idx] / out[0, idx] * Ff[c, idx] * norm + 0.5 * (f * f))
        out[1, idx] = e
        for c in range(3):
            out[2 + c, idx] += out[0, idx] * Ff[c, idx] * norm
    return out.reshape(U.shape)


def check_forcing_probe(lib, base, ov, sub_option, want):
    """rgpu_add_forcing (K_add_forcing through launch_planes, in place) once on forcing_probe_inputs: the whole array, ghost cells
    included, equal to numpy's, bit for bit, for either library.  sub_option: the option "xcd_sub", None = as created.
    want: the facts the shape claims for the kernel's block (assert_facts keys without the block prefix)"""
    old = lib.set_option("xcd_sub", sub_option) if sub_option is not None else None
    try:
        p = lib.params_from_ini(ini(base), ov)
        assert p.three_d and not p.mhdEnabled and p.randomForcingEnabled, (base, ov)
        gw = p.ghostWidth
        plane = (p.nx + 2 * gw) * (p.ny + 2 * gw)
        facts = plane_map_facts(plane, K_BLOCK, effective_sub(lib), p.nz)
        assert_facts({"map": facts}, {"map." + k: v for k, v in want.items()}, "forcing probe %s [%s] xcd_sub %r" % (base, ov, sub_option))
        U, F = forcing_probe_inputs(p)
        ref = forcing_probe_expected(p, U, F, 0.5)
        sv = Solver(p, lib)
        try:
            sv.set_forcing_field(F)
            sv.upload(U, both=False)
            sv.add_forcing(0, 0.5)
            got = sv.getDataHost(0)
        finally:
            sv.close()
    finally:
        if sub_option is not None:
            lib.set_option("xcd_sub", old)
    bad = got != ref
    if bad.any():
        v, k, j, i = (int(x[0]) for x in np.nonzero(bad))
        twice = int((bad & (got == 2.0 * ref - U)).sum())
        raise AssertionError("forcing probe %s [%s] xcd_sub %r (%s): %d doubles differ from numpy's (%d of them as if forced twice, %d as if "
                             "never); first at (v, k, j, i) = %r: %r, expected %r" % (base, ov, sub_option, facts, int(bad.sum()), twice,
                                                                                      int((bad & (got == U)).sum()), (v, k, j, i), got[v, k, j, i], ref[v, k, j, i]))
    return facts


# ---- C. which path a configuration takes, and runs against an oracle that is asked once ----------------------------------------------
def assert_flat_path(lib, base, ov):
    """one timed step on a context of its own: the phase timers say which kernels ran -- the flat prim / trace / flux kernels (and elec
    for 3D MHD), no tiled sweep.  (Timers make mhd3d_core pick the serial schedule: the compared runs are untimed.)"""
    p = lib.params_from_ini(ini(base), ov)
    U0 = lib.init_condition(ini(base), ov, p)
    sv = Solver(p, lib)
    try:
        pc.attach_gravity(lib, base, ov, p, sv=sv)
        sv.start(U0, 0)
        sv.enable_timers(True)
        sv.reset_timers()
        sv.oneStepIntegration()
        t = sv.timers()
        sv.enable_timers(False)
    finally:
        sv.close()
    names = ["prim", "trace", "flux"] + (["elec"] if p.mhdEnabled and p.three_d else [])
    what = "%s [%s]: phase seconds of one timed step %r" % (base, ov, t)
    for n in names:
        assert t[n] > 0.0, what
    assert t["sweep"] == 0.0, what
    return t


class OnceOracle:
    """the oracle with run() remembered per (parameters, initial state, gravity field, forcing field, steps): the variants of one case
    (launch options, the two libraries) are compared with ONE oracle run.  Results are handed out as copies."""
    _runs = {}
    MAX_BYTES = 1 << 30

    def __init__(self, oracle):
        self._o = oracle
        self._g = self._f = None

    def __getattr__(self, name):
        return getattr(self._o, name)

    @staticmethod
    def _digest(a):
        return None if a is None else hashlib.sha1(np.ascontiguousarray(a).view(np.uint8)).hexdigest()

    def set_gravity_field(self, G):
        self._g = self._digest(G)
        self._o.set_gravity_field(G)

    def set_forcing_field(self, F):
        self._f = self._digest(F)
        self._o.set_forcing_field(F)

    def run(self, p, U0, nsteps, tEnd=1e300):
        key = (bytes(p), self._digest(U0), self._g, self._f, int(nsteps), float(tEnd))
        runs = OnceOracle._runs
        if key not in runs:
            U, dts, t = self._o.run(p, U0, nsteps, tEnd)
            runs[key] = (U.copy(), np.array(dts, copy=True), t)
            while sum(v[0].nbytes for v in runs.values()) > self.MAX_BYTES and len(runs) > 1:
                runs.pop(next(iter(runs)))
        U, dts, t = runs[key]
        return U.copy(), dts.copy(), t


def check_variants_vs_oracle(lib, oracle, base, ov, nsteps, variants, exact, chunk_want=None):
    """pc.check_run_vs_oracle for every variant -- [(option, value) or None = as created] -- of one case on one library, and every
    variant equal to the first: state, every dt, totalTime (one library's code objects: equal bits whatever the launch order).
    chunk_want: {variant: C} the model must give for the whole-box update of that variant (3D MHD)"""
    once = oracle if isinstance(oracle, OnceOracle) else OnceOracle(oracle)
    first = None
    for var in variants:
        old = lib.set_option(var[0], var[1]) if var is not None else None
        try:
            p = lib.params_from_ini(ini(base), ov)
            if chunk_want is not None:
                ks = p.nz + 2 * p.ghostWidth
                cf = chunk_facts(ks, lib.get_option("chunks"), ks)
                assert cf["C"] == chunk_want[var], "%s [%s] %r: the model says C = %d (%r), the case claims %d" % (base, ov, var, cf["C"], cf, chunk_want[var])
            out = {}
            pc.check_run_vs_oracle(lib, once, base, ov, nsteps, exact=exact, out=out)
        finally:
            if var is not None:
                lib.set_option(var[0], old)
        if first is None:
            first = out
            continue
        what = "%s [%s] %d steps, %s library: variant %r against %r" % (base, ov, nsteps, lib.arithmetic, var, variants[0])
        assert out["dts"] == first["dts"] and out["t"] == first["t"], what
        nbad = int((out["state"] != first["state"]).sum())
        assert nbad == 0, "%s: %d doubles differ" % (what, nbad)
