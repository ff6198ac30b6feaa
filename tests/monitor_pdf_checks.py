"""Checks of the PDF monitor (rgpu_state_pdfs, rgpu_run_steps_pdfs; include/rgpu.h, "PDF monitors") shared by
tests/test_monitor_pdf_host.py (the test-only host emulation, not gpu) and tests/test_monitor_pdf_gpu.py (-m gpu).

`model(C, spec)` is the definition in numpy: the channels are twelve of the sixteen per-cell terms of monitor_planes_checks.cell_terms
(imported, not copied) and v2 = (ekin + ekin) / rho; `classes` is the classification of include/rgpu.h.  Counts are integers, so the
model is exact: every comparison is np.array_equal on uint64."""
import ctypes as C

import numpy as np
import pytest

import ensemble_checks as ec
import monitor_maps_checks as mm
import monitor_planes_checks as mp
from ramsesgpu_amd import _capi
from ramsesgpu_amd.solver import RgpuError, Solver, pdf_axis, pdf_edges

NQ = 13
COLUMNS = (0, 1, 2, 3, 4, 5, 6, 8, 10, 11, 12, 9)   # channel q < 12 of a cell is this column of the plane monitor's per-cell terms
MAGNETIC = ("emag", "bx", "by", "bz", "absdivb")     # exactly +0.0 in every cell of a hydro state

initial_state = mp.initial_state
option = mm.option

# the spec sets of the seam shapes.  EIGHT: linear and octave, signed and unsigned channels; JOINT: (122 + 3)^2 = 15625 words with the
# 1D of its first axis asked for separately (the marginal); FULL: 125 x 128 + 380 + 4 = the word budget exactly; ONEBIN: one bin each
ONE = [("rho", "log2", -8, 8, 3)]
EIGHT = [("rho", "log2", -8, 8, 3), ("mx", "lin", -2.0, 2.0, 50), ("E", "log2", -6, 10, 2), ("ekin", "lin", 0.0, 1.0, 33), ("emag", "log2", -30, 4, 1),
         ("bz", "lin", -1.5, 1.5, 40), ("absdivb", "log2", -60, 0, 0), ("v2", "log2", -20, 6, 2)]
JOINT = [(("rho", "log2", -30, 31, 1), ("eint", "lin", 0.0, 8.0, 122))]
FULL = [(("rho", "log2", -30, 31, 1), ("eint", "lin", -1.0, 9.0, 125)), ("my", "lin", -3.0, 3.0, 377), ("v2", "lin", 0.0, 1.0, 1)]
ONEBIN = [("rho", "lin", -1e300, 1e300, 1), ("E", "log2", 0, 1, 0), (("mz", "lin", -1e9, 1e9, 1), ("rho", "log2", -1, 0, 0))]
SPEC_SETS = {"one": ONE, "eight": EIGHT, "joint": JOINT, "full": FULL, "onebin": ONEBIN}


def is_joint(spec):
    return isinstance(spec[0], (tuple, list))


def words(spec):
    return (pdf_axis(spec[0]).nbins + 3) * (pdf_axis(spec[1]).nbins + 3) if is_joint(spec) else pdf_axis(spec).nbins + 3


assert sum(words(s) for s in FULL) == _capi.PDF_MAX_WORDS and words(JOINT[0]) == 125 * 125


def cell_channels(U, p):
    """the thirteen channels of a ghost-inclusive 3D state over its interior: [13][nz][ny][nx]"""
    with np.errstate(all="ignore"):
        T = mp.cell_terms(U, p)
        return np.array([T[c] for c in COLUMNS] + [(T[5] + T[5]) / T[0]])


def classes(axis, x):
    """the class of every x on the axis: 0 .. nbins - 1 the bins, nbins under, nbins + 1 over, nbins + 2 nan"""
    a = pdf_axis(axis)
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(all="ignore"):
        if a.scale == 0:
            inv = np.float64(a.nbins) / (np.float64(a.hi) - np.float64(a.lo))
            b = np.minimum(np.nan_to_num(np.floor((x - a.lo) * inv), nan=0.0, posinf=a.nbins, neginf=0.0), a.nbins - 1).astype(np.int64)
            cls = np.where(x < a.lo, a.nbins, np.where(x >= a.hi, a.nbins + 1, b))
        else:
            ax = np.abs(x)
            shift = np.uint64(52 - a.sub)
            key0 = int(np.float64(a.lo).view(np.uint64) >> shift)
            b = (np.ascontiguousarray(ax).view(np.uint64) >> shift).astype(np.int64) - key0
            cls = np.where(ax < a.lo, a.nbins, np.where(ax >= a.hi, a.nbins + 1, b))
    return np.where(np.isnan(x), a.nbins + 2, cls)


def model(Ch, spec):
    """the table of spec over the cells whose channels are Ch[13][...]: uint64, (na + 3,) or (na + 3, nb + 3)"""
    axes = spec if is_joint(spec) else (spec,)
    idx = [classes(a, Ch[pdf_axis(a).channel]).ravel() for a in axes]
    shape = tuple(pdf_axis(a).nbins + 3 for a in axes)
    flat = idx[0] if len(axes) == 1 else idx[0] * shape[1] + idx[1]
    assert flat.min() >= 0 and flat.max() < int(np.prod(shape))
    return np.bincount(flat, minlength=int(np.prod(shape))).astype(np.uint64).reshape(shape)


def assert_same_words(got, want, what):
    assert got.dtype == np.uint64 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    assert np.array_equal(got, want), (what, np.argwhere(got != want)[:5])


def check_tables(sv, p, U, specs, what, Ch=None):
    """Solver.state_pdfs of specs == the model of the downloaded state U; every table sums to the cells; the marginal of every joint
    table over b == the 1D table of a, taken in a call of its own"""
    Ch = cell_channels(U, p) if Ch is None else Ch
    got = sv.state_pdfs(specs)
    assert len(got) == len(specs)
    for spec, g in zip(specs, got):
        assert_same_words(g, model(Ch, spec), (what, spec))
        assert int(g.sum()) == p.nx * p.ny * p.nz, (what, spec)
        if is_joint(spec):
            assert_same_words(g.sum(axis=1, dtype=np.uint64), sv.state_pdfs([spec[0]])[0], (what, spec, "marginal"))
    return got


def check_seams(lib, base, ov, sets=SPEC_SETS):
    """a lone context before stepping and after 3 steps, every spec set: check_tables; the call changes neither the checksum nor the
    device-ready flag; the steps after a sample run as ever"""
    p = lib.params_from_ini(ec.ini(base), ov)
    U0 = initial_state(lib, base, ov, p)
    sv = Solver(p, lib)
    try:
        sv.start(U0, 0)
        for steps in (0, 3):
            if steps:
                assert sv.run_steps(steps) == steps
            par = sv.nStep % 2
            ready, checksum = lib.lib.rgpu_device_time_step_ready(sv.ctx, par), sv.state_checksum(par)
            U = sv.getDataHost()
            Ch = cell_channels(U, p)
            for name, specs in sets.items():
                check_tables(sv, p, U, specs, (base, ov, steps, name), Ch)
            assert lib.lib.rgpu_device_time_step_ready(sv.ctx, par) == ready and sv.state_checksum(par) == checksum
        assert sv.run_steps(2) == 2
    finally:
        sv.close()


CRAFT_OCTAVE = ("rho", "log2", -3, 3, 2)
CRAFT_LINEAR = ("rho", "lin", 0.25, 8.0, 31)


def crafted_values():
    """lo, hi and their neighbours, every sub-bin edge of CRAFT_OCTAVE and its neighbours, zeros, a subnormal, negative values, the
    infinities and NaN"""
    vals = []
    for e in list(pdf_edges(CRAFT_OCTAVE)) + list(pdf_edges(CRAFT_LINEAR)):
        vals += [e, np.nextafter(e, 0.0), np.nextafter(e, np.inf)]
    vals += [0.0, -0.0, 5e-324, 2.0 ** -1022, -1.5, -0.125, -8.0, np.nextafter(-8.0, 0.0), np.inf, -np.inf, np.nan, 1e308, 3.0, 0.3]
    return np.array(vals, dtype=np.float64)


def check_octave_model_against_searchsorted():
    """numpy only: the integer rule of the octave bins == a search in the exact edges"""
    a = pdf_axis(CRAFT_OCTAVE)
    edges = pdf_edges(CRAFT_OCTAVE)
    assert len(edges) == a.nbins + 1 and edges[0] == a.lo and edges[-1] == a.hi and (np.diff(edges) > 0).all()
    x = np.concatenate([crafted_values(), np.random.RandomState(7).uniform(-9.0, 9.0, 4000)])
    ax = np.abs(x)
    naive = np.where(np.isnan(x), a.nbins + 2, np.where(ax < a.lo, a.nbins, np.where(ax >= a.hi, a.nbins + 1, np.searchsorted(edges, ax, side="right") - 1)))
    assert np.array_equal(classes(CRAFT_OCTAVE, x), naive)


def check_crafted_state(lib, base="implode3d", ov="mesh.nx=20;mesh.ny=9;mesh.nz=5"):
    """a state whose density is written cell by cell with crafted_values: every value lands where the model puts it, on the octave and
    on the linear axis, alone and jointly; the channels a wild density reaches (ekin, eint, v2) are classified as the model does"""
    check_octave_model_against_searchsorted()
    p = lib.params_from_ini(ec.ini(base), ov)
    U = initial_state(lib, base, ov, p).copy()
    gw, vals = p.ghostWidth, crafted_values()
    n = p.nx * p.ny * p.nz
    assert len(vals) <= n
    inner = U[_capi.ID, gw:gw + p.nz, gw:gw + p.ny, gw:gw + p.nx]
    inner[...] = np.resize(vals, n).reshape(inner.shape)
    specs = [CRAFT_OCTAVE, CRAFT_LINEAR, (CRAFT_OCTAVE, CRAFT_LINEAR), ("ekin", "log2", -20, 20, 1), ("eint", "lin", -10.0, 10.0, 20), ("v2", "log2", -20, 20, 0)]
    sv = Solver(p, lib)
    try:
        sv.upload(U)
        got = sv.state_pdfs(specs, 0)
    finally:
        sv.close()
    Ch = cell_channels(U, p)
    assert np.array_equal(Ch[0], inner, equal_nan=True)
    for spec, g in zip(specs, got):
        assert_same_words(g, model(Ch, spec), spec)
        assert int(g.sum()) == n
    a = pdf_axis(CRAFT_OCTAVE)
    reps, rest = divmod(n, len(vals))
    count = lambda pred: sum(reps + (1 if k < rest else 0) for k, v in enumerate(vals) if pred(v))
    assert int(got[0][a.nbins + 2]) == count(np.isnan) and int(got[0][a.nbins + 1]) == count(lambda v: abs(v) >= a.hi) and int(got[0][a.nbins]) == count(lambda v: abs(v) < a.lo)
    assert int(got[0][0]) == count(lambda v: a.lo <= abs(v) < a.lo * 1.25)


def check_against_the_monitor(lib, base, ov):
    """min_rho of rgpu_state_monitor3d lies in the lowest non-empty bin of a covering octave spec of rho, max_absdivb in the highest
    non-empty bin of absdivb (below lo where every bin is empty); in a hydro state the magnetic channels are all in the class of 0"""
    p = lib.params_from_ini(ec.ini(base), ov)
    sv = Solver(p, lib)
    try:
        sv.start(initial_state(lib, base, ov, p), 0)
        assert sv.run_steps(3) == 3
        mon = sv.state_monitor()
        rho_axis, div_axis = ("rho", "log2", -40, 40, 3), ("absdivb", "log2", -100, 20, 2)
        rho, div = sv.state_pdfs([rho_axis, div_axis])
        n = p.nx * p.ny * p.nz
        edges = pdf_edges(rho_axis)
        assert not rho[-3:].any()
        b = int(np.flatnonzero(rho[:-3])[0])
        assert edges[b] <= mon[7] < edges[b + 1], (mon[7], edges[b], edges[b + 1])
        edges = pdf_edges(div_axis)
        assert not div[-2:].any()
        filled = np.flatnonzero(div[:-3])
        if len(filled):
            assert edges[filled[-1]] <= mon[9] < edges[filled[-1] + 1], (mon[9], edges[filled[-1]], edges[filled[-1] + 1])
        else:
            assert mon[9] < edges[0] and int(div[-3]) == n
        if not p.mhdEnabled:
            for name in MAGNETIC:
                lin, octave = sv.state_pdfs([(name, "lin", -1.0, 1.0, 2), (name, "log2", -40, 40, 0)])
                assert int(lin[1]) == n and int(octave[-3]) == n, name   # 0 is the low edge of the upper linear bin; below every octave
    finally:
        sv.close()


RUN_SPECS = [("rho", "log2", -8, 8, 3), (("rho", "log2", -4, 4, 2), ("eint", "lin", 0.0, 4.0, 29)), ("mx", "lin", -1.0, 1.0, 41)]
_STEPPED = {}   # (library path, base, ov, end time): {"sv": a lone Solver at step n, "at": {n: (tables, t)}} -- computed once, shared, left alone


def stepped_reference(lib, base, ov, p, U0, n, tEnd=None):
    """the second lone context: stepped singly (rgpu_run_steps one at a time) to step n; returns (rgpu_state_pdfs of RUN_SPECS there,
    its time).  Steps are taken in ascending n; the results are kept."""
    key = (lib.path, base, ov, tEnd)
    end = float("inf") if tEnd is None else tEnd
    ent = _STEPPED.get(key)
    if ent is None:
        sv = Solver(p, lib)
        sv.start(U0, 0)
        ent = _STEPPED[key] = {"sv": sv, "at": {}}
    sv = ent["sv"]
    while sv.nStep < n:
        assert sv.run_steps(1, end) == 1
        ent["at"][sv.nStep] = (sv.state_pdfs(RUN_SPECS), sv.totalTime)
    return ent["at"][n]


def close_references():
    for ent in _STEPPED.values():
        ent["sv"].close()
    _STEPPED.clear()


batch_samples = mm.batch_samples


def check_run(lib, base, ov, nsteps, every, pieces=None, tEnd=None, expect_batch=None):
    """One lone context run for nsteps (in `pieces`) through rgpu_run_steps_pdfs with RUN_SPECS, one through rgpu_run_steps_log:
      * the same return values, dt_log, nStep, t, dt, checksum and state, bit for bit (sampling only reads)
      * the sample steps are the multiples of `every` among the steps that ran, mon_t the accumulated dt log
      * every sample == rgpu_state_pdfs of a second lone context stepped singly to that step, every word
      * the last sample, when it is of the final state, == the model on the monitored context's own download
      * the other monitors' counters stay 0; expect_batch: None, or a function (steps that ran, device-ready flag) -> the wanted
        rgpu_pdf_batch_samples
    Returns (done, steps sampled, tables: per spec [n][...], batch samples)."""
    p = lib.params_from_ini(ec.ini(base), ov)
    U0 = initial_state(lib, base, ov, p)
    specs = RUN_SPECS
    end = float("inf") if tEnd is None else tEnd
    runs = []
    for sampled in (True, False):
        sv = Solver(p, lib)
        try:
            sv.start(U0, 0)
            done, log, steps, ts, vals = 0, [], [], [], [[] for _ in specs]
            for n in (pieces or [nsteps]):
                if sampled:
                    d, s = sv.run_steps_pdfs(n, every, specs, end)
                    steps += [int(x) for x in s.step]
                    ts += [float(x) for x in s.t]
                    for m, a in enumerate(s.pdfs):
                        assert a.shape[0] == len(s.step) and a.dtype == np.uint64
                        vals[m] += list(a)
                else:
                    d = sv.run_steps(n, end)
                done += d
                log += list(sv.dt_log)
            L = lib.lib
            runs.append({"done": done, "log": log, "nStep": sv.nStep, "t": sv.totalTime, "dt": sv.dt, "checksum": sv.state_checksum(sv.nStep % 2), "full": sv.getDataHost(),
                         "ready": L.rgpu_device_time_step_ready(sv.ctx, sv.nStep % 2), "batch": L.rgpu_pdf_batch_samples(sv.ctx),
                         "other": L.rgpu_monitor_batch_samples(sv.ctx) + L.rgpu_monitor_planes_batch_samples(sv.ctx) + L.rgpu_map_batch_samples(sv.ctx),
                         "steps": steps, "ts": ts, "vals": vals})
        finally:
            sv.close()
    a, b = runs
    assert (a["done"], a["nStep"], a["t"], a["dt"], a["checksum"], a["log"]) == (b["done"], b["nStep"], b["t"], b["dt"], b["checksum"], b["log"]), "sampling changed the run"
    assert np.array_equal(a["full"], b["full"], equal_nan=True), "sampling changed the state"
    assert b["batch"] == 0 and a["other"] == 0 and b["other"] == 0
    assert a["steps"] == [s for s in range(1, a["done"] + 1) if s % every == 0], (a["steps"], a["done"])
    assert a["ts"] == [ec.time_of(a["log"][:s]) for s in a["steps"]], "mon_t against the accumulated dt log"
    n = p.nx * p.ny * p.nz
    for k, s in enumerate(a["steps"]):
        ref, t = stepped_reference(lib, base, ov, p, U0, s, tEnd)
        for m, spec in enumerate(specs):
            assert_same_words(a["vals"][m][k], ref[m], (s, spec, "against rgpu_state_pdfs of a lone context stepped singly"))
            assert int(a["vals"][m][k].sum()) == n
    if a["steps"] and a["steps"][-1] == a["nStep"]:
        Ch = cell_channels(a["full"], p)
        for m, spec in enumerate(specs):
            assert_same_words(a["vals"][m][-1], model(Ch, spec), (spec, "the last sample against the model of the downloaded state"))
    if expect_batch is not None:
        assert a["batch"] == expect_batch(a["done"], a["ready"]), (a["batch"], a["done"], a["ready"])
    return a["done"], a["steps"], [np.array(v) for v in a["vals"]], a["batch"]


def check_refusals(L, ini, slab=True):
    """the refusals of include/rgpu.h, each with its code and the words of its message; nothing has run afterwards"""
    Axis, Spec = _capi.RgpuPdfAxis, _capi.RgpuPdfSpec
    none = Axis(0, 0, 0, 0, 0.0, 0.0)
    rho = Axis(0, 1, 16 << 3, 3, 2.0 ** -8, 2.0 ** 8)
    lin = Axis(1, 0, 50, 0, -2.0, 2.0)
    good = (Spec * 2)(Spec(rho, none), Spec(rho, lin))
    W = 131 + 131 * 53
    assert L.lib.rgpu_pdf_words(C.byref(good[0])) == 131 and L.lib.rgpu_pdf_words(C.byref(good[1])) == 131 * 53 and L.lib.rgpu_pdf_words(None) == 0
    out = (C.c_ulonglong * W)()
    n, t, d, mn = C.c_int(0), C.c_double(0.0), C.c_double(0.0), C.c_int(7)
    ms, mt, mv = (C.c_int * 5)(), (C.c_double * 5)(), (C.c_ulonglong * (5 * W))()
    full = [C.byref(n), C.byref(t), C.byref(d), good, C.byref(mn), ms, mt, mv]

    def call(ctx, nsteps, every, npdfs, args):
        mn.value = 7
        a, b, c_, specs, e, f, g, h = args
        return L.lib.rgpu_run_steps_pdfs(ctx, nsteps, 1e300, a, b, c_, None, every, npdfs, specs, e, f, g, h)
    p2 = L.params_from_ini(ini("orszag-tang"), "mesh.nx=16;mesh.ny=16")
    p3 = L.params_from_ini(ini("orszag-tang3d"), "mesh.nx=16;mesh.ny=12;mesh.nz=8")
    sv = Solver(p2, L)
    try:
        sv.start(L.init_condition(ini("orszag-tang"), "mesh.nx=16;mesh.ny=16", p2), 0)
        assert L.lib.rgpu_state_pdfs(sv.ctx, 0, 2, good, out) == -5 and b"3D" in L.lib.rgpu_last_error(sv.ctx)   # RGPU_EUNSUPPORTED
        assert call(sv.ctx, 4, 2, 2, full) == -5 and b"3D" in L.lib.rgpu_last_error(sv.ctx) and mn.value == 0 and n.value == 0
        with pytest.raises(RgpuError):
            sv.state_pdfs([("rho", "log2", -8, 8, 3)])
    finally:
        sv.close()
    if slab:
        ps = L.params_from_ini(ini("orszag-tang3d"), "mesh.nx=16;mesh.ny=16;mesh.nz=16", slab=(0, 2))
        sv = Solver(ps, L)
        try:
            assert L.lib.rgpu_state_pdfs(sv.ctx, 0, 2, good, out) == -1                                           # RGPU_EINVAL
            assert call(sv.ctx, 4, 2, 2, full) == -1 and n.value == 0 and mn.value == 0
        finally:
            sv.close()
    sv = Solver(p3, L)
    try:
        sv.start(L.init_condition(ini("orszag-tang3d"), "mesh.nx=16;mesh.ny=12;mesh.nz=8", p3), 0)
        assert L.lib.rgpu_state_pdfs(sv.ctx, 0, 2, good, None) == -1 and L.lib.rgpu_state_pdfs(sv.ctx, 0, 2, None, out) == -1 and L.lib.rgpu_state_pdfs(None, 0, 2, good, out) == -1
        for every in (0, -2):
            assert call(sv.ctx, 4, every, 2, full) == -1 and b"every" in L.lib.rgpu_last_error(sv.ctx) and mn.value == 0
        for hole in range(8):
            args = list(full)
            args[hole] = None
            assert call(sv.ctx, 4, 2, 2, args) == -1 and b"null pointer" in L.lib.rgpu_last_error(sv.ctx), hole
            assert mn.value == (7 if hole == 4 else 0)
        assert call(sv.ctx, -1, 2, 2, full) == -1 and mn.value == 0
        assert call(None, 4, 2, 2, full) == -1
        for npdfs in (0, -1, _capi.PDF_MAX + 1):
            assert call(sv.ctx, 4, 2, npdfs, full) == -1 and b"npdfs" in L.lib.rgpu_last_error(sv.ctx) and mn.value == 0
            assert L.lib.rgpu_state_pdfs(sv.ctx, 0, npdfs, good, out) == -1 and b"npdfs" in L.lib.rgpu_last_error(sv.ctx)
        # a bad axis -- channel, scale, range, the power-of-two rule, nbins, sub -- as axis a of a 1D spec and as axis b of a joint one
        bad_axes = [Axis(-1, 0, 4, 0, 0.0, 1.0), Axis(13, 0, 4, 0, 0.0, 1.0), Axis(0, 2, 4, 0, 0.0, 1.0), Axis(0, -1, 4, 0, 0.0, 1.0),
                    Axis(0, 0, 4, 0, 1.0, 1.0), Axis(0, 0, 4, 0, 2.0, 1.0), Axis(0, 0, 4, 0, 0.0, float("inf")), Axis(0, 0, 4, 0, float("nan"), 1.0), Axis(0, 0, -1, 0, 0.0, 1.0),
                    Axis(0, 1, 4, 0, 3.0, 48.0), Axis(0, 1, 4, 0, 1.0, 24.0), Axis(0, 1, 4, 0, -16.0, -1.0), Axis(0, 1, 4, 0, 0.0, 16.0), Axis(0, 1, 1030, 0, 5e-324, 2.0 ** -44),
                    Axis(0, 1, 4, 0, 16.0, 1.0), Axis(0, 1, 5, 0, 1.0, 16.0), Axis(0, 1, 4, 1, 1.0, 16.0), Axis(0, 1, 4 << 7, 7, 1.0, 16.0), Axis(0, 1, 4, -1, 1.0, 16.0),
                    Axis(0, 1, 0, 0, 1.0, 1.0), Axis(0, 0, 20000, 0, 0.0, 1.0)]
        for bad in bad_axes:
            cases = [(0, Spec(bad, none)), (1, Spec(bad, none))] + ([(1, Spec(rho, bad))] if bad.nbins != 0 else [])   # (b.nbins == 0: a 1D spec)
            for where, spec in cases:
                specs = (Spec * 2)(good[0], good[0])
                specs[where] = spec
                args = list(full)
                args[3] = specs
                what = (bad.channel, bad.scale, bad.nbins, bad.sub, bad.lo, bad.hi, where)
                assert call(sv.ctx, 4, 2, 2, args) == -1 and b"pdf %d:" % where in L.lib.rgpu_last_error(sv.ctx) and mn.value == 0, what
                assert L.lib.rgpu_state_pdfs(sv.ctx, 0, 2, specs, out) == -1 and b"pdf %d:" % where in L.lib.rgpu_last_error(sv.ctx), what
                assert L.lib.rgpu_pdf_words(C.byref(spec)) == 0, what
        # a joint spec above the budget on its own; specs within it that exceed it together
        big = Spec(Axis(0, 0, 125, 0, 0.0, 1.0), Axis(1, 0, 126, 0, 0.0, 1.0))
        assert L.lib.rgpu_pdf_words(C.byref(big)) == 0
        half = Spec(Axis(0, 0, 125, 0, 0.0, 1.0), Axis(1, 0, 61, 0, 0.0, 1.0))   # 128 x 64 words
        assert L.lib.rgpu_pdf_words(C.byref(half)) == 8192
        for specs, npdfs in (((Spec * 2)(good[0], big), 2), ((Spec * 3)(half, half, Spec(Axis(0, 0, 1, 0, 0.0, 1.0), none)), 3)):
            args = list(full)
            args[3] = specs
            assert call(sv.ctx, 4, 2, npdfs, args) == -1 and b"words" in L.lib.rgpu_last_error(sv.ctx) and mn.value == 0
            assert L.lib.rgpu_state_pdfs(sv.ctx, 0, npdfs, specs, out) == -1 and b"words" in L.lib.rgpu_last_error(sv.ctx)
        assert n.value == 0 and t.value == 0.0 and L.lib.rgpu_pdf_batch_samples(sv.ctx) == 0 and not any(out) and not any(mv)   # nothing ran
        assert call(sv.ctx, 4, 2, 2, full) == 4 and n.value == 4 and mn.value == 2 and list(ms)[:2] == [2, 4]
        assert sum(mv[:131]) == 16 * 12 * 8 and sum(mv[W:W + 131]) == 16 * 12 * 8
        assert call(sv.ctx, 0, 2, 2, full) == 0 and mn.value == 0
    finally:
        sv.close()
    assert L.lib.rgpu_pdf_batch_samples(None) == 0


def parse_pdfs_list(path):
    """[(step, t, pdf, spec, file)] of <prefix>_pdfs.txt, whose header is checked"""
    lines = open(path).read().splitlines()
    assert lines[0] == "# nStep totalTime pdf spec file"
    rows = [ln.split() for ln in lines[1:]]
    assert all(len(r) == 5 for r in rows)
    return [(int(r[0]), float(r[1]), int(r[2]), r[3], r[4]) for r in rows]


def check_driver_files(lib, run, tmp_path, base="implode3d", ov="mesh.nx=24;mesh.ny=24;mesh.nz=12", prefix="implode3d"):
    """`run(overrides)` drives the run driver.  [pdfs] enabled=yes every=3 with a 1D and a joint spec, 10 steps: the .npy files load with
    np.load and equal Solver.run_steps_pdfs, <prefix>_pdfs.txt lists them; with enabled=no nothing is written; with [monitor] on as
    well the monitor file is byte for byte the one of a run without [pdfs]; with [maps] on as well the maps take the batches and the
    PDFs are the same words"""
    common = ov + ";run.nstepmax=10;run.noutput=1000;output.outputVtk=no;output.outputHdf5=no;output.outputDir=%s"
    texts = ["rho:log2:-8:8:3", "rho:log2:-4:4:2,eint:lin:0:4:29"]
    pdfs = ";pdfs.every=3;pdfs.pdf0=%s;pdfs.pdf1=%s" % tuple(texts)
    for name, extra in (("pdfs", ";pdfs.enabled=yes" + pdfs), ("off", ";pdfs.enabled=no" + pdfs), ("both", ";pdfs.enabled=yes" + pdfs + ";monitor.enabled=yes;monitor.every=2"),
                        ("monitor", ";monitor.enabled=yes;monitor.every=2"), ("maps", ";pdfs.enabled=yes" + pdfs + ";maps.enabled=yes;maps.every=2;maps.map0=z:6")):
        d = tmp_path / name
        d.mkdir()
        run(common % d + extra)
    assert not list((tmp_path / "off").glob("*_pdf*")) and not list((tmp_path / "monitor").glob("*_pdf*"))
    assert open(tmp_path / "both" / (prefix + "_monitor.txt"), "rb").read() == open(tmp_path / "monitor" / (prefix + "_monitor.txt"), "rb").read()
    p = lib.params_from_ini(ec.ini(base), ov)
    specs = [("rho", "log2", -8, 8, 3), (("rho", "log2", -4, 4, 2), ("eint", "lin", 0.0, 4.0, 29))]
    sv = Solver(p, lib)
    try:
        sv.start(lib.init_condition(ec.ini(base), ov, p), 0)
        done, series = sv.run_steps_pdfs(10, 3, specs)
    finally:
        sv.close()
    assert done == 10 and list(series.step) == [3, 6, 9]
    for name in ("pdfs", "both", "maps"):
        d = tmp_path / name
        rows = parse_pdfs_list(d / (prefix + "_pdfs.txt"))
        want = [(s, t, m, texts[m], "%s_pdf%d_%07d.npy" % (prefix, m, s)) for s, t in zip(series.step, series.t) for m in range(2)]
        assert rows == want, (rows, want)
        assert sorted(f.name for f in d.glob("*_pdf*.npy")) == sorted(r[4] for r in rows)
        for k, s in enumerate(series.step):
            for m in range(2):
                got = np.load(d / ("%s_pdf%d_%07d.npy" % (prefix, m, s)))
                assert got.dtype == np.dtype("<u8") and got.flags["C_CONTIGUOUS"]
                assert_same_words(got, series.pdfs[m][k], (name, s, m))
