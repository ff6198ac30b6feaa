"""Checks of the map monitor (rgpu_state_maps, rgpu_run_steps_mapped; include/rgpu.h, "map monitors") shared by
tests/test_monitor_maps_host.py (the test-only host emulation, not gpu) and tests/test_monitor_maps_gpu.py (-m gpu).

`model(U, p, spec)` is the definition in numpy: the channels are twelve of the sixteen per-cell terms of
monitor_planes_checks.cell_terms (imported, not copied), and a pixel is `acc = acc + term_plane` in a Python loop over w from +0.0 --
element-wise and sequential, hence the exact bits; np.sum is not used.  It must equal the libraries' doubles bit for bit."""
import contextlib
import math

import numpy as np

import ensemble_checks as ec
import monitor_planes_checks as mp
from ramsesgpu_amd import _capi
from ramsesgpu_amd.solver import Solver

NQ = 12
COLUMNS = (0, 1, 2, 3, 4, 5, 6, 8, 10, 11, 12, 15)   # channel q of a cell is this column of the plane monitor's per-cell terms
HYDRO_ZERO = (6, 8, 9, 10)                            # emag, bx, by, bz: exactly +0.0 in every pixel of a hydro state
NAN_DENSITY = (0, 5, 7, 11)                           # rho, ekin, eint, rho2: the channels a NaN density reaches
AXES = "xyz"

initial_state = mp.initial_state


def extent(p, axis):
    return (p.nx, p.ny, p.nz)[AXES.index(axis)]


def cell_channels(U, p):
    """the twelve channels of a ghost-inclusive 3D state over its interior: [12][nz][ny][nx]"""
    T = mp.cell_terms(U, p)
    return np.array([T[c] for c in COLUMNS])


def model(U, p, spec, T=None):
    """[12][nv][nu] of spec = (axis, lo, hi): the planes w = lo .. hi - 1 along the axis added in ascending order from +0.0"""
    axis, lo, hi = spec
    with np.errstate(all="ignore"):
        T = cell_channels(U, p) if T is None else T
        planes = np.moveaxis(T, 3 - AXES.index(axis), 1)   # [12][w][v][u]: dropping an axis of (k, j, i) leaves (v, u) in place
        acc = np.zeros(planes.shape[:1] + planes.shape[2:])
        for w in range(lo, hi):
            acc = acc + planes[:, w]
    return acc


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def assert_same_bits(got, want, what):
    """every double, as uint64: -0.0 is mapped to +0.0 on neither side (the model produces +0.0 too)"""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(bits(got) != bits(want))
    assert bad.size == 0, (what, len(bad), bad[:5], got[tuple(bad[0])], want[tuple(bad[0])])


@contextlib.contextmanager
def option(lib, name, value):
    """a diagnostic option of the library for the length of a block, restored afterwards"""
    if value is None:
        yield
        return
    old = lib.lib.rgpu_get_option(name.encode())
    lib.lib.rgpu_set_option(name.encode(), int(value))
    try:
        yield
    finally:
        lib.lib.rgpu_set_option(name.encode(), old)


def seam_specs(p):
    """per axis: all, [1, n - 1), the single cells 0 and n - 1 (the latter reads its high faces from the ghost layer) and a middle cell;
    on x also the ranges that straddle the seam between the first and the second 64-wide tile, where the box has one"""
    out = []
    for axis in AXES:
        n = extent(p, axis)
        for s in ((0, n), (1, n - 1), (0, 1), (n - 1, n), (n // 2, n // 2 + 1)):
            if (axis,) + s not in out:
                out.append((axis,) + s)
    if p.nx > 65:
        out += [("x", 63, 65), ("x", 62, 66)]
    return out


def take_maps(sv, specs, parity=None):
    """Solver.state_maps, RGPU_MAP_MAX specs per call"""
    out = []
    for k in range(0, len(specs), _capi.MAP_MAX):
        out += sv.state_maps(specs[k:k + _capi.MAP_MAX], parity)
    return out


def check_seams(lib, base, ov, x_variants=(None,)):
    """a lone context before stepping and after 3 steps, every spec of seam_specs: the map == the model, every double as uint64; x maps
    with each of x_variants (option "map_x_tiled"; None: as the library chooses); the call changes neither the checksum nor the
    device-ready flag; the hydro channels that are exactly +0.0; the slice identity and the any-order bound below"""
    p = lib.params_from_ini(ec.ini(base), ov)
    U0 = initial_state(lib, base, ov, p)
    specs = seam_specs(p)
    sv = Solver(p, lib)
    try:
        sv.start(U0, 0)
        for steps in (0, 3):
            if steps:
                assert sv.run_steps(steps) == steps
            par = sv.nStep % 2
            ready, checksum = lib.lib.rgpu_device_time_step_ready(sv.ctx, par), sv.state_checksum(par)
            U = sv.getDataHost()
            T = cell_channels(U, p)
            for variant in x_variants:
                with option(lib, "map_x_tiled", variant):
                    chosen = [s for s in specs if s[0] == "x" or variant == x_variants[0]]
                    maps = take_maps(sv, chosen)
                for spec, got in zip(chosen, maps):
                    assert np.isfinite(got).all(), spec
                    assert_same_bits(got, model(U, p, spec, T), (base, ov, steps, spec, variant))
                    if not p.mhdEnabled:
                        assert not bits(got[list(HYDRO_ZERO)]).any(), spec   # +0.0: every bit clear
                if variant == x_variants[0]:
                    check_slice_identity(p, U, dict(zip(chosen, maps)))
                    check_any_order_bound(p, T, dict(zip(chosen, maps))[("z", 0, p.nz)], sv.state_monitor())
            assert lib.lib.rgpu_device_time_step_ready(sv.ctx, par) == ready and sv.state_checksum(par) == checksum
        assert sv.run_steps(2) == 2   # (the steps after a sample run as ever)
    finally:
        sv.close()


def check_slice_identity(p, U, maps):
    """independent of the model: rho, mx, my, mz, E of a single-cell map are the interior plane of the download"""
    gw = p.ghostWidth
    inner = U[:, gw:gw + p.nz, gw:gw + p.ny, gw:gw + p.nx]
    seen = set()
    for (axis, lo, hi), got in maps.items():
        if hi != lo + 1:
            continue
        seen.add(axis)
        for q, var in enumerate((_capi.ID, _capi.IU, _capi.IV, _capi.IW, _capi.IP)):
            assert np.array_equal(got[q], np.take(inner[var], lo, axis=2 - AXES.index(axis))), (axis, lo, _capi.MAP_NAMES[q])
    assert seen == set(AXES)


def check_any_order_bound(p, T, zmap, monitor):
    """the full z map: the pixels of channels 0 - 6 summed (math.fsum: no error of its own beyond one rounding) stay within
    N 2^-53 sum|terms| of the column of rgpu_state_monitor3d, N = nx ny nz -- the bound include/rgpu.h states for any summation order"""
    N = p.nx * p.ny * p.nz
    for q in range(7):
        scale = math.fsum(abs(float(x)) for x in T[q].ravel())
        total = math.fsum(float(x) for x in zmap[q].ravel())
        print("any-order bound", _capi.MAP_NAMES[q], total, monitor[q], abs(total - monitor[q]), N * 2.0 ** -53 * scale)
        assert abs(total - monitor[q]) <= N * 2.0 ** -53 * scale, (_capi.MAP_NAMES[q], total, monitor[q], scale)


def check_nan_cell(lib, base, ov):
    """one NaN density at an interior cell: in every map whose range holds the cell exactly one pixel is NaN, in exactly rho, ekin, eint
    and rho2; every other double is the clean state's, bit for bit; maps whose range does not hold the cell are untouched"""
    p = lib.params_from_ini(ec.ini(base), ov)
    U0 = initial_state(lib, base, ov, p)
    gw = p.ghostWidth
    cell = {"x": p.nx - 2, "y": p.ny // 2, "z": p.nz // 2}
    specs = []
    for axis in AXES:
        n, c = extent(p, axis), cell[axis]
        specs += [(axis, 0, n), (axis, c, c + 1), (axis, c - 1, c + 1), (axis, 0, c), (axis, c + 1, n)]
    sv = Solver(p, lib)
    try:
        sv.upload(U0)
        clean = take_maps(sv, specs, 0)
        U1 = U0.copy()
        U1[_capi.ID, gw + cell["z"], gw + cell["y"], gw + cell["x"]] = np.nan
        sv.upload(U1)
        dirty = take_maps(sv, specs, 0)
    finally:
        sv.close()
    T0 = cell_channels(U0, p)
    for spec, a, b in zip(specs, clean, dirty):
        axis, lo, hi = spec
        assert not np.isnan(a).any()
        assert_same_bits(a, model(U0, p, spec, T0), ("clean", spec))
        if not lo <= cell[axis] < hi:
            assert_same_bits(b, a, ("untouched", spec))
            continue
        u, v = [cell[x] for x in AXES if x != axis]   # (x, y), (x, z) or (y, z): u is the first
        nan = np.argwhere(np.isnan(b))
        assert sorted(map(tuple, nan)) == sorted((q, v, u) for q in NAN_DENSITY), (spec, nan)
        keep = ~np.isnan(b)
        assert (bits(b)[keep] == bits(a)[keep]).all(), spec
        assert np.array_equal(b, model(U1, p, spec), equal_nan=True), spec


def run_specs(p):
    """the three maps of the mapped runs: a z slice, a range along y, everything along x"""
    return [("z", p.nz // 2, p.nz // 2 + 1), ("y", 2, p.ny - 3), ("x", 0, p.nx)]


_STEPPED = {}   # (library path, base, ov, end time): {"sv": a lone Solver at step n, "at": {n: (maps, t)}} -- computed once, shared, left alone


def stepped_reference(lib, base, ov, p, U0, n, tEnd=None):
    """the second lone context: stepped singly (rgpu_run_steps one at a time) to step n; returns (rgpu_state_maps of run_specs there,
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
        ent["at"][sv.nStep] = (sv.state_maps(run_specs(p)), sv.totalTime)
    return ent["at"][n]


def close_references():
    for ent in _STEPPED.values():
        ent["sv"].close()
    _STEPPED.clear()


def batch_samples(every):
    """rgpu_map_batch_samples of one call of `done` steps from step 0: the qualifying steps behind the first, plain step -- on the
    device path, which the context must be on afterwards"""
    def want(done, ready):
        assert ready == 1, "the context does not take its time step from the device"
        return len([s for s in range(2, done + 1) if s % every == 0])
    return want


def check_mapped(lib, base, ov, nsteps, every, pieces=None, tEnd=None, expect_batch=None):
    """One lone context run for nsteps (in `pieces`) through rgpu_run_steps_mapped with run_specs, one through rgpu_run_steps_log:
      * the same return values, dt_log, nStep, t, dt, checksum and state, bit for bit (sampling only reads)
      * the sample steps are the multiples of `every` among the steps that ran, mon_t the accumulated dt log
      * every sample == rgpu_state_maps of a second lone context stepped singly to that step, every double as uint64
      * the last sample, when it is of the final state, == the model on the monitored context's own download
      * the monitor's and the plane monitor's counters stay 0; expect_batch: None, or a function (steps that ran, device-ready flag)
        -> the wanted rgpu_map_batch_samples
    Returns (done, steps sampled, maps: per spec [n][12][nv][nu], batch samples)."""
    p = lib.params_from_ini(ec.ini(base), ov)
    U0 = initial_state(lib, base, ov, p)
    specs = run_specs(p)
    end = float("inf") if tEnd is None else tEnd
    runs = []
    for mapped in (True, False):
        sv = Solver(p, lib)
        try:
            sv.start(U0, 0)
            done, log, steps, ts, vals = 0, [], [], [], [[] for _ in specs]
            for n in (pieces or [nsteps]):
                if mapped:
                    d, s = sv.run_steps_mapped(n, every, specs, end)
                    steps += [int(x) for x in s.step]
                    ts += [float(x) for x in s.t]
                    for m, a in enumerate(s.maps):
                        assert a.shape[0] == len(s.step) and a.shape[1] == NQ
                        vals[m] += list(a)
                else:
                    d = sv.run_steps(n, end)
                done += d
                log += list(sv.dt_log)
            runs.append({"done": done, "log": log, "nStep": sv.nStep, "t": sv.totalTime, "dt": sv.dt, "checksum": sv.state_checksum(sv.nStep % 2), "full": sv.getDataHost(),
                         "ready": lib.lib.rgpu_device_time_step_ready(sv.ctx, sv.nStep % 2), "batch": lib.lib.rgpu_map_batch_samples(sv.ctx),
                         "other": lib.lib.rgpu_monitor_batch_samples(sv.ctx) + lib.lib.rgpu_monitor_planes_batch_samples(sv.ctx), "steps": steps, "ts": ts, "vals": vals})
        finally:
            sv.close()
    a, b = runs
    assert (a["done"], a["nStep"], a["t"], a["dt"], a["checksum"], a["log"]) == (b["done"], b["nStep"], b["t"], b["dt"], b["checksum"], b["log"]), "sampling changed the run"
    assert np.array_equal(a["full"], b["full"], equal_nan=True), "sampling changed the state"
    assert b["batch"] == 0 and a["other"] == 0 and b["other"] == 0
    assert a["steps"] == [s for s in range(1, a["done"] + 1) if s % every == 0], (a["steps"], a["done"])
    assert a["ts"] == [ec.time_of(a["log"][:s]) for s in a["steps"]], "mon_t against the accumulated dt log"
    for k, s in enumerate(a["steps"]):
        ref, t = stepped_reference(lib, base, ov, p, U0, s, tEnd)
        for m, spec in enumerate(specs):
            assert_same_bits(a["vals"][m][k], ref[m], (s, spec, "against rgpu_state_maps of a lone context stepped singly"))
    if a["steps"] and a["steps"][-1] == a["nStep"]:
        for m, spec in enumerate(specs):
            assert_same_bits(a["vals"][m][-1], model(a["full"], p, spec), (spec, "the last sample against the model of the downloaded state"))
    if expect_batch is not None:
        assert a["batch"] == expect_batch(a["done"], a["ready"]), (a["batch"], a["done"], a["ready"])
    return a["done"], a["steps"], [np.array(v) for v in a["vals"]], a["batch"]


def sample_kib(lib, base, ov, samples):
    """the "map_log_kib" under which the log of run_specs on this box holds exactly `samples` samples (0: less than one)"""
    p = lib.params_from_ini(ec.ini(base), ov)
    bytes_ = 8 * sum(NQ * extent(p, a) * extent(p, b) for a, b in (("x", "y"), ("x", "z"), ("y", "z")))
    kib = -(-samples * bytes_ // 1024) if samples else bytes_ // 1024 - 1
    assert kib > 0 and kib * 1024 // bytes_ == samples, (kib, bytes_)
    return kib


def parse_maps_list(path):
    """[(step, t, map, axis, lo, hi, file)] of <prefix>_maps.txt, whose header is checked"""
    lines = open(path).read().splitlines()
    assert lines[0] == "# nStep totalTime map axis lo hi file"
    rows = [ln.split() for ln in lines[1:]]
    assert all(len(r) == 7 for r in rows)
    return [(int(r[0]), float(r[1]), int(r[2]), r[3], int(r[4]), int(r[5]), r[6]) for r in rows]


def check_driver_files(lib, run, tmp_path, base="implode3d", ov="mesh.nx=24;mesh.ny=24;mesh.nz=12", prefix="implode3d"):
    """`run(overrides)` drives the run driver.  [maps] enabled=yes every=3 map0=z:6 map1=x:all, 10 steps: the .npy files load with np.load
    and equal Solver.run_steps_mapped, <prefix>_maps.txt lists them; with enabled=no nothing is written; with [monitor] on as well the
    monitor file is byte for byte the one of a run without [maps]"""
    common = ov + ";run.nstepmax=10;run.noutput=1000;output.outputVtk=no;output.outputHdf5=no;output.outputDir=%s"
    maps = ";maps.every=3;maps.map0=z:6;maps.map1=x:all"
    for name, extra in (("maps", ";maps.enabled=yes" + maps), ("off", ";maps.enabled=no" + maps), ("both", ";maps.enabled=yes" + maps + ";monitor.enabled=yes;monitor.every=2"),
                        ("monitor", ";monitor.enabled=yes;monitor.every=2")):
        d = tmp_path / name
        d.mkdir()
        run(common % d + extra)
    assert not list((tmp_path / "off").glob("*_map*")) and not list((tmp_path / "monitor").glob("*_map*"))
    assert open(tmp_path / "both" / (prefix + "_monitor.txt"), "rb").read() == open(tmp_path / "monitor" / (prefix + "_monitor.txt"), "rb").read()
    p = lib.params_from_ini(ec.ini(base), ov)
    specs = [("z", 6, 7), ("x", 0, p.nx)]
    sv = Solver(p, lib)
    try:
        sv.start(lib.init_condition(ec.ini(base), ov, p), 0)
        done, series = sv.run_steps_mapped(10, 3, specs)
    finally:
        sv.close()
    assert done == 10 and list(series.step) == [3, 6, 9]
    for name in ("maps", "both"):
        d = tmp_path / name
        rows = parse_maps_list(d / (prefix + "_maps.txt"))
        want = [(s, t, m, specs[m][0], specs[m][1], specs[m][2], "%s_map%d_%07d.npy" % (prefix, m, s)) for s, t in zip(series.step, series.t) for m in range(2)]
        assert rows == want, (rows, want)
        assert sorted(f.name for f in d.glob("*.npy")) == sorted(r[6] for r in rows)
        for k, s in enumerate(series.step):
            for m in range(2):
                got = np.load(d / ("%s_map%d_%07d.npy" % (prefix, m, s)))
                assert got.dtype == np.dtype("<f8") and got.flags["C_CONTIGUOUS"]
                assert_same_bits(got, series.maps[m][k], (name, s, m))
