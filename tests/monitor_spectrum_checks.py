"""Checks of the spectrum monitor (rgpu_state_spectra, rgpu_run_steps_spectra; include/rgpu.h, "spectrum monitors") shared by
tests/test_monitor_spectrum_host.py (the test-only host emulation, not gpu) and tests/test_monitor_spectrum_gpu.py (-m gpu).

`model(Ch, spec, shape)` is the definition in numpy: numpy.fft.fftn of every channel of the mask, |.|^2 / N^2 binned with
numpy.bincount by the integer shell rule, which `shell_of` writes out separately from the library and from solver.spectrum_shells and
which `check_shell_rule` holds against floor(sqrt(q) + 0.5) on every shape used.  The channels are formed in numpy from the same
ghost-inclusive array: seven of the sixteen per-cell terms of monitor_planes_checks.cell_terms (imported, not copied), v = m / rho and
w = m / sqrt(rho).

Tolerance.  An FFT is backward stable in L2: if e bounds the relative L2 error of the transforms, Cauchy-Schwarz gives
|dP[s]| <= e (P[s] + 2 sqrt(P[s] Ptot)) + e^2 Ptot.  E = 1e-12 is the project's round-off gate for the contracted library (README,
DESIGN 4.1); `normalised_error` is the least e with which a result meets the bound, and `assert_within_bound` applies the bound to
every shell of every case and returns that e, so that a run with -s shows what each library reaches.  M is compared word for word."""
import ctypes as C

import numpy as np
import pytest

import ensemble_checks as ec
import monitor_maps_checks as mm
import monitor_planes_checks as mp
from ramsesgpu_amd import _capi
from ramsesgpu_amd.solver import RgpuError, Solver, spectrum_shells, spectrum_spec

E = 1e-12
NAMES = _capi.SPECTRUM_NAMES
WEIGHTS = [(1, 1, 1), (0, 1, 0), (4, 1, 4)]

initial_state = mp.initial_state
option = mm.option
batch_samples = mm.batch_samples
assert_same_bits = mm.assert_same_bits


def shape_of(p):
    return (p.nx, p.ny, p.nz)


def folded(n):
    k = np.arange(n, dtype=np.int64)
    return np.minimum(k, n - k)


def shell_of(q):
    """the integer rule: shell s is the s >= 0 with s^2 - s + 1 <= q <= s^2 + s -- searched for, no root taken"""
    q = np.asarray(q, dtype=np.int64)
    s = np.arange(int(np.sqrt(float(q.max()))) + 3, dtype=np.int64)
    top = s * s + s
    return np.searchsorted(top, q.ravel(), side="left").reshape(q.shape)   # the first s with q <= s^2 + s: then q >= (s - 1)^2 + (s - 1) + 1 = s^2 - s + 1


def shells(shape, weights):
    """[nz][ny][nx] shell of every mode, and S"""
    nx, ny, nz = shape
    wx, wy, wz = weights
    q = (wx * folded(nx))[None, None, :] ** 2 + (wy * folded(ny))[None, :, None] ** 2 + (wz * folded(nz))[:, None, None] ** 2
    corner = (wx * (nx // 2)) ** 2 + (wy * (ny // 2)) ** 2 + (wz * (nz // 2)) ** 2
    return shell_of(q), int(shell_of(np.array([corner]))[0]) + 1, q


def check_shell_rule(shape, weights):
    """the integer rule == floor(sqrt(q) + 0.5) on this shape (q is far below 2^52: the root of an edge s^2 + s + 1/4 is never met);
    solver.spectrum_shells == the bincount of it"""
    sh, S, q = shells(shape, weights)
    assert np.array_equal(sh, np.floor(np.sqrt(q.astype(np.float64)) + 0.5).astype(np.int64)), (shape, weights)
    assert sh.max() == S - 1
    M = np.bincount(sh.ravel(), minlength=S)
    S2, M2 = spectrum_shells(shape, weights)
    assert S2 == S and np.array_equal(M2, M) and int(M.sum()) == shape[0] * shape[1] * shape[2]
    return S, M


def cell_channels(U, p):
    """the thirteen channels of a ghost-inclusive 3D state over its interior: [13][nz][ny][nx]"""
    with np.errstate(all="ignore"):
        T = mp.cell_terms(U, p)
        rho, m, b = T[0], [T[1], T[2], T[3]], [T[10], T[11], T[12]]
        root = np.sqrt(rho)
        return np.array([rho] + m + [x / rho for x in m] + [x / root for x in m] + b)


def mask_of(spec):
    return spectrum_spec(spec).channels


def model(Ch, spec, shape):
    """(P, M) of spec over the channels Ch[13][nz][ny][nx]"""
    s = spectrum_spec(spec)
    sh, S, _ = shells(shape, (s.wx, s.wy, s.wz))
    N = float(shape[0] * shape[1] * shape[2])
    P = np.zeros(S)
    for ch in range(len(NAMES)):
        if s.channels >> ch & 1:
            F = np.fft.fftn(Ch[ch]) / N
            P += np.bincount(sh.ravel(), weights=(F.real ** 2 + F.imag ** 2).ravel(), minlength=S)
    return P, np.bincount(sh.ravel(), minlength=S).astype(np.float64)


def normalised_error(got, want):
    """the least e with |got - want| <= e (want + 2 sqrt(want Ptot)) + e^2 Ptot in every shell"""
    tot = float(want.sum())
    if tot == 0.0:
        return 0.0 if not np.any(got) else np.inf
    d = np.abs(got - want)
    a = want + 2.0 * np.sqrt(want * tot)
    den = a + np.sqrt(a * a + 4.0 * tot * d)   # the positive root of tot e^2 + a e - d, in its stable form; 0 / 0 where a shell holds nothing on either side
    return float(np.max(np.where(d == 0.0, 0.0, 2.0 * d / np.where(den == 0.0, 1.0, den))))


LARGEST = {}   # library path -> the largest normalised error it reached in this session


def assert_within_bound(got, want, what, lib=None):
    P, M = got
    wP, wM = want
    assert P.shape == wP.shape and M.shape == wM.shape, (what, P.shape, wP.shape)
    assert np.array_equal(M, wM), (what, "mode counts", np.argwhere(M != wM)[:5])
    tot = float(wP.sum())
    bound = E * (wP + 2.0 * np.sqrt(wP * tot)) + E * E * tot
    bad = np.argwhere(~(np.abs(P - wP) <= bound))
    e = normalised_error(P, wP)
    print("normalised error %.3e  %s" % (e, (what,)))
    if lib is not None:
        LARGEST[lib.path] = max(LARGEST.get(lib.path, 0.0), e)
    assert bad.size == 0, (what, len(bad), bad[:5].ravel(), P[bad[0][0]], wP[bad[0][0]], e)
    return e


def random_state(lib, base, ov, seed=11):
    """white noise in every channel: a ghost-inclusive state of the context's shape, density in [0.5, 1.5), momenta and faces normal"""
    p = lib.params_from_ini(ec.ini(base), ov)
    U = initial_state(lib, base, ov, p).copy()
    rng = np.random.RandomState(seed)
    U[_capi.ID] = rng.uniform(0.5, 1.5, U[_capi.ID].shape)
    for v in (_capi.IU, _capi.IV, _capi.IW):
        U[v] = rng.standard_normal(U[v].shape)
    if p.mhdEnabled:
        for v in (_capi.IA, _capi.IB, _capi.IC):
            U[v] = rng.standard_normal(U[v].shape)
    U[_capi.IP] = 10.0 + rng.uniform(0.0, 1.0, U[_capi.IP].shape)
    return p, U


# odd and even numbers of channels; one channel; the shorthands; all thirteen
CHANNEL_SETS = [("rho",), "w", "v", "b", ("rho", "mx"), ("mx", "my", "mz", "bx"), NAMES]


def check_noise(lib, base, ov):
    """white noise: every shell is populated, so the bound is nearly a relative one.  Every channel set x every weight against the
    model; Parseval against the plain sum of squares; the sum of M; four specs in one call == the same specs alone, bit for bit; a
    repeat call bit for bit"""
    p, U = random_state(lib, base, ov)
    shape = shape_of(p)
    N = shape[0] * shape[1] * shape[2]
    Ch = cell_channels(U, p)
    sv = Solver(p, lib)
    worst = 0.0
    try:
        sv.upload(U)
        for weights in WEIGHTS:
            S, M = check_shell_rule(shape, weights)
            specs = [(ch, weights) for ch in CHANNEL_SETS]
            alone = [sv.state_spectra([s], 0)[0] for s in specs]
            for s, g in zip(specs, alone):
                want = model(Ch, s, shape)
                worst = max(worst, assert_within_bound(g, want, (base, ov, s), lib))
                assert len(g[0]) == S and np.array_equal(g[1], M.astype(np.float64)) and float(g[1].sum()) == N
                mask = mask_of(s)
                squares = sum(float(np.sum(Ch[c] ** 2)) for c in range(len(NAMES)) if mask >> c & 1) / N
                assert abs(g[0].sum() - squares) <= 1e-12 * squares + 1e-300, (s, g[0].sum(), squares)   # Parseval
            for at in range(0, len(specs), 4):   # sets that share channels, together
                for (P, M2), (aP, aM) in zip(sv.state_spectra(specs[at:at + 4], 0), alone[at:at + 4]):
                    assert_same_bits(P, aP, (weights, at, "together against alone"))
                    assert_same_bits(M2, aM, (weights, at))
            again = sv.state_spectra([specs[1]], 0)[0]
            assert_same_bits(again[0], alone[1][0], "a repeat call")
    finally:
        sv.close()
    return worst


def plane_wave(shape, k, A, phase=0.0):
    nx, ny, nz = shape
    i, j, l = np.arange(nx)[None, None, :], np.arange(ny)[None, :, None], np.arange(nz)[:, None, None]
    return A * np.cos(2.0 * np.pi * (k[0] * i / nx + k[1] * j / ny + k[2] * l / nz) + phase)


def check_plane_waves(lib, base, ov):
    """density 1, mx = A cos(2 pi k.x + phase): vx = wx = mx.  The power of mx lands in the shell of k: A^2 / 2, or A^2 cos^2(phase) at
    zero and at the Nyquist points; every other shell within the bound (the model's value there is round-off)"""
    p, U = random_state(lib, base, ov)
    shape = nx, ny, nz = shape_of(p)
    gw = p.ghostWidth
    U[_capi.ID] = 1.0
    waves = [((0, 0, 0), 3, 0.0), ((1, 1, 0), 2, 0.0), ((1, 1, 1), 5, 0.7), ((nx // 2, 0, 0), 4, 0.0), ((0, ny // 2, 0), 4, 0.0), ((0, 0, nz // 2), 4, 0.0),
             ((nx // 2, ny // 2, nz // 2), 7, 0.0), ((1, -1, 0), 3, 0.3), ((-1, 1, 1), 3, 0.3), ((-1, -2, -1), 6, 1.1), ((1, 2, 1), 6, 1.1)]
    sv = Solver(p, lib)
    try:
        for k, A, phase in waves:
            U[_capi.IU] = 0.0
            U[_capi.IU, gw:gw + nz, gw:gw + ny, gw:gw + nx] = plane_wave(shape, k, A, phase)
            sv.upload(U)
            Ch = cell_channels(U, p)
            for weights in WEIGHTS:
                S, M = check_shell_rule(shape, weights)
                got = sv.state_spectra([(("mx",), weights), (("vx", "wx"), weights)], 0)
                assert_within_bound(got[0], model(Ch, (("mx",), weights), shape), (k, weights), lib)
                assert_within_bound(got[1], model(Ch, (("vx", "wx"), weights), shape), (k, weights, "vx wx"), lib)
                q = sum((w * min(abs(c) % n, n - abs(c) % n)) ** 2 for w, c, n in zip(weights, k, shape))
                s = int(shell_of(np.array([q]))[0])
                alone = all(c % n in (0, n // 2) for c, n in zip(k, shape))   # k == -k on the lattice
                power = A * A * np.cos(phase) ** 2 if alone else A * A / 2.0
                want = np.zeros(S)
                want[s] = power
                tot = power
                bound = E * (want + 2.0 * np.sqrt(want * tot)) + E * E * tot
                assert np.all(np.abs(got[0][0] - want) <= bound), (k, weights, s, got[0][0][s], power)
                assert np.all(np.abs(got[1][0] - 2.0 * want) <= 2.0 * bound), (k, weights, s, "vx wx")
    finally:
        sv.close()


def check_shell_edges():
    """k = (1, 1, 0) has q = 2, the last of shell 1; k = (1, 1, 1) has q = 3, the first of shell 2"""
    assert list(shell_of(np.array([0, 1, 2, 3, 6, 7, 12, 13]))) == [0, 1, 1, 2, 2, 3, 3, 4]


RUN_SPECS = [("w", (1, 1, 1)), ("b", (4, 1, 4)), (("rho",), (0, 1, 0))]
_STEPPED = {}   # (library path, base, ov, end time): {"sv": a lone Solver at step n, "at": {n: (spectra, t)}} -- computed once, shared, left alone


def stepped_reference(lib, base, ov, p, U0, n, tEnd=None):
    """the second lone context: stepped singly (rgpu_run_steps one at a time) to step n; returns (rgpu_state_spectra of RUN_SPECS there,
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
        ent["at"][sv.nStep] = (sv.state_spectra(RUN_SPECS), sv.totalTime)
    return ent["at"][n]


def close_references():
    for ent in _STEPPED.values():
        ent["sv"].close()
    _STEPPED.clear()


def check_run(lib, base, ov, nsteps, every, pieces=None, tEnd=None, expect_batch=None):
    """One lone context run for nsteps (in `pieces`) through rgpu_run_steps_spectra with RUN_SPECS, one through rgpu_run_steps_log:
      * the same return values, dt_log, nStep, t, dt, checksum and state, bit for bit (sampling only reads)
      * the sample steps are the multiples of `every` among the steps that ran, mon_t the accumulated dt log
      * every sample == rgpu_state_spectra of a second lone context stepped singly to that step, bit for bit
      * the last sample, when it is of the final state, against the model on the monitored context's own download, within the bound
      * the other monitors' counters stay 0; expect_batch: None, or a function (steps that ran, device-ready flag) -> the wanted
        rgpu_spectrum_batch_samples
    Returns (done, steps sampled, batch samples)."""
    p = lib.params_from_ini(ec.ini(base), ov)
    U0 = initial_state(lib, base, ov, p)
    specs = RUN_SPECS
    end = float("inf") if tEnd is None else tEnd
    runs = []
    for sampled in (True, False):
        sv = Solver(p, lib)
        try:
            sv.start(U0, 0)
            done, log, steps, ts, power, modes = 0, [], [], [], [[] for _ in specs], [[] for _ in specs]
            for n in (pieces or [nsteps]):
                if sampled:
                    d, s = sv.run_steps_spectra(n, every, specs, end)
                    steps += [int(x) for x in s.step]
                    ts += [float(x) for x in s.t]
                    for m in range(len(specs)):
                        assert s.power[m].shape[0] == len(s.step) and s.modes[m].shape == s.power[m].shape
                        power[m] += list(s.power[m])
                        modes[m] += list(s.modes[m])
                else:
                    d = sv.run_steps(n, end)
                done += d
                log += list(sv.dt_log)
            L = lib.lib
            runs.append({"done": done, "log": log, "nStep": sv.nStep, "t": sv.totalTime, "dt": sv.dt, "checksum": sv.state_checksum(sv.nStep % 2), "full": sv.getDataHost(),
                         "ready": L.rgpu_device_time_step_ready(sv.ctx, sv.nStep % 2), "batch": L.rgpu_spectrum_batch_samples(sv.ctx),
                         "other": L.rgpu_monitor_batch_samples(sv.ctx) + L.rgpu_monitor_planes_batch_samples(sv.ctx) + L.rgpu_map_batch_samples(sv.ctx) + L.rgpu_pdf_batch_samples(sv.ctx),
                         "steps": steps, "ts": ts, "power": power, "modes": modes})
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
            assert_same_bits(a["power"][m][k], ref[m][0], (s, spec, "against rgpu_state_spectra of a lone context stepped singly"))
            assert_same_bits(a["modes"][m][k], ref[m][1], (s, spec, "modes"))
    if a["steps"] and a["steps"][-1] == a["nStep"]:
        Ch = cell_channels(a["full"], p)
        for m, spec in enumerate(specs):
            assert_within_bound((a["power"][m][-1], a["modes"][m][-1]), model(Ch, spec, shape_of(p)), (base, ov, spec, "the last sample against the model"), lib)
    if expect_batch is not None:
        assert a["batch"] == expect_batch(a["done"], a["ready"]), (a["batch"], a["done"], a["ready"])
    return a["done"], a["steps"], a["batch"]


def check_refusals(L, ini, slab=True):
    """the refusals of include/rgpu.h, each with its code and the words of its message; nothing has run afterwards"""
    Spec = _capi.RgpuSpectrumSpec
    good = (Spec * 2)(Spec(0b1110000000, 1, 1, 1), Spec(1, 0, 1, 0))
    out = (C.c_double * 4096)()
    n, t, d, mn = C.c_int(0), C.c_double(0.0), C.c_double(0.0), C.c_int(7)
    ms, mt, mv = (C.c_int * 5)(), (C.c_double * 5)(), (C.c_double * (5 * 4096))()
    full = [C.byref(n), C.byref(t), C.byref(d), good, C.byref(mn), ms, mt, mv]
    err = lambda ctx: L.lib.rgpu_last_error(ctx)

    def call(ctx, nsteps, every, nspec, args):
        mn.value = 7
        a, b, c_, specs, e, f, g, h = args
        return L.lib.rgpu_run_steps_spectra(ctx, nsteps, 1e300, a, b, c_, None, every, nspec, specs, e, f, g, h)
    p2 = L.params_from_ini(ini("orszag-tang"), "mesh.nx=16;mesh.ny=16")
    sv = Solver(p2, L)
    try:
        sv.start(L.init_condition(ini("orszag-tang"), "mesh.nx=16;mesh.ny=16", p2), 0)
        assert L.lib.rgpu_state_spectra(sv.ctx, 0, 2, good, out) == -5 and b"3D" in err(sv.ctx)   # RGPU_EUNSUPPORTED
        assert call(sv.ctx, 4, 2, 2, full) == -5 and b"3D" in err(sv.ctx) and mn.value == 0 and n.value == 0
        assert L.lib.rgpu_spectrum_shells(sv.ctx, C.byref(good[0])) == 0
        with pytest.raises(RgpuError):
            sv.state_spectra([("w", (1, 1, 1))])
    finally:
        sv.close()
    for ov, name in (("mesh.nx=65;mesh.ny=16;mesh.nz=8", b"nx = 65"), ("mesh.nx=16;mesh.ny=12;mesh.nz=8", b"ny = 12"), ("mesh.nx=16;mesh.ny=16;mesh.nz=6", b"nz = 6")):
        pb = L.params_from_ini(ini("orszag-tang3d"), ov)
        sv = Solver(pb, L)
        try:
            sv.start(L.init_condition(ini("orszag-tang3d"), ov, pb), 0)
            assert L.lib.rgpu_state_spectra(sv.ctx, 0, 2, good, out) == -5 and name in err(sv.ctx), err(sv.ctx)
            assert call(sv.ctx, 4, 2, 2, full) == -5 and name in err(sv.ctx) and mn.value == 0 and n.value == 0
            assert L.lib.rgpu_spectrum_shells(sv.ctx, C.byref(good[0])) == 0
        finally:
            sv.close()
    if slab:
        ps = L.params_from_ini(ini("orszag-tang3d"), "mesh.nx=16;mesh.ny=16;mesh.nz=16", slab=(0, 2))
        sv = Solver(ps, L)
        try:
            assert L.lib.rgpu_state_spectra(sv.ctx, 0, 2, good, out) == -1                                           # RGPU_EINVAL
            assert call(sv.ctx, 4, 2, 2, full) == -1 and n.value == 0 and mn.value == 0
        finally:
            sv.close()
    ov = "mesh.nx=16;mesh.ny=8;mesh.nz=8"
    p3 = L.params_from_ini(ini("orszag-tang3d"), ov)
    sv = Solver(p3, L)
    try:
        sv.start(L.init_condition(ini("orszag-tang3d"), ov, p3), 0)
        assert L.lib.rgpu_spectrum_shells(sv.ctx, C.byref(good[0])) == 11 and L.lib.rgpu_spectrum_shells(sv.ctx, C.byref(good[1])) == 5   # q = 64 + 16 + 16 = 96 lies in shell 10 (91 .. 110); |ky| <= 4
        assert L.lib.rgpu_state_spectra(sv.ctx, 0, 2, good, None) == -1 and L.lib.rgpu_state_spectra(sv.ctx, 0, 2, None, out) == -1 and L.lib.rgpu_state_spectra(None, 0, 2, good, out) == -1
        for every in (0, -2):
            assert call(sv.ctx, 4, every, 2, full) == -1 and b"every" in err(sv.ctx) and mn.value == 0
        for hole in range(8):
            args = list(full)
            args[hole] = None
            assert call(sv.ctx, 4, 2, 2, args) == -1 and b"null pointer" in err(sv.ctx), hole
            assert mn.value == (7 if hole == 4 else 0)
        assert call(sv.ctx, -1, 2, 2, full) == -1 and mn.value == 0
        assert call(None, 4, 2, 2, full) == -1
        for nspec in (0, -1, _capi.SPECTRUM_MAX + 1):
            assert call(sv.ctx, 4, 2, nspec, full) == -1 and b"nspec" in err(sv.ctx) and mn.value == 0
            assert L.lib.rgpu_state_spectra(sv.ctx, 0, nspec, good, out) == -1 and b"nspec" in err(sv.ctx)
        # an empty mask, bits beyond the channels, a weight outside 0 .. 64, all weights zero, more than 4096 shells (64 x 8 = 512 per axis is within)
        bad_specs = [(Spec(0, 1, 1, 1), b"mask"), (Spec(1 << 13, 1, 1, 1), b"mask"), (Spec(0xffffffff, 1, 1, 1), b"mask"), (Spec(1, -1, 1, 1), b"wx"), (Spec(1, 1, 65, 1), b"wy"),
                     (Spec(1, 1, 1, 1000), b"wz"), (Spec(1, 0, 0, 0), b"zero")]
        for bad, word in bad_specs:
            for where in (0, 1):
                specs = (Spec * 2)(good[0], good[0])
                specs[where] = bad
                args = list(full)
                args[3] = specs
                what = (bad.channels, bad.wx, bad.wy, bad.wz, where)
                assert call(sv.ctx, 4, 2, 2, args) == -1 and b"spectrum %d:" % where in err(sv.ctx) and word in err(sv.ctx) and mn.value == 0, (what, err(sv.ctx))
                assert L.lib.rgpu_state_spectra(sv.ctx, 0, 2, specs, out) == -1 and b"spectrum %d:" % where in err(sv.ctx), what
                assert L.lib.rgpu_spectrum_shells(sv.ctx, C.byref(bad)) == 0, what
        assert n.value == 0 and t.value == 0.0 and L.lib.rgpu_spectrum_batch_samples(sv.ctx) == 0 and not any(out) and not any(mv)   # nothing ran
        W = 2 * (11 + 5)
        assert call(sv.ctx, 4, 2, 2, full) == 4 and n.value == 4 and mn.value == 2 and list(ms)[:2] == [2, 4]
        assert sum(mv[11:22]) == 16 * 8 * 8 and sum(mv[W + 11:W + 22]) == 16 * 8 * 8 and sum(mv[W + 27:W + 32]) == 16 * 8 * 8
        assert call(sv.ctx, 0, 2, 2, full) == 0 and mn.value == 0
    finally:
        sv.close()
    # more than 4096 shells: 1024 cells along x with weight 8 (no box of the suite is that long in three directions: one will do)
    ov = "mesh.nx=1024;mesh.ny=4;mesh.nz=4"
    pl = L.params_from_ini(ini("orszag-tang3d"), ov)
    sv = Solver(pl, L)
    try:
        sv.start(L.init_condition(ini("orszag-tang3d"), ov, pl), 0)
        many = (Spec * 2)(good[0], Spec(1, 9, 1, 1))
        assert L.lib.rgpu_spectrum_shells(sv.ctx, C.byref(many[1])) == 0 and L.lib.rgpu_spectrum_shells(sv.ctx, C.byref(Spec(1, 7, 1, 1))) == 3585
        assert L.lib.rgpu_state_spectra(sv.ctx, 0, 2, many, out) == -1 and b"spectrum 1:" in err(sv.ctx) and b"shells" in err(sv.ctx)
        args = list(full)
        args[3] = many
        assert call(sv.ctx, 4, 2, 2, args) == -1 and b"spectrum 1:" in err(sv.ctx) and mn.value == 0 and n.value == 4
    finally:
        sv.close()
    assert L.lib.rgpu_spectrum_batch_samples(None) == 0


def parse_spectra_list(path):
    """[(step, t, spectrum, spec, file)] of <prefix>_spectra.txt, whose header is checked"""
    lines = open(path).read().splitlines()
    assert lines[0] == "# nStep totalTime spectrum spec file"
    rows = [ln.split() for ln in lines[1:]]
    assert all(len(r) == 5 for r in rows)
    return [(int(r[0]), float(r[1]), int(r[2]), r[3], r[4]) for r in rows]


def check_driver_files(lib, run, tmp_path, base="implode3d", ov="mesh.nx=32;mesh.ny=16;mesh.nz=8", prefix="implode3d"):
    """`run(overrides)` drives the run driver.  [spectra] enabled=yes every=3 with two specs, 10 steps: the .npy files load with np.load,
    are shaped [2, S] and equal Solver.run_steps_spectra bit for bit, <prefix>_spectra.txt lists them; with enabled=no nothing is
    written; with [monitor] on as well the monitor file is byte for byte the one of a run without [spectra]; with [pdfs] on as well the
    PDFs take the batches and the spectra are the same doubles"""
    common = ov + ";run.nstepmax=10;run.noutput=1000;output.outputVtk=no;output.outputHdf5=no;output.outputDir=%s"
    texts = ["w 1 1 1", "rho,mx 0 1 0"]
    spectra = ";spectra.every=3;spectra.spectrum0=%s;spectra.spectrum1=%s" % tuple(texts)
    for name, extra in (("spectra", ";spectra.enabled=yes" + spectra), ("off", ";spectra.enabled=no" + spectra), ("both", ";spectra.enabled=yes" + spectra + ";monitor.enabled=yes;monitor.every=2"),
                        ("monitor", ";monitor.enabled=yes;monitor.every=2"), ("pdfs", ";spectra.enabled=yes" + spectra + ";pdfs.enabled=yes;pdfs.every=2;pdfs.pdf0=rho:lin:0:2:8")):
        d = tmp_path / name
        d.mkdir()
        run(common % d + extra)
    assert not list((tmp_path / "off").glob("*_spectr*")) and not list((tmp_path / "monitor").glob("*_spectr*"))
    assert open(tmp_path / "both" / (prefix + "_monitor.txt"), "rb").read() == open(tmp_path / "monitor" / (prefix + "_monitor.txt"), "rb").read()
    p = lib.params_from_ini(ec.ini(base), ov)
    specs = [("w", (1, 1, 1)), (("rho", "mx"), (0, 1, 0))]
    sv = Solver(p, lib)
    try:
        sv.start(lib.init_condition(ec.ini(base), ov, p), 0)
        done, series = sv.run_steps_spectra(10, 3, specs)
    finally:
        sv.close()
    assert done == 10 and list(series.step) == [3, 6, 9]
    for name in ("spectra", "both", "pdfs"):
        d = tmp_path / name
        rows = parse_spectra_list(d / (prefix + "_spectra.txt"))
        want = [(s, t, m, texts[m].replace(" ", ":"), "%s_spectrum%d_%07d.npy" % (prefix, m, s)) for s, t in zip(series.step, series.t) for m in range(2)]
        assert rows == want, (rows, want)
        assert sorted(f.name for f in d.glob("*_spectrum*.npy")) == sorted(r[4] for r in rows)
        for k, s in enumerate(series.step):
            for m in range(2):
                got = np.load(d / ("%s_spectrum%d_%07d.npy" % (prefix, m, s)))
                assert got.dtype == np.dtype("<f8") and got.flags["C_CONTIGUOUS"] and got.shape == (2, series.power[m].shape[1])
                assert_same_bits(got[0], series.power[m][k], (name, s, m))
                assert_same_bits(got[1], series.modes[m][k], (name, s, m, "modes"))
