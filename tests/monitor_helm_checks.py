"""Checks of the Helmholtz spectra (rgpu_state_helm_spectra, rgpu_run_steps_helm_spectra; include/rgpu.h, "Helmholtz spectra") shared
by tests/test_monitor_helm_host.py (the test-only host emulation, not gpu) and tests/test_monitor_helm_gpu.py (-m gpu).

`model(Ch, spec, shape)` is the definition in numpy: numpy.fft.fftn of the three channels of the field, the per-mode formulas of the
header with the signed folded wave numbers (the Nyquist index is -n / 2), numpy.bincount by the integer shell rule of
tests/monitor_spectrum_checks.py (imported, not copied).  The channels are that module's cell_channels.

Tolerance: the backward-error bound of the spectrum monitor, for each of Psol and Pcomp in every shell,
|dP_c[s]| <= e (P_c[s] + 2 sqrt(P_c[s] Ptot)) + e^2 Ptot with e = E = 1e-12 and Ptot = sum_s (Psol + Pcomp) of the model.  It carries
over because both projections are contractions of u^: an error of relative L2 size e in the transforms is one of at most that size
in kappa x u^ / |kappa| and in kappa . u^ / |kappa|, and Cauchy-Schwarz does the rest.  `assert_within_gate` applies it and returns
the least e the result needs; LARGEST keeps the largest per library.  M is compared word for word."""
import ctypes as C

import numpy as np
import pytest

import ensemble_checks as ec
import forcing_clock_checks as fc
import monitor_spectrum_checks as ms
from ramsesgpu_amd import _capi
from ramsesgpu_amd.solver import RgpuError, Solver, helm_spec

E = ms.E
FIELDS = _capi.HELM_NAMES
WEIGHTS = [(1, 1, 1), (4, 1, 4), (3, 5, 7)]
LARGEST = {}   # library path -> the largest normalised error it reached in this session

assert_same_bits = ms.assert_same_bits
shape_of = ms.shape_of


def signed(n):
    k = np.arange(n, dtype=np.int64)
    return np.where(k < n // 2, k, k - n)


def kappa(shape, weights):
    """the weighted signed wave vector of every mode, three float arrays that broadcast to [nz][ny][nx]"""
    nx, ny, nz = shape
    wx, wy, wz = weights
    return ((wx * signed(nx))[None, None, :].astype(np.float64), (wy * signed(ny))[None, :, None].astype(np.float64), (wz * signed(nz))[:, None, None].astype(np.float64))


def split_modes(F, shape, weights):
    """(T, L) per mode of the transforms F[3][nz][ny][nx]"""
    kx, ky, kz = kappa(shape, weights)
    q = kx * kx + ky * ky + kz * kz
    d = (kx * F[0] + ky * F[1]) + kz * F[2]
    cx, cy, cz = ky * F[2] - kz * F[1], kz * F[0] - kx * F[2], kx * F[1] - ky * F[0]
    ab2 = lambda z: z.real ** 2 + z.imag ** 2
    qq = np.where(q == 0, 1.0, q)
    L = np.where(q == 0, 0.0, ab2(d) / qq)
    T = np.where(q == 0, (ab2(F[0]) + ab2(F[1])) + ab2(F[2]), ((ab2(cx) + ab2(cy)) + ab2(cz)) / qq)
    return T, L


def triple(spec):
    s = helm_spec(spec)
    return [1 + 3 * s.field + a for a in range(3)], (s.wx, s.wy, s.wz)


def model(Ch, spec, shape):
    """(Psol, Pcomp, M) of spec over the channels Ch[13][nz][ny][nx]"""
    chans, weights = triple(spec)
    sh, S, _ = ms.shells(shape, weights)
    N = float(shape[0] * shape[1] * shape[2])
    T, L = split_modes([np.fft.fftn(Ch[c]) / N for c in chans], shape, weights)
    return (np.bincount(sh.ravel(), weights=T.ravel(), minlength=S), np.bincount(sh.ravel(), weights=L.ravel(), minlength=S),
            np.bincount(sh.ravel(), minlength=S).astype(np.float64))


def needed_e(got, want, tot):
    """the least e with |got - want| <= e (want + 2 sqrt(want tot)) + e^2 tot in every shell"""
    if tot == 0.0:
        return 0.0 if not np.any(got) else np.inf
    d = np.abs(got - want)
    a = want + 2.0 * np.sqrt(want * tot)
    den = a + np.sqrt(a * a + 4.0 * tot * d)
    return float(np.max(np.where(d == 0.0, 0.0, 2.0 * d / np.where(den == 0.0, 1.0, den))))


def assert_within_gate(got, want, what, lib=None):
    assert len(got) == 3 and all(g.shape == w.shape for g, w in zip(got, want)), (what, [g.shape for g in got], [w.shape for w in want])
    assert np.array_equal(got[2], want[2]), (what, "mode counts", np.argwhere(got[2] != want[2])[:5])
    tot = float(want[0].sum() + want[1].sum())
    worst = 0.0
    for part, P, wP in (("solenoidal", got[0], want[0]), ("compressive", got[1], want[1])):
        bound = E * (wP + 2.0 * np.sqrt(wP * tot)) + E * E * tot
        e = needed_e(P, wP, tot)
        print("normalised error %.3e  %s" % (e, (what, part)))
        worst = max(worst, e)
        if lib is not None:
            LARGEST[lib.path] = max(LARGEST.get(lib.path, 0.0), e)
        bad = np.argwhere(~(np.abs(P - wP) <= bound))
        assert bad.size == 0, (what, part, len(bad), bad[:5].ravel(), P[bad[0][0]], wP[bad[0][0]], e)
    return worst


def check_noise(lib, base, ov, weight_sets=WEIGHTS):
    """white noise: every field x every weight set against the model within the gate; Parseval; Psol + Pcomp against P of
    rgpu_state_spectra for the same channels within twice the bound; M word for word; the four fields in one call == each alone, bit
    for bit; a repeat call bit for bit.  A hydro state: the b spectra are exactly +0.0"""
    p, U = ms.random_state(lib, base, ov)
    shape = shape_of(p)
    N = shape[0] * shape[1] * shape[2]
    Ch = ms.cell_channels(U, p)
    sv = Solver(p, lib)
    try:
        sv.upload(U)
        for weights in weight_sets:
            S, M = ms.check_shell_rule(shape, weights)
            specs = [(f, weights) for f in FIELDS]
            alone = [sv.state_helm_spectra([s], 0)[0] for s in specs]
            try:
                plain = sv.state_spectra(specs, 0)
            except RgpuError as e:   # the spectrum monitor has no cap on its binning workgroups: on 4 x 1024 x 4 it refuses (3, 5, 7)
                assert "scratch" in str(e), e
                plain = [None] * len(specs)
            for s, g, other in zip(specs, alone, plain):
                want = model(Ch, s, shape)
                assert_within_gate(g, want, (base, ov, s), lib)
                assert len(g[0]) == S and np.array_equal(g[2], M.astype(np.float64)) and float(g[2].sum()) == N
                squares = sum(float(np.sum(Ch[c] ** 2)) for c in triple(s)[0]) / N
                assert abs((g[0].sum() + g[1].sum()) - squares) <= 1e-12 * squares + 1e-300, (s, g[0].sum(), g[1].sum(), squares)   # Parseval
                tot = float(want[0].sum() + want[1].sum())
                wP = want[0] + want[1]
                if other is not None:
                    assert_same_bits(g[2], other[1], (s, "M against rgpu_state_spectra"))
                    assert np.all(np.abs((g[0] + g[1]) - other[0]) <= 2.0 * (E * (wP + 2.0 * np.sqrt(wP * tot)) + E * E * tot)), (s, "Psol + Pcomp against P")
                if s[0] == "b" and not p.mhdEnabled:
                    assert not np.any(g[0]) and not np.any(g[1]) and not np.any(np.signbit(g[0])) and not np.any(np.signbit(g[1])), (s, "a hydro state has no b")
            for got, want in zip(sv.state_helm_spectra(specs, 0), alone):
                for a, b in zip(got, want):
                    assert_same_bits(a, b, (weights, "together against alone"))
            for a, b in zip(sv.state_helm_spectra([specs[2]], 0)[0], alone[2]):
                assert_same_bits(a, b, "a repeat call")
    finally:
        sv.close()


def put_momentum(U, p, m):
    """rho = 1 and the momentum m[3][nz][ny][nx] over the interior of a ghost-inclusive state"""
    gw, (nx, ny, nz) = p.ghostWidth, shape_of(p)
    U[_capi.ID] = 1.0
    for a, v in enumerate((_capi.IU, _capi.IV, _capi.IW)):
        U[v] = 0.0
        U[v, gw:gw + nz, gw:gw + ny, gw:gw + nx] = m[a]


def pure_field(shape, weights, part, seed=5):
    """a noise field [3][nz][ny][nx] projected in numpy onto its solenoidal or its compressive part with the kappa of the weights, the
    Nyquist planes and the mean zeroed (there kappa(-k) = -kappa(k) fails or kappa vanishes, and the field would not stay real)"""
    nx, ny, nz = shape
    F = np.array([np.fft.fftn(a) for a in np.random.RandomState(seed).standard_normal((3, nz, ny, nx))])
    F[:, nz // 2, :, :] = 0.0
    F[:, :, ny // 2, :] = 0.0
    F[:, :, :, nx // 2] = 0.0
    F[:, 0, 0, 0] = 0.0
    k = kappa(shape, weights)
    q = k[0] * k[0] + k[1] * k[1] + k[2] * k[2]
    along = (k[0] * F[0] + k[1] * F[1] + k[2] * F[2]) / np.where(q == 0, 1.0, q)
    comp = np.array([k[a] * along for a in range(3)])
    G = comp if part == "compressive" else F - comp
    out = np.array([np.fft.ifftn(G[a]) for a in range(3)])
    assert np.max(np.abs(out.imag)) <= 1e-12 * np.max(np.abs(out.real))
    return np.ascontiguousarray(out.real)


def check_pure_fields(lib, base, ov, weight_sets=WEIGHTS):
    """m purely solenoidal, then purely compressive: the wrong part holds at most e^2 Ptot in every shell -- the model alone leaves
    1e-32 .. 5e-32 of Ptot there, and a sign or axis error in the projection tens of percent -- and the right part meets the gate"""
    p, U = ms.random_state(lib, base, ov)
    shape = shape_of(p)
    sv = Solver(p, lib)
    try:
        for weights in weight_sets:
            for part in ("solenoidal", "compressive"):
                put_momentum(U, p, pure_field(shape, weights, part))
                sv.upload(U)
                spec = ("m", weights)
                want = model(ms.cell_channels(U, p), spec, shape)
                got = sv.state_helm_spectra([spec], 0)[0]
                tot = float(want[0].sum() + want[1].sum())
                wrong = got[1] if part == "solenoidal" else got[0]
                print("pure %s field %s %s: wrong part / Ptot = %.3e (model %.3e)" % (part, ov, weights, wrong.max() / tot, (want[1] if part == "solenoidal" else want[0]).max() / tot))
                assert tot > 0 and np.all(wrong <= E * E * tot), (ov, weights, part, float(wrong.max() / tot))
                assert_within_gate(got, want, (ov, weights, part), lib)
    finally:
        sv.close()


def check_plane_waves(lib, base, ov):
    """single waves of the momentum at density 1 (needs nx >= 8).  x^ sin(2 pi 3 i / nx): longitudinal, Pcomp[3 wx] = 0.5 and nothing
    else; y^ sin(same): transverse, Psol[3 wx] = 0.5 and nothing else; (1, 1, 0) cos(2 pi (2 i / nx + j / ny)), total power 1: all of it
    compressive with weights (1, 2, 1) (kappa = (2, 2, 0)), 0.9 of it with (1, 1, 1) (kappa = (2, 1, 0): 9 / (5 x 2)) -- the weights
    steer the direction, not only the shell.  Each also against the model within the gate"""
    p, U = ms.random_state(lib, base, ov)
    shape = nx, ny, nz = shape_of(p)
    assert nx >= 8
    zero = np.zeros((nz, ny, nx))
    sine = ms.plane_wave(shape, (3, 0, 0), 1.0, -np.pi / 2)   # cos(a - pi / 2) = sin(a)
    oblique = ms.plane_wave(shape, (2, 1, 0), 1.0)
    cases = [("x^ sin", [sine, zero, zero], w, 9 * w[0] * w[0], 0.0, 0.5) for w in WEIGHTS] + [("y^ sin", [zero, sine, zero], w, 9 * w[0] * w[0], 0.5, 0.0) for w in WEIGHTS] + \
        [("oblique", [oblique, oblique, zero], (1, 2, 1), 8, 0.0, 1.0), ("oblique", [oblique, oblique, zero], (1, 1, 1), 5, 0.1, 0.9)]
    sv = Solver(p, lib)
    try:
        for name, m, weights, q, sol, comp in cases:
            put_momentum(U, p, m)
            sv.upload(U)
            S, M = ms.check_shell_rule(shape, weights)
            got = sv.state_helm_spectra([("m", weights)], 0)[0]
            assert_within_gate(got, model(ms.cell_channels(U, p), ("m", weights), shape), (name, weights), lib)
            s = int(ms.shell_of(np.array([q]))[0])
            tot = sol + comp
            for P, power in ((got[0], sol), (got[1], comp)):
                want = np.zeros(S)
                want[s] = power
                assert np.all(np.abs(P - want) <= E * (want + 2.0 * np.sqrt(want * tot)) + E * E * tot), (name, weights, s, P[s], power)
    finally:
        sv.close()


RUN_SPECS = [("w", (1, 1, 1)), ("b", (4, 1, 4)), ("v", (3, 5, 7))]
_STEPPED = {}   # (library path, base, ov, end time): {"sv": a lone Solver at step n, "at": {n: (spectra, t)}} -- computed once, shared, left alone


def stepped_reference(lib, base, ov, p, U0, n, tEnd=None):
    """the second lone context: stepped singly to step n; returns (rgpu_state_helm_spectra of RUN_SPECS there, its time)"""
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
        ent["at"][sv.nStep] = (sv.state_helm_spectra(RUN_SPECS), sv.totalTime)
    return ent["at"][n]


def close_references():
    for ent in _STEPPED.values():
        ent["sv"].close()
    _STEPPED.clear()


def counters(L, ctx):
    return (L.rgpu_monitor_batch_samples(ctx) + L.rgpu_monitor_planes_batch_samples(ctx) + L.rgpu_map_batch_samples(ctx) + L.rgpu_pdf_batch_samples(ctx) +
            L.rgpu_spectrum_batch_samples(ctx))


def check_run(lib, base, ov, nsteps, every, pieces=None, expect_batch=None):
    """monitor_spectrum_checks.check_run for rgpu_run_steps_helm_spectra: sampling changes neither the run nor the state; the sample steps
    are the multiples of `every`, mon_t the accumulated dt log; every sample == rgpu_state_helm_spectra of a second lone context
    stepped singly to that step, bit for bit; the last sample, when it is of the final state, against the model on the download; the
    other five counters stay 0.  Returns (done, steps sampled, batch samples)."""
    p = lib.params_from_ini(ec.ini(base), ov)
    U0 = ms.initial_state(lib, base, ov, p)
    specs = RUN_SPECS
    runs = []
    for sampled in (True, False):
        sv = Solver(p, lib)
        try:
            sv.start(U0, 0)
            done, log, steps, ts, parts = 0, [], [], [], [[[] for _ in specs] for _ in range(3)]
            for n in (pieces or [nsteps]):
                if sampled:
                    d, s = sv.run_steps_helm_spectra(n, every, specs)
                    steps += [int(x) for x in s.step]
                    ts += [float(x) for x in s.t]
                    for i, series in enumerate((s.solenoidal, s.compressive, s.modes)):
                        for m in range(len(specs)):
                            assert series[m].shape[0] == len(s.step)
                            parts[i][m] += list(series[m])
                else:
                    d = sv.run_steps(n)
                done += d
                log += list(sv.dt_log)
            L = lib.lib
            runs.append({"done": done, "log": log, "nStep": sv.nStep, "t": sv.totalTime, "dt": sv.dt, "checksum": sv.state_checksum(sv.nStep % 2), "full": sv.getDataHost(),
                         "ready": L.rgpu_device_time_step_ready(sv.ctx, sv.nStep % 2), "batch": L.rgpu_helm_batch_samples(sv.ctx), "other": counters(L, sv.ctx),
                         "steps": steps, "ts": ts, "parts": parts})
        finally:
            sv.close()
    a, b = runs
    assert (a["done"], a["nStep"], a["t"], a["dt"], a["checksum"], a["log"]) == (b["done"], b["nStep"], b["t"], b["dt"], b["checksum"], b["log"]), "sampling changed the run"
    assert np.array_equal(a["full"], b["full"], equal_nan=True), "sampling changed the state"
    assert b["batch"] == 0 and a["other"] == 0 and b["other"] == 0
    assert a["steps"] == [s for s in range(1, a["done"] + 1) if s % every == 0], (a["steps"], a["done"])
    assert a["ts"] == [ec.time_of(a["log"][:s]) for s in a["steps"]], "mon_t against the accumulated dt log"
    for k, s in enumerate(a["steps"]):
        ref, t = stepped_reference(lib, base, ov, p, U0, s)
        for m, spec in enumerate(specs):
            for i in range(3):
                assert_same_bits(a["parts"][i][m][k], ref[m][i], (s, spec, i, "against rgpu_state_helm_spectra of a lone context stepped singly"))
    if a["steps"] and a["steps"][-1] == a["nStep"]:
        Ch = ms.cell_channels(a["full"], p)
        for m, spec in enumerate(specs):
            assert_within_gate(tuple(a["parts"][i][m][-1] for i in range(3)), model(Ch, spec, shape_of(p)), (base, ov, spec, "the last sample against the model"), lib)
    if expect_batch is not None:
        assert a["batch"] == expect_batch(a["done"], a["ready"]), (a["batch"], a["done"], a["ready"])
    return a["done"], a["steps"], a["batch"], a


def check_cut_run(lib, base, ov):
    """a run cut into two calls gives the series of one call"""
    one = check_run(lib, base, ov, 10, 3)[3]
    two = check_run(lib, base, ov, 10, 3, pieces=[4, 6])[3]
    assert one["steps"] == two["steps"] == [3, 6, 9] and one["ts"] == two["ts"]
    for i in range(3):
        for m in range(len(RUN_SPECS)):
            for x, y in zip(one["parts"][i][m], two["parts"][i][m]):
                assert_same_bits(x, y, ("cut run", i, m))


def check_driven(lib, nsteps=6, every=3):
    """turbulence_hydro_ou at 16^3 from rest, ksi = 1 and ksi = 0, sampled inside the device-clock batches: the library against the
    model on the downloaded state within the gate, and the compressive fraction sum Pcomp / sum P of v larger for ksi = 0 than for
    ksi = 1 -- the ordering only.  Measured on the host emulation: 0.998688 (ksi = 1) and 0.998703 (ksi = 0): the process of this code
    (ou_forcing.h, a quirk kept from the reference: the identity term of its projection tensor is zero) kicks along k for every ksi,
    so both runs are compressive and ksi moves the fraction by 1.5e-5 only.  Returns the fractions (ksi = 1, ksi = 0)"""
    frac = []
    for ksi in (1, 0):
        s = fc.setup(lib, ("turbulence_hydro_ou", "mesh.nx=16;mesh.ny=16;mesh.nz=16;" + fc.PERT_OU, False), "turbulence-Ornstein-Uhlenbeck.ksi=%d" % ksi)
        with fc.option(lib, "forcing_clock", 1):
            sv = fc.fresh(lib, s)
            try:
                done, series = sv.run_steps_helm_spectra(nsteps, every, [("v", (1, 1, 1)), ("w", (1, 1, 1))])
                assert done == nsteps and list(series.step) == list(range(every, nsteps + 1, every))
                assert lib.lib.rgpu_helm_batch_samples(sv.ctx) == len(series.step) and sv.forcing_batch_steps() == nsteps, "the forced steps and their samples ran inside the batches"
                Ch = ms.cell_channels(sv.getDataHost(), s.p)
                for m, spec in enumerate([("v", (1, 1, 1)), ("w", (1, 1, 1))]):
                    got = (series.solenoidal[m][-1], series.compressive[m][-1], series.modes[m][-1])
                    assert_within_gate(got, model(Ch, spec, shape_of(s.p)), ("ksi = %d" % ksi, spec), lib)
                frac.append(float(series.compressive[0][-1].sum() / (series.compressive[0][-1].sum() + series.solenoidal[0][-1].sum())))
            finally:
                sv.close()
    print("compressive fraction of v after %d steps: ksi = 1: %.6f, ksi = 0: %.6f  (%s)" % (nsteps, frac[0], frac[1], lib.arithmetic))
    assert frac[1] > frac[0], frac
    return frac


def check_refusals(L, ini, slab=True):
    """the refusals of the spectrum monitors, plus a zero weight and a field outside 0 .. 3; nothing has run afterwards"""
    Spec = _capi.RgpuHelmSpec
    good = (Spec * 2)(Spec(2, 1, 1, 1), Spec(0, 4, 1, 4))
    out = (C.c_double * 8192)()
    n, t, d, mn = C.c_int(0), C.c_double(0.0), C.c_double(0.0), C.c_int(7)
    ms_, mt, mv = (C.c_int * 5)(), (C.c_double * 5)(), (C.c_double * (5 * 8192))()
    full = [C.byref(n), C.byref(t), C.byref(d), good, C.byref(mn), ms_, mt, mv]
    err = lambda ctx: L.lib.rgpu_last_error(ctx)

    def call(ctx, nsteps, every, nspec, args):
        mn.value = 7
        a, b, c_, specs, e, f, g, h = args
        return L.lib.rgpu_run_steps_helm_spectra(ctx, nsteps, 1e300, a, b, c_, None, every, nspec, specs, e, f, g, h)
    p2 = L.params_from_ini(ini("orszag-tang"), "mesh.nx=16;mesh.ny=16")
    sv = Solver(p2, L)
    try:
        sv.start(L.init_condition(ini("orszag-tang"), "mesh.nx=16;mesh.ny=16", p2), 0)
        assert L.lib.rgpu_state_helm_spectra(sv.ctx, 0, 2, good, out) == -5 and b"3D" in err(sv.ctx)   # RGPU_EUNSUPPORTED
        assert call(sv.ctx, 4, 2, 2, full) == -5 and b"3D" in err(sv.ctx) and mn.value == 0 and n.value == 0
        assert L.lib.rgpu_helm_shells(sv.ctx, C.byref(good[0])) == 0
        with pytest.raises(RgpuError):
            sv.state_helm_spectra([("w", (1, 1, 1))])
    finally:
        sv.close()
    for ov, name in (("mesh.nx=65;mesh.ny=16;mesh.nz=8", b"nx = 65"), ("mesh.nx=16;mesh.ny=12;mesh.nz=8", b"ny = 12"), ("mesh.nx=16;mesh.ny=16;mesh.nz=6", b"nz = 6")):
        pb = L.params_from_ini(ini("orszag-tang3d"), ov)
        sv = Solver(pb, L)
        try:
            sv.start(L.init_condition(ini("orszag-tang3d"), ov, pb), 0)
            assert L.lib.rgpu_state_helm_spectra(sv.ctx, 0, 2, good, out) == -5 and name in err(sv.ctx), err(sv.ctx)
            assert call(sv.ctx, 4, 2, 2, full) == -5 and name in err(sv.ctx) and mn.value == 0 and n.value == 0
            assert L.lib.rgpu_helm_shells(sv.ctx, C.byref(good[0])) == 0
        finally:
            sv.close()
    if slab:
        ps = L.params_from_ini(ini("orszag-tang3d"), "mesh.nx=16;mesh.ny=16;mesh.nz=16", slab=(0, 2))
        sv = Solver(ps, L)
        try:
            assert L.lib.rgpu_state_helm_spectra(sv.ctx, 0, 2, good, out) == -1                                      # RGPU_EINVAL
            assert call(sv.ctx, 4, 2, 2, full) == -1 and n.value == 0 and mn.value == 0
        finally:
            sv.close()
    ov = "mesh.nx=16;mesh.ny=8;mesh.nz=8"
    p3 = L.params_from_ini(ini("orszag-tang3d"), ov)
    sv = Solver(p3, L)
    try:
        sv.start(L.init_condition(ini("orszag-tang3d"), ov, p3), 0)
        assert L.lib.rgpu_helm_shells(sv.ctx, C.byref(good[0])) == 11 and L.lib.rgpu_helm_shells(sv.ctx, C.byref(good[1])) == 37   # q = 96: shell 10; q = 1024 + 16 + 256 = 1296 = 36^2
        assert L.lib.rgpu_state_helm_spectra(sv.ctx, 0, 2, good, None) == -1 and L.lib.rgpu_state_helm_spectra(sv.ctx, 0, 2, None, out) == -1 and L.lib.rgpu_state_helm_spectra(None, 0, 2, good, out) == -1
        for every in (0, -2):
            assert call(sv.ctx, 4, every, 2, full) == -1 and b"every" in err(sv.ctx) and mn.value == 0
        for hole in range(8):
            args = list(full)
            args[hole] = None
            assert call(sv.ctx, 4, 2, 2, args) == -1 and b"null pointer" in err(sv.ctx), hole
            assert mn.value == (7 if hole == 4 else 0)
        assert call(sv.ctx, -1, 2, 2, full) == -1 and mn.value == 0
        assert call(None, 4, 2, 2, full) == -1
        for nspec in (0, -1, _capi.HELM_MAX + 1):
            assert call(sv.ctx, 4, 2, nspec, full) == -1 and b"nspec" in err(sv.ctx) and mn.value == 0
            assert L.lib.rgpu_state_helm_spectra(sv.ctx, 0, nspec, good, out) == -1 and b"nspec" in err(sv.ctx)
        # a field outside 0 .. 3, a zero weight on each axis, a weight outside 1 .. 64
        bad_specs = [(Spec(-1, 1, 1, 1), b"field"), (Spec(4, 1, 1, 1), b"field"), (Spec(2, 0, 1, 1), b"zero"), (Spec(2, 1, 0, 1), b"zero"), (Spec(2, 1, 1, 0), b"zero"),
                     (Spec(2, 0, 0, 0), b"zero"), (Spec(2, -1, 1, 1), b"wx"), (Spec(2, 1, 65, 1), b"wy"), (Spec(2, 1, 1, 1000), b"wz")]
        for bad, word in bad_specs:
            for where in (0, 1):
                specs = (Spec * 2)(good[0], good[0])
                specs[where] = bad
                args = list(full)
                args[3] = specs
                what = (bad.field, bad.wx, bad.wy, bad.wz, where)
                assert call(sv.ctx, 4, 2, 2, args) == -1 and b"spectrum %d:" % where in err(sv.ctx) and word in err(sv.ctx) and mn.value == 0, (what, err(sv.ctx))
                assert L.lib.rgpu_state_helm_spectra(sv.ctx, 0, 2, specs, out) == -1 and b"spectrum %d:" % where in err(sv.ctx), what
                assert L.lib.rgpu_helm_shells(sv.ctx, C.byref(bad)) == 0, what
        assert n.value == 0 and t.value == 0.0 and L.lib.rgpu_helm_batch_samples(sv.ctx) == 0 and not any(out) and not any(mv)   # nothing ran
        W = 3 * (11 + 37)
        assert call(sv.ctx, 4, 2, 2, full) == 4 and n.value == 4 and mn.value == 2 and list(ms_)[:2] == [2, 4]
        assert sum(mv[22:33]) == 16 * 8 * 8 and sum(mv[W + 22:W + 33]) == 16 * 8 * 8 and sum(mv[W + 33 + 74:W + 33 + 111]) == 16 * 8 * 8
        assert call(sv.ctx, 0, 2, 2, full) == 0 and mn.value == 0
        assert counters(L.lib, sv.ctx) == 0
    finally:
        sv.close()
    ov = "mesh.nx=1024;mesh.ny=4;mesh.nz=4"
    pl = L.params_from_ini(ini("orszag-tang3d"), ov)
    sv = Solver(pl, L)
    try:
        sv.start(L.init_condition(ini("orszag-tang3d"), ov, pl), 0)
        many = (Spec * 2)(good[0], Spec(2, 9, 1, 1))
        assert L.lib.rgpu_helm_shells(sv.ctx, C.byref(many[1])) == 0 and L.lib.rgpu_helm_shells(sv.ctx, C.byref(Spec(2, 7, 1, 1))) == 3585
        assert L.lib.rgpu_state_helm_spectra(sv.ctx, 0, 2, many, out) == -1 and b"spectrum 1:" in err(sv.ctx) and b"shells" in err(sv.ctx)
    finally:
        sv.close()
    assert L.lib.rgpu_helm_batch_samples(None) == 0


def check_driver_files(lib, run, tmp_path, base="implode3d", ov="mesh.nx=32;mesh.ny=16;mesh.nz=8", prefix="implode3d"):
    """`run(overrides)` drives the run driver.  [helmholtz] enabled=yes every=3 with two specs, 10 steps: the .npy files load with np.load,
    are shaped [3, S] and equal Solver.run_steps_helm_spectra bit for bit, <prefix>_helmholtz.txt lists them; with enabled=no nothing is
    written; with [spectra] on as well the spectra take the batches and both sets of files hold the same doubles as alone"""
    common = ov + ";run.nstepmax=10;run.noutput=1000;output.outputVtk=no;output.outputHdf5=no;output.outputDir=%s"
    texts = ["w 1 1 1", "m 4 1 4"]
    helm = ";helmholtz.every=3;helmholtz.spectrum0=%s;helmholtz.spectrum1=%s" % tuple(texts)
    for name, extra in (("helm", ";helmholtz.enabled=yes" + helm), ("off", ";helmholtz.enabled=no" + helm),
                        ("both", ";helmholtz.enabled=yes" + helm + ";spectra.enabled=yes;spectra.every=2;spectra.spectrum0=w 1 1 1")):
        d = tmp_path / name
        d.mkdir()
        run(common % d + extra)
    assert not list((tmp_path / "off").glob("*_helmholtz*"))
    p = lib.params_from_ini(ec.ini(base), ov)
    specs = [("w", (1, 1, 1)), ("m", (4, 1, 4))]
    sv = Solver(p, lib)
    try:
        sv.start(lib.init_condition(ec.ini(base), ov, p), 0)
        done, series = sv.run_steps_helm_spectra(10, 3, specs)
    finally:
        sv.close()
    assert done == 10 and list(series.step) == [3, 6, 9]
    for name in ("helm", "both"):
        d = tmp_path / name
        lines = open(d / (prefix + "_helmholtz.txt")).read().splitlines()
        assert lines[0] == "# nStep totalTime spectrum spec file"
        rows = [(int(r[0]), float(r[1]), int(r[2]), r[3], r[4]) for r in (ln.split() for ln in lines[1:])]
        want = [(s, t, m, texts[m].replace(" ", ":"), "%s_helmholtz%d_%07d.npy" % (prefix, m, s)) for s, t in zip(series.step, series.t) for m in range(2)]
        assert rows == want, (rows, want)
        assert sorted(f.name for f in d.glob("*_helmholtz*.npy")) == sorted(r[4] for r in rows)
        for k, s in enumerate(series.step):
            for m in range(2):
                got = np.load(d / ("%s_helmholtz%d_%07d.npy" % (prefix, m, s)))
                assert got.dtype == np.dtype("<f8") and got.flags["C_CONTIGUOUS"] and got.shape == (3, series.modes[m].shape[1])
                for i, series_i in enumerate((series.solenoidal, series.compressive, series.modes)):
                    assert_same_bits(got[i], series_i[m][k], (name, s, m, i))
    assert len(list((tmp_path / "both").glob("*_spectrum0_*.npy"))) == 5
