"""Driven turbulence inside the device-clock batches of rgpu_run_steps* (option "forcing_clock"; csrc/api/forcing.h): checks shared by the
CPU emulation tests (tests/test_forcing_clock_emu.py) and the GPU ones (tests/test_forcing_clock_gpu.py).

The yardstick is the literal loop of the SAME library: a second Solver with "forcing_clock" = 0, or a loop of oneStepIntegration.  On the
exact library and on the emulation everything is compared bit for bit -- the dt sequence, the time, the interior state, its checksum and
the 471 doubles of rgpu_ou_forcing_get_state, generator included; on the contracted library within the project's contracted gate
(relative L2 1e-12 on the state, parity_checks.assert_same; 1e-11 on a dt, parity_checks.check_run_vs_oracle): the body of a kick may
contract differently in two functors.

  run_batched / run_literal   a Run of the same steps through rgpu_run_steps (in one call or in pieces) and through the literal loop
  assert_same_run             the comparison above
  check_same_run              8 steps in one call, as 3 + 5, and a literal step behind them (check 1), with the counter and the
                              readiness of check 2
  check_end_time              tEnd reached inside a batch; the generator is rewound (check 3)
  check_planted               a fast cell on the first / last interior cell, the tile seams, the last z plane: the scan that rides in the
                              last kick sees every cell (check 5)
  check_spectra / check_pdfs  the monitors behind forced steps (check 6)
  check_unchanged_surfaces    rgpu_clock_capable, rgpu_clock_open, rgpu_inv_dt_fusable; viscosity and gravity keep the literal loop"""
import collections
import ctypes as C

import numpy as np

import cfl_plant_checks as cp
import parity_checks as pc
from conftest import ini
from ramsesgpu_amd.solver import Solver, interior

PERT_T = "turbulence.initialDensityPerturbationAmplitude=0.1"
PERT_OU = "turbulence-Ornstein-Uhlenbeck.initialDensityPerturbationAmplitude=0.1"
HYDRO_BOX = "mesh.nx=20;mesh.ny=18;mesh.nz=10"     # partial 16 x 16 tiles in x and in y
MHD_BOX = "mesh.nx=18;mesh.ny=12;mesh.nz=10"       # the 16 x 8 tiles of the 3D MHD sweep
# name -> (parameter file, overrides, both): both = the Ornstein-Uhlenbeck file with the random forcing switched on in the parameters
# (no parameter file selects the two problems at once; the step runs both stages, random first)
CASES = {
    "hydro": ("turbulence_hydro", HYDRO_BOX + ";" + PERT_T, False),
    "hydro_ou": ("turbulence_hydro_ou", HYDRO_BOX + ";" + PERT_OU, False),
    "mhd": ("turbulence_mhd", MHD_BOX + ";" + PERT_T, False),
    "mhd_ou": ("turbulence_mhd_ou", MHD_BOX + ";" + PERT_OU, False),
    "hydro_both": ("turbulence_hydro_ou", HYDRO_BOX + ";" + PERT_OU, True),
}
FOUR = ("hydro", "hydro_ou", "mhd", "mhd_ou")
OU_STATE = 471      # RGPU_OU_STATE_DOUBLES
EUNSUPPORTED = -5   # RGPU_EUNSUPPORTED
DT_RTOL = 1e-11     # the contracted library's dt (parity_checks.check_run_vs_oracle)

Run = collections.namedtuple("Run", "dts t dt nStep state checksum ou ready batch_steps")
Setup = collections.namedtuple("Setup", "base ov p U0 F")


def setup(lib, case, extra=""):
    """parameters, initial state and driving field of a case; extra: further overrides"""
    base, ov, both = CASES[case] if case in CASES else case
    ov = ov + (";" + extra if extra else "")
    p = lib.params_from_ini(ini(base), ov)
    F = lib.init_forcing(ini(base), ov, p)
    if both:
        # a smooth driving field of unit order, the energy input rate of the shipped turbulence files' order
        p.randomForcingEnabled = 1
        p.randomForcingEdot = 0.5
        nv, ks, js, is_ = p.shape
        z, y, x = np.meshgrid(np.arange(ks) / ks, np.arange(js) / js, np.arange(is_) / is_, indexing="ij")
        F = np.stack([np.sin(2 * np.pi * (y + 0.3 * z)), np.cos(2 * np.pi * (z + x)), np.sin(2 * np.pi * (x - y) + 1.0)])
    U0 = lib.init_condition(ini(base), ov, p)
    assert U0.std(axis=(1, 2, 3))[0] > 0, "the density is uniform: the perturbation override did not take"
    U0.flags.writeable = False
    return Setup(base, ov, p, U0, F)


def fresh(lib, s, U0=None):
    sv = Solver(s.p, lib)
    try:
        G = lib.init_gravity(ini(s.base), s.ov, s.p)
        if G is not None:
            sv.set_gravity_field(G)
        if s.F is not None:
            sv.set_forcing_field(s.F)
        sv.start(np.array(s.U0 if U0 is None else U0), 0)
    except Exception:
        sv.close()
        raise
    return sv


def ou_state(lib, sv):
    if not sv.p.ouForcingEnabled:
        return None
    st = np.zeros(OU_STATE)
    assert lib.lib.rgpu_ou_forcing_get_state(sv.ctx, st.ctypes.data_as(C.POINTER(C.c_double))) == 0
    return st


def snapshot(lib, sv, dts):
    par = sv.nStep % 2
    ready = int(lib.lib.rgpu_device_time_step_ready(sv.ctx, par))   # (before anything below can touch the context)
    return Run([float(d) for d in dts], sv.totalTime, sv.dt, sv.nStep, interior(sv.getDataHost(), sv.p).copy(), sv.state_checksum(par),
               ou_state(lib, sv), ready, sv.forcing_batch_steps())


class option:
    """`with option(lib, name, value)`: the option set, and put back"""

    def __init__(self, lib, name, value):
        self.lib, self.name, self.value = lib, name, value

    def __enter__(self):
        self.old = self.lib.set_option(self.name, self.value)
        assert self.old >= 0, self.name

    def __exit__(self, *a):
        self.lib.set_option(self.name, self.old)


def run_literal(lib, s, nsteps, U0=None, tEnd=float("inf")):
    """the reference's loop, one host turn per step: oneStepIntegration while t < tEnd"""
    sv = fresh(lib, s, U0)
    try:
        dts = []
        while sv.nStep < nsteps and sv.totalTime < tEnd:
            dts.append(sv.oneStepIntegration())
        return snapshot(lib, sv, dts)
    finally:
        sv.close()


def run_batched(lib, s, pieces, U0=None, tEnd=float("inf"), clock=1, keep=False):
    """rgpu_run_steps, one call per entry of `pieces`; clock: the option "forcing_clock" of the run.  keep: (Run, the open Solver)"""
    with option(lib, "forcing_clock", clock):
        sv = fresh(lib, s, U0)
        try:
            dts, done = [], []
            for n in pieces:
                done.append(sv.run_steps(n, tEnd))
                dts += list(sv.dt_log)
            run = snapshot(lib, sv, dts)
        except Exception:
            sv.close()
            raise
        if keep:
            return run, sv, done
        sv.close()
        return run, None, done


def assert_same_run(got, ref, what, exact=True):
    assert got.nStep == ref.nStep and len(got.dts) == len(ref.dts), "%s: %d steps (%d dts), the literal loop %d (%d)" % (what, got.nStep, len(got.dts), ref.nStep, len(ref.dts))
    if exact:
        assert got.dts == ref.dts, "%s: dt sequence %r, the literal loop's %r" % (what, got.dts, ref.dts)
        assert got.t == ref.t and got.dt == ref.dt, "%s: ends at t = %r with dt = %r, the literal loop at %r with %r" % (what, got.t, got.dt, ref.t, ref.dt)
        assert got.checksum == ref.checksum, "%s: state checksum %x, the literal loop's %x" % (what, got.checksum, ref.checksum)
    else:
        assert all(abs(a / b - 1.0) < DT_RTOL for a, b in zip(got.dts + [got.t, got.dt], ref.dts + [ref.t, ref.dt])), "%s: dt sequence %r, the literal loop's %r" % (what, got.dts, ref.dts)
    pc.assert_same(got.state, ref.state, what + ", interior state", exact=exact)
    assert (got.ou is None) == (ref.ou is None)
    if got.ou is not None:
        # mode, proj and the generator (seed digits, spare flag and value) depend on no arithmetic of the device: equal in every library
        gen = np.r_[0:93, 186:OU_STATE]
        assert np.array_equal(got.ou[gen], ref.ou[gen]), "%s: modes, projection or generator of the forcing process differ: %r" % (what, np.nonzero(got.ou[gen] != ref.ou[gen])[0])
        if exact:
            assert np.array_equal(got.ou, ref.ou), "%s: %d of the %d doubles of the forcing process differ" % (what, int((got.ou != ref.ou).sum()), OU_STATE)
        else:
            pc.assert_same(got.ou[93:186], ref.ou[93:186], what + ", force of the process", exact=False)


# ---- checks 1 and 2 -------------------------------------------------------------------------------------------------------------------
N = 8


def check_same_run(lib, case, exact=True):
    s = setup(lib, case)
    what = "%s [%s], %s library" % (s.base, s.ov, lib.arithmetic)
    ref = run_literal(lib, s, N)
    ref1 = run_literal(lib, s, N + 1)
    assert ref.batch_steps == 0 and ref.ready == 0, (what, "the literal loop", ref.batch_steps, ref.ready)
    off, _, done = run_batched(lib, s, [N], clock=0)
    assert done == [N] and off.batch_steps == 0 and off.ready == 0, "%s: forcing_clock = 0 batched %d steps, readiness %d" % (what, off.batch_steps, off.ready)
    assert_same_run(off, ref, what + ": run_steps(%d) with forcing_clock = 0" % N, exact)
    one, _, done = run_batched(lib, s, [N])
    assert done == [N], (what, done)
    assert_same_run(one, ref, what + ": run_steps(%d)" % N, exact)
    # it was a batch: every step, the first included (priming), and the state it left has its maxima in the slots
    assert one.batch_steps == N and one.ready == 1, "%s: %d of %d steps ran in a batch, readiness %d" % (what, one.batch_steps, N, one.ready)
    two, sv, done = run_batched(lib, s, [3, N - 3], keep=True)
    try:
        assert done == [3, N - 3], (what, done)
        assert_same_run(two, ref, what + ": run_steps(3), run_steps(%d)" % (N - 3), exact)
        assert two.batch_steps == N and two.ready == 1
        # a literal step behind the batches: the literal loop's next dt and state
        sv.oneStepIntegration()
        nxt = snapshot(lib, sv, two.dts + [sv.dt])
        assert_same_run(nxt, ref1, what + ": a literal step behind the batches", exact)
        assert nxt.batch_steps == N and nxt.ready == 0
    finally:
        sv.close()


# ---- check 3 --------------------------------------------------------------------------------------------------------------------------
def check_end_time(lib, case, exact=True, nsteps=8):
    s = setup(lib, case)
    what = "%s [%s], %s library, end time inside the batch" % (s.base, s.ov, lib.arithmetic)
    cut = nsteps // 2
    full = run_literal(lib, s, nsteps)
    t_cut = 0.0
    for d in full.dts[:cut]:
        t_cut += d
    tEnd = t_cut - 0.25 * full.dts[cut - 1]      # reached during step `cut`
    ref_cut = run_literal(lib, s, nsteps, tEnd=tEnd)
    assert ref_cut.nStep == cut, (what, ref_cut.nStep, cut)
    ref_more = run_literal(lib, s, cut + 4)
    got, sv, done = run_batched(lib, s, [nsteps], tEnd=tEnd, keep=True)
    try:
        assert done == [cut], "%s: run_steps(%d, tEnd) did %r steps, the literal loop %d" % (what, nsteps, done, cut)
        assert_same_run(got, ref_cut, what, exact)       # the process too: the generator stands where the literal loop's does
        assert got.batch_steps == cut and got.ready == 1, (what, got.batch_steps, got.ready)
        assert sv.run_steps(5, tEnd) == 0
        assert sv.run_steps(4, 1e30) == 4
        more = snapshot(lib, sv, got.dts + list(sv.dt_log))
        assert_same_run(more, ref_more, what + ", then 4 more steps", exact)
        assert more.batch_steps == cut + 4
    finally:
        sv.close()


# ---- check 4 --------------------------------------------------------------------------------------------------------------------------
def check_two_batches(lib, exact=True, nsteps=260):
    """more steps than a batch holds (RGPU_CLOCK_BATCH = 256) in one call"""
    s = setup(lib, ("turbulence_hydro_ou", "mesh.nx=8;mesh.ny=8;mesh.nz=8;" + PERT_OU, False))
    what = "%s [%s], %s library, %d steps in one call" % (s.base, s.ov, lib.arithmetic, nsteps)
    ref, _, done = run_batched(lib, s, [nsteps], clock=0)
    assert done == [nsteps] and ref.batch_steps == 0
    got, _, done = run_batched(lib, s, [nsteps])
    assert done == [nsteps] and got.batch_steps == nsteps and got.ready == 1, (what, done, got.batch_steps, got.ready)
    assert_same_run(got, ref, what, exact)


# ---- check 5 --------------------------------------------------------------------------------------------------------------------------
def planted_cells(p):
    """the first and the last interior cell, the seams of the first tile in x and in y, the last interior z plane"""
    _, _, sx, sy, _ = cp.tile_shape(p)
    mx, my, mz = p.nx // 2, p.ny // 2, p.nz // 2
    cells = [("first", (0, 0, 0)), ("last", (p.nx - 1, p.ny - 1, p.nz - 1))]
    cells += [("seam-x-%d" % i, (i, my, mz)) for i in sx] + [("seam-y-%d" % j, (mx, j, mz)) for j in sy]
    cells.append(("z-high", (mx, my, p.nz - 1)))
    assert all(0 <= c[a] < n for _, c in cells for a, n in enumerate((p.nx, p.ny, p.nz)))
    return cells


PLANT_SPEED = 8.0     # of the planted cell, in units of the fastest cell's sum over the directions of c + |v| in the initial state


def planted_state(s, cell, oracle):
    """the initial state of the case with the momentum of one cell raised"""
    U = np.array(s.U0)
    idx = cp._index(s.p, cell)
    ie, iw = 1, 4                      # the state's variables: rho, E, rho u, rho v, rho w.  Along z: tangential to the seams in x and y
    mom = PLANT_SPEED * U[(0,) + idx] * oracle.compute_inv_dt(s.p, U) * min(s.p.dx, s.p.dy, s.p.dz)
    if not s.p.cIso > 0:               # adiabatic: the energy follows, the pressure stays
        U[(ie,) + idx] += 0.5 * (mom ** 2 - U[(iw,) + idx] ** 2) / U[(0,) + idx]
    U[(iw,) + idx] = mom
    return U


def check_planted(lib, oracle, case, name, exact=True):
    s = setup(lib, case)
    cell = dict(planted_cells(s.p))[name]
    what = "%s [%s] planted at %s %r, %s library" % (s.base, s.ov, name, cell, lib.arithmetic)
    U0 = planted_state(s, cell, oracle)
    ref = run_literal(lib, s, 3, U0=U0)
    # on the CPU, first: the planted cell sets the second dt of the literal run -- masking it and its neighbours in the state after step 1
    # drops the oracle's 1/dt of that state (the generator's proof of cfl_plant_checks.planted_reference)
    sv = fresh(lib, s, U0)
    try:
        sv.oneStepIntegration()
        U1 = sv.getDataHost().copy()
    finally:
        sv.close()
    # (the target set: the cell and every neighbour within one cell, diagonals included, across the periodic faces -- at cfl < 1 a step carries the pulse no further,
    #  and on this rough background it does spread along the diagonals)
    plant = cp.Plant(name, cell, (cp.Z, 1), ())
    n = (s.p.nx, s.p.ny, s.p.nz)
    assert all(b == cp.PERIODIC for b in s.p.bc), "the neighbours of a face cell are taken across periodic faces"
    block = [cp._index(s.p, ((cell[0] + a) % n[0], (cell[1] + b) % n[1], (cell[2] + c) % n[2])) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1)]
    ratio = cp.masking_ratio(oracle, s.p, U1, block, cp.far_cell(s.p, plant))
    print("forcing clock: %s: 1/dt with the target set masked / unmasked = %.3f" % (what, ratio))
    if not ratio <= cp.MASK_CAP:
        raise cp.PlantError("%s: masking the target set leaves %.3f of the oracle's 1/dt: the planted cell does not set the second dt" % (what, ratio))
    # ... and one cell alone holds the maximum: of the 27, the one whose masking lowers the oracle's 1/dt most lowers it when it alone
    # is masked, so a scan that lost exactly that cell gives another dt.  It is the planted cell, or (adiabatic hydro: the pulse has moved
    # on along z) a neighbour along z -- it lies where the placement is about: on the same x for a seam in x, the same y for a seam in
    # y, the same z for the last plane, the same cell for the two corners
    far = cp.far_cell(s.p, plant)
    single = [cp.masking_ratio(oracle, s.p, U1, [c], far) for c in block]
    best = block[int(np.argmin(single))]
    print("forcing clock: %s: the cell that sets the second dt is %r (array index; the plant is %r), masked alone it leaves %.4f" % (what, best, cp._index(s.p, cell), min(single)))
    if not min(single) < 1.0:
        raise cp.PlantError("%s: no single cell of the target set holds the maximum of the oracle's 1/dt" % what)
    here = cp._index(s.p, cell)      # (k, j, i)
    axes = {"seam-x": (2,), "seam-y": (1,), "z-high": (0,)}.get(name[:6], (0, 1, 2))
    if not all(best[a] == here[a] for a in axes):
        raise cp.PlantError("%s: the cell that sets the second dt, %r, is not where the placement is about (%r, axes %r)" % (what, best, here, axes))
    inv1 = oracle.compute_inv_dt(s.p, U1)
    assert abs(s.p.cfl / inv1 / ref.dts[1] - 1.0) < 1e-9, (what, s.p.cfl / inv1, ref.dts[1])     # (the oracle scans the state the library left)
    got, _, done = run_batched(lib, s, [3], U0=U0)
    assert done == [3] and got.batch_steps == 3, (what, done, got.batch_steps)
    if exact:
        assert got.dts == ref.dts, "%s: dt sequence %r, the literal loop's %r" % (what, got.dts, ref.dts)
    else:
        assert all(abs(a / b - 1.0) < DT_RTOL for a, b in zip(got.dts, ref.dts)), "%s: dt sequence %r, the literal loop's %r" % (what, got.dts, ref.dts)


# ---- check 6 --------------------------------------------------------------------------------------------------------------------------
def _monitored(lib, s, call, counter, clock):
    with option(lib, "forcing_clock", clock):
        sv = fresh(lib, s)
        try:
            done, series = call(sv)
            return done, series, int(getattr(lib.lib, counter)(sv.ctx)), sv.forcing_batch_steps(), snapshot(lib, sv, sv.dt_log)
        finally:
            sv.close()


def check_spectra(lib, exact=True, nsteps=8, every=2):
    s = setup(lib, ("turbulence_hydro_ou", "mesh.nx=16;mesh.ny=16;mesh.nz=16;" + PERT_OU, False))
    what = "%s [%s], %s library, spectra every %d steps" % (s.base, s.ov, lib.arithmetic, every)
    call = lambda sv: sv.run_steps_spectra(nsteps, every, [("w", (1, 1, 1)), ("v", (1, 1, 1))])
    d0, ref, n0, b0, run0 = _monitored(lib, s, call, "rgpu_spectrum_batch_samples", 0)
    d1, got, n1, b1, run1 = _monitored(lib, s, call, "rgpu_spectrum_batch_samples", 1)
    assert d0 == d1 == nsteps and (n0, b0) == (0, 0), (what, d0, d1, n0, b0)
    assert list(got.step) == list(ref.step) == list(range(every, nsteps + 1, every)), (what, got.step, ref.step)
    assert n1 == len(got.step) and b1 == nsteps, "%s: %d of %d samples and %d of %d steps inside batches" % (what, n1, len(got.step), b1, nsteps)
    assert_same_run(run1, run0, what, exact)
    for m in range(2):
        assert np.array_equal(got.modes[m], ref.modes[m])
        if exact:
            assert np.array_equal(got.t, ref.t) and np.array_equal(got.power[m], ref.power[m]), "%s: the samples of spec %d differ from the forcing_clock = 0 run's" % (what, m)
        else:
            pc.assert_same(got.power[m], ref.power[m], what + ", power of spec %d" % m, exact=False)


def check_pdfs(lib, exact=True, nsteps=8, every=2):
    s = setup(lib, "hydro_ou")
    what = "%s [%s], %s library, PDFs every %d steps" % (s.base, s.ov, lib.arithmetic, every)
    specs = [("rho", "log2", -2, 2, 3), (("mx", "lin", -0.5, 0.5, 16), ("rho", "lin", 0.5, 1.5, 8))]
    call = lambda sv: sv.run_steps_pdfs(nsteps, every, specs)
    d0, ref, n0, b0, run0 = _monitored(lib, s, call, "rgpu_pdf_batch_samples", 0)
    d1, got, n1, b1, run1 = _monitored(lib, s, call, "rgpu_pdf_batch_samples", 1)
    assert d0 == d1 == nsteps and (n0, b0) == (0, 0), (what, d0, d1, n0, b0)
    assert list(got.step) == list(ref.step) == list(range(every, nsteps + 1, every)), (what, got.step, ref.step)
    assert n1 == len(got.step) and b1 == nsteps, "%s: %d of %d samples and %d of %d steps inside batches" % (what, n1, len(got.step), b1, nsteps)
    assert_same_run(run1, run0, what, exact)
    cells = s.p.nx * s.p.ny * s.p.nz
    for m in range(len(specs)):
        assert (got.pdfs[m].reshape(len(got.step), -1).sum(axis=1) == cells).all()
        if exact:
            assert np.array_equal(got.t, ref.t) and np.array_equal(got.pdfs[m], ref.pdfs[m]), "%s: the counts of spec %d differ from the forcing_clock = 0 run's" % (what, m)
        elif np.array_equal(run1.state, run0.state):   # counts are integers: equal where the states are, and under round-off a cell on
            assert np.array_equal(got.pdfs[m], ref.pdfs[m]), "%s: equal states, other counts of spec %d" % (what, m)   # a bin edge may change its class -- only the totals above are defined


# ---- check 7 --------------------------------------------------------------------------------------------------------------------------
def check_against_oracle(lib, oracle, case, nsteps=5, contracted=False):
    """the round-off agreement the forced runs are held to (parity_checks.check_run_vs_oracle): the kicks use the device's cos and the
    parallel sums"""
    s = setup(lib, case)
    what = "%s [%s], %s library, %d batched steps vs oracle" % (s.base, s.ov, lib.arithmetic, nsteps)
    try:
        oracle.set_gravity_field(None)
        oracle.set_forcing_field(s.F)
        ref, dts_ref, _ = oracle.run(s.p, np.array(s.U0), nsteps)
    finally:
        oracle.set_forcing_field(None)
    got, _, done = run_batched(lib, s, [nsteps])
    assert done == [nsteps] and got.batch_steps == nsteps, (what, done, got.batch_steps)
    np.testing.assert_allclose(np.array(got.dts), dts_ref, rtol=1e-11 if contracted else 1e-12, atol=0)   # (check_run_vs_oracle's two bounds)
    pc.assert_same(got.state, interior(ref, s.p), what, exact=False)


# ---- check 8 --------------------------------------------------------------------------------------------------------------------------
def check_unchanged_surfaces(lib, case):
    s = setup(lib, case)
    sv = fresh(lib, s)
    try:
        L = lib.lib
        assert L.rgpu_clock_capable(sv.ctx) == 0
        L.rgpu_clock_open.restype = C.c_int
        L.rgpu_clock_open.argtypes = [C.c_void_p, C.c_double, C.c_double]
        assert L.rgpu_clock_open(sv.ctx, 0.0, 1e30) == EUNSUPPORTED
        assert L.rgpu_inv_dt_fusable(sv.ctx) == 0
        assert sv.run_steps(2) == 2 and sv.forcing_batch_steps() == 2      # (the refused open left nothing behind)
        assert L.rgpu_clock_capable(sv.ctx) == 0 and L.rgpu_inv_dt_fusable(sv.ctx) == 0
    finally:
        sv.close()


def check_stays_literal(lib, case, extra, exact=True, nsteps=4):
    """a forced context with something else that keeps a step out of a batch (viscosity, gravity): the literal loop, the same results"""
    s = setup(lib, case, extra)
    what = "%s [%s], %s library" % (s.base, s.ov, lib.arithmetic)
    ref = run_literal(lib, s, nsteps)
    got, _, done = run_batched(lib, s, [nsteps])
    assert done == [nsteps] and got.batch_steps == 0 and got.ready == 0, (what, done, got.batch_steps, got.ready)
    assert_same_run(got, ref, what, exact)
