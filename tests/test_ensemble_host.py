"""The ensemble of 2D boxes (rgpu_ensemble_*, include/rgpu.h) without a GPU: the whole API on the test-only host emulation -- which has
no tiled kernels, so every round is taken member by member through the single-context loop (fused_steps == 0) -- against the oracle
and a lone Solver; the argument checks; and the product library's refusal to run without a device."""
import ctypes as C

import numpy as np
import pytest

import ensemble_checks as ec
from conftest import ini
from ramsesgpu_amd import _capi
from ramsesgpu_amd.ensemble import Ensemble
from ramsesgpu_amd.solver import RgpuError, interior

MIXED_FACES = "mesh.boundary_xmin=1;mesh.boundary_ymax=1;mesh.boundary_xmax=2;mesh.boundary_ymin=3;mesh.boundary_ymax=3"
CASES = [
    ("orszag-tang", "mesh.nx=37;mesh.ny=29", 3, 8),             # 2D MHD, periodic; no tile size divides 37 x 29
    ("blast2d", "mesh.nx=37;mesh.ny=29;" + MIXED_FACES, 4, 8),   # 2D hydro, reflecting / outflow / periodic faces mixed
]


@pytest.mark.parametrize("base,ov,members,nsteps", CASES, ids=[c[0] for c in CASES])
def test_every_member_equals_a_lone_solver_and_the_oracle(base, ov, members, nsteps, emu_lib, oracle):
    """members with perturbed initial states, member 1 with an end time inside its 4th step: state, nStep, t, dt, the dt sequence and
    done of every member == a lone Solver == the oracle; then rgpu_compute_dt and one more step on a member context alone == the
    oracle's next step"""
    cut = nsteps // 2
    ends = lambda m, dts: ec.end_inside_step(dts, cut) if m == 1 else None
    done, stop, fused, ens, U0s, refs = ec.check_ensemble(emu_lib, oracle, base, ov, members, nsteps, tEnds=ends, keep=True)
    try:
        assert done == [cut if m == 1 else nsteps for m in range(members)] and stop == [1 if m == 1 else 0 for m in range(members)]
        assert fused == 0   # the emulation has no ensemble kernels: every round member by member
        p = ens.p
        for m in (0, 1, members - 1):
            v = ens.member(m)
            more, dts_more, _ = oracle.run(p, U0s[m], v.nStep + 1)
            assert v.compute_dt(v.nStep % 2) == float(dts_more[-1])
            v.oneStepIntegration()
            assert v.dt == float(dts_more[-1]) and v.nStep == len(dts_more)
            assert np.array_equal(interior(v.getDataHost(), p), interior(more, p))
    finally:
        ens.close()


def test_split_calls_and_a_second_call_with_a_later_end(emu_lib, oracle):
    """3 + the rest equals one call; a member stopped by its end time goes on when a later call moves the end"""
    base, ov, n = "orszag-tang", "mesh.nx=37;mesh.ny=29", 9
    ec.check_ensemble(emu_lib, oracle, base, ov, 3, n, pieces=[3, n - 3])
    p = emu_lib.params_from_ini(ini(base), ov)
    U0s = ec.member_states(emu_lib, base, ov, p, 3)
    refs = [oracle.run(p, U, n) for U in U0s]
    ens = Ensemble(p, 3, emu_lib)
    try:
        ens.start(U0s)
        ends = [float("inf"), ec.end_inside_step(refs[1][1], 4), float("inf")]
        done, stop, _ = ens.run_steps(5, ends)
        assert done == [5, 4, 5] and stop == [0, 1, 0]
        done, stop, _ = ens.run_steps(4, None)   # members at steps 5, 4, 5: mixed parity
        assert done == [4, 4, 4] and stop == [0, 0, 0]
        for m, want in enumerate((9, 8, 9)):
            v = ens.member(m)
            ref, dts, _ = oracle.run(p, U0s[m], want)
            assert v.nStep == want and v.totalTime == ec.time_of(dts) and v.dt == float(dts[-1])
            assert np.array_equal(interior(v.getDataHost(), p), interior(ref, p))
    finally:
        ens.close()


def _create(lib, p, members):
    _capi.declare_ensemble_api(lib.lib)
    ens = C.c_void_p()
    rc = lib.lib.rgpu_ensemble_create(C.byref(p) if p is not None else None, members, C.byref(ens))
    msg = lib.lib.rgpu_ensemble_last_error(ens).decode() if ens else ""
    return rc, ens, msg


def test_argument_checks(emu_lib):
    L = emu_lib
    p2 = L.params_from_ini(ini("orszag-tang"), "mesh.nx=16;mesh.ny=16")
    for members in (0, -3, 1025):
        rc, ens, msg = _create(L, p2, members)
        assert rc == -1 and "members" in msg, (members, rc, msg)           # RGPU_EINVAL
        L.lib.rgpu_ensemble_destroy(ens)
        assert L.lib.rgpu_ensemble_device_bytes(C.byref(p2), members) == 0
    rc, ens, msg = _create(L, None, 2)
    assert rc == -1 and "NULL" in msg
    L.lib.rgpu_ensemble_destroy(ens)
    p3 = L.params_from_ini(ini("orszag-tang3d"), "mesh.nx=16;mesh.ny=16;mesh.nz=16")
    rc, ens, msg = _create(L, p3, 2)
    assert rc == -5 and "2D" in msg, (rc, msg)                             # RGPU_EUNSUPPORTED
    L.lib.rgpu_ensemble_destroy(ens)
    assert L.lib.rgpu_ensemble_device_bytes(C.byref(p3), 2) == 0
    ps = p2.copy()
    ps.slab_rank, ps.slab_count = 0, 2
    rc, ens, msg = _create(L, ps, 2)
    assert rc == -5 and "slab" in msg, (rc, msg)
    L.lib.rgpu_ensemble_destroy(ens)
    L.lib.rgpu_ensemble_destroy(None)

    rc, ens, msg = _create(L, p2, 3)
    assert rc == 0 and L.lib.rgpu_ensemble_members(ens) == 3
    assert L.lib.rgpu_ensemble_member(ens, -1) is None and L.lib.rgpu_ensemble_member(ens, 3) is None
    ctxs = [L.lib.rgpu_ensemble_member(ens, m) for m in range(3)]
    assert all(ctxs) and len(set(ctxs)) == 3
    assert L.lib.rgpu_ensemble_device_bytes(C.byref(p2), 3) >= 3 * L.lib.rgpu_device_bytes(C.byref(p2))
    L.lib.rgpu_destroy(ctxs[1])           # refused: the member belongs to the ensemble and stays usable
    q = _capi.RgpuParams()
    assert L.lib.rgpu_get_params(ctxs[1], C.byref(q)) == 0 and q.nx == 16
    assert L.lib.rgpu_ensemble_run_steps(ens, 2, None, None, None, None, None, None, None, None) == -1
    assert b"null pointer" in L.lib.rgpu_ensemble_last_error(ens)
    L.lib.rgpu_ensemble_destroy(ens)
    with pytest.raises(RgpuError) as e:
        Ensemble(p3, 2, L)
    assert "(-5)" in str(e.value)


def test_end_time_zero_takes_no_step(emu_lib, oracle):
    """tEnd[m] = 0: done[m] == 0 and stop[m] == 1, the member's state untouched; the others run"""
    base, ov = "orszag-tang", "mesh.nx=21;mesh.ny=19"
    p = emu_lib.params_from_ini(ini(base), ov)
    U0s = ec.member_states(emu_lib, base, ov, p, 3)
    ens = Ensemble(p, 3, emu_lib)
    try:
        ens.start(U0s)
        before = ens.member(2).getDataHost(0)
        done, stop, fused = ens.run_steps(4, [float("inf"), float("inf"), 0.0])
        assert done == [4, 4, 0] and stop == [0, 0, 1] and fused == 0
        v = ens.member(2)
        assert v.nStep == 0 and v.totalTime == 0.0 and v.dt_log == [] and np.array_equal(v.getDataHost(0), before)
        ref, dts, _ = oracle.run(p, U0s[0], 4)
        assert ens.member(0).dt_log == [float(d) for d in dts] and np.array_equal(interior(ens.member(0).getDataHost(), p), interior(ref, p))
    finally:
        ens.close()


def test_member_view_does_not_destroy_the_context(emu_lib):
    p = emu_lib.params_from_ini(ini("blast2d"), "mesh.nx=16;mesh.ny=16")
    ens = Ensemble(p, 2, emu_lib)
    try:
        v = ens.member(1)
        ctx = v.ctx.value
        U = emu_lib.init_condition(ini("blast2d"), "mesh.nx=16;mesh.ny=16", p)
        v.start(U, 0)
        assert v.run_steps(2) == 2   # a member alone through the single-context loop
        with pytest.raises(IndexError):
            ens.member(2)
        assert ens.device_bytes() > 0 and ctx == emu_lib.lib.rgpu_ensemble_member(ens.ens, 1)
    finally:
        ens.close()
    assert not ens.ens and not v.ctx


def test_product_library_refuses_without_a_gpu(product_lib):
    """no device: rgpu_ensemble_create fails with RGPU_ENODEVICE (-2), as rgpu_create does -- no CPU fallback in the product"""
    try:
        import torch
        if torch.cuda.is_available():
            pytest.skip("a GPU is present: the failure path cannot be observed here")
    except ImportError:
        pass
    p = product_lib.params_from_ini(ini("orszag-tang"), "mesh.nx=16;mesh.ny=16")
    rc, ens, msg = _create(product_lib, p, 4)
    assert rc == -2 and "no CPU fallback" in msg, (rc, msg)
    product_lib.lib.rgpu_ensemble_destroy(ens)
    with pytest.raises(RgpuError) as e:
        Ensemble(p, 4, product_lib)
    assert "(-2)" in str(e.value)
