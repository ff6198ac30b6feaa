"""Parameter scans (rgpu_ensemble_create_scan, Ensemble.scan) without a GPU: the API on the test-only host emulation -- which has no
tiled kernels, so every round is taken member by member through each member's own context (fused_steps == 0) -- against the oracle
and a lone Solver created from the member's set; the argument checks; and the product library's refusal to run without a device."""
import ctypes as C

import numpy as np
import pytest

import ensemble_checks as ec
import ensemble_scan_checks as sc
from conftest import ini
from ramsesgpu_amd import _capi
from ramsesgpu_amd.ensemble import Ensemble
from ramsesgpu_amd.solver import RgpuError, interior

MIXED_FACES = "mesh.boundary_xmin=1;mesh.boundary_ymax=1;mesh.boundary_xmax=2;mesh.boundary_ymin=3;mesh.boundary_ymax=3"   # as tests/test_ensemble_host.py
CASES = [
    ("orszag-tang", "mesh.nx=37;mesh.ny=29"),                  # 2D MHD, periodic; no tile size divides 37 x 29
    ("blast2d", "mesh.nx=37;mesh.ny=29;" + MIXED_FACES),       # 2D hydro, reflecting / outflow / periodic faces mixed
]


@pytest.mark.parametrize("base,ov", CASES, ids=[c[0] for c in CASES])
def test_gamma_scan_every_member_equals_a_lone_solver_and_the_oracle(base, ov, emu_lib, oracle):
    n = 8
    done, stop, fused = sc.check_scan(emu_lib, oracle, base, ov, sc.GAMMA, n)
    assert done == [n] * len(sc.GAMMA) and stop == [0] * len(sc.GAMMA)
    assert fused == 0   # the emulation has no ensemble kernels: every round member by member


def test_cfl_and_box_scan_with_an_end_time(emu_lib, oracle):
    """cfl and the box extents (hence dx, dy) differ; member 1 ends inside its 4th step"""
    n, cut = 8, 4
    ends = lambda m, dts: ec.end_inside_step(dts, cut) if m == 1 else None
    done, stop, fused = sc.check_scan(emu_lib, oracle, "orszag-tang", "mesh.nx=21;mesh.ny=19", sc.CFL_BOX, n, tEnds=ends)
    assert done == [n, cut, n] and stop == [0, 1, 0] and fused == 0
    ovs, ps = sc.scan_sets(emu_lib, "orszag-tang", "mesh.nx=21;mesh.ny=19", sc.CFL_BOX)
    assert len({p.dx for p in ps}) == 2 and len({p.dy for p in ps}) == 2 and len({p.cfl for p in ps}) == 3   # the sets are what they claim


def _create_scan(lib, sets, members=None):
    _capi.declare_ensemble_api(lib.lib)
    arr = (_capi.RgpuParams * len(sets))(*sets) if sets else None
    n = len(sets) if members is None else members
    ens = C.c_void_p()
    rc = lib.lib.rgpu_ensemble_create_scan(arr, n, C.byref(ens))
    msg = lib.lib.rgpu_ensemble_last_error(ens).decode() if ens else ""
    nbytes = lib.lib.rgpu_ensemble_scan_device_bytes(arr, n)
    return rc, ens, msg, nbytes


def test_argument_checks(emu_lib):
    L = emu_lib
    p = L.params_from_ini(ini("blast2d"), "mesh.nx=16;mesh.ny=16")
    pm = L.params_from_ini(ini("orszag-tang"), "mesh.nx=16;mesh.ny=16")

    def refused(sets, code, *words, members=None):
        rc, ens, msg, nbytes = _create_scan(L, sets, members)
        assert ens.value, "the ensemble object is returned even on failure"
        assert rc == code and all(w in msg for w in words), (rc, msg, words)
        assert nbytes == 0, (nbytes, msg)
        L.lib.rgpu_ensemble_destroy(ens)

    # a shared field that differs: RGPU_EINVAL, the message names the field and the first offending member
    q = p.copy(); q.riemannSolver = (p.riemannSolver + 1) % 3
    refused([p, p.copy(), q, q], -1, "riemannSolver", "member 2")
    q = p.copy(); q.nx = p.nx + 1
    refused([p, q], -1, "nx", "member 1")
    q = p.copy(); q.slope_type = 2.0 if p.slope_type == 1.0 else 1.0
    refused([p, p.copy(), p.copy(), q], -1, "slope_type", "member 3")
    q = pm.copy(); q.cIso = 1.0
    assert pm.cIso == 0.0
    refused([pm, q], -1, "cIso", "member 1")
    refused([q, pm, pm], -1, "cIso", "member 1")
    # what rgpu_ensemble_create refuses, with its code
    p3 = L.params_from_ini(ini("orszag-tang3d"), "mesh.nx=16;mesh.ny=16;mesh.nz=16")
    refused([p3, p3.copy()], -5, "2D")                        # RGPU_EUNSUPPORTED
    refused([pm, pm.copy()], -1, "members", members=0)
    refused([pm] * 4, -1, "members", members=1025)
    refused(None, -1, "NULL", members=2)
    bad = pm.copy(); bad.abi_version = 0
    refused([pm, bad], -1, "member 1", "abi_version")
    assert L.lib.rgpu_ensemble_create_scan(None, 2, None) == -1

    # a good scan
    q1, q2 = pm.copy(), pm.copy()
    q1.gamma0, q2.cfl = 1.5, 0.3
    rc, ens, msg, nbytes = _create_scan(L, [pm, q1, q2])
    assert rc == 0 and L.lib.rgpu_ensemble_members(ens) == 3, (rc, msg)
    assert nbytes >= sum(L.lib.rgpu_device_bytes(C.byref(s)) for s in (pm, q1, q2))
    ctxs = [L.lib.rgpu_ensemble_member(ens, m) for m in range(3)]
    assert all(ctxs) and len(set(ctxs)) == 3 and L.lib.rgpu_ensemble_member(ens, 3) is None
    L.lib.rgpu_destroy(ctxs[1])           # refused: the member belongs to the ensemble and stays usable
    got = _capi.RgpuParams()
    for m, want in enumerate((pm, q1, q2)):   # member m holds set m
        assert L.lib.rgpu_get_params(ctxs[m], C.byref(got)) == 0
        assert (got.gamma0, got.cfl, got.nx) == (want.gamma0, want.cfl, want.nx)
    L.lib.rgpu_ensemble_destroy(ens)
    with pytest.raises(RgpuError) as e:
        Ensemble.scan([p3, p3.copy()], L)
    assert "(-5)" in str(e.value)


def test_scan_of_equal_sets_equals_the_uniform_ensemble(emu_lib):
    base, ov, M, n = "orszag-tang", "mesh.nx=21;mesh.ny=19", 3, 5
    p = emu_lib.params_from_ini(ini(base), ov)
    U0s = ec.member_states(emu_lib, base, ov, p, M)
    a, b = Ensemble(p, M, emu_lib), Ensemble.scan([p.copy() for _ in range(M)], emu_lib)
    try:
        assert b.device_bytes() >= a.device_bytes() > 0
        outs = []
        for e in (a, b):
            e.start(U0s)
            outs.append(e.run_steps(n))
        assert outs[0] == outs[1]
        for m in range(M):
            va, vb = a.member(m), b.member(m)
            assert (va.nStep, va.totalTime, va.dt, va.dt_log) == (vb.nStep, vb.totalTime, vb.dt, vb.dt_log)
            assert np.array_equal(interior(va.getDataHost(), p), interior(vb.getDataHost(), p))
            assert va.state_checksum(va.nStep % 2) == vb.state_checksum(vb.nStep % 2)
    finally:
        a.close()
        b.close()


def test_product_library_refuses_without_a_gpu(product_lib):
    """no device: rgpu_ensemble_create_scan fails with RGPU_ENODEVICE (-2), as rgpu_ensemble_create does"""
    try:
        import torch
        if torch.cuda.is_available():
            pytest.skip("a GPU is present: the failure path cannot be observed here")
    except ImportError:
        pass
    p = product_lib.params_from_ini(ini("orszag-tang"), "mesh.nx=16;mesh.ny=16")
    q = p.copy(); q.gamma0 = 1.5
    rc, ens, msg, nbytes = _create_scan(product_lib, [p, q])
    assert rc == -2 and "no CPU fallback" in msg, (rc, msg)
    assert nbytes > 0   # a valid scan: the byte count does not need a device
    product_lib.lib.rgpu_ensemble_destroy(ens)
    with pytest.raises(RgpuError) as e:
        Ensemble.scan([p, q], product_lib)
    assert "(-2)" in str(e.value)
