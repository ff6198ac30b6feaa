"""The oracle's z-window step (orc_godunov_unsplit_zwindow, parity_checks.zwindow / step_in_windows), pinned on the CPU: windows of
uneven widths that tile [0, nz), stepped one after another from cuts of the same state, stitched together, equal the oracle's
whole-box step in every double -- sequential and threaded.  This is what lets tests/test_fullsize_windows.py check the bench-size
steps of the GPU against the oracle."""
import numpy as np
import pytest

import parity_checks as pc
from conftest import ini

# four families: the rotating shearing box, plain periodic 3D MHD, hydro between reflecting walls, outflow faces (2 = NEUMANN)
CASES = [
    ("mhd_mri_3d", "mesh.nx=8;mesh.ny=12;mesh.nz=13"),
    ("orszag-tang3d", "mesh.nx=10;mesh.ny=9;mesh.nz=13"),
    ("implode3d", "mesh.nx=10;mesh.ny=9;mesh.nz=13;hydro.riemannSolver=hllc"),
    ("orszag-tang3d", "mesh.nx=9;mesh.ny=10;mesh.nz=13;mesh.boundary_xmin=2;mesh.boundary_xmax=2;mesh.boundary_zmin=2;mesh.boundary_zmax=2"),
]
WIDTHS = [1, 2, 5, 5]          # uneven, then the rest of the 13 planes
STATES = ["stress", "evolved"]


def _state(lib, oracle, base, ov, kind):
    """(p, state the step starts from, dt, t): a rough stress state with its ghosts filled by the oracle, or the oracle's state after
    three steps of the problem (its ghosts as the oracle's run leaves them)"""
    p = lib.params_from_ini(ini(base), ov)
    if kind == "stress":
        t = 2.0
        U = pc.stress_state(p, 3, "rough")
        oracle.make_all_boundaries(p, U, t, 0.0)
        return p, U, 0.3 * oracle.compute_dt(p, U), t
    U, dts, t = oracle.run_sequential(p, lib.init_condition(ini(base), ov, p), 3)
    return p, U, oracle.compute_dt(p, U), t


@pytest.mark.parametrize("kind", STATES)
@pytest.mark.parametrize("base,ov", CASES, ids=["%s[%s]" % c for c in CASES])
def test_windows_stitch_to_the_whole_box_step(base, ov, kind, product_lib, oracle):
    p, U, dt, t = _state(product_lib, oracle, base, ov, kind)
    gw, rot = p.ghostWidth, bool(p.mhdEnabled) and p.Omega0 > 0
    if not rot:
        oracle.make_all_boundaries(p, U, 0.0, 0.0)      # the plain path fills its input at the start of the step: the windows are cut after
    ref = oracle.godunov_unsplit(p, U.copy(), dt, t)
    assert np.isfinite(ref).all()
    threaded = [1] + ([3] if oracle._mt_threads(p) > 1 else [])
    for order in (WIDTHS, WIDTHS[::-1]):
        for nt in threaded:
            got = np.full_like(ref, np.nan)
            for k0, w, out in pc.step_in_windows(oracle, p, U, dt, t, order, nthreads=nt):
                got[:, gw + k0:gw + k0 + w] = out[:, gw:gw + w]
            # every plane of the box, x and y ghost columns included (on the plain path they are the input's filled ghosts)
            inner = (slice(None), slice(gw, -gw))
            nbad = int((got[inner] != ref[inner]).sum())
            assert nbad == 0, "%s [%s] %s, widths %r, %d threads: %d of %d doubles differ from the whole-box step" % (
                base, ov, kind, order, nt, nbad, ref[inner].size)


def test_window_params_and_cut(product_lib):
    p = product_lib.params_from_ini(ini("mhd_mri_3d"), "mesh.nx=8;mesh.ny=12;mesh.nz=13")
    U = np.arange(np.prod(p.shape), dtype=np.float64).reshape(p.shape)
    q, W = pc.zwindow(p, U, 5, 2)
    gw = p.ghostWidth
    assert (q.nz, q.nz_global, q.dz, q.nx, q.ny) == (2, p.nz_global, p.dz, p.nx, p.ny)
    assert q.zMin == p.zMin + 5 * p.dz and q.zMax == p.zMin + 7 * p.dz
    assert W.shape == tuple(q.shape) == (p.nbVar, 2 + 2 * gw) + tuple(p.shape[2:])
    assert np.array_equal(W, U[:, 5:7 + 2 * gw]) and W.flags["C_CONTIGUOUS"]
    assert p.nz == 13                                    # the box's parameters are untouched
    for nz in (13, 512):
        q = product_lib.params_from_ini(ini("mhd_mri_3d"), "mesh.nx=512;mesh.ny=512;mesh.nz=%d" % nz)
        ws = pc.window_widths(q)
        assert sum(ws) == nz and max(ws) - min(ws) <= 1
        cells = (max(ws) + 2 * gw) * (q.nx + 2 * gw) * (q.ny + 2 * gw)
        assert cells * 8 * (182 + 2 * q.nbVar) <= pc.WINDOW_SCRATCH


def test_offset_crossings_and_sweep_plans_at_bench_size(product_lib):
    """the layout facts of the issue's sizes, from api/ctx.h's layout: U crosses 2^32 bytes in IV near plane 446 and 2^33 in IC near
    plane 375 at 518^3; at config 5 U's element index crosses 2^31 in IC and F's in component 7.  The 512^3 shearing box sweeps its
    513 Riemann planes in one segment; its MhLastX launch has one base segment whose last round is cut into 16 sub-segments (the
    comment of launch_mhd3d_sweep); the 3-plane update ends in a partial segment."""
    p = product_lib.params_from_ini(ini("mhd_mri_3d"), "mesh.nx=512;mesh.ny=512;mesh.nz=512")
    cross = pc.offset_crossing_planes(p)
    assert ("U", "2^32 bytes", 3, 446) in cross and ("U", "2^33 bytes", 7, 375) in cross, cross
    plan = pc.sweep_plan_facts(p)
    assert plan["mhd3d_sweep MhMain"][:2] == (1, 1)
    assert plan["mhd3d_sweep MhLastX"][:2] == (1, 16) and plan["mhd3d_sweep MhLastX"][2] == list(range(3, 515, 32))
    assert plan["mhd3d update"][2][-1] == 516 and (p.nz + 2 * p.ghostWidth) % 3 != 0
    c5 = product_lib.params_from_ini(ini("mhd_mri_3d"), "mesh.nx=512;mesh.ny=1024;mesh.nz=512")
    cross5 = pc.offset_crossing_planes(c5)
    assert any(a == "U" and w == "2^31 elements" and v == 7 for a, w, v, _ in cross5), cross5
    assert any(a == "F" and w == "2^31 elements" and v == 7 for a, w, v, _ in cross5), cross5
