"""The flat per-cell kernels on the device, where their own launch machinery engages (helpers and the model: tests/flat_path_checks.py).

The product runs the flat kernels for every context with a per-cell gravity field (Keplerian disk, stratified MRI box, mhd_mri_3d with
gravity.static=yes) and everywhere under RGPU_TILED=0.  Two things belong to that path alone and are executed nowhere but on a GPU
(the CPU emulation runs rg_launch_planes as a linear loop on one stream):

  * the XCD-aware workgroup order of rg_kernel_planes -- it departs from linear order only on planes of more than 8 workgroups and cuts a
    band into several sub-bands only beyond 8 x xcd_sub cells;
  * the chunked two-stream schedule of the flat 3D MHD step -- its steady state needs C >= 3 chunks.

  A  (CPU) the model of the map covers every cell of every plane exactly once; the forcing probe's comparison notices a workgroup
     skipped or repeated
  B  exact cover of rg_kernel_planes measured on the device: rgpu_add_forcing, in place, on exactly representable inputs
  C  gravity-field runs against the oracle at shapes where the model says the map and the schedule engage, over "xcd_sub" and "chunks"
  E  RGPU_TILED=0 in a fresh child process (tests/flat_worker.py), one case per step family, per library
(D and F extend tests/test_gpu_parity.py.)  The checker is the oracle; the exact library is held to equal bits, the contracted one to
parity_checks.L2_TOLERANCE through exact=False of the existing helpers."""
import os
import subprocess
import sys

import numpy as np
import pytest

import flat_path_checks as fp
import parity_checks as pc
from conftest import ROOT, ini

gpu = pytest.mark.gpu


def _lib(request, arith):
    return request.getfixturevalue("gpu_lib" if arith == "exact" else "gpu_contracted_lib")


# ---- A. the model: exact cover, and the figures the shapes below rest on --------------------------------------------------------
def test_plane_map_model_covers_every_cell_exactly_once():
    """plane_map_workgroups (rg_launch_planes + rg_kernel_planes restated) over plane_cells 1 .. 3000, 1 .. 3 planes, both block sizes and
    five sub-band sizes: every cell of every plane is passed to the kernel body exactly once -- the specification the kernel is held
    to on the device (B).  Along the way: every combination of the two guards (live / idle) and nsub > 1 really occur in the sweep."""
    seen = set()
    for block in (fp.K_BLOCK_HEAVY, fp.K_BLOCK):
        for sub in (0, 64, 256, 1024, 4096):
            for nplanes in (1, 2, 3):
                for plane in range(1, 3001):
                    f, wgs = fp.plane_map_workgroups(plane, block, sub, nplanes)
                    assert len(wgs) == f["grid"]
                    cnt = fp.cover_counts(wgs, plane * nplanes)
                    if not (cnt == 1).all():
                        bad = int(np.argmax(cnt != 1))
                        raise AssertionError("plane_cells %d, %d planes, block %d, sub %d (%r): cell %d of plane %d is visited %d times"
                                             % (plane, nplanes, block, sub, f, bad % plane, bad // plane, int(cnt[bad])))
                    if not f["linear"]:
                        band = f["band"]
                        seen.add((any(ib >= band for ib, _, _ in wgs), any(ib < band and a == b for ib, a, b in wgs), f["nsub"] > 1))
    assert {(g1, g2) for g1, g2, _ in seen} == {(False, False), (False, True), (True, False), (True, True)}, seen
    assert any(n for _, _, n in seen)


def test_plane_map_model_on_the_shapes_of_this_module():
    """the figures quoted next to the cases below, from the model"""
    f = fp.plane_map_facts(48 * 54, 256, 4096, 12)           # the forcing probe's plane
    assert (f["bpp"], f["band"], f["nsub"], f["idle_xcds"], f["off_guard_live"], f["reordered"]) == (11, 2, 1, 2, True, True), f
    f = fp.plane_map_facts(230 * 214, 256, 4096, 2)          # > 8 x 4096 cells: two sub-bands of 13 slots for a band of 25
    assert (f["bpp"], f["band"], f["nsub"], f["T"], f["in_band_guard_live"]) == (193, 25, 2, 13, True), f
    f = fp.plane_map_facts(50 * 56, 256, 256, 46)            # 2800 cells at xcd_sub 256: two sub-bands for either block, ragged last XCD
    g = fp.plane_map_facts(50 * 56, 64, 256, 46)
    assert (f["nsub"], g["nsub"], f["off_guard_live"], g["off_guard_live"]) == (2, 2, True, True), (f, g)
    f, g = fp.plane_map_facts(234 * 154, 256, 4096), fp.plane_map_facts(234 * 154, 64, 4096)      # Keplerian disk 230 x 150, one plane
    assert (f["nsub"], g["nsub"], f["in_band_guard_live"], g["in_band_guard_live"]) == (2, 2, False, True), (f, g)
    assert fp.plane_map_facts(46 * 30, 256, 4096)["reordered"] is False      # the largest flat plane of the suite before this module
    # the chunk schedule: rgpu_create's clamps and mhd3d_chunked's C
    assert fp.chunk_facts(46, -1, 46) == {"nchunks": 5, "serial": False, "C": 5, "cuts": [9, 18, 27, 36, 46]}
    assert fp.chunk_facts(46, 40, 46)["nchunks"] == 23 and fp.chunk_facts(46, 40, 46)["C"] == 6          # both clamps act
    assert fp.chunk_facts(46, 1, 46)["serial"] and fp.chunk_facts(46, -1, 46, timers=True)["serial"] and fp.chunk_facts(46, -1, 15)["serial"]
    assert fp.chunk_facts(22, -1, 22)["C"] == 2 and fp.chunk_facts(46, -1, 23)["C"] == 3


def test_forcing_probe_notices_a_skipped_or_repeated_workgroup(product_lib):
    """the comparison of B, on the CPU: K_add_forcing run by the model's enumeration equals the numpy expectation; with one workgroup
    of the enumeration dropped, or one repeated, it does not (the in-place kernel forces a cell once per visit)"""
    p = product_lib.params_from_ini(ini("turbulence_hydro"), "mesh.nx=44;mesh.ny=50;mesh.nz=3")
    gw = p.ghostWidth
    plane = (p.nx + 2 * gw) * (p.ny + 2 * gw)
    assert plane == 2592
    U, F = fp.forcing_probe_inputs(p)
    ref = fp.forcing_probe_expected(p, U, F, 0.5)
    inside = fp.interior_mask(p)
    I = (slice(None),) + (slice(gw, -gw),) * 3
    assert (ref[I][1:] != U[I][1:]).all() and np.array_equal(ref[0], U[0])         # every interior cell changes in every forced component
    for sub in (0, 256, 4096):
        _, wgs = fp.plane_map_workgroups(plane, fp.K_BLOCK, sub, p.nz)
        assert np.array_equal(fp.forcing_by_workgroups(p, U, F, 0.5, wgs, gw * plane), ref)
        live = [n for n, (_, a, b) in enumerate(wgs) if inside[gw * plane + a:gw * plane + b].any()]      # workgroups with interior cells
        for victim in (live[0], live[len(live) // 2], live[-1]):
            dropped = wgs[:victim] + wgs[victim + 1:]
            repeated = wgs[:victim + 1] + wgs[victim:]
            for broken in (dropped, repeated):
                got = fp.forcing_by_workgroups(p, U, F, 0.5, broken, gw * plane)
                _, a, b = wgs[victim]
                ndiff = int((got[1] != ref[1]).sum())
                assert not np.array_equal(got, ref) and 0 < ndiff <= b - a, (sub, victim, ndiff)


# ---- B. exact cover on the device -----------------------------------------------------------------------------------------------
# 44 x 50 x 12 (+ 2 ghost cells): planes of 48 x 54 = 2592 cells, 11 workgroups of 256 -> bands of 2, XCD 5 partly filled, XCDs 6, 7 idle.
# 226 x 210 x 2: planes of 230 x 214 = 49220 cells > 8 x 4096 -> the default sub-band size gives two sub-bands of 13 slots for a band of 25.
FORCING_SHAPES = [
    ("mesh.nx=44;mesh.ny=50;mesh.nz=12", {
        0: {"linear": True},
        256: {"band": 2, "nsub": 2, "idle_xcds": 2, "off_guard_live": True, "reordered": True},
        1024: {"band": 2, "nsub": 1, "T": 2, "idle_xcds": 2, "off_guard_live": True, "reordered": True},
        None: {"band": 2, "nsub": 1, "T": 2, "idle_xcds": 2, "off_guard_live": True, "reordered": True}}),
    ("mesh.nx=226;mesh.ny=210;mesh.nz=2", {
        0: {"linear": True},
        256: {"band": 25, "nsub": 25, "T": 1},
        1024: {"band": 25, "nsub": 7, "T": 4, "in_band_guard_live": True},
        None: {"band": 25, "nsub": 2, "T": 13, "in_band_guard_live": True, "reordered": True}}),
]


@gpu
@pytest.mark.parametrize("arith", ["exact", "contracted"])
@pytest.mark.parametrize("sub", [0, 256, 1024, None], ids=["xcd_sub=0", "xcd_sub=256", "xcd_sub=1024", "xcd_sub-default"])
@pytest.mark.parametrize("ov,want", FORCING_SHAPES, ids=["44x50x12", "226x210x2"])
def test_forcing_probe_exact_cover(ov, want, sub, arith, request):
    """rgpu_add_forcing once on rho = 1, zero momenta, constant energy and an integer forcing field: a cell visited twice is forced
    twice, a cell missed not at all, a ghost cell must stay as it was -- every double equal to numpy's, for both libraries"""
    lib = _lib(request, arith)
    if sub is None:
        assert lib.get_option("xcd_sub") < 0, "the default sub-band size is what this case is about"
    fp.check_forcing_probe(lib, "turbulence_hydro", ov, sub, want[sub])


# ---- C. gravity-field runs at shapes where the map and the schedule engage --------------------------------------------------------
STRAT = ";hydro.slope_type=2.0;MRI.amp=0.3"
SUBS = [None, ("xcd_sub", 0), ("xcd_sub", 256)]
CHUNKS = [("chunks", 1), ("chunks", 2), ("chunks", 3), ("chunks", 40)]      # 40 > ksize / 2 = 23: clamped to 23 by rgpu_create, C to 6 by the span
C_OF = {None: 5, ("xcd_sub", 0): 5, ("xcd_sub", 256): 5, ("chunks", 1): 1, ("chunks", 2): 2, ("chunks", 3): 3, ("chunks", 40): 6}
# (base, overrides, steps, variants, facts at the default options, facts at xcd_sub = 256, C per variant)
GRAVITY_FIELD_RUNS = [
    ("strat-44x50x40", "mhd_mri_3d_stratified", "mesh.nx=44;mesh.ny=50;mesh.nz=40" + STRAT, 3, SUBS + CHUNKS,
     {"plane_cells": 2800, "ksize": 46, "b256.band": 2, "b64.band": 6, "b256.reordered": True, "b64.reordered": True, "chunks.nchunks": 5, "chunks.C": 5},
     {"b256.nsub": 2, "b64.nsub": 2, "b256.off_guard_live": True, "b64.off_guard_live": True}, C_OF),
    ("mri-gravity-40x36x40", "mhd_mri_3d", "mesh.nx=40;mesh.ny=36;mesh.nz=40;gravity.static=yes", 3, SUBS + CHUNKS,
     {"plane_cells": 1932, "ksize": 46, "b64.band": 4, "b64.reordered": True, "chunks.nchunks": 5, "chunks.C": 5},
     {"b64.band": 4, "b64.reordered": True}, C_OF),
    ("kepler2d-230x150", "Keplerian_disk2d", "mesh.nx=230;mesh.ny=150", 4, SUBS,
     {"plane_cells": 36036, "ksize": 1, "b256.nsub": 2, "b64.nsub": 2, "b256.in_band_guard_live": False, "b64.in_band_guard_live": True,
      "b256.reordered": True, "b64.reordered": True},
     {"b256.nsub": 18, "b64.nsub": 18}, None),
    ("kepler3d-44x50x24", "Keplerian_disk2d", "mesh.nx=44;mesh.ny=50;mesh.nz=24", 3, SUBS,
     {"plane_cells": 2592, "ksize": 28, "b256.band": 2, "b64.band": 6, "b256.reordered": True, "b64.reordered": True, "b256.idle_xcds": 2},
     {"b256.nsub": 2, "b64.nsub": 2}, None),
    ("strat-224x208x16", "mhd_mri_3d_stratified", "mesh.nx=224;mesh.ny=208;mesh.nz=16" + STRAT, 2, [None],
     {"plane_cells": 49220, "ksize": 22, "b256.band": 25, "b256.nsub": 2, "b256.T": 13, "b256.in_band_guard_live": True, "b64.nsub": 2,
      "chunks.nchunks": 2, "chunks.C": 2},
     None, {None: 2}),
]


@gpu
@pytest.mark.parametrize("arith", ["exact", "contracted"])
@pytest.mark.parametrize("base,ov,nsteps,variants,facts,facts256,c_of", [c[1:] for c in GRAVITY_FIELD_RUNS], ids=[c[0] for c in GRAVITY_FIELD_RUNS])
def test_gravity_field_runs_vs_oracle(base, ov, nsteps, variants, facts, facts256, c_of, arith, oracle, request):
    """a context with a per-cell gravity field, at a shape where the model says the XCD order and (3D MHD) the steady state of the chunk
    schedule engage: the phase timers of a timed step name the flat kernels and no sweep; then every variant of "xcd_sub" and "chunks",
    untimed, equals the oracle (one oracle run) and every other variant -- state, every dt, totalTime"""
    lib = _lib(request, arith)
    p = lib.params_from_ini(ini(base), ov)
    assert p.gravityEnabled == 2 and lib.get_option("xcd_sub") < 0 and lib.get_option("chunks") < 0
    what = "%s [%s]" % (base, ov)
    fp.assert_facts(fp.box_facts(p, fp.DEFAULT_XCD_SUB), facts, what + " at the default options")
    if facts256 is not None:
        fp.assert_facts(fp.box_facts(p, 256), facts256, what + " at xcd_sub 256")
    if p.mhdEnabled and len(variants) > 1:
        assert fp.box_facts(p, fp.DEFAULT_XCD_SUB)["chunks"]["C"] >= 3, "the steady state of the pipeline needs three chunks"
    fp.assert_flat_path(lib, base, ov)
    fp.check_variants_vs_oracle(lib, oracle, base, ov, nsteps, variants, exact=arith == "exact", chunk_want=c_of)


def test_every_shape_engages_what_it_claims(product_lib):
    """the engagement facts of B, C and E against the model, without a GPU (the GPU tests assert them again before they compare): a
    table that has gone wrong shows here"""
    import flat_worker
    for ov, want in FORCING_SHAPES:
        p = product_lib.params_from_ini(ini("turbulence_hydro"), ov)
        assert p.randomForcingEnabled and not p.mhdEnabled
        plane = (p.nx + 2 * p.ghostWidth) * (p.ny + 2 * p.ghostWidth)
        for sub, facts in want.items():
            got = fp.plane_map_facts(plane, fp.K_BLOCK, fp.DEFAULT_XCD_SUB if sub is None else sub, p.nz)
            fp.assert_facts({"map": got}, {"map." + k: v for k, v in facts.items()}, "forcing probe [%s] xcd_sub %r" % (ov, sub))
    for _, base, ov, _, variants, facts, facts256, c_of in GRAVITY_FIELD_RUNS:
        p = product_lib.params_from_ini(ini(base), ov)
        assert p.gravityEnabled == 2, (base, ov)
        fp.assert_facts(fp.box_facts(p, fp.DEFAULT_XCD_SUB), facts, base + " [" + ov + "]")
        if facts256 is not None:
            fp.assert_facts(fp.box_facts(p, 256), facts256, base + " [" + ov + "] at xcd_sub 256")
        ks = p.nz + 2 * p.ghostWidth
        for var in variants:
            if c_of is not None:
                assert fp.chunk_facts(ks, var[1] if var and var[0] == "chunks" else -1, ks)["C"] == c_of[var], (base, var)
    for name, base, ov, _, option, facts in flat_worker.case_list():
        p = product_lib.params_from_ini(ini(base), ov)
        fp.assert_facts(fp.box_facts(p, option[1] if option else fp.DEFAULT_XCD_SUB), facts, name)
        if p.three_d or not p.mhdEnabled:     # (every case but the flat 2D MHD one, which has no plane map)
            assert fp.box_facts(p, fp.DEFAULT_XCD_SUB)["b64"]["band"] >= 2, name


# ---- E. RGPU_TILED=0, in a process of its own -------------------------------------------------------------------------------------
# tiled_enabled() reads the environment once per process, so each library gets one fresh child (never os.exec*: the child is started with
# subprocess and holds the GPU next to this process, two at a time).  Seen on MI355X: the worker's own clock 4.7 - 4.9 s for its twelve
# cases (3 s of it the oracle's 224 x 208 x 16 run), 6.7 - 7.2 s for the whole test with the start of the process; the limit is 8 x that.
WORKER_LIMIT_S = 60


@gpu
@pytest.mark.parametrize("arith", ["exact", "contracted"])
def test_flat_kernels_everywhere_vs_oracle(arith, request, oracle, tmp_path):
    """RGPU_TILED=0: "a second, independently tested implementation of every step" (include/rgpu.h) -- tests/flat_worker.py runs one case
    per step family against the oracle, each at a shape with a multi-workgroup band, and the two >= 200^2 planes of
    test_xcd_sub_band_sizes_vs_oracle at xcd_sub 0 / 2048 / 4096; it stops at its first failure"""
    _lib(request, arith)                                     # fails here without a GPU or without the library
    out = str(tmp_path / "flat_worker.txt")
    env = dict(os.environ, RGPU_TILED="0")
    env.pop("RGPU_LIB", None)
    env.pop("RGPU_TEST_OPTIONS", None)
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "flat_worker.py"), arith, out], env=env, stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, universal_newlines=True, timeout=WORKER_LIMIT_S)
    lines = open(out).read().splitlines() if os.path.exists(out) else []
    print("\n".join(lines))
    assert res.returncode == 0, "\n".join(lines[-3:]) + "\n" + res.stdout[-3000:]
    import flat_worker
    assert [ln.split()[0] for ln in lines] == ["OK"] * len(flat_worker.case_list()) + ["DONE"], lines
