"""The order of the chunked two-stream schedule of the flat 3D MHD step (mhd3d_chunked, csrc/api/step_mhd.h), on the CPU: which stream
a launch goes to, which event it waits on, which planes it covers.  On the device a missing wait is a race that usually passes
(tests/test_flat_path_gpu.py compares states); here the test-only emulation logs every device operation in issue order
(tests/emu/rg_backend.h: rgpu_emu_oplog_enable / rgpu_emu_oplog_text) and the log of ONE step through rgpu_godunov_unsplit is read.
The emulation's tiled kernels answer "not covered", so every 3D MHD box is a flat one.  What a shape engages -- how many chunks, where
they end -- comes from flat_path_checks.chunk_facts, the model test_flat_path_gpu.py uses."""
import ctypes as C
import re

import pytest

import flat_path_checks as fp
from conftest import ini
from ramsesgpu_amd.solver import Solver

MAIN, SECOND = 0, 1   # the emulation's stream handles: the context's stream, rg_stream_create's
# the stages of the step, by the functor of their launch, with the planes each covers beyond the update's [a, b): [a - lo, b + hi)
STAGES = [("prim", "K_mhd_prim", 2, 2), ("elec", "K_mhd_elec", 1, 2), ("trace", "K_mhd_trace3d", 1, 1), ("riemann", "K_mhd_flux3d", 0, 1),
          ("save", "K_shear_save_emf", 0, 1), ("remap", "K_shear_remap", 0, 1), ("update", "K_mhd_update3d", 0, 0)]
UPDATE_SEG = 3        # planes per thread of the update's z march (Mhd3dStep::update_as)
CONFIGS = [("orszag-tang3d", "mesh.nx=8;mesh.ny=8;mesh.nz=%d", False), ("mhd_mri_3d", "mesh.nx=8;mesh.ny=8;mesh.nz=%d", True)]
# nz, option "chunks" (None: as created), the chunk ends chunk_facts must give (None: the serial schedule)
SHAPES = [(26, None, [8, 16, 24, 32]), (26, 2, [16, 32]), (8, None, None)]


def one_step_log(lib, base, ov, chunks):
    """(params, chunk facts, operations of one rgpu_godunov_unsplit): each operation a dict -- at (position), kind, s (stream), and
    event, or idx0 / n / stage for a launch of one of STAGES (other launches, the ghost fills, are dropped)"""
    L = lib.lib
    L.rgpu_emu_oplog_text.restype = C.c_char_p
    old = lib.set_option("chunks", chunks) if chunks is not None else None
    try:
        p = lib.params_from_ini(ini(base), ov)
        U0 = lib.init_condition(ini(base), ov, p)
        ks = p.nz + 2 * p.ghostWidth
        facts = fp.chunk_facts(ks, lib.get_option("chunks"), ks)
        L.rgpu_emu_oplog_enable(1)
        sv = Solver(p, lib)
        try:
            sv.start(U0, 0)
            dt = sv.compute_dt(0)
            skip = len(L.rgpu_emu_oplog_text())
            sv.godunov_unsplit(0, dt)
            text = L.rgpu_emu_oplog_text()[skip:].decode()
        finally:
            sv.close()
            L.rgpu_emu_oplog_enable(0)
    finally:
        if old is not None:
            lib.set_option("chunks", old)
    ops = []
    for line in text.splitlines():
        kind, rest = line.split(" ", 1)
        op = {"at": len(ops), "kind": kind, "s": int(re.search(r"\bs=(\d+)", rest).group(1))}
        if kind in ("record", "wait"):
            op["event"] = int(re.search(r"event=(\d+)", rest).group(1))
        elif kind.startswith("launch"):
            op["idx0"], op["n"] = (int(re.search(r"%s=(\d+)" % k, rest).group(1)) for k in ("idx0", "n"))
            op["stage"] = next((name for name, functor, _, _ in STAGES if re.search(r"\b%s\b" % functor, rest)), None)
            if op["stage"] is None:
                continue
        ops.append(op)
    for i, op in enumerate(ops):
        op["at"] = i
    return p, facts, ops


def recorded_before(ops, wait):
    """the record of the event a wait names: the last one issued in front of the wait"""
    recs = [o for o in ops[:wait["at"]] if o["kind"] == "record" and o["event"] == wait["event"]]
    assert recs, "a wait on event %d that nothing recorded: %r" % (wait["event"], wait)
    return recs[-1]


def last_wait_before(ops, op):
    """the last wait on op's stream in front of it"""
    waits = [o for o in ops[:op["at"]] if o["kind"] == "wait" and o["s"] == op["s"]]
    assert waits, "nothing orders %r behind the other stream" % op
    return waits[-1]


def planes_of(p, op):
    """the planes [lo, hi) a stage launch covers, from idx0 and n -- the update's launch says only how many z segments it has"""
    gw = p.ghostWidth
    sk, jsize = (p.nx + 2 * gw) * (p.ny + 2 * gw), p.ny + 2 * gw
    per = jsize if op["stage"] in ("save", "remap") else sk   # the shear kernels run over (j, k), the others over cells
    assert op["idx0"] % per == 0 and op["n"] % per == 0, op
    return op["idx0"] // per, (op["idx0"] + op["n"]) // per


@pytest.mark.parametrize("nz,chunks,cuts", SHAPES, ids=["nz26-default", "nz26-chunks2", "nz8-serial"])
@pytest.mark.parametrize("base,ov,shear", CONFIGS, ids=["plain", "shearing-box"])
def test_one_flat_step(base, ov, shear, nz, chunks, cuts, emu_lib):
    p, facts, ops = one_step_log(emu_lib, base, ov % nz, chunks)
    ks = nz + 2 * p.ghostWidth
    print(facts)
    for o in ops:
        print(o)
    assert p.three_d and p.mhdEnabled and bool(p.shearingBoxEnabled) == shear
    stages = [s for s in STAGES if shear or s[0] not in ("save", "remap")]
    by_stage = {name: [o for o in ops if o.get("stage") == name] for name, _, _, _ in stages}
    if cuts is None:
        assert facts["serial"] and facts["C"] == 1
        assert all(o["s"] == MAIN for o in ops) and not any(o["kind"] == "wait" for o in ops)
        ends = [ks]
    else:
        assert not facts["serial"] and facts["C"] == len(cuts) and facts["cuts"] == cuts
        ends = cuts
    C_ = len(ends)
    # per stage one launch per chunk, over exactly the planes the chunk adds: no plane twice, none left out
    for name, _, lo_halo, hi_halo in stages:
        launches = by_stage[name]
        assert len(launches) == C_, (name, launches)
        done = 0   # clip(a - lo_halo, ..) with a = 0
        for ci, o in enumerate(launches):
            want_hi = min(ends[ci] + hi_halo, ks)
            if name == "update":
                sk = (p.nx + 2 * p.ghostWidth) * (p.ny + 2 * p.ghostWidth)   # one thread per column and z segment of the chunk's planes
                assert o["idx0"] == 0 and o["n"] == sk * ((want_hi - done + UPDATE_SEG - 1) // UPDATE_SEG), (ci, o)
            else:
                assert planes_of(p, o) == (done, want_hi), (name, ci, o, done, want_hi)
            done = want_hi
        assert done == ks
    if cuts is None:
        order = [o["stage"] for o in ops if "stage" in o]
        assert order == [name for name, _, _, _ in stages]
        return
    # the second stream starts behind an event recorded on the context's stream in front of every launch of the step
    on_second = [o for o in ops if o["s"] == SECOND]
    first_launch = min(o["at"] for o in ops if "stage" in o)
    assert on_second[0]["kind"] == "wait"
    fork = recorded_before(ops, on_second[0])
    assert fork["s"] == MAIN and fork["at"] < first_launch
    for name in by_stage:
        want = SECOND if name in ("riemann", "save", "remap") else MAIN
        assert all(o["s"] == want for o in by_stage[name]), name
    for ci in range(C_):
        # the Riemann launch (and the shear pair behind it) waits for the context's stream behind this chunk's trace
        riemann = by_stage["riemann"][ci]
        w = last_wait_before(ops, riemann)
        rec = recorded_before(ops, w)
        assert rec["s"] == MAIN and by_stage["trace"][ci]["at"] < rec["at"] < w["at"] < riemann["at"], (ci, rec, w)
        if ci + 1 < C_:
            assert rec["at"] < by_stage["trace"][ci + 1]["at"]
        last_on_second = riemann
        if shear:
            save, remap = by_stage["save"][ci], by_stage["remap"][ci]
            assert riemann["at"] < save["at"] < remap["at"]
            assert last_wait_before(ops, save) is w and last_wait_before(ops, remap) is w
            last_on_second = remap
        # the update waits for the second stream behind this chunk's Riemann stage, and is queued behind the next chunk's prim / elec / trace
        update = by_stage["update"][ci]
        wu = last_wait_before(ops, update)
        recu = recorded_before(ops, wu)
        assert recu["s"] == SECOND and last_on_second["at"] < recu["at"] < wu["at"] < update["at"], (ci, recu, wu)
        if ci + 1 < C_:
            assert recu["at"] < by_stage["riemann"][ci + 1]["at"]
            for name in ("prim", "elec", "trace"):
                assert by_stage[name][ci + 1]["at"] < update["at"], (ci, name)
