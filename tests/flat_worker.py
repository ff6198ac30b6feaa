"""Worker of tests/test_flat_path_gpu.py::test_flat_kernels_everywhere_vs_oracle: one process under RGPU_TILED=0 (read once per
process: csrc/hip/tiled_hydro.h tiled_enabled), where every step runs the flat per-cell kernels.

    python tests/flat_worker.py exact|contracted RESULT_FILE

Runs a fixed list of cases against the oracle, one after another, and writes one line per case to RESULT_FILE ("OK <seconds> <case>");
it stops at the first case that fails or errors ("FAIL <case>: ...") and starts nothing after it.  The last line of a clean run is
"DONE <seconds>".  Every case first asserts from the model (tests/flat_path_checks.py) what its shape engages, and from the phase
timers of one timed step that the flat kernels ran and no tiled sweep."""
import os
import sys
import time
import traceback

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for d in (ROOT, HERE):
    if d not in sys.path:
        sys.path.insert(0, d)


def case_list():
    """[(name, base, overrides, steps, option or None, facts)]: one case per step family at a shape whose flux kernels (workgroups of 64)
    fill more than one workgroup per XCD band, then the two >= 200^2 planes of test_xcd_sub_band_sizes_vs_oracle at three sub-band
    sizes (the option is process-wide and read by rgpu_create: every value gets a context of its own)"""
    cases = [
        ("hydro2d", "kelvin_helmholtz_gpu_2d", "mesh.nx=96;mesh.ny=64", 4, None, {"b256.band": 4, "b64.band": 14, "b256.reordered": True}),
        # the flat 2D MHD kernels are launched over a linear index range (rg_launch): no plane map to engage, the path alone
        ("mhd2d", "orszag-tang", "mesh.nx=96;mesh.ny=80", 4, None, {"plane_cells": 102 * 86}),
        ("hydro3d-walls", "implode3d", "mesh.nx=40;mesh.ny=36;mesh.nz=24;hydro.riemannSolver=hllc", 3, None, {"b64.band": 4, "b64.reordered": True}),
        ("mhd3d-plain", "orszag-tang3d", "mesh.nx=40;mesh.ny=36;mesh.nz=40", 3, None, {"b64.band": 4, "b64.reordered": True, "chunks.C": 5}),
        ("mhd3d-shearing-box", "mhd_mri_3d", "mesh.nx=40;mesh.ny=36;mesh.nz=40;MRI.amp=0.3", 3, None, {"b64.band": 4, "b64.reordered": True, "chunks.C": 5}),
        ("mhd3d-dissipative", "orszag-tang3d", "mesh.nx=24;mesh.ny=20;mesh.nz=16;hydro.nu=0.01;MHD.eta=0.02", 3, None, {"b64.band": 2, "b64.reordered": True, "chunks.C": 2}),
    ]
    # planes of 230 x 214 = 49220 (MHD, 3 ghost cells) and 212 x 228 = 48336 cells (hydro, 2): bands of 25 and 24 workgroups of 256
    mri = {0: {"b256.linear": True, "chunks.C": 2}, 2048: {"b256.band": 25, "b256.nsub": 4, "b256.T": 7, "b256.in_band_guard_live": True},
           4096: {"b256.band": 25, "b256.nsub": 2, "b256.T": 13, "b256.in_band_guard_live": True}}
    imp = {0: {"b256.linear": True}, 2048: {"b256.band": 24, "b256.nsub": 3, "b256.T": 8}, 4096: {"b256.band": 24, "b256.nsub": 2, "b256.T": 12}}
    for sub in (0, 2048, 4096):
        cases.append(("mri-224x208x16-xcd_sub=%d" % sub, "mhd_mri_3d", "mesh.nx=224;mesh.ny=208;mesh.nz=16", 2, ("xcd_sub", sub), mri[sub]))
        cases.append(("implode-208x224x8-xcd_sub=%d" % sub, "implode3d", "mesh.nx=208;mesh.ny=224;mesh.nz=8;hydro.riemannSolver=hllc", 2, ("xcd_sub", sub), imp[sub]))
    return cases


def main():
    arith, out = sys.argv[1], sys.argv[2]
    assert os.environ.get("RGPU_TILED") == "0", "this worker is the RGPU_TILED=0 process"
    import flat_path_checks as fp
    import parity_checks as pc
    from conftest import ini
    from oracle_api import Oracle
    from ramsesgpu_amd.solver import Library, lib_path
    lib = Library(lib_path(arith))
    assert lib.arithmetic == arith
    oracle = fp.OnceOracle(Oracle(os.path.join(ROOT, "oracle", "liboracle.so")))
    t_all = time.time()
    with open(out, "w") as f:
        for name, base, ov, nsteps, option, facts in case_list():
            t0 = time.time()
            old = lib.set_option(*option) if option else None
            try:
                p = lib.params_from_ini(ini(base), ov)
                fp.assert_facts(fp.box_facts(p, fp.effective_sub(lib)), facts, name)
                fp.assert_flat_path(lib, base, ov)
                pc.check_run_vs_oracle(lib, oracle, base, ov, nsteps, exact=arith == "exact")
            except BaseException as e:   # noqa: B902 -- whatever it was: report it, start nothing more
                f.write("FAIL %s: %s\n" % (name, " ".join(str(e).split())[:1500]))
                f.flush()
                traceback.print_exc()
                return 1
            finally:
                if option:
                    lib.set_option(option[0], old)
            f.write("OK %.1f %s\n" % (time.time() - t0, name))
            f.flush()
        f.write("DONE %.1f\n" % (time.time() - t_all))
    return 0


if __name__ == "__main__":
    sys.exit(main())
