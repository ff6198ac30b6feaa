"""Kernel-level numbers of the 3D monitor: three steps, then rgpu_history_mri (MHD boxes: K_hist_rows, the other one-pass
streaming reduction over the state) and rgpu_state_monitor3d eight times each, then 20 monitored steps with a sample every 10 -- to be
run under a kernel trace of its own, one process per box:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o t -- python scripts/monitor_kernel_probe.py mhd_mri_3d "mesh.nx=256;mesh.ny=256;mesh.nz=256"

and read OUT/*kernel_stats.csv: the average duration of monitor_vol_cols_kernel, monitor_vol_planes_kernel, monitor_vol_finish_kernel
and rg_kernel<256, K_hist_rows>.  Bytes per second of the column pass = interior cells x variables x 8 / its duration.  The numbers
recorded so far are in profiles/monitor3d_kernel_trace.json.  Needs a GPU."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ramsesgpu_amd.solver import Library, Solver, lib_path  # noqa: E402


def main():
    base, ov = sys.argv[1], sys.argv[2]
    lib = Library(lib_path(sys.argv[3] if len(sys.argv) > 3 else "contracted"))
    ini = os.path.join(ROOT, "configs", base + ".ini")
    p = lib.params_from_ini(ini, ov)
    sv = Solver(p, lib)
    sv.start(lib.init_condition(ini, ov, p), 0)
    sv.run_steps(3)
    for _ in range(8):
        if p.mhdEnabled:
            sv.history_mri()
        sv.state_monitor()
    done, s = sv.run_steps_monitored(20, 10)
    print(base, ov, "steps", done, "samples", [int(x) for x in s.step], "taken inside batches:", lib.lib.rgpu_monitor_batch_samples(sv.ctx))
    sv.close()


if __name__ == "__main__":
    main()
