"""What a context allocates for its run loop (the clock records, the history log, the monitor log: DeviceMirror members of rgpu_ctx,
csrc/api/ctx.h) lives and dies with it: tests/cpp/run_loop_lifetime.cpp is a stand-alone program over the host emulation that runs all
three loops across a batch boundary, a launch failure inside a batch, an ensemble and a refused creation, built here under the address
and undefined-behaviour sanitizers of g++ (an executable: it brings its own runtime) and run once."""
import os
import subprocess

from conftest import CONFIGS, ROOT

HOST = ("ini_config.cpp", "host_params.cpp", "init_conditions.cpp", "host_capi.cpp", "run_driver.cpp", "hdf5_io.cpp")


def test_run_loop_lifetime_under_sanitizers(tmp_path):
    csrc = os.path.join(ROOT, "ramsesgpu_amd", "csrc")
    exe = str(tmp_path / "run_loop_lifetime")
    # (the runtimes linked statically: the program does not depend on what else the process has loaded before it)
    subprocess.check_call(["g++", "-std=c++17", "-O0", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-Wno-unknown-pragmas",
                           "-I", os.path.join(ROOT, "tests", "emu"), "-I", csrc, "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "run_loop_lifetime.cpp"), os.path.join(csrc, "rgpu_api.cpp")] +
                          [os.path.join(csrc, "host", f) for f in HOST] + ["-ldl", "-o", exe])
    out = subprocess.run([exe, CONFIGS], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    print(out.stdout)
    assert out.returncode == 0 and "run_loop_lifetime: ok" in out.stdout, out.stdout
