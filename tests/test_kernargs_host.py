"""The kernarg image of every launch site (zignal_amd/csrc/fz_kernargs.hpp: KernArgs) under AddressSanitizer + UBSan, byte for byte
against the layout of the kernels' argument structs as tests/cpp/kernargs_layout.cpp writes it out: six header sizes, with and without
the stream-major window, 0 / 1 / 2 / 3 / 300 float coefficients (300 passes the 1 KiB kept inline), no float64 tail / 0 / 3 doubles;
the header rewritten with the tails in place.  A stand-alone host program: no HIP, no library."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "zignal_amd", "csrc")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_kernarg_images_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "kernargs_layout")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(HERE, "cpp", "kernargs_layout.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-4000:]
    assert "kernarg images: 180 cases, 0 failures" in out.stdout, out.stdout
