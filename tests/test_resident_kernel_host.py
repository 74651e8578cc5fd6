"""The resident-collate kernel's own source, compiled with g++ as host code and run lane by lane under AddressSanitizer
and UBSan (tests/host_math/host_resident.cpp: a stand-alone program, exact-size buffers, every misalignment of source
and destination) against a per-graph memcpy collate.  No GPU: what it checks is the index arithmetic -- no load past a
resident tensor, no store outside a destination, no misaligned 16-byte access, the right bytes."""
import os
import subprocess

from conftest import REPO

HOST = os.path.join(REPO, "tests", "host_math")


def test_collate_kernel_on_the_host_under_sanitizers(tmp_path):
    exe = str(tmp_path / "host_resident")
    subprocess.check_call(["g++", "-std=c++17", "-x", "c++", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(HOST, "hip_shim"), "-o", exe, os.path.join(HOST, "host_resident.cpp")])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert "collate equals memcpy in 252 runs" in run.stdout
