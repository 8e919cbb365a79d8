"""The device-free parts of genomad_amd/csrc/gnn_nn_host.h - Landing's offsets (alignment, totals, empty slices, the eight-slice
limit) and the texts of the shared argument checks - from a stand-alone program (tests/native/nn_host_check.cpp) built for the host
with AddressSanitizer and UBSan and run directly: no GPU, nothing loaded into Python."""
import os
import subprocess

from tests.conftest import ROOT


def test_landing_offsets_and_shared_check_texts(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "nn_host_check")
    build = subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Wall", "-Xarch_host", "-fsanitize=address,undefined",
                            "-Xarch_host", "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "genomad_amd", "csrc"),
                            os.path.join(ROOT, "tests", "native", "nn_host_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
