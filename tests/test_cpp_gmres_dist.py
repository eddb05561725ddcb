"""l3k::DistributedCsr::gmresSolve of the C++ host shim (include/l3k/operator.hpp): the host program compiles against l3k.h on CPU; on
the GPU two rank threads solve the non-symmetric chain of tests/gmres_dist_ref.py by the collective GMRES over the in-process
transport, against the exact solution."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "gmres_dist_shim.cpp")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def _build(out):
    cmd = [HIPCC, "-std=c++20", "-O1", "--offload-arch=gfx950", f"-I{ROOT}/include", SRC, f"-L{ROOT}/l3ster_amd/lib", "-ll3k",
           f"-Wl,-rpath,{ROOT}/l3ster_amd/lib", "-pthread", "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def test_cpp_gmres_dist_compiles_and_links(tmp_path):
    _build(str(tmp_path / "gmres_dist_shim"))


@pytest.mark.gpu
def test_cpp_gmres_dist_runs(tmp_path):
    exe = str(tmp_path / "gmres_dist_shim")
    _build(exe)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr
