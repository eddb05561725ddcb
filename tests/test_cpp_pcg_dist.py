"""l3k::DistributedCsr::pcgSolve and ::chebyshev of the C++ host shim (include/l3k/operator.hpp): the host program compiles against
l3k.h on CPU; on the GPU it assembles the reference's Diffusion2D problem as one rank of a world of one over the in-process
transport and runs the collective solve against the single-rank one and against the exact solution."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "pcg_dist_shim.cpp")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def _build(out):
    cmd = [HIPCC, "-std=c++20", "-O1", "--offload-arch=gfx950", f"-I{ROOT}/include", SRC, f"-L{ROOT}/l3ster_amd/lib", "-ll3k",
           f"-Wl,-rpath,{ROOT}/l3ster_amd/lib", "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def test_cpp_pcg_dist_compiles_and_links(tmp_path):
    _build(str(tmp_path / "pcg_dist_shim"))


@pytest.mark.gpu
def test_cpp_pcg_dist_runs(tmp_path):
    exe = str(tmp_path / "pcg_dist_shim")
    _build(exe)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr
