"""l3k::TriangularPreconditioner, the C++ mirror of l3k_tri_* (include/l3k/operator.hpp): compiles and links against l3k.h on CPU; on
the GPU the program solves the reference's makeSPDMatrix(100) with CG and GMRES under ILU(0) (one iteration each) and under SGS, and
checks the solutions, the pieces and the refusals."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "tri_shim.cpp")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def build(out):
    cmd = [HIPCC, "-std=c++20", "-O1", "--offload-arch=gfx950", f"-I{ROOT}/include", SRC, f"-L{ROOT}/l3ster_amd/lib", "-ll3k",
           f"-Wl,-rpath,{ROOT}/l3ster_amd/lib", "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


def test_cpp_tri_compiles_and_links(tmp_path):
    build(str(tmp_path / "tri_shim"))


@pytest.mark.gpu
def test_cpp_tri_runs(tmp_path):
    exe = build(str(tmp_path / "tri_shim"))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr
