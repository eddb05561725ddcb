"""l3k::AssembledSystem of the C++ host shim (include/l3k/operator.hpp): the host program compiles against l3k.h on CPU; on the GPU
it runs the reference's Diffusion2DAssembledTest through beginAssembly / assembleProblem / endAssembly / solve on a quad mesh."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "diffusion2d_assembled.cpp")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def _build(out):
    cmd = [HIPCC, "-std=c++20", "-O1", "--offload-arch=gfx950", f"-I{ROOT}/include", SRC, f"-L{ROOT}/l3ster_amd/lib", "-ll3k",
           f"-Wl,-rpath,{ROOT}/l3ster_amd/lib", "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def test_cpp_assembled_system_compiles_and_links(tmp_path):
    _build(str(tmp_path / "diffusion2d_assembled"))


@pytest.mark.gpu
def test_cpp_assembled_system_runs(tmp_path):
    exe = str(tmp_path / "diffusion2d_assembled")
    _build(exe)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr
