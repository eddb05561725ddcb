"""l3k::ExportDefinition / l3k::PvtuExporter, the C++ mirror of l3k_vtk_* (include/l3k/operator.hpp): compiles and links against l3k.h on
CPU; on the GPU the program's files are byte-identical to the Python route's on the same mesh and field storage."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "vtk_shim.cpp")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def build(out):
    cmd = [HIPCC, "-std=c++20", "-O1", "--offload-arch=gfx950", f"-I{ROOT}/include", SRC, f"-L{ROOT}/l3ster_amd/lib", "-ll3k",
           f"-Wl,-rpath,{ROOT}/l3ster_amd/lib", "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


def test_cpp_vtk_compiles_and_links(tmp_path):
    build(str(tmp_path / "vtk_shim"))


@pytest.mark.gpu
def test_cpp_vtk_files_match_the_python_route(tmp_path):
    import torch

    from l3ster_amd import system, vtk
    torch.cuda.set_device(0)
    ctx = system.Context(0, torch.cuda.current_stream().cuda_stream)
    part = system.CubePartition((3, 2, 2), 2, perturb=0.1)
    fields = np.random.default_rng(11).standard_normal((4, part.n_local_nodes + 5))
    fields_file = str(tmp_path / "fields.bin")
    fields.tofile(fields_file)
    exe = build(str(tmp_path / "vtk_shim"))
    r = subprocess.run([exe, fields_file, str(tmp_path / "cpp" / "solution.pvtu")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr

    exporter = vtk.PvtuExporter(system.DeviceMesh(ctx, part, 1), chunk_bytes=4096)
    export_def = vtk.ExportDefinition(str(tmp_path / "py" / "solution.pvtu"))
    export_def.define_field("T", [2]).define_field("flux", [3, 0]).define_field("velocity", [1, 3, 0])
    exporter.export_solution(export_def, torch.as_tensor(fields).cuda())
    assert sorted(os.listdir(tmp_path / "cpp")) == sorted(os.listdir(tmp_path / "py")) == ["solution.pvtu", "solution_0.vtu"]
    for name in ("solution.pvtu", "solution_0.vtu"):
        assert (tmp_path / "cpp" / name).read_bytes() == (tmp_path / "py" / name).read_bytes(), name
