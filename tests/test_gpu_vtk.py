"""The ParaView export on the device (l3k_vtk_*, l3ster_amd.vtk): the base64 stream encoder alone against base64.b64encode, whole
.vtu / .pvtu files byte for byte against the restatement of tests/vtk_ref.py (all but the Position array, which is compared after
decoding), a check that does not go through the restatement (a linear field of the decoded coordinates, sub-cell volumes), a
partition with ghost nodes, the refusals, and one Diffusion2D solve exported end to end."""
import base64
import ctypes as C
import os
import struct

import numpy as np
import pytest
import torch

import vtk_ref as R
from l3ster_amd import capi, solve, system, vtk

pytestmark = pytest.mark.gpu

GROUPS = [("T", [2]), ("flux", [4, 1]), ("velocity", [3, 0, 2])]  # non-adjacent, non-ascending rows
N_FIELDS, PAD = 5, 7  # ld = local nodes + PAD


@pytest.fixture(scope="module")
def ctx():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    torch.cuda.set_device(0)
    return system.Context(0, torch.cuda.current_stream().cuda_stream)


def definition(file_name, groups=GROUPS):
    d = vtk.ExportDefinition(str(file_name))
    for name, inds in groups:
        d.define_field(name, inds)
    return d


def host_fields(part, seed=3):
    return np.random.default_rng(seed).standard_normal((N_FIELDS, part.n_local_nodes + PAD))


# ------------------------------------------------------------------------------------------------------------ the encoder alone
def expected_text(data):
    return base64.b64encode(struct.pack("<Q", len(data)) + data)


@pytest.mark.parametrize("n", list(range(0, 41)))
def test_encoder_every_short_length(ctx, n):
    """every payload length 0 .. 40 (the ABI takes a byte count): 0, 1 and 2 left-over stream bytes, with and without padding; the
    bytes behind the payload are not read into the text"""
    data = bytes(np.random.default_rng(n).integers(0, 256, n + 16, dtype=np.uint8))
    buf = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    lib = capi.load()
    want = expected_text(data[:n])
    text = torch.full((len(want) + 16,), 0x2a, dtype=torch.uint8, device="cuda")
    capi.check(lib.l3k_vtk_encode(ctx._h, buf.data_ptr(), n, text.data_ptr(), len(want)))
    got = bytes(text.cpu().numpy())
    assert got[:len(want)] == want
    assert got[len(want):] == b"*" * 16  # nothing written behind the text


def test_encoder_all_byte_values_and_doubles(ctx):
    data = bytes(range(256)) * 3 + bytes(range(255, -1, -1))
    assert bytes(vtk.encode(ctx, torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()).cpu().numpy()) == expected_text(data)
    x = torch.as_tensor(np.random.default_rng(0).standard_normal(1001)).cuda()
    assert bytes(vtk.encode(ctx, x).cpu().numpy()) == expected_text(x.cpu().numpy().tobytes())


def test_encoder_past_one_sweep_of_its_grid(ctx):
    """8 MiB + 5 bytes: at 16 text bytes per lane one sweep of the largest grid (1024 workgroups of 256 lanes) covers 4 MiB of text"""
    n = (8 << 20) + 5
    data = np.random.default_rng(1).integers(0, 256, n, dtype=np.uint8)
    got = vtk.encode(ctx, torch.as_tensor(data).cuda()).cpu().numpy()
    want = np.frombuffer(expected_text(data.tobytes()), dtype=np.uint8)
    assert got.shape == want.shape and np.array_equal(got, want)


def test_encoder_refuses_a_small_buffer_and_misaligned_pointers(ctx):
    lib = capi.load()
    buf = torch.zeros(64, dtype=torch.uint8, device="cuda")
    text = torch.zeros(64, dtype=torch.uint8, device="cuda")
    need = len(expected_text(bytes(16)))
    assert lib.l3k_vtk_encode(ctx._h, buf.data_ptr(), 16, text.data_ptr(), need - 1) == -1
    assert f"{need} text bytes" in lib.l3k_last_error().decode()
    assert lib.l3k_vtk_encode(ctx._h, buf.data_ptr() + 4, 16, text.data_ptr(), need) == -1
    assert lib.l3k_vtk_encode(ctx._h, buf.data_ptr(), 16, text.data_ptr() + 8, need) == -1
    assert lib.l3k_vtk_encode(ctx._h, None, 16, text.data_ptr(), need) == -1
    torch.cuda.synchronize()
    assert not text.any()


# ------------------------------------------------------------------------------------------------------------------ whole files
def hexes(ne, p, perturb=0.1):
    return lambda: system.CubePartition(ne, p, perturb=perturb)


def quads(ne, p, perturb=0.1):
    return lambda: system.SquarePartition(ne, p, perturb=perturb)


MESHES = {
    "hex 3^3 p1": hexes(3, 1), "hex 3^3 p2": hexes(3, 2), "hex 3^3 p4": hexes(3, 4),
    "hex 2x1x1 p6": hexes((2, 1, 1), 6), "hex 2x1x1 p8": hexes((2, 1, 1), 8),
    "quad 3^2 p1": quads(3, 1), "quad 3^2 p2": quads(3, 2), "quad 3^2 p4": quads(3, 4), "quad 3^2 p8": quads(3, 8),
    "hex 11^3 p1": hexes(11, 1), "quad 33^2 p1": quads(33, 1),  # more elements than workgroups of one launch
}


def split_position(file_bytes, n_points):
    """(everything but the Position text, the decoded Position [n, 3])"""
    at = file_bytes.index(b'<AppendedData encoding="base64">\n  _') + len(b'<AppendedData encoding="base64">\n  _')
    first, count = R.position_span(n_points)
    text = file_bytes[at + first:at + first + count]
    raw = base64.b64decode(text)
    assert struct.unpack("<Q", raw[:8])[0] == 24 * n_points
    return file_bytes[:at + first] + file_bytes[at + first + count:], np.frombuffer(raw[8:], dtype="<f8").reshape(-1, 3)


@pytest.mark.parametrize("mesh", MESHES.keys())
def test_files_byte_for_byte(ctx, tmp_path, mesh):
    part = MESHES[mesh]()
    fields = host_fields(part)
    d_fields = torch.as_tensor(fields).cuda()
    dmesh = system.DeviceMesh(ctx, part, 1)
    files = {}
    for tag, chunk in (("default", 0), ("small", 4096)):
        exporter = vtk.PvtuExporter(dmesh, chunk_bytes=chunk)
        info = exporter.info()
        assert info["chunk_bytes"] % 16 == 0 and (chunk == 0 or info["chunk_bytes"] <= 4096)
        exporter.export_solution(definition(tmp_path / tag / "out.pvtu"), d_fields)
        assert sorted(os.listdir(tmp_path / tag)) == ["out.pvtu", "out_0.vtu"]
        files[tag] = ((tmp_path / tag / "out_0.vtu").read_bytes(), (tmp_path / tag / "out.pvtu").read_bytes())
    assert files["default"] == files["small"]  # the chunking leaves no trace
    vtu, pvtu = files["default"]
    assert pvtu == R.pvtu_bytes("out.pvtu", 1, GROUPS)
    coords = part.node_coords()
    got_rest, got_pos = split_position(vtu, part.n_local_nodes)
    want_rest, _ = split_position(R.vtu_bytes(part, GROUPS, fields, coords), part.n_local_nodes)
    assert got_rest == want_rest
    # Position: both sides are an 8-term sum of 3-factor products of values of at most max |vertex coordinate|
    scale = np.abs(part.elem_verts).max()
    err = np.abs(got_pos - coords).max()
    print(f"{mesh}: {len(vtu)} bytes, Position error {err:.2e} (bound {1e-14 * scale:.2e})")
    assert err <= 1e-14 * scale
    if part.dim == 2:
        assert np.array_equal(got_pos[:, 2].view(np.int64), np.zeros(part.n_local_nodes, np.int64))  # exactly +0.0


def test_many_chunks_on_a_tiny_mesh_and_two_creations(ctx, tmp_path):
    """chunk_bytes = 16 (and 1, which is raised to it): every array crosses many chunks, odd and even counts; two exporters created
    on one mesh give identical file bytes, Position included"""
    part = system.CubePartition((2, 1, 1), 2, perturb=0.1)
    d_fields = torch.as_tensor(host_fields(part)).cuda()
    dmesh = system.DeviceMesh(ctx, part, 1)
    out = []
    for i, chunk in enumerate((0, 0, 16, 1, 48, 4100)):
        exporter = vtk.PvtuExporter(dmesh, chunk_bytes=chunk)
        info = exporter.info()
        largest = (max(info["encoded_bytes"][:2]) + 15) // 16 * 16  # no chunk is larger than the largest array's text
        if chunk:  # rounded down to a multiple of 16, at least 16
            assert info["chunk_bytes"] == min(max(chunk // 16 * 16, 16), largest)
        else:
            assert info["chunk_bytes"] == largest  # (the default is far above this mesh's arrays)
        exporter.export_solution(definition(tmp_path / str(i) / "a.pvtu"), d_fields)
        exporter.export_solution(definition(tmp_path / str(i) / "b.pvtu"), d_fields)  # the exporter is reusable
        out.append((tmp_path / str(i) / "a_0.vtu").read_bytes())
        assert (tmp_path / str(i) / "b_0.vtu").read_bytes() == out[-1]
    assert all(o == out[0] for o in out)


# ------------------------------------------------------------------------------------------- not through the restatement
def test_linear_field_and_subcell_volumes(ctx, tmp_path):
    part = system.CubePartition(3, 4)
    xyz = part.node_coords()
    fields = np.zeros((2, part.n_local_nodes))
    fields[1] = xyz[:, 0] + 2 * xyz[:, 1] + 3 * xyz[:, 2]
    exporter = vtk.PvtuExporter(system.DeviceMesh(ctx, part, 1))
    exporter.export_solution(definition(tmp_path / "lin", [("f", [1])]), torch.as_tensor(fields).cuda())
    got = vtk.read_vtu(str(tmp_path / "lin_0.vtu"))
    pos = got["points"]
    assert np.abs(got["point_data"]["f"] - (pos[:, 0] + 2 * pos[:, 1] + 3 * pos[:, 2])).max() <= 1e-14
    assert np.array_equal(got["types"], np.full(27 * 64, 12, np.uint8))
    assert np.array_equal(got["offsets"], 8 * np.arange(1, 27 * 64 + 1))
    cells = pos[got["connectivity"].astype(np.int64).reshape(-1, 8)]  # [cell][VTK vertex][xyz]
    # VTK_HEXAHEDRON: 0-1-2-3 counter-clockwise seen from inside, 4-7 above them: volume of the (here axis-parallel) cell
    e1, e2, e3 = cells[:, 1] - cells[:, 0], cells[:, 3] - cells[:, 0], cells[:, 4] - cells[:, 0]
    vol = np.einsum("ci,ci->c", np.cross(e1, e2), e3)
    assert (vol > 0).all()
    assert np.allclose(cells[:, 2] - cells[:, 0], e1 + e2, atol=1e-14) and np.allclose(cells[:, 6] - cells[:, 0], e1 + e2 + e3, atol=1e-14)
    assert abs(vol.sum() - 1.0) <= 1e-13


def test_quad_subcells_are_counter_clockwise(ctx, tmp_path):
    part = system.SquarePartition(3, 4, perturb=0.1)
    exporter = vtk.PvtuExporter(system.DeviceMesh(ctx, part, 1))
    exporter.export_solution(definition(tmp_path / "q", []), torch.zeros((1, part.n_local_nodes), dtype=torch.float64, device="cuda"))
    got = vtk.read_vtu(str(tmp_path / "q_0.vtu"))
    c = got["points"][got["connectivity"].astype(np.int64).reshape(-1, 4)]
    area = 0.5 * sum(c[:, i, 0] * c[:, (i + 1) % 4, 1] - c[:, (i + 1) % 4, 0] * c[:, i, 1] for i in range(4))  # shoelace
    assert (area > 0).all() and abs(area.sum() - 1.0) <= 1e-13
    assert np.array_equal(got["types"], np.full(9 * 16, 9, np.uint8)) and got["point_data"] == {}


# ---------------------------------------------------------------------------------------------------------------- partition
def test_partition_with_ghost_nodes(ctx, tmp_path):
    groups = [("T", [0])]
    parts = [system.CubePartition((4, 2, 2), 2, parts=(2, 1, 1), rank=r) for r in range(2)]
    assert parts[1].n_ghost_nodes > 0
    for r, part in enumerate(parts):
        fields = host_fields(part, seed=r)
        exporter = vtk.PvtuExporter(system.DeviceMesh(ctx, part, 1), rank=r, world=2)
        exporter.export_solution(definition(tmp_path / f"rank{r}" / "part.pvtu", groups), torch.as_tensor(fields).cuda())
        want_files = ["part.pvtu", "part_0.vtu"] if r == 0 else ["part_1.vtu"]  # the .pvtu is rank 0's
        assert sorted(os.listdir(tmp_path / f"rank{r}")) == want_files
        got = vtk.read_vtu(str(tmp_path / f"rank{r}" / f"part_{r}.vtu"))
        assert got["n_points"] == part.n_owned_nodes + part.n_ghost_nodes == len(got["points"])
        assert got["connectivity"].max() < got["n_points"]
        assert np.array_equal(got["connectivity"], R.topology(part.elem_nodes, 3, 2)[0])
        assert np.array_equal(got["point_data"]["T"], fields[0, :part.n_local_nodes])
        assert np.abs(got["points"] - part.node_coords()).max() <= 1e-14
    pvtu = (tmp_path / "rank0" / "part.pvtu").read_bytes()
    assert pvtu == R.pvtu_bytes("part.pvtu", 2, groups)
    assert pvtu.count(b"<Piece Source=") == 2 and b'"part_0.vtu"' in pvtu and b'"part_1.vtu"' in pvtu


# ----------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_no_file(ctx, tmp_path):
    part = system.CubePartition(2, 2)
    n = part.n_local_nodes
    exporter = vtk.PvtuExporter(system.DeviceMesh(ctx, part, 1))
    fields = torch.zeros((3, n + 2), dtype=torch.float64, device="cuda")
    target = tmp_path / "refused"
    target.mkdir()
    name = target / "x.pvtu"
    cases = [
        ([("w", [])], fields, "Field groupings must have size 1 (scalar), 2 (2D), or 3 (3D)"),
        ([("w", [0, 1, 2, 0])], fields, "Field groupings must have size 1 (scalar), 2 (2D), or 3 (3D)"),
        ([("T", [0]), ("w", [1, 3])], fields, "Out of bounds index"),
        ([("T", [-1])], fields, "Out of bounds index"),
        ([("T", [0])], fields[:, :n - 1].contiguous(), "leading dimension"),
        ([("", [0])], fields, "name of field group 0"),
        ([("T", [0]), ('a"b', [1])], fields, "name of field group 1"),
        ([("a<b", [0])], fields, "name"), ([("a>b", [0])], fields, "name"), ([("a&b", [0])], fields, "name"),
    ]
    for groups, f, message in cases:
        with pytest.raises(system.L3KError, match=message.replace("(", r"\(").replace(")", r"\)")):
            exporter.export_solution(definition(name, groups), f)
    for rank, world in ((1, 1), (-1, 2), (0, 0)):
        bad = vtk.PvtuExporter(exporter.mesh, rank=rank, world=world)
        with pytest.raises(system.L3KError, match="outside \\[0, n_ranks"):
            bad.export_solution(definition(name, [("T", [0])]), fields)
    lib = capi.load()
    names, one = (C.c_char_p * 1)(b"T"), (C.c_int * 1)(1)
    zero = (C.c_int * 1)(0)
    assert lib.l3k_vtk_export(exporter._h, None, 0, 1, 1, names, one, zero, fields.data_ptr(), n + 2, 3) == -1
    assert lib.l3k_vtk_export(exporter._h, str(name).encode(), 0, 1, 1, names, one, zero, None, n + 2, 3) == -1
    assert lib.l3k_vtk_export(exporter._h, str(name).encode(), 0, 1, 1, None, one, zero, fields.data_ptr(), n + 2, 3) == -1
    assert os.listdir(target) == []
    # a path whose directory cannot be created: a regular file stands where the directory would be
    (target / "file").write_bytes(b"x")
    with pytest.raises(system.L3KError, match="cannot create the directory"):
        exporter.export_solution(definition(target / "file" / "sub" / "x.pvtu", [("T", [0])]), fields)
    assert os.listdir(target) == ["file"]
    # the exporter still works, and missing parent directories are created
    exporter.export_solution(definition(target / "a" / "b" / "x.pvtu", [("T", [0])]), fields)
    assert sorted(os.listdir(target / "a" / "b")) == ["x.pvtu", "x_0.vtu"]


# --------------------------------------------------------------------------------------------------------------- end to end
def test_diffusion2d_solution_end_to_end(ctx, tmp_path):
    """tests/Diffusion2D.hpp as tests/test_gpu_chol.py sets it up (4 x 4 quads of order 2, Dirichlet T = x left and right, adiabatic
    walls, direct solve), l3k_update_solution into the field storage, then T as a scalar and the flux as a 2-row group"""
    U = 3
    part = system.SquarePartition(4, 2)
    mesh = system.DeviceMesh(ctx, part, U, part.dirichlet_mask(U, sides=(2, 3)))
    n = part.n_local_nodes * U
    fe, fs = part.boundary_sides([2, 3])
    g = system.values_at_nodes(mesh, system.RESIDUAL_COORDX2D, [0], torch.zeros(n, dtype=torch.float64, device="cuda"), face_elem=fe,
                               face_side=fs)
    asm = system.AssembledSystem(mesh).begin()
    asm.add(system.MatrixFreeSystem(mesh, system.KERNEL_DIFFUSION2D))
    asm.add(system.BoundaryTerm(mesh, system.KERNEL_ADIABATIC2D, *part.boundary_sides([0, 1])))
    op = asm.end(g[None, :])
    x = solve.direct_solve(op, asm.rhs[0], torch.zeros(n, dtype=torch.float64, device="cuda"))
    fields = torch.zeros((U, part.n_local_nodes + 1), dtype=torch.float64, device="cuda")
    system.update_solution(mesh, x[None, :], [0, 1, 2], fields, [0, 1, 2])
    exporter = vtk.PvtuExporter(mesh)
    exporter.export_solution(definition(tmp_path / "diffusion.pvtu", [("T", [0]), ("flux", [1, 2])]), fields)
    got = vtk.read_vtu(str(tmp_path / "diffusion_0.vtu"))
    sol = x.cpu().numpy().reshape(-1, U)
    assert np.abs(sol[:, 0]).max() > 0.5  # (T = x reaches 1 on the right side)
    assert np.array_equal(got["point_data"]["T"].view(np.int64), sol[:, 0].view(np.int64))  # bit for bit
    assert np.array_equal(got["point_data"]["flux"][:, :2].view(np.int64), sol[:, 1:].copy().view(np.int64))
    assert np.array_equal(got["point_data"]["flux"][:, 2].view(np.int64), np.zeros(len(sol), np.int64))
    assert (got["scalars"], got["vectors"]) == ("T", "flux")
    assert np.abs(got["point_data"]["T"] - got["points"][:, 0]).max() < 1e-8  # the exact solution is T = x
    assert (tmp_path / "diffusion.pvtu").read_bytes() == R.pvtu_bytes("diffusion.pvtu", 1, [("T", [0]), ("flux", [1, 2])])
