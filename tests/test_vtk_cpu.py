"""The host side of the ParaView export without a device: l3k_vtk_sizes and its 2^32 guard, the .pvtu / .vtu XML text byte for byte
against the restatement of tests/vtk_ref.py, the refusals that need no device, vtk.read_vtu on a file the restatement wrote, and
host/vtk_text.cpp under ASan + UBSan in a stand-alone driver (tests/sanitize/vtk_text_driver.cpp)."""
import ctypes as C
import os
import shutil
import subprocess
import xml.etree.ElementTree as ET

import numpy as np
import pytest

import vtk_ref as R
from l3ster_amd import capi, system, vtk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT = 2 ** 32 - 1

GROUP_SETS = {
    "one scalar": [("T", [0])],
    "one 2-row group": [("flux", [1, 2])],
    "scalar + vector": [("T", [0]), ("velocity", [3, 1, 2])],
    "vector + scalar": [("velocity", [3, 1, 2]), ("T", [0])],
    "two vectors": [("flux", [1, 2]), ("velocity", [3, 1, 2])],
}
FILE_NAMES = ["res.pvtu", "res", "out/dir.d/res.pvtu", "out/dir.d/res", "out/res.step.7"]


def definition(file_name, groups):
    d = vtk.ExportDefinition(file_name)
    for name, inds in groups:
        d.define_field(name, inds)
    return d


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("order", [1, 2, 4, 6, 8])
def test_sizes_match_the_restatement(dim, order):
    part = system.SquarePartition((3, 2), order) if dim == 2 else system.CubePartition((2, 1, 2), order)
    info = vtk.sizes(dim, order, part.n_elems, part.n_local_nodes)
    conn, offsets, types = R.topology(part.elem_nodes, dim, order)
    raw = [24 * part.n_local_nodes, conn.nbytes, offsets.nbytes, types.nbytes]
    assert (info["n_points"], info["n_cells"], info["n_conn"]) == (part.n_local_nodes, len(types), len(conn))
    assert info["raw_bytes"] == raw
    assert info["encoded_bytes"] == [len(R.encoded(bytes(n))) for n in raw] == [R.encoded_len(n) for n in raw]
    assert np.array_equal(offsets[:2], [2 ** dim, 2 * 2 ** dim][:len(offsets)]) and conn.max() < part.n_local_nodes


@pytest.mark.parametrize("dim,order", [(2, 1), (2, 8), (3, 1), (3, 3), (3, 8)])
def test_uint32_guard_on_both_counts(dim, order):
    per_elem = (2 * order) ** dim
    most = LIMIT // per_elem  # the most elements whose connectivity a UInt32 array can index
    info = vtk.sizes(dim, order, most, LIMIT)
    assert info["n_conn"] == most * per_elem <= LIMIT and info["n_points"] == LIMIT
    with pytest.raises(system.L3KError, match=rf"1 local nodes and {(most + 1) * per_elem} connectivity entries"):
        vtk.sizes(dim, order, most + 1, 1)
    with pytest.raises(system.L3KError, match=rf"{LIMIT + 1} local nodes and {per_elem} connectivity entries"):
        vtk.sizes(dim, order, 1, LIMIT + 1)


@pytest.mark.parametrize("groups", GROUP_SETS.values(), ids=GROUP_SETS.keys())
@pytest.mark.parametrize("n_ranks", [1, 3])
@pytest.mark.parametrize("file_name", FILE_NAMES)
def test_pvtu_text_byte_for_byte(groups, n_ranks, file_name):
    text = vtk.pvtu_text(definition(file_name, groups), n_ranks)
    assert text == R.pvtu_bytes(file_name, n_ranks, groups)
    root = ET.fromstring(text)  # well-formed, and the pieces carry no directory
    pieces = [p.get("Source") for p in root.iter("Piece")]
    assert len(pieces) == n_ranks and all("/" not in p for p in pieces)


@pytest.mark.parametrize("groups", GROUP_SETS.values(), ids=GROUP_SETS.keys())
def test_vtu_header_text_byte_for_byte(groups):
    n_points, n_cells = 1234567, 7654321
    lens = [R.encoded_len(24 * n_points), R.encoded_len(32 * n_cells), R.encoded_len(4 * n_cells), R.encoded_len(n_cells)]
    text = vtk.vtu_header_text(definition("x", groups), n_points, n_cells, lens)
    assert text == R.vtu_header(n_points, n_cells, lens, groups)


def test_both_files_name_the_same_active_arrays():
    """Scalars in front of Vectors, the first of each kind, in the .vtu and the .pvtu alike (the reference's .pvtu labels a second
    vector group as Scalars when there is no scalar group: not reproduced)"""
    for groups in GROUP_SETS.values():
        d = definition("x", groups)
        want = R.active_arrays(groups).encode()
        assert b"<PPointData" + want + b">" in vtk.pvtu_text(d, 2)
        assert b"<PointData" + want + b">" in vtk.vtu_header_text(d, 1, 1, [1, 1, 1, 1])
    assert R.active_arrays(GROUP_SETS["two vectors"]) == ' Vectors="flux"'
    assert R.active_arrays(GROUP_SETS["vector + scalar"]) == ' Scalars="T" Vectors="velocity"'


def test_file_names():
    assert R.vtu_name("out/dir.d/res.pvtu", 3) == "out/dir.d/res_3.vtu" and R.pvtu_name("out/dir.d/res") == "out/dir.d/res.pvtu"
    assert R.vtu_name("out/res.step.7", 0) == "out/res.step_0.vtu"


def test_refusals_without_a_device():
    lib = capi.load()
    names = (C.c_char_p * 2)(b"T", b"v")
    need = C.c_size_t()

    def pvtu(names=names, n_comps=(1, 3), n_ranks=1, path=b"x"):
        return lib.l3k_vtk_pvtu_text(path, n_ranks, 2, names, (C.c_int * 2)(*n_comps), None, 0, C.byref(need))

    assert pvtu() == 0 and need.value > 0
    for n_comps in [(0, 1), (1, 4), (-1, 1)]:
        assert pvtu(n_comps=n_comps) == -1
        assert "Field groupings must have size 1 (scalar), 2 (2D), or 3 (3D)" in lib.l3k_last_error().decode()
    for bad in [b"", b'a"b', b"a<b", b"a>b", b"a&b"]:
        assert pvtu(names=(C.c_char_p * 2)(b"T", bad)) == -1
        assert "name of field group 1" in lib.l3k_last_error().decode()
    assert pvtu(n_ranks=0) == -1 and "outside [0, n_ranks" in lib.l3k_last_error().decode()
    assert pvtu(path=None) == -1 and pvtu(names=None) == -1
    assert lib.l3k_vtk_pvtu_text(b"x", 1, 2, names, (C.c_int * 2)(1, 3), None, 0, None) == -1
    # a buffer one byte short is refused and left alone
    buf = C.create_string_buffer(b"\xaa" * need.value, need.value)
    assert lib.l3k_vtk_pvtu_text(b"x", 1, 2, names, (C.c_int * 2)(1, 3), buf, need.value - 1, None) == -1
    assert buf.raw == b"\xaa" * need.value
    assert lib.l3k_vtk_sizes(3, 2, 1, 1, None) == -1
    for args in [(1, 2, 1, 1), (4, 2, 1, 1), (3, 0, 1, 1), (3, 9, 1, 1), (3, 2, -1, 1), (3, 2, 1, -1)]:
        assert lib.l3k_vtk_sizes(*args, C.byref(capi.VtkInfo())) == -1, args
    # the device entry points refuse null handles before they touch a device
    out = C.c_void_p()
    assert lib.l3k_vtk_create(None, None, C.byref(out)) == -1 and out.value is None
    assert lib.l3k_vtk_export(None, b"x", 0, 1, 0, None, None, None, None, 0, 0) == -1
    assert lib.l3k_vtk_encode(None, None, 0, None, 0) == -1
    assert lib.l3k_vtk_info_get(None, None) == -1 and lib.l3k_vtk_destroy(None) == 0


@pytest.mark.parametrize("dim", [2, 3])
def test_read_vtu_round_trips_a_restated_file(tmp_path, dim):
    part = system.SquarePartition(3, 2, perturb=0.1) if dim == 2 else system.CubePartition(2, 3, perturb=0.1)
    rng = np.random.default_rng(5)
    fields = rng.standard_normal((4, part.n_local_nodes + 3))
    groups = [("T", [2]), ("flux", [3, 0]), ("velocity", [1, 3, 0])]
    path = tmp_path / "restated_0.vtu"
    path.write_bytes(R.vtu_bytes(part, groups, fields))
    got = vtk.read_vtu(str(path))
    conn, offsets, types = R.topology(part.elem_nodes, dim, part.order)
    assert got["n_points"] == part.n_local_nodes and got["n_cells"] == len(types)
    assert np.array_equal(got["points"], part.node_coords())
    assert np.array_equal(got["connectivity"], conn) and got["connectivity"].dtype == np.uint32
    assert np.array_equal(got["offsets"], offsets) and np.array_equal(got["types"], types) and got["types"].dtype == np.uint8
    n = part.n_local_nodes
    assert np.array_equal(got["point_data"]["T"], fields[2, :n])
    assert np.array_equal(got["point_data"]["flux"], np.stack([fields[3, :n], fields[0, :n], np.zeros(n)], axis=1))
    assert not np.signbit(got["point_data"]["flux"][:, 2]).any()
    assert np.array_equal(got["point_data"]["velocity"], fields[[1, 3, 0], :n].T)
    assert (got["scalars"], got["vectors"]) == ("T", "flux")


def test_vtk_text_under_asan_and_ubsan(tmp_path):
    """host/vtk_text.cpp in a stand-alone program of its own (nothing is loaded into Python under a sanitizer)"""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "vtk_text_driver")
    build = subprocess.run([cxx, "-std=c++20", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-Iinclude", "-Il3ster_amd/csrc", "tests/sanitize/vtk_text_driver.cpp",
                            "l3ster_amd/csrc/host/vtk_text.cpp", "-o", exe], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout + r.stderr[-4000:]
    assert "vtk text driver: ok" in r.stdout
    for word in ("ERROR: AddressSanitizer", "runtime error:", "ERROR: LeakSanitizer"):
        assert word not in r.stderr, r.stderr[-4000:]
