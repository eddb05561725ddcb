"""gmsh.read_mesh: quads / hexes with their boundary elements and physical ids (mesh::readMesh, mesh/ReadMesh.hpp:197-242,286-302)
against the reference's own answers for its square file (tests/MeshTests.cpp:19-41), an independent parse of the multi-domain
file, the refusals, read_hexes; and partition.local_sides on stand-in parts.  No device."""
import os
from types import SimpleNamespace

import numpy as np
import pytest

from l3ster_amd import gmsh, partition

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SQUARE = os.path.join(GOLDEN, "gmsh_ascii4_square.msh")
MULTIDOM = os.path.join(GOLDEN, "gmsh_ascii4_square_multidom.msh")


def test_square_file_gives_the_reference_answers():
    m = gmsh.read_mesh(SQUARE)
    assert m.dim == 2
    assert m.verts.shape == (121, 3) and m.conn.shape == (100, 4) and m.conn.dtype == np.uint32  # MeshTests.cpp:24-35
    assert int(m.conn.max()) + 1 == 121
    ids, counts = np.unique(m.bnd_id, return_counts=True)
    assert ids.tolist() == [2, 3, 4, 5] and counts.tolist() == [10] * 4  # :37-41
    assert m.bnd_conn.shape == (40, 2) and m.bnd_id.dtype == np.int32
    assert np.unique(m.elem_domain).size == 1 and m.elem_domain.dtype == np.int32
    c = m.verts[m.conn.astype(np.int64)]  # v = i + 2j: the signed area of both corner triangles
    cross = lambda a, b: a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]  # noqa: E731
    assert np.all(cross(c[:, 1] - c[:, 0], c[:, 2] - c[:, 0]) > 0) and np.all(cross(c[:, 2] - c[:, 3], c[:, 1] - c[:, 3]) > 0)
    # every boundary line is an edge of exactly one quad
    edges = {}
    for q in m.conn.astype(np.int64):
        for a, b in ((0, 1), (2, 3), (0, 2), (1, 3)):
            key = frozenset((int(q[a]), int(q[b])))
            edges[key] = edges.get(key, 0) + 1
    assert all(edges.get(frozenset(l), 0) == 1 for l in m.bnd_conn.astype(np.int64).tolist())


def test_multi_domain_file_against_a_direct_parse():
    lines = open(MULTIDOM).read().split("\n")
    at = lines.index("$Entities")
    n_pts, n_curves, n_surfs, _ = (int(v) for v in lines[at + 1].split())
    surf_tag = {}
    for l in lines[at + 2 + n_pts + n_curves: at + 2 + n_pts + n_curves + n_surfs]:
        tok = l.split()
        assert int(tok[7]) == 1
        surf_tag[int(tok[0])] = int(tok[8])
    at = lines.index("$Elements")
    want, pos = {}, at + 2
    for _ in range(int(lines[at + 1].split()[0])):
        edim, ent, etype, nb = (int(v) for v in lines[pos].split())
        assert (edim, etype) == (2, 3)
        want[surf_tag[ent]] = want.get(surf_tag[ent], 0) + nb
        pos += 1 + nb
    m = gmsh.read_mesh(MULTIDOM)
    ids, counts = np.unique(m.elem_domain, return_counts=True)
    assert dict(zip(ids.tolist(), counts.tolist())) == want and len(want) == 4
    assert m.dim == 2 and m.conn.shape == (16, 4) and m.bnd_conn.shape == (0, 2) and m.bnd_id.shape == (0,)


HEADER = "$MeshFormat\n4.1 0 8\n$EndMeshFormat\n"
TRI_NODES = "$Nodes\n1 3 1 3\n2 1 0 3\n1\n2\n3\n0 0 0\n1 0 0\n0 1 0\n$EndNodes\n"
QUAD_NODES = "$Nodes\n1 4 1 4\n2 1 0 4\n1\n2\n3\n4\n0 0 0\n1 0 0\n1 1 0\n0 1 0\n$EndNodes\n"
QUAD_ELEMS = "$Elements\n1 1 1 1\n2 1 3 1\n1 1 2 3 4\n$EndElements\n"


def surface_entity(phys):
    return "$Entities\n0 0 1 0\n1 0 0 0 1 1 0 " + phys + " 0\n$EndEntities\n"


@pytest.mark.parametrize("name,text,match", [
    ("v22", "$MeshFormat\n2.2 0 8\n$EndMeshFormat\n$Nodes\n1\n1 0 0 0\n$EndNodes\n$Elements\n0\n$EndElements\n", "4.1 ASCII"),
    ("triangle", HEADER + surface_entity("1 7") + TRI_NODES + "$Elements\n1 1 1 1\n2 1 2 1\n1 1 2 3\n$EndElements\n", "element type 2"),
    ("two_tags", HEADER + surface_entity("2 7 8") + QUAD_NODES + QUAD_ELEMS, "2 physical tags"),
    ("no_tag", HEADER + surface_entity("0") + QUAD_NODES + QUAD_ELEMS, "entity 1 of dimension 2"),
])
def test_refusals(tmp_path, name, text, match):
    path = tmp_path / (name + ".msh")
    path.write_text(text)
    with pytest.raises(ValueError, match=match):
        gmsh.read_mesh(str(path))


def test_a_single_quad_is_read(tmp_path):
    """(the accepted twin of the refusal inputs: the same strings with one physical tag)"""
    path = tmp_path / "quad.msh"
    path.write_text(HEADER + surface_entity("1 7") + QUAD_NODES + QUAD_ELEMS)
    m = gmsh.read_mesh(str(path))
    assert m.conn.tolist() == [[0, 1, 3, 2]] and m.elem_domain.tolist() == [7] and m.bnd_conn.shape == (0, 2)


def write_hex_file(path):
    """Two stacked unit cubes with gmsh tags in a shuffled order, volume entity 4 -> physical 9, and the bottom quad (surface entity 2
    -> physical 3) and one line (no surface of a hex mesh: ignored) as lower-dimensional elements."""
    pts = [(i, j, k) for k in range(3) for j in range(2) for i in range(2)]
    tags = [12, 3, 7, 1, 9, 4, 10, 2, 6, 11, 5, 8]
    tag = {p: t for p, t in zip(pts, tags)}
    gm = lambda k: [tag[(0, 0, k)], tag[(1, 0, k)], tag[(1, 1, k)], tag[(0, 1, k)]]  # noqa: E731  (counter-clockwise)
    text = HEADER + "$Entities\n0 1 1 1\n5 0 0 0 1 0 0 1 1 0\n2 0 0 0 1 1 0 1 3 0\n4 0 0 0 1 1 2 1 9 0\n$EndEntities\n"
    text += "$Nodes\n1 12 1 12\n3 4 0 12\n" + "\n".join(str(t) for t in tags) + "\n" + "\n".join("%g %g %g" % p for p in pts) + "\n$EndNodes\n"
    text += "$Elements\n3 4 1 4\n1 5 1 1\n1 %d %d\n" % (tag[(0, 0, 0)], tag[(1, 0, 0)])
    text += "2 2 3 1\n2 " + " ".join(str(t) for t in gm(0)) + "\n"
    text += "3 4 5 2\n3 " + " ".join(str(t) for t in gm(0) + gm(1)) + "\n4 " + " ".join(str(t) for t in gm(1) + gm(2)) + "\n$EndElements\n"
    open(path, "w").write(text)
    return pts, tag, tags


def test_read_mesh_agrees_with_read_hexes(tmp_path):
    path = str(tmp_path / "hexes.msh")
    pts, tag, tags = write_hex_file(path)
    verts, conn, entity = gmsh.read_hexes(path)
    m = gmsh.read_mesh(path)
    assert m.dim == 3
    assert np.array_equal(m.verts, verts) and np.array_equal(m.conn, conn) and m.conn.dtype == conn.dtype
    assert entity.tolist() == [4, 4] and m.elem_domain.tolist() == [9, 9]  # the physical id, not the entity tag
    index = {t: i for i, t in enumerate(tags)}
    assert m.bnd_conn.tolist() == [[index[tag[p]] for p in ((0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0))]] and m.bnd_id.tolist() == [3]
    # lexicographic local vertices: vertex i + 2j + 4k of the first hex sits at (i, j, k)
    assert np.array_equal(verts[conn[0].astype(np.int64)], np.array([(i, j, k) for k in range(2) for j in range(2) for i in range(2)], float))


def test_local_sides_split_the_sides_among_the_parts():
    rng = np.random.default_rng(5)
    n_elems, world = 40, 3
    owner = rng.integers(0, world, n_elems)
    parts = [SimpleNamespace(elem_global=rng.permutation(np.nonzero(owner == r)[0])) for r in range(world)]
    fe = rng.integers(0, n_elems, 60).astype(np.int64)  # several sides of one element, elements without sides
    fs = rng.integers(0, 6, 60).astype(np.uint8)
    back = []
    for part in parts:
        le, ls = partition.local_sides(part, fe, fs)
        assert le.dtype == np.int64 and ls.dtype == np.uint8 and le.shape == ls.shape
        assert np.all((le >= 0) & (le < part.elem_global.size))  # local indices
        mine = np.isin(fe, part.elem_global)
        assert np.array_equal(part.elem_global[le], fe[mine]) and np.array_equal(ls, fs[mine])  # mapped back, input order kept
        back += list(zip(part.elem_global[le].tolist(), ls.tolist()))
    assert sorted(back) == sorted(zip(fe.tolist(), fs.tolist()))  # the union is the input, each side once
    le, ls = partition.local_sides(SimpleNamespace(elem_global=np.zeros(0, np.int64)), fe, fs)  # a rank without elements
    assert le.size == 0 and ls.size == 0
