"""Hexahedra of a gmsh 4.1 ASCII mesh file: vertex coordinates and the connectivity in the reference's local vertex order
v = i + 2j + 4k (mesh/ReadMesh.hpp reads gmsh 2.2 / 4.1 files and reorders the same way; only what the device path needs:
$Nodes and the type-5 blocks of $Elements -- lower-dimensional boundary elements are faces of the hexahedra and carry no
nodes of their own).  read_mesh reads quads or hexes together with their boundary elements and the physical ids of both."""
import collections

import numpy as np

# gmsh corner order of an 8-node hexahedron: bottom face counter-clockwise, then the top face -> lexicographic
GMSH_HEX_TO_LEX = (0, 1, 3, 2, 4, 5, 7, 6)


def read_hexes(path):
    """Returns (verts float64 [n][3], conn uint32 [n_hexes][8], entity int32 [n_hexes]: the volume entity tag of each hex)."""
    lines = open(path).read().split("\n")
    if "$MeshFormat" not in lines or not lines[lines.index("$MeshFormat") + 1].startswith("4.1 0"):
        raise ValueError("only gmsh 4.1 ASCII files are read")
    pos = lines.index("$Nodes") + 1
    n_blocks, n_nodes = (int(v) for v in lines[pos].split()[:2])
    pos += 1
    tags, xyz = [], []
    for _ in range(n_blocks):
        nb = int(lines[pos].split()[3])
        pos += 1
        tags += [int(lines[pos + i]) for i in range(nb)]
        xyz += [[float(v) for v in lines[pos + nb + i].split()[:3]] for i in range(nb)]
        pos += 2 * nb
    if len(tags) != n_nodes:
        raise ValueError("node count mismatch")
    index_of = {t: i for i, t in enumerate(tags)}
    pos = lines.index("$Elements") + 1
    n_blocks = int(lines[pos].split()[0])
    pos += 1
    conn, entity = [], []
    for _ in range(n_blocks):
        _, ent, etype, nb = (int(v) for v in lines[pos].split())
        pos += 1
        if etype == 5:
            for i in range(nb):
                v = [index_of[int(t)] for t in lines[pos + i].split()[1:9]]
                conn.append([v[g] for g in GMSH_HEX_TO_LEX])
                entity.append(ent)
        pos += nb
    return np.array(xyz, dtype=np.float64).reshape(-1, 3), np.array(conn, dtype=np.uint32).reshape(-1, 8), np.array(entity, dtype=np.int32)


# gmsh corner order of a 4-node quadrangle: counter-clockwise -> lexicographic v = i + 2j
GMSH_QUAD_TO_LEX = (0, 1, 3, 2)
# gmsh element type -> (dimension, nodes) of what is read; triangles (2), tets (4), prisms (6), ... are not
_ELEMENT_TYPES = {1: (1, 2), 3: (2, 4), 5: (3, 8)}

GmshMesh = collections.namedtuple("GmshMesh", "dim verts conn elem_domain bnd_conn bnd_id")
GmshMesh.__doc__ = """What read_mesh returns: dim, verts float64 [n][3], conn uint32 [n_elems][2^dim] (lexicographic local vertex
order), elem_domain int32 [n_elems] (physical id), bnd_conn uint32 [n_bnd][2^(dim-1)] (vertex ids of the dim-1 elements, in the
order and orientation of the file), bnd_id int32 [n_bnd] (physical id)."""


def _read_nodes(lines):
    pos = lines.index("$Nodes") + 1
    n_blocks, n_nodes = (int(v) for v in lines[pos].split()[:2])
    pos += 1
    tags, xyz = [], []
    for _ in range(n_blocks):
        nb = int(lines[pos].split()[3])
        pos += 1
        tags += [int(lines[pos + i]) for i in range(nb)]
        xyz += [[float(v) for v in lines[pos + nb + i].split()[:3]] for i in range(nb)]
        pos += 2 * nb
    if len(tags) != n_nodes:
        raise ValueError("node count mismatch")
    return {t: i for i, t in enumerate(tags)}, np.array(xyz, dtype=np.float64).reshape(-1, 3)


def _read_entities(lines):
    """{(entity dimension, entity tag): physical tag}; an entity without a physical tag is absent (mesh/ReadMesh.hpp:197-242)."""
    physical = {}
    if "$Entities" not in lines:
        return physical
    pos = lines.index("$Entities") + 1
    counts = [int(v) for v in lines[pos].split()]
    pos += 1
    for edim, n in enumerate(counts):
        for _ in range(n):
            tok = lines[pos].split()
            pos += 1
            at = 4 if edim == 0 else 7  # tag, then a point (x y z) or a bounding box (6 numbers)
            n_phys = int(tok[at])
            if n_phys > 1:
                raise ValueError(f"entity {int(tok[0])} of dimension {edim} has {n_phys} physical tags: at most one is read")
            if n_phys == 1:
                physical[(edim, int(tok[0]))] = int(tok[at + 1])
    return physical


def read_mesh(path):
    """The quadrilaterals or hexahedra of a gmsh 4.1 ASCII file with their boundary elements and physical ids, as
    mesh::readMesh(path, boundary_ids, gmsh_tag) reads them (mesh/ReadMesh.hpp:197-242 $Entities, :286-302 $Elements: the domain id
    of an element is the physical tag of its entity).  dim is the highest dimension that has elements; it must hold quads (dim 2) or
    hexes (dim 3) only; the elements of dimension dim - 1 are the boundary elements, lower ones are ignored.  Nothing is repaired
    beyond the reference's flip of clockwise planar quads: an element with a non-positive Jacobian is reported by the
    degenerate-element errors of the device path.  Returns a GmshMesh."""
    lines = [l.rstrip("\r") for l in open(path).read().split("\n")]
    if "$MeshFormat" not in lines or not lines[lines.index("$MeshFormat") + 1].startswith("4.1 0"):
        raise ValueError("only gmsh 4.1 ASCII files are read")
    physical = _read_entities(lines)
    index_of, verts = _read_nodes(lines)
    pos = lines.index("$Elements") + 1
    n_blocks = int(lines[pos].split()[0])
    pos += 1
    blocks = []  # (dimension, entity, type, first line, count)
    for _ in range(n_blocks):
        edim, ent, etype, nb = (int(v) for v in lines[pos].split())
        blocks.append((edim, ent, etype, pos + 1, nb))
        pos += 1 + nb
    with_elems = [b for b in blocks if b[4] > 0]
    if not with_elems:
        raise ValueError("the file holds no elements")
    dim = max(b[0] for b in with_elems)  # (an element has the dimension of its entity)
    if dim < 2:
        raise ValueError(f"the highest element dimension is {dim}: quads or hexes are needed")
    conn, elem_domain, bnd_conn, bnd_id = [], [], [], []
    to_lex = GMSH_QUAD_TO_LEX if dim == 2 else GMSH_HEX_TO_LEX
    for edim, ent, etype, first, nb in with_elems:
        if edim < dim - 1:
            continue
        if _ELEMENT_TYPES.get(etype, (None,))[0] != edim:
            raise ValueError(f"gmsh element type {etype} in dimension {edim} of a {dim}-D mesh: only lines (1), quads (3) and "
                             "hexes (5) are read")
        if (edim, ent) not in physical:
            raise ValueError(f"entity {ent} of dimension {edim} has elements but no physical tag")
        nn = _ELEMENT_TYPES[etype][1]
        for i in range(nb):
            v = [index_of[int(t)] for t in lines[first + i].split()[1:1 + nn]]
            if edim == dim:
                conn.append([v[g] for g in to_lex])
                elem_domain.append(physical[(edim, ent)])
            else:
                bnd_conn.append(v)
                bnd_id.append(physical[(edim, ent)])
    conn = np.array(conn, dtype=np.uint32).reshape(-1, 2 ** dim)
    if dim == 2:
        # gmsh writes the quads of a surface whose normal points down clockwise: the reference flips a quad that lies in a plane
        # z = const and has a negative normal by swapping its local vertices 1 and 2 (mesh/ReadMesh.hpp:70-90); nothing else is touched
        c = verts[conn.astype(np.int64)]
        flat = np.all(np.abs(c[:, 1:, 2] - c[:, :1, 2]) < 1e-9, axis=1)
        u, v = c[:, 1] - c[:, 0], c[:, 2] - c[:, 0]
        flip = flat & (u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0] < 0.)
        conn[flip] = conn[flip][:, [0, 2, 1, 3]]
    return GmshMesh(dim, verts, conn, np.array(elem_domain, dtype=np.int32),
                    np.array(bnd_conn, dtype=np.uint32).reshape(-1, 2 ** (dim - 1)), np.array(bnd_id, dtype=np.int32))
