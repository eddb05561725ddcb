"""Host restatements for the unstructured-mesh tests: which element side a boundary element is (a dictionary over vertex sets),
and a scrambler that hides the structure of a generated mesh (element order, vertex ids, local frames) while keeping track of
where every side went.  Side numbering as in include/l3k.h: hexes z-, z+, y-, y+, x-, x+ on local vertices v = i + 2j + 4k, quads
y-, y+, x-, x+ on v = i + 2j."""
import itertools

import numpy as np

# local vertices of every side, listed so that consecutive entries share an edge (a cycle around the side)
SIDE_VERTS = {
    2: ((0, 1), (2, 3), (0, 2), (1, 3)),
    3: ((0, 1, 3, 2), (4, 5, 7, 6), (0, 1, 5, 4), (2, 3, 7, 6), (0, 2, 6, 4), (1, 3, 7, 5)),
}


def match_by_dictionary(conn, bnd_conn):
    """The specification of l3k_boundary_match: frozenset(side vertices) -> the lowest (element, side) that has them.  Returns
    (face_elem int64, face_side uint8, n_unmatched, n_interior)."""
    conn = np.asarray(conn).astype(np.int64)
    dim = {4: 2, 8: 3}[conn.shape[1]]
    first, seen = {}, {}
    for e in range(conn.shape[0]):  # ascending (e, side): the first to arrive is the lowest
        for s, lv in enumerate(SIDE_VERTS[dim]):
            key = frozenset(conn[e, list(lv)].tolist())
            first.setdefault(key, (e, s))
            seen[key] = seen.get(key, 0) + 1
    fe, fs, n_unmatched, n_interior = [], [], 0, 0
    for b in np.asarray(bnd_conn).astype(np.int64).tolist():
        key = frozenset(b)
        if len(key) != len(b) or key not in first:
            fe.append(-1), fs.append(255)
            n_unmatched += 1
        else:
            fe.append(first[key][0]), fs.append(first[key][1])
            n_interior += seen[key] > 1
    return np.array(fe, dtype=np.int64), np.array(fs, dtype=np.uint8), n_unmatched, n_interior


def proper_symmetries(dim):
    """The orientation-preserving symmetries of the reference square (4) or cube (24) as permutations of the local vertices:
    the new local vertex v holds the old local vertex perm[v]."""
    perms = []
    for axes in itertools.permutations(range(dim)):
        for signs in itertools.product((-1, 1), repeat=dim):
            R = np.zeros((dim, dim), int)
            for r in range(dim):
                R[r, axes[r]] = signs[r]
            if round(np.linalg.det(R)) != 1:
                continue
            perm = []
            for v in range(2 ** dim):
                d = R @ np.array([2 * ((v >> a) & 1) - 1 for a in range(dim)])
                perm.append(int(sum((d[a] > 0) << a for a in range(dim))))
            perms.append(perm)
    assert len(perms) == {2: 4, 3: 24}[dim]
    return np.array(perms)


def scramble(conn, rng):
    """Permutes the elements, renumbers the vertices by a random permutation and re-orients every element by a random proper
    symmetry.  Returns (new_conn uint32, elem_of [n]: the old index of every new element, new_vertex [n_vertices]: the new id of
    every old vertex (ids up to conn.max()), side_map [n][2 dim]: the new side of every old side of the new element n)."""
    conn = np.asarray(conn).astype(np.int64)
    n, nv = conn.shape
    dim = {4: 2, 8: 3}[nv]
    sym = proper_symmetries(dim)
    elem_of = rng.permutation(n)
    new_vertex = rng.permutation(int(conn.max()) + 1)
    pick = sym[rng.integers(0, sym.shape[0], n)]
    new_conn = new_vertex[np.take_along_axis(conn[elem_of], pick, axis=1)]
    side_sets = [frozenset(lv) for lv in SIDE_VERTS[dim]]
    side_map = np.empty((n, 2 * dim), dtype=np.int64)
    for e in range(n):
        for s_old, old in enumerate(side_sets):
            now = frozenset(v for v in range(nv) if int(pick[e, v]) in old)  # the new local vertices that hold the old side's
            side_map[e, s_old] = side_sets.index(now)
    return new_conn.astype(np.uint32), elem_of, new_vertex, side_map


def boundary_of_structured(part, rng=None):
    """The boundary elements of a structured order-1 system.CubePartition / SquarePartition from its elem_boundary bits: (bnd_conn
    [m][2^(dim-1)] vertex ids, element [m], side [m]).  With rng every one is written from a random start, in a random direction
    around the side (quads: rotations and reflections of the four vertices; lines: either direction)."""
    dim = part.dim
    conn = part.elem_nodes.astype(np.int64)
    bc, be, bs = [], [], []
    for s, lv in enumerate(SIDE_VERTS[dim]):
        for e in np.nonzero(part.elem_boundary & (1 << s))[0]:
            cyc = conn[e, list(lv)]
            if rng is not None:
                cyc = np.roll(cyc[::-1] if rng.integers(2) else cyc, int(rng.integers(len(lv))))
            bc.append(cyc), be.append(int(e)), bs.append(s)
    return np.array(bc, dtype=np.uint32), np.array(be, dtype=np.int64), np.array(bs, dtype=np.int64)


def scrambled_structured(part, rng):
    """An order-1 structured mesh as an unstructured one: (verts [n][3], conn, bnd_conn, true_elem, true_side, cube_side [m]: the
    side of the cube / square every boundary element lies on)."""
    conn = part.elem_nodes.astype(np.int64)
    bnd, be, bs = boundary_of_structured(part, rng)
    new_conn, elem_of, new_vertex, side_map = scramble(conn, rng)
    new_elem = np.empty(conn.shape[0], dtype=np.int64)
    new_elem[elem_of] = np.arange(conn.shape[0])
    verts = np.empty((part.n_local_nodes, 3))
    verts[new_vertex] = part.node_coords()
    true_elem = new_elem[be]
    return verts, new_conn, new_vertex[bnd.astype(np.int64)].astype(np.uint32), true_elem, side_map[true_elem, bs].astype(np.uint8), bs
