"""Host restatements for the periodic-boundary tests (numpy only): the all-pairs node match with exactly the rule of
l3k_periodic_match, the union-by-lowest-id merge with compaction of l3k_periodic_merge, and the prolongation P between the merged
and the unmerged numbering (x_un[old] = x_m[node_map[old]] per dof)."""
import numpy as np


def side_nodes(dim, order):
    """[2 dim][(order+1)^(dim-1)] element-local nodes of every side (the last axis first, low side before high side)."""
    n = order + 1
    idx = np.arange(n ** dim).reshape((n,) * dim)
    return np.stack([np.take(idx, at, axis=axis).reshape(-1) for axis in range(dim) for at in (0, order)])


def gll(n):
    """The n Gauss-Lobatto-Legendre points: -1, 1 and the roots of P'_{n-1}."""
    if n == 2:
        return np.array([-1.0, 1.0])
    d = np.polynomial.legendre.Legendre.basis(n - 1).deriv()
    inner = np.sort(d.roots().real)
    inner = inner - d(inner) / d.deriv()(inner)  # one Newton step takes the companion-matrix roots to a few ulp
    return np.concatenate([[-1.0], inner, [1.0]])


def side_node_locations(mesh, face_elem, face_side):
    """(ids int64 [m] ascending, loc [m][3]) of the unique nodes of the listed sides: the bi-/tri-linear image of the element's
    vertices at the GLL position, from the first side that lists the node; z = 0 on quads."""
    dim, n = mesh.dim, mesh.order + 1
    g = gll(n)
    l = np.stack([(1 - g) / 2, (1 + g) / 2], axis=1)
    if dim == 2:
        shape = np.einsum("xi,yj->yxji", l, l).reshape(n ** 2, 4)
    else:
        shape = np.einsum("xi,yj,zk->zyxkji", l, l, l).reshape(n ** 3, 8)
    sn = side_nodes(dim, mesh.order)
    ids, loc = [], []
    for e, s in zip(np.asarray(face_elem).tolist(), np.asarray(face_side).tolist()):
        ids.append(mesh.elem_nodes[e, sn[s]].astype(np.int64))
        loc.append(shape[sn[s]] @ mesh.elem_verts[e])
    if not ids:
        return np.zeros(0, np.int64), np.zeros((0, 3))
    ids, loc = np.concatenate(ids), np.concatenate(loc)
    if dim == 2:
        loc[:, 2] = 0.0
    uniq, first = np.unique(ids, return_index=True)
    return uniq, loc[first]


def brute_force_match(mesh, src, dst, translation, tolerance=1e-12):
    """Every source node against every destination node: s matches d iff |x_s + t - x_d| < tolerance (strict); the nearest wins, ties
    to the lowest id; pairs with s == d are dropped.  Returns (pair_src, pair_dst uint32, n_unmatched, n_ambiguous, first_unmatched)."""
    s_id, s_loc = side_node_locations(mesh, *src)
    d_id, d_loc = side_node_locations(mesh, *dst)
    t = np.zeros(3)
    t[:mesh.dim] = np.asarray(translation, dtype=np.float64).reshape(-1)[:mesh.dim]
    ps, pd, n_unmatched, n_ambiguous, first = [], [], 0, 0, -1
    for s, x in zip(s_id.tolist(), s_loc + t):
        dist = np.sqrt(((x[None, :] - d_loc) ** 2).sum(axis=1)) if d_id.size else np.zeros(0)
        ok = np.nonzero(dist < tolerance)[0]
        if ok.size == 0:
            first = s if n_unmatched == 0 else first
            n_unmatched += 1
            continue
        n_ambiguous += ok.size > 1
        best = ok[np.lexsort((d_id[ok], dist[ok]))[0]]  # by distance, then by id
        if int(d_id[best]) != s:
            ps.append(s), pd.append(int(d_id[best]))
    return np.array(ps, dtype=np.uint32), np.array(pd, dtype=np.uint32), n_unmatched, n_ambiguous, first


def merge(elem_nodes, n_nodes, n_noninternal, pair_a, pair_b):
    """Connected components of the pair graph by relabelling to the lowest id until nothing changes; node_map[old] = rank of old's
    representative among the kept nodes in ascending old id.  Returns (new elem_nodes uint32, node_map uint32, n_nodes,
    n_noninternal, n_components: the components of two nodes or more)."""
    a = np.asarray(pair_a, dtype=np.int64).reshape(-1)
    b = np.asarray(pair_b, dtype=np.int64).reshape(-1)
    rep = np.arange(n_nodes, dtype=np.int64)
    while True:
        low = np.minimum(rep[a], rep[b])
        new = rep.copy()
        np.minimum.at(new, a, low)
        np.minimum.at(new, b, low)
        new = new[new]  # (pointer jumping)
        if np.array_equal(new, rep):
            break
        rep = new
    kept = rep == np.arange(n_nodes)
    rank = np.cumsum(kept) - 1
    node_map = rank[rep]
    n_out = int(kept.sum())
    n_components = int(np.unique(rep[~kept]).size)
    return (node_map[np.asarray(elem_nodes).astype(np.int64)].astype(np.uint32), node_map.astype(np.uint32), n_out,
            n_noninternal - (n_nodes - n_out), n_components)


def internal_local_nodes(dim, order):
    """element-local indices of the element-internal nodes (every index in 1 .. order - 1), ascending"""
    n = order + 1
    idx = np.arange(n ** dim)
    inner = np.ones(n ** dim, dtype=bool)
    for a in range(dim):
        c = (idx // n ** a) % n
        inner &= (c >= 1) & (c <= order - 1)
    return idx[inner]


def check_numbering(elem_nodes, n_nodes, n_noninternal, dim, order, old_elem_nodes=None):
    """The numbering class l3k_mesh_create, the condensation and PartitionedMesh rely on: ids compact; every non-internal id below
    every internal id; each element's internal ids contiguous, in the element order and (with old_elem_nodes) in the old order."""
    en = np.asarray(elem_nodes).astype(np.int64)
    inner = internal_local_nodes(dim, order)
    outer = np.setdiff1d(np.arange(en.shape[1]), inner)
    assert np.array_equal(np.unique(en), np.arange(n_nodes))
    assert en[:, outer].max() < n_noninternal
    m = inner.size
    if m:
        assert np.array_equal(en[:, inner], n_noninternal + np.arange(en.shape[0])[:, None] * m + np.arange(m)[None, :])
        if old_elem_nodes is not None:
            old = np.asarray(old_elem_nodes).astype(np.int64)[:, inner]
            assert np.array_equal(np.argsort(old.ravel(), kind="stable"), np.argsort(en[:, inner].ravel(), kind="stable"))
    assert n_noninternal + en.shape[0] * m == n_nodes


def prolong(node_map, x_m, dofs_per_node):
    """P x_m: the merged vector [..., n_merged * dofs_per_node] on the unmerged numbering"""
    nm = np.asarray(node_map).astype(np.int64)
    x = np.asarray(x_m)
    return x.reshape(*x.shape[:-1], -1, dofs_per_node)[..., nm, :].reshape(*x.shape[:-1], -1)


def restrict(node_map, y_un, dofs_per_node, n_merged):
    """P^T y_un: the rows of the images of a merged node summed"""
    nm = np.asarray(node_map).astype(np.int64)
    y = np.asarray(y_un)
    y = y.reshape(*y.shape[:-1], -1, dofs_per_node)
    out = np.zeros(y.shape[:-2] + (n_merged, dofs_per_node))
    np.add.at(out, (Ellipsis, nm, slice(None)), y)
    return out.reshape(*y.shape[:-2], -1)
