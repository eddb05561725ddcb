"""Static condensation on the host (no GPU): the element-boundary / element-internal node split, the condensed CSR graph, and
the identity the device path relies on -- internal dofs are never shared between elements, so the Schur complement of the
assembled global matrix over ALL internal dofs equals the sum of the element Schur complements scattered over the primary dofs
(StaticCondensationManager.hpp:322-408: condenseSystem per element, endAssembly sums)."""
import numpy as np
import pytest

import oracle_lib as O
from l3ster_amd import system

COUNTS = {1: (8, 0), 2: (26, 1), 3: (56, 8), 4: (98, 27), 5: (152, 64), 6: (218, 125), 7: (296, 216), 8: (386, 343)}


@pytest.mark.parametrize("p", range(1, 9))
def test_element_node_split(p):
    primary, internal = system.element_node_split(p)
    n = p + 1
    assert (len(primary), len(internal)) == COUNTS[p]
    assert len(primary) == n ** 3 - (p - 1) ** 3 and len(internal) == (p - 1) ** 3
    assert np.all(np.diff(primary) > 0) and np.all(np.diff(internal) > 0)
    assert len(np.intersect1d(primary, internal)) == 0
    assert np.array_equal(np.union1d(primary, internal), np.arange(n ** 3))
    ix, iy, iz = internal % n, (internal // n) % n, internal // (n * n)
    assert np.all((ix >= 1) & (ix <= p - 1) & (iy >= 1) & (iy <= p - 1) & (iz >= 1) & (iz <= p - 1))
    jx, jy, jz = primary % n, (primary // n) % n, primary // (n * n)
    assert np.all((jx == 0) | (jx == p) | (jy == 0) | (jy == p) | (jz == 0) | (jz == p))
    # (dofs at U = 4, as the issue's table states them)
    assert 4 * len(primary) == {1: 32, 2: 104, 3: 224, 4: 392, 5: 608, 6: 872, 7: 1184, 8: 1544}[p]


def _scipy_graph(part, p, dpn, field_inds):
    import scipy.sparse as sp
    primary, _ = system.element_node_split(p)
    dofs = (part.elem_nodes.astype(np.int64)[:, primary][:, :, None] * dpn + np.asarray(field_inds)[None, None, :])
    dofs = dofs.reshape(part.n_elems, -1)
    nd = dofs.shape[1]
    rows, cols = np.repeat(dofs, nd, axis=1).ravel(), np.tile(dofs, (1, nd)).ravel()
    n = part.n_local_nodes * dpn
    G = sp.coo_matrix((np.ones(len(rows)), (rows, cols)), shape=(n, n)).tocsr()
    G.sort_indices()
    return G.indptr.astype(np.int64), G.indices.astype(np.int32)


@pytest.mark.parametrize("ne,p,dpn,fi", [(2, 2, 4, [0, 1, 2, 3]), ((3, 2, 1), 3, 5, [0, 2, 3]), (2, 4, 1, [0]), (2, 1, 2, [1, 0])])
def test_condensed_graph_matches_scipy(ne, p, dpn, fi):
    part = system.CubePartition(ne, p)
    rp, ci = system.condensed_graph(part.elem_nodes, p, dpn, fi)
    rp_ref, ci_ref = _scipy_graph(part, p, dpn, fi)
    assert rp.dtype == np.int64 and ci.dtype == np.int32
    assert np.array_equal(rp, rp_ref) and np.array_equal(ci, ci_ref)
    _, internal = system.element_node_split(p)
    inner_rows = (part.elem_nodes[:, internal].astype(np.int64)[:, :, None] * dpn + np.asarray(fi)).ravel()
    assert np.all(rp[inner_rows + 1] == rp[inner_rows])  # the rows of internal dofs are empty


def element_schur(K, F, p, U):
    """numpy restatement of condenseSystem: S = K_bb - K_bi K_ii^-1 K_ib, g = F_b - K_bi K_ii^-1 F_i (F [Nd, R])"""
    primary, internal = system.element_node_split(p)
    b = (primary[:, None] * U + np.arange(U)).ravel()
    i = (internal[:, None] * U + np.arange(U)).ravel()
    if len(i) == 0:
        return K.copy(), F.copy()
    X = np.linalg.solve(K[np.ix_(i, i)], np.concatenate([K[np.ix_(i, b)], F[i]], axis=1))
    S = K[np.ix_(b, b)] - K[np.ix_(b, i)] @ X[:, :len(b)]
    g = F[b] - K[np.ix_(b, i)] @ X[:, len(b):]
    return S, g


@pytest.mark.parametrize("p", [2, 3])
def test_global_schur_is_sum_of_element_schurs(p):
    kid, U, R, kpar = system.KERNEL_DIFFUSION3D, 4, 2, [0.7, 1.3]
    part = system.CubePartition(2, p, perturb=0.15)
    nq = system.n_qps1d(p, 1)
    n = part.n_local_nodes * U
    A, rhs = np.zeros((n, n)), np.zeros((n, R))
    A_c, rhs_c = np.zeros((n, n)), np.zeros((n, R))
    primary, internal = system.element_node_split(p)
    inner = set()
    for e in range(part.n_elems):
        K, F = O.assemble_local(kid, p, nq, R, part.elem_verts[e], None, kpar)
        dofs = (part.elem_nodes[e].astype(np.int64)[:, None] * U + np.arange(U)).ravel()
        A[np.ix_(dofs, dofs)] += K
        rhs[dofs] += F
        S, g = element_schur(K, F, p, U)
        bd = (part.elem_nodes[e, primary].astype(np.int64)[:, None] * U + np.arange(U)).ravel()
        A_c[np.ix_(bd, bd)] += S
        rhs_c[bd] += g
        inner.update((part.elem_nodes[e, internal].astype(np.int64)[:, None] * U + np.arange(U)).ravel().tolist())
    i = np.array(sorted(inner))
    b = np.setdiff1d(np.arange(n), i)
    X = np.linalg.solve(A[np.ix_(i, i)], np.concatenate([A[np.ix_(i, b)], rhs[i]], axis=1))
    S_glob = A[np.ix_(b, b)] - A[np.ix_(b, i)] @ X[:, :len(b)]
    g_glob = rhs[b] - A[np.ix_(b, i)] @ X[:, len(b):]
    scale = np.abs(A).max()
    assert np.abs(S_glob - A_c[np.ix_(b, b)]).max() < 1e-10 * scale
    assert np.abs(g_glob - rhs_c[b]).max() < 1e-10 * max(1.0, np.abs(rhs).max())
    assert not A_c[i].any() and not rhs_c[i].any()  # nothing lands on internal rows
