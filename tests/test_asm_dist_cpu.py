"""The sub-assembled form of the assembled system on a partitioned mesh, restated densely in numpy (tests/asm_dist_ref.py) and proved
on the host against the whole mesh: sum_r R_r^T A_r R_r after the rank-local Dirichlet step with the owner rule and the export-add
of the right-hand sides IS the whole mesh's matrix and right-hand side after tests/csr_ref.py's Dirichlet step; the row classes;
the summed diagonal.  No GPU: the reference of tests/test_gpu_asm_dist.py.

Bar: 1e-12 |A|_max entrywise -- the two sides sum the same element matrices in another order, at most 4 (quads) or
8 (hexes) terms per entry, and the Dirichlet step subtracts at most a row's length of products: a few hundred roundings of 1.1e-16
on terms bounded by |A|_max |g|_max with |g| <= 1."""
import numpy as np
import pytest

import asm_dist_ref as AD
import csr_ref

_CASES = {}


def case(kind):
    if kind not in _CASES:
        q = AD.quad_case(device="cpu") if kind == "quad" else AD.cube_case()
        q.W = AD.local_system(q, q.whole, q.sides, np.arange(q.whole.n_elems))
        q.L = [AD.local_system(q, q.parts[r], q.part_sides[r], q.elem_of[r]) for r in range(q.world)]
        _CASES[kind] = q
    return _CASES[kind]


@pytest.mark.parametrize("kind", ["quad", "cube"])
def test_meshes_have_all_three_row_classes(kind):
    q = case(kind)
    assert any(m.n_ghost_nodes > 0 for m in q.parts)
    full = []
    for r in range(q.world):
        row_ptr, col_ind, _ = AD.csr_of(q.L[r][0], q.L[r][2])
        interior, border, ghost = AD.row_classes(row_ptr, col_ind, q.n_owned(r))
        n = q.parts[r].n_local_nodes * q.U
        # a partition of the rows, each list ascending
        assert np.array_equal(np.sort(np.concatenate([interior, border, ghost])), np.arange(n))
        for rows in (interior, border, ghost):
            assert np.all(np.diff(rows) > 0)
        assert np.array_equal(ghost, np.arange(q.n_owned(r), n))
        dense = q.L[r][2]
        assert not dense[np.ix_(interior, np.arange(q.n_owned(r), n))].any()  # no interior row holds a ghost column
        assert all(dense[i, q.n_owned(r):].any() for i in border)
        full.append(interior.size > 0 and border.size > 0 and ghost.size > 0)
    assert any(full)


def test_an_empty_owned_row_is_interior():
    row_ptr = np.array([0, 2, 2, 3, 4], dtype=np.int64)  # rows 0, 1 (empty), 2 owned; row 3 a ghost
    col_ind = np.array([0, 3, 2, 3], dtype=np.int32)
    interior, border, ghost = AD.row_classes(row_ptr, col_ind, 3)
    assert interior.tolist() == [1, 2] and border.tolist() == [0] and ghost.tolist() == [3]


@pytest.mark.parametrize("kind", ["quad", "cube"])
def test_local_matrices_sum_to_the_whole_matrix(kind):
    q = case(kind)
    A = AD.sum_of_ranks(q, [L[0] for L in q.L])
    scale = np.abs(q.W[0]).max()
    print(f"{kind}: max|sum_r R^T A_r R - A| / |A|_max = {np.abs(A - q.W[0]).max() / scale:.2e}")
    assert np.abs(A - q.W[0]).max() <= 1e-12 * scale
    rhs = AD.export_add(q, [L[1] for L in q.L])
    assert np.abs(rhs[0] - q.W[1]).max() <= 1e-12 * max(np.abs(q.W[1]).max(), 1.0)


@pytest.mark.parametrize("kind", ["quad", "cube"])
def test_owner_rule_is_the_dirichlet_step_on_the_whole_matrix(kind):
    q = case(kind)
    g = AD.prescribed_values(q)
    # the whole mesh through csr_ref's step
    row_ptr, col_ind, values = AD.csr_of(q.W[0], q.W[2])
    new, rhs_w, _ = csr_ref.dirichlet_ref(row_ptr, col_ind, values, q.mask, g, q.W[1][None, :])
    A_w, rhs_w = AD.dense_of(row_ptr, col_ind, new), np.asarray(rhs_w, dtype=np.float64)
    # the ranks: the values imported to the ghost rows, the owner rule, the sum and the export-add
    mats, vecs = [], []
    for r in range(q.world):
        Ar, br = AD.dirichlet_owner_rule(q.L[r][0], q.L[r][1], q.local_mask(r), g[:, q.local_dofs(r)], q.n_owned(r))
        mats.append(Ar)
        vecs.append(br)
        flagged_ghost = np.flatnonzero(q.local_mask(r)[q.n_owned(r):]) + q.n_owned(r)
        assert not Ar[flagged_ghost].any() and not br[:, flagged_ghost].any()
    A, rhs = AD.sum_of_ranks(q, mats), AD.export_add(q, vecs)
    scale = np.abs(q.W[0]).max()
    print(f"{kind}: matrix {np.abs(A - A_w).max() / scale:.2e}, rhs {np.abs(rhs - rhs_w).max() / scale:.2e} of |A|_max")
    assert np.abs(A - A_w).max() <= 1e-12 * scale
    assert np.abs(rhs - rhs_w).max() <= 1e-12 * scale
    # the flagged rows are identity rows holding the value, each exactly once
    flagged = np.flatnonzero(q.mask)
    assert np.array_equal(A[flagged], np.eye(A.shape[0])[flagged]) and np.array_equal(rhs[0, flagged], g[0, flagged])
    # the summed diagonal: the local diagonals export-added are the diagonal of the whole matrix
    diag = AD.export_add(q, [np.diag(M)[None, :] for M in mats])[0]
    want, _ = csr_ref.diag_ref(row_ptr, col_ind, new)
    assert np.abs(diag - want).max() <= 1e-12 * scale
