"""Pins the numpy restatements of tests/csr_ref.py against the dense definitions: l3k_csr_dirichlet as "masked rows become the
identity, A_fd is zeroed, f_f - A_fd g", l3k_csr_diag with its minv and the empty-row rule, the longdouble product and the
row-wise bound helper -- on a 12 x 12 matrix written out by hand and on a random 200 x 200 one.  No GPU, no libl3k."""
import numpy as np
import pytest

import csr_ref as R
from cg_ref import EPS, LD

# 12 x 12 by hand: row 3 is empty, rows 5 and 9 store no diagonal, row 7 stores a negative one, row 11 a zero one
HAND_ROWS = [
    {0: 4.0, 1: -1.0, 4: 0.5},
    {0: -1.0, 1: 5.0, 2: -2.0},
    {1: -2.0, 2: 6.0, 6: 1.5, 10: -0.25},
    {},
    {0: 0.5, 4: 3.0, 5: 1.0, 8: -1.0},
    {4: 1.0, 6: 2.0},
    {2: 1.5, 5: 2.0, 6: 7.0, 7: -3.0},
    {6: -3.0, 7: -8.0, 11: 1.0},
    {4: -1.0, 8: 2.5},
    {8: 0.75, 10: 1.25},
    {2: -0.25, 9: 1.25, 10: 9.0},
    {7: 1.0, 11: 0.0},
]


def hand_matrix():
    row_ptr = np.concatenate([[0], np.cumsum([len(r) for r in HAND_ROWS])]).astype(np.int64)
    col_ind = np.array([c for r in HAND_ROWS for c in sorted(r)], dtype=np.int32)
    values = np.array([r[c] for r in HAND_ROWS for c in sorted(r)], dtype=np.float64)
    return row_ptr, col_ind, values


def random_matrix(n=200, seed=5):
    rng = np.random.default_rng(seed)
    lens = rng.choice([0, 1, 3, 4, 5, 15, 16, 17, 40], size=n)
    row_ptr, col_ind = R.strided_graph(n, lens)
    return row_ptr, col_ind, rng.standard_normal(col_ind.size)


def dense(row_ptr, col_ind, values):
    n = row_ptr.size - 1
    A, stored = np.zeros((n, n)), np.zeros((n, n), dtype=bool)
    rows = R.row_of_entry(row_ptr)
    A[rows, col_ind] = values
    stored[rows, col_ind] = True
    return A, stored


CASES = [hand_matrix, random_matrix]


@pytest.mark.parametrize("make", CASES)
def test_graph_is_valid_csr(make):
    row_ptr, col_ind, values = make()
    n = row_ptr.size - 1
    assert row_ptr[0] == 0 and (np.diff(row_ptr) >= 0).all() and row_ptr[-1] == col_ind.size == values.size
    assert col_ind.min() >= 0 and col_ind.max() < n
    inner = np.ones(col_ind.size, dtype=bool)
    inner[row_ptr[:-1][np.diff(row_ptr) > 0]] = False  # the first entry of a row has no predecessor in it
    assert (np.diff(col_ind.astype(np.int64))[inner[1:]] > 0).all()
    rows = R.row_of_entry(row_ptr)
    has_diag = np.zeros(n, dtype=bool)
    has_diag[rows[col_ind == rows]] = True
    assert has_diag.any() and (~has_diag & (np.diff(row_ptr) > 0)).any() and (np.diff(row_ptr) == 0).any()


@pytest.mark.parametrize("make", CASES)
def test_apply_ref_and_row_bound(make):
    row_ptr, col_ind, values = make()
    n = row_ptr.size - 1
    A, _ = dense(row_ptr, col_ind, values)
    x = np.random.default_rng(1).standard_normal(n)
    y, absy = R.apply_ref(row_ptr, col_ind, values, x)
    assert y.dtype == LD and np.array_equal(y == 0, (np.diff(row_ptr) == 0) | (y == 0))
    assert np.abs(y - A.astype(LD) @ x.astype(LD)).max() <= 64 * 2.0 ** -64 * max(1.0, float(absy.max()))
    assert np.allclose(np.asarray(absy, dtype=np.float64), np.abs(A) @ np.abs(x), rtol=1e-14, atol=0)
    # the float64 product in another order stays inside the bound; the bound is 0 on an empty row and 3 EPS |t| for one term
    lens = np.diff(row_ptr)
    bound = R.row_bound(lens, absy)
    assert (np.abs((A[:, ::-1] @ x[::-1]).astype(LD) - y) <= bound).all()
    assert (bound[lens == 0] == 0).all()
    assert R.row_bound([1], [2.0])[0] == 4 * EPS * 2.0 and R.row_bound([1000], [1.0])[0] == 1003 * EPS


@pytest.mark.parametrize("make", CASES)
@pytest.mark.parametrize("damping,threshold", [(1.0, 0.0), (0.8, 1e-3)])
def test_diag_ref_vs_dense(make, damping, threshold):
    row_ptr, col_ind, values = make()
    A, stored = dense(row_ptr, col_ind, values)
    diag, minv = R.diag_ref(row_ptr, col_ind, values, damping, threshold)
    assert np.array_equal(diag, np.where(np.diag(stored), np.diag(A), 0.0))
    lens = np.diff(row_ptr)
    for i in range(row_ptr.size - 1):
        if lens[i] == 0:
            assert minv[i] == 0.0  # the PCG freezes the row
        else:
            d = diag[i]
            with np.errstate(divide="ignore"):
                assert minv[i] == (-damping if d < 0 else damping) / np.float64(max(abs(d), threshold))


def test_diag_ref_hand_values():
    diag, minv = R.diag_ref(*hand_matrix())
    assert diag.tolist() == [4.0, 5.0, 6.0, 0.0, 3.0, 0.0, 7.0, -8.0, 2.5, 0.0, 9.0, 0.0]
    assert minv[3] == 0.0 and minv[7] == -0.125 and minv[0] == 0.25
    assert np.isinf(minv[[5, 9, 11]]).all()  # a non-empty row without a usable diagonal and threshold 0: the formula's 1 / 0
    assert np.isfinite(R.diag_ref(*hand_matrix(), threshold=0.5)[1]).all()


@pytest.mark.parametrize("make", CASES)
@pytest.mark.parametrize("ncols", [1, 3])
def test_dirichlet_ref_vs_dense_definition(make, ncols):
    row_ptr, col_ind, values = make()
    n = row_ptr.size - 1
    A, stored = dense(row_ptr, col_ind, values)
    rng = np.random.default_rng(3)
    mask = (rng.random(n) < 0.3) & np.diag(stored)
    assert mask.any() and (~mask).any()
    g = np.where(mask, rng.standard_normal((ncols, n)), 0.0)
    rhs = rng.standard_normal((ncols, n))
    new, out, absv = R.dirichlet_ref(row_ptr, col_ind, values, mask.astype(np.uint8), g, rhs)
    B, _ = dense(row_ptr, col_ind, new)
    d, f = np.flatnonzero(mask), np.flatnonzero(~mask)
    assert np.array_equal(B[np.ix_(d, np.arange(n))], np.eye(n)[d])  # the masked rows are identity rows
    assert not B[np.ix_(f, d)].any()  # A_fd is zeroed
    assert np.array_equal(B[np.ix_(f, f)], A[np.ix_(f, f)])  # A_ff is untouched
    assert set(np.unique(new)) <= set(np.unique(values)) | {0.0, 1.0}
    assert np.array_equal(out[:, d], g[:, d].astype(LD))
    ref = rhs[:, f].astype(LD) - (A[np.ix_(f, d)].astype(LD) @ g[:, d].astype(LD).T).T  # f_f - A_fd g
    assert np.abs(out[:, f] - ref).max() <= 64 * 2.0 ** -64 * max(1.0, float(absv.max()))
    assert np.allclose(np.asarray(absv[:, f], dtype=np.float64), np.abs(rhs[:, f]) + (np.abs(A[np.ix_(f, d)]) @ np.abs(g[:, d]).T).T,
                       rtol=1e-14, atol=0)
    assert not absv[:, d].any()


@pytest.mark.parametrize("make", CASES)
def test_dirichlet_ref_refuses_masked_row_without_diagonal(make):
    row_ptr, col_ind, values = make()
    n = row_ptr.size - 1
    _, stored = dense(row_ptr, col_ind, values)
    bad = int(np.flatnonzero(~np.diag(stored))[0])
    mask = np.zeros(n, dtype=np.uint8)
    mask[bad] = 1
    with pytest.raises(ValueError, match=f"Dirichlet row {bad} has no stored diagonal"):
        R.dirichlet_ref(row_ptr, col_ind, values, mask, np.zeros(n), np.zeros(n))
