"""The symbolic phase of the band Cholesky solver without a GPU: l3k_chol_order against the numpy restatement (tests/chol_ref.py),
the invariants of the block envelope, the restatement's own factorisation against numpy, refusals, and the public surface."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import chol_ref as R
from l3ster_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def order(n, row_ptr, col_ind, block=0, max_bytes=0):
    """l3k_chol_order: (rc, perm [n_active], heights, nb, n_active, bytes)"""
    lib = capi.load()
    row_ptr = np.ascontiguousarray(row_ptr, dtype=np.int64)
    col_ind = np.ascontiguousarray(col_ind, dtype=np.int32)
    perm = np.full(max(n, 1), -7, dtype=np.int32)
    heights = np.full(n // 32 + 1, -7, dtype=np.int32)
    nb, na, nbytes = C.c_int(block), C.c_int64(-1), C.c_size_t(max_bytes)
    rc = lib.l3k_chol_order(n, row_ptr.ctypes.data_as(capi.c_int64_p), col_ind.ctypes.data_as(capi.c_int32_p),
                            perm.ctypes.data_as(capi.c_int32_p), heights.ctypes.data_as(capi.c_int32_p), C.byref(nb), C.byref(na),
                            C.byref(nbytes))
    if rc != 0:
        return rc, None, None, nb.value, na.value, nbytes.value
    nblk = (na.value + nb.value - 1) // nb.value
    assert np.all(perm[na.value:n] == -1)
    return rc, perm[:na.value].copy(), heights[:nblk].copy(), nb.value, na.value, nbytes.value


def grid_pattern(nx, ny):
    """5-point stencil on an nx x ny grid"""
    n = nx * ny
    P = np.eye(n, dtype=bool)
    idx = np.arange(n).reshape(ny, nx)
    for a, b in ((idx[:, :-1], idx[:, 1:]), (idx[:-1, :], idx[1:, :])):
        P[a.ravel(), b.ravel()] = P[b.ravel(), a.ravel()] = True
    return P


def permuted(P, seed):
    q = np.random.default_rng(seed).permutation(P.shape[0])
    return P[np.ix_(q, q)]


def with_empty_rows(P, seed, n_empty):
    """P embedded in a larger pattern with n_empty empty rows (and columns) interleaved"""
    n = P.shape[0] + n_empty
    keep = np.sort(np.random.default_rng(seed).permutation(n)[:P.shape[0]])
    Q = np.zeros((n, n), dtype=bool)
    Q[np.ix_(keep, keep)] = P
    return Q


def two_components():
    a, b = grid_pattern(7, 5), grid_pattern(3, 11)
    P = np.zeros((a.shape[0] + b.shape[0],) * 2, dtype=bool)
    P[:a.shape[0], :a.shape[0]] = a
    P[a.shape[0]:, a.shape[0]:] = b
    return permuted(P, 5)


PATTERNS = {
    "grid": lambda: grid_pattern(13, 9),
    "grid_wide": lambda: grid_pattern(90, 80),
    "grid_permuted": lambda: permuted(grid_pattern(13, 9), 1),
    "two_components": two_components,
    "empty_rows": lambda: with_empty_rows(permuted(grid_pattern(11, 6), 2), 3, 17),
    "n0": lambda: np.zeros((0, 0), dtype=bool),
    "n1": lambda: np.ones((1, 1), dtype=bool),
    "n1_empty": lambda: np.zeros((1, 1), dtype=bool),
}


def csr(P):
    return R.csr_from_dense(P.astype(np.float64), P)[:2]


@pytest.mark.parametrize("name", sorted(PATTERNS))
@pytest.mark.parametrize("block", [0, 32, 64])
def test_order_matches_the_restatement(name, block):
    P = PATTERNS[name]()
    n = P.shape[0]
    row_ptr, col_ind = csr(P)
    rc, perm, heights, nb, n_active, nbytes = order(n, row_ptr, col_ind, block)
    assert rc == 0, capi.load().l3k_last_error()
    rperm, rheights, rnb, rbytes = R.symbolic(n, row_ptr, col_ind, block)
    assert n_active == len(R.active_rows(row_ptr)) == len(rperm)
    assert nb == rnb and (block == 0 or nb == block)
    assert np.array_equal(perm, rperm)
    assert np.array_equal(heights, rheights)
    assert nbytes == rbytes
    # ---- invariants: a permutation of the active rows; every lower-triangle entry inside the envelope; K + H(K) monotone
    assert np.array_equal(np.sort(perm), R.active_rows(row_ptr))
    inv = R.inverse(n, perm)
    rows = np.repeat(np.arange(n), np.diff(row_ptr))
    pi, pj = inv[rows], inv[col_ind]
    low = pi >= pj
    assert np.all(pi[low] // nb - pj[low] // nb <= heights[pj[low] // nb])
    ends = np.arange(len(heights)) + heights
    assert np.all(np.diff(ends) >= 0) and (len(ends) == 0 or ends[-1] == len(heights) - 1)


def test_wide_grid_takes_blocks_of_64_and_a_lens_shaped_profile():
    row_ptr, col_ind = csr(PATTERNS["grid_wide"]())
    rc, perm, heights, nb, _, _ = order(7200, row_ptr, col_ind)
    assert rc == 0 and nb == 64
    # the profile of a reverse Cuthill-McKee ordering starts narrow: a single global bandwidth would waste the difference
    assert heights[0] < heights.max()


def envelope_entries(P, block):
    """Entries the block envelope of l3k_chol_order holds for pattern P"""
    row_ptr, col_ind = csr(P)
    rc, perm, heights, nb, _, _ = order(P.shape[0], row_ptr, col_ind, block)
    assert rc == 0
    return int((len(heights) + heights.sum()) * nb * nb)


def identity_order_envelope(P, nb):
    n = P.shape[0]
    row_ptr, col_ind = csr(P)
    h = R.envelope(n, row_ptr, col_ind, np.arange(n, dtype=np.int32), nb)
    return int((len(h) + h.sum()) * nb * nb)


@pytest.mark.parametrize("block", [32, 64])
def test_ordering_undoes_a_random_permutation(block):
    """the envelope after ordering a randomly permuted grid is no larger than that of the grid in its natural numbering"""
    for nx, ny in ((13, 9), (90, 80)):
        G = grid_pattern(nx, ny)
        assert envelope_entries(permuted(G, 11), block) <= identity_order_envelope(G, block)


def spd_band(n, bw, seed):
    """B B^T + I with B lower triangular of half-bandwidth bw: positive definite, and of half-bandwidth bw itself"""
    i, j = np.indices((n, n))
    B = np.where((i >= j) & (i - j <= bw), np.random.default_rng(seed).standard_normal((n, n)), 0.)
    return B @ B.T + np.eye(n)


@pytest.mark.parametrize("n,bw,nb", [(100, 7, 32), (150, 40, 32), (200, 70, 64), (97, 96, 32)])
def test_restatement_factor_matches_numpy_inside_the_envelope_and_is_zero_outside(n, bw, nb):
    A = spd_band(n, bw, n + bw)
    q = np.random.default_rng(n).permutation(n)
    A = A[np.ix_(q, q)]
    row_ptr, col_ind, values = R.csr_from_dense(A)
    perm, h, nb, _ = R.symbolic(n, row_ptr, col_ind, nb)
    m = len(h) * nb
    Ap = np.eye(m)
    Ap[:n, :n] = A[np.ix_(perm, perm)]
    L = R.block_cholesky(Ap, h, nb)
    Lnp = np.linalg.cholesky(Ap)
    mask = R.envelope_mask(h, nb)
    assert np.all(L[~mask] == 0.)
    assert np.all(Lnp[~mask & np.tril(np.ones_like(mask))] == 0.)  # the envelope is closed under fill
    assert np.max(np.abs(L - Lnp)) <= 1e-12 * np.max(np.abs(Lnp))
    b = np.random.default_rng(3).standard_normal(n)
    x = R.solve(n, row_ptr, col_ind, values, b, np.zeros(n), nb)
    assert np.linalg.norm(A @ x - b) <= 1e-12 * np.linalg.norm(A, 2) * np.linalg.norm(x)


def test_refusals():
    lib = capi.load()
    # (0, 2) stored, (2, 0) not
    P = np.eye(4, dtype=bool)
    P[0, 2] = True
    P[1, 3] = P[3, 1] = True
    rc, *_ = order(4, *csr(P))
    assert rc == -1
    msg = lib.l3k_last_error().decode()
    assert "(0, 2)" in msg and "(2, 0)" in msg, msg
    assert R.first_unsymmetric_pair(4, *csr(P)) == (0, 2)
    # the memory guard names the bytes needed
    G = grid_pattern(13, 9)
    rc, _, _, nb, _, nbytes = order(117, *csr(G), max_bytes=1)
    assert rc == -1
    need = R.symbolic(117, *csr(G))[3]
    assert nbytes == need
    msg = lib.l3k_last_error().decode()
    assert str(need) in msg and "largest H" in msg, msg
    assert order(117, *csr(G), max_bytes=need)[0] == 0
    assert order(117, *csr(G), max_bytes=need - 1)[0] == -1
    # other block sizes, invalid graphs
    assert order(117, *csr(G), block=48)[0] == -1
    row_ptr, col_ind = csr(G)
    bad = col_ind.copy()
    bad[3] = 117
    assert order(117, row_ptr, bad)[0] == -1
    assert order(117, row_ptr[::-1].copy(), col_ind)[0] == -1


def test_surface():
    lib = capi.load()
    assert lib.l3k_version() == 101
    header = open(os.path.join(ROOT, "include", "l3k.h")).read()
    assert re.search(r"#define L3K_VERSION 101\b", header)
    for name in ("l3k_chol_create", "l3k_chol_factor", "l3k_chol_solve", "l3k_chol_info_get", "l3k_chol_destroy", "l3k_chol_order"):
        assert re.search(r"\bint " + name + r"\(", header), name
        assert name in capi.SIGNATURES and hasattr(lib, name)
    for name in ("l3k_chol_opts", "l3k_chol_info"):
        assert re.search(r"\}\s*" + name + ";", header), name
    from l3ster_amd import solve
    assert hasattr(solve, "CholeskySolver") and hasattr(solve, "direct_solve")
    cpp = open(os.path.join(ROOT, "include", "l3k", "operator.hpp")).read()
    assert "class Cholesky" in cpp
    # a solver needs a device operator: without one the Python layer refuses before any native call
    with pytest.raises(capi.L3KError):
        solve.CholeskySolver(object())
    from l3ster_amd import system
    with pytest.raises(capi.L3KError, match="DistributedCsrOperator"):
        solve.CholeskySolver(object.__new__(system.DistributedCsrOperator))
