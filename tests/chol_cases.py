"""Designed systems for the band Cholesky solver (l3k_chol_*): envelopes that are tall, jagged or split, with a prescribed factor.

The exact cases.  For each pattern S below the solver's ordering (reverse Cuthill-McKee, tests/chol_ref.py restates it) is the
reversal of the natural order of the active rows (tests/test_chol_cases_cpu.py asserts it), so in that order the lower triangle
is a full envelope and Cholesky fills nothing outside S.  The factor is prescribed: L0 lower triangular in the solver's order on
the pattern tril(S[perm][:, perm]), integers in [-2, 2] off the diagonal and 1, 2 or 4 on it, A[perm, perm] = L0 L0^T stored on S
(explicit zeros included), x0 integers in [-8, 8], b = A x0.  Every intermediate of a right-looking Cholesky of A and of both
substitutions is then an integer far below 2^53, the divisions are by 1, 2 or 4 and the square roots of 1, 4 or 16: the result
depends on no order of summation, on no FMA contraction and on no accumulation order of the matrix cores.  A correct solver
returns x0 bit for bit although kappa_2(A) is around 1e19; a wrong or missing term anywhere gives garbage.

The hub case is real-valued and its order is no reversal: its envelope is tall and almost empty.

Builders return Case(A dense [n, n], pattern bool [n, n], perm (perm[new] = old, active rows only), L0 [n_active, n_active] or
None, active rows).  numpy only; every builder is cached, so callers copy what they change."""
import functools
from collections import namedtuple

import numpy as np

import chol_ref as R

Case = namedtuple("Case", "A pattern perm L0 active")


# ------------------------------------------------------------------------------------------------------------ patterns
def dense_pattern(n):
    return np.ones((n, n), dtype=bool)


def band_pattern(n, bw):
    i, j = np.indices((n, n))
    return np.abs(i - j) <= bw


def block_diagonal(parts):
    n = sum(p.shape[0] for p in parts)
    S = np.zeros((n, n), dtype=bool)
    at = 0
    for p in parts:
        S[at:at + p.shape[0], at:at + p.shape[0]] = p
        at += p.shape[0]
    return S


def stair_pattern(sizes, overlap):
    """Dense diagonal blocks of the given sizes, each sharing its first `overlap` rows with the block before"""
    n = sum(sizes) - overlap * (len(sizes) - 1)
    S = np.zeros((n, n), dtype=bool)
    at = 0
    for s in sizes:
        S[at:at + s, at:at + s] = True
        at += s - overlap
    return S


def components_pattern(n_isolated):
    """band(150, 50), n_isolated rows that store their diagonal only, band(333, 200), one such row, band(70, 1)"""
    return block_diagonal([band_pattern(150, 50), np.eye(n_isolated, dtype=bool), band_pattern(333, 200), np.eye(1, dtype=bool),
                           band_pattern(70, 1)])


def dumbbell_pattern(clique=150, chain=200):
    """Two dense cliques joined by a chain: the chain's ends are tied to the last row of one clique and the first of the other"""
    n = 2 * clique + chain
    S = block_diagonal([dense_pattern(clique), band_pattern(chain, 1), dense_pattern(clique)])
    for a in (clique - 1, clique + chain - 1):
        S[a, a + 1] = S[a + 1, a] = True
    assert S.shape == (n, n)
    return S


def hub_pattern(leaves=300, clique=100):
    """Row 0 is the hub: joined to rows 1 .. leaves, which store nothing else off the diagonal, and to the first row of a dense
    clique.  The ordering starts in the clique and numbers the leaves last, so after the reversal the hub's row reaches back over
    all of them: block columns of height 9, 8, .. 1 (blocks of 32) that hold one row of entries each"""
    n = 1 + leaves + clique
    S = np.eye(n, dtype=bool)
    S[0, 1:leaves + 2] = S[1:leaves + 2, 0] = True
    S[leaves + 1:, leaves + 1:] = True
    return S


# ------------------------------------------------------------------------------------------------------------ systems
def fill_stays_inside(L0, Sp):
    """Does L0 L0^T, taken structurally, store nothing outside the pattern Sp?"""
    B = (L0 != 0).astype(np.float64)
    return not np.any((B @ B.T > 0) & ~Sp)


def exact_system(S, seed, diag_two_rows=()):
    """Case of the pattern S (every row active) with the prescribed integer factor.  diag_two_rows: ordered rows r that get
    L0[r, r] = 2 and zeros below it in column r -- rows whose diagonal entry of A can be changed without touching any other pivot
    (the designed pivots of pivot_variants)"""
    n = S.shape[0]
    assert np.array_equal(S, S.T) and np.all(np.diag(S))
    perm = np.arange(n - 1, -1, -1, dtype=np.int32)
    Sp = S[np.ix_(perm, perm)]
    rng = np.random.default_rng(seed)
    L0 = np.tril(Sp, -1) * rng.integers(-2, 3, (n, n)).astype(np.float64)
    L0[np.arange(n), np.arange(n)] = rng.choice([1., 2., 4.], n)
    for r in diag_two_rows:
        L0[r + 1:, r] = 0.
        L0[r, r] = 2.
    assert fill_stays_inside(L0, Sp)
    Ap = L0 @ L0.T
    assert np.all(Ap == np.rint(Ap)) and np.abs(Ap).max() < 2. ** 20
    A = np.zeros((n, n))
    A[np.ix_(perm, perm)] = Ap
    return Case(A, S.copy(), perm, L0, np.arange(n))


def embedded(case, n_empty, seed=0):
    """The same system with n_empty empty rows and columns interleaved (frozen rows: the solver leaves x alone there).  The active
    rows keep their relative order, so the ordering is still their reversal"""
    na = case.A.shape[0]
    n = na + n_empty
    keep = np.sort(np.random.default_rng(seed).permutation(n)[:na])
    A, S = np.zeros((n, n)), np.zeros((n, n), dtype=bool)
    A[np.ix_(keep, keep)] = case.A
    S[np.ix_(keep, keep)] = case.pattern
    return Case(A, S, keep[case.perm].astype(np.int32), case.L0, keep)


PATTERNS = {
    "dense96": lambda: dense_pattern(96),
    "dense807": lambda: dense_pattern(807),
    "dense1671": lambda: dense_pattern(1671),
    "stair": lambda: stair_pattern([40, 300, 20, 150, 90], 5),
    "components": lambda: components_pattern(100),
    "components200": lambda: components_pattern(200),
    "dumbbell": dumbbell_pattern,
}
EMBEDDED = {"stair_embedded": ("stair", 45), "components_embedded": ("components", 23)}
EXACT = sorted(PATTERNS) + sorted(EMBEDDED)
SEEDS = {name: 100 + k for k, name in enumerate(sorted(PATTERNS))}


@functools.lru_cache(maxsize=None)
def exact(name):
    if name in EMBEDDED:
        base, n_empty = EMBEDDED[name]
        return embedded(exact(base), n_empty, seed=n_empty)
    return exact_system(PATTERNS[name](), SEEDS[name])


@functools.lru_cache(maxsize=None)
def hub():
    """Random values, strictly diagonally dominant by rows (so positive definite); the order comes from the restatement"""
    S = hub_pattern()
    n = S.shape[0]
    rng = np.random.default_rng(77)
    V = np.triu(rng.uniform(-1., 1., (n, n)), 1) * S
    A = V + V.T
    A[np.arange(n), np.arange(n)] = np.abs(A).sum(axis=1) + rng.uniform(0.5, 1.5, n)
    row_ptr, col_ind, _ = R.csr_from_dense(A, S)
    return Case(A, S, R.rcm(n, row_ptr, col_ind), None, np.arange(n))


def solution(case, ncols, seed):
    """(X0, B) [ncols, n]: distinct integer vectors in [-8, 8] and B_c = A X0_c; both exactly 0 (+0) on the rows that are not active"""
    n = case.A.shape[0]
    rng = np.random.default_rng(seed)
    X0 = np.zeros((ncols, n))
    X0[:, case.active] = rng.integers(-8, 9, (ncols, len(case.active)))
    if ncols > 1:
        assert len({x.tobytes() for x in X0}) == ncols
    B = X0 @ case.A.T + 0.  # (+ 0.: no -0 in b, whatever the order in which the product summed)
    assert np.all(B == np.rint(B)) and np.abs(B).max() < 2. ** 30
    return X0, B


# ------------------------------------------------------------------------------------------------------------ designed pivots
def pivot_places(n_active, heights, nb):
    """The ordered rows at which the pivot tests strike, by name: column 0 and column nb - 1 of block column 0, column 0 of block
    column 2, the last active row, and (where the envelope has one) a row inside an interior run of H = 0"""
    places = {"first": 0, "end_of_block_0": nb - 1, "start_of_block_2": 2 * nb, "last": n_active - 1}
    K = interior_empty_block(heights)
    if K is not None and (K + 1) * nb <= n_active:
        places["in_empty_run"] = K * nb + 5
    return places


def interior_empty_block(heights):
    """A block column K with H(K) = 0 = H(K - 1) and a non-empty block column on either side; None if there is none.  (H(K - 1) = 0
    as well, so that nothing of an earlier block column reaches the rows of K)"""
    h = np.asarray(heights)
    for K in range(1, len(h) - 1):
        if h[K] == 0 and h[K - 1] == 0 and h[:K].max() > 0 and h[K + 1:].max() > 0:
            return K
    return None


@functools.lru_cache(maxsize=None)
def pivot_case(name, nb):
    """(case, places): the exact case `name` rebuilt with L0[r, r] = 2 and an empty column below it at every place r for blocks of
    nb.  Lowering A's diagonal entry of ordered row r by 4 makes pivot r exactly 0, lowering it by 3 makes it exactly 1; no other
    pivot moves in either case, because column r of the factor stays 0 below the diagonal"""
    base = exact(name)
    n = len(base.perm)
    row_ptr, col_ind, _ = R.csr_from_dense(base.A, base.pattern)
    heights = R.envelope(base.A.shape[0], row_ptr, col_ind, base.perm, nb)
    places = pivot_places(n, heights, nb)
    return exact_system(PATTERNS[name](), SEEDS[name] + 1000 + nb, tuple(sorted(set(places.values())))), places


def with_diagonal(case, changes):
    """A copy of the case's matrix with delta added to the diagonal entry of ordered row r for every (r, delta) in changes"""
    A = case.A.copy()
    for r, delta in changes:
        A[case.perm[r], case.perm[r]] += delta
    return A


# ------------------------------------------------------------------------------------------------------------ host arithmetic
def host_cholesky(Ap):
    """Unblocked right-looking Cholesky of Ap (already ordered) in plain float64, with the solver's rule for a pivot that is not
    positive and finite: it is replaced by 1 and counted.  Returns (L, the bad pivots' rows, the pivots as met)"""
    W = np.tril(Ap).astype(np.float64)
    n = W.shape[0]
    bad, pivots = [], np.zeros(n)
    for c in range(n):
        d = pivots[c] = W[c, c]
        if not (np.isfinite(d) and d > 0.):
            bad.append(c)
            d = 1.
        piv = np.sqrt(d)
        W[c, c] = piv
        W[c + 1:, c] /= piv
        nz = np.nonzero(W[c + 1:, c])[0]
        if len(nz):  # (the rows outside [lo, hi) have a 0 in column c: their update is - 0)
            lo, hi = c + 1 + nz[0], c + 2 + nz[-1]
            W[lo:hi, lo:hi] -= np.tril(np.outer(W[lo:hi, c], W[lo:hi, c]))
    return W, bad, pivots


def host_cholesky_left(Ap):
    """The same factorisation left-looking (column c is finished by one matrix-vector product with the columns before it): a
    different order of the same sums, several times quicker in numpy.  Same rule for bad pivots, same return"""
    n = Ap.shape[0]
    L = np.zeros((n, n))
    bad, pivots = [], np.zeros(n)
    for c in range(n):
        v = Ap[c:, c] - L[c:, :c] @ L[c, :c]
        d = pivots[c] = v[0]
        if not (np.isfinite(d) and d > 0.):
            bad.append(c)
            d = 1.
        piv = np.sqrt(d)
        L[c, c] = piv
        L[c + 1:, c] = v[1:] / piv
    return L, bad, pivots


def host_solve(L, b):
    """x with L L^T x = b by two column-oriented substitutions in plain float64"""
    n = L.shape[0]
    w = np.array(b, dtype=np.float64)
    for c in range(n):
        w[c] /= L[c, c]
        w[c + 1:] -= L[c + 1:, c] * w[c]
    for c in range(n - 1, -1, -1):
        w[c] /= L[c, c]
        w[:c] -= L[c, :c] * w[c]
    return w
