"""The designed systems of tests/chol_cases.py are what they claim, without a GPU: the library's ordering (l3k_chol_order) and the
restatement's agree on them and, for the exact cases, equal the reversal of the active rows; the block envelopes have the
heights the GPU tests rely on (tall, with interior H = 0 runs, with jumps); a plain float64 factorisation on the host returns the
prescribed factor, and the two substitutions the prescribed solution, exactly; the designed pivots are exactly 0 (or 1) where
they are meant to be."""
import numpy as np
import pytest

import chol_cases as CC
import chol_ref as R
from test_chol_cpu import order

HEIGHTS_32 = {
    "dense807": list(range(25, -1, -1)),
    "stair": [2, 1, 5, 4, 3, 2, 1, 10, 9, 8, 7, 6, 5, 4, 3, 2, 2, 1, 0],
    "components": [1, 1, 7, 7, 7, 7, 6, 5, 4, 3, 2, 1, 0, 0, 0, 2, 2, 2, 2, 1, 0],
    "dumbbell": [4, 3, 2, 1, 1, 1, 1, 1, 1, 1, 5, 4, 3, 2, 1, 0],
    "hub": [9, 8, 7, 6, 5, 4, 3, 2, 1, 3, 2, 1, 0],
}
HEIGHTS_64 = {"components200": [1, 4, 4, 3, 2, 1, 0, 0, 0, 1, 1, 0]}


def get(name):
    return CC.hub() if name == "hub" else CC.exact(name)


def both_orders(case, block):
    """(perm, heights) of l3k_chol_order after asserting that the restatement gives the same"""
    n = case.A.shape[0]
    row_ptr, col_ind, _ = R.csr_from_dense(case.A, case.pattern)
    rc, perm, heights, nb, n_active, _ = order(n, row_ptr, col_ind, block)
    assert rc == 0 and nb == block and n_active == len(case.active)
    rperm, rheights, _, _ = R.symbolic(n, row_ptr, col_ind, block)
    assert np.array_equal(perm, rperm) and np.array_equal(heights, rheights)
    return perm, heights


def interior_zeros(h):
    h = np.asarray(h)
    return [K for K in range(1, len(h) - 1) if h[K] == 0 and h[:K].max() > 0 and h[K + 1:].max() > 0]


@pytest.mark.parametrize("name", CC.EXACT)
def test_exact_cases_are_ordered_by_reversal(name):
    case = CC.exact(name)
    assert np.array_equal(case.active, R.active_rows(R.csr_from_dense(case.A, case.pattern)[0]))
    assert np.array_equal(case.perm, case.active[::-1])
    for block in (32, 64):
        perm, _ = both_orders(case, block)
        assert np.array_equal(perm, case.perm)
    # the prescribed factor lives on the ordered pattern, and so does its product
    Sp = case.pattern[np.ix_(case.perm, case.perm)]
    assert not np.any((case.L0 != 0) & ~np.tril(Sp)) and CC.fill_stays_inside(case.L0, Sp)
    assert np.array_equal(case.A[np.ix_(case.perm, case.perm)], case.L0 @ case.L0.T)
    off = case.L0[np.tril_indices_from(case.L0, -1)]
    assert set(np.unique(off)) <= {-2., -1., 0., 1., 2.} and set(np.unique(np.diag(case.L0))) <= {1., 2., 4.}


def test_sizes():
    sizes = {name: len(CC.exact(name).active) for name in CC.EXACT}
    assert sizes == {"dense96": 96, "dense807": 807, "dense1671": 1671, "stair": 580, "components": 654, "components200": 754,
                     "dumbbell": 500, "stair_embedded": 580, "components_embedded": 654}
    assert CC.exact("stair_embedded").A.shape[0] == 625 and CC.exact("components_embedded").A.shape[0] == 677
    assert CC.hub().A.shape[0] == 401


@pytest.mark.parametrize("name", sorted(HEIGHTS_32))
def test_heights_with_blocks_of_32(name):
    _, heights = both_orders(get(name), 32)
    assert heights.tolist() == HEIGHTS_32[name]


def test_heights_with_blocks_of_64():
    _, h = both_orders(CC.exact("dense1671"), 64)
    assert h.tolist() == list(range(26, -1, -1))
    _, h = both_orders(CC.exact("components200"), 64)
    assert h.tolist() == HEIGHTS_64["components200"]
    # the embedded variants have the envelopes of their bases
    for name, (base, _) in CC.EMBEDDED.items():
        for block in (32, 64):
            assert np.array_equal(both_orders(CC.exact(name), block)[1], both_orders(CC.exact(base), block)[1])


def test_the_envelopes_are_tall_split_and_jagged():
    """What the GPU tests count on, stated on its own so that a later change of the cases cannot quietly empty them"""
    for block, names in ((32, ["dense807", "stair", "components", "dumbbell", "hub"]), (64, ["dense1671", "components200", "stair"])):
        hs = [both_orders(get(name), block)[1] for name in names]
        assert max(int(h.max()) for h in hs) >= 24, block  # more than 300 block pairs in one update launch
        assert any(interior_zeros(h) for h in hs), block  # the H == 0 path between non-empty block columns
        assert any(np.any(np.diff(h) > 1) for h in hs), block  # heights that jump up
    # the hub's order is no reversal, and its envelope is almost empty: 45 blocks below the diagonal hold one row each
    hub = CC.hub()
    assert not np.array_equal(hub.perm, hub.active[::-1])
    assert np.array_equal(both_orders(hub, 32)[0], hub.perm)
    lower = np.tril(hub.pattern[np.ix_(hub.perm, hub.perm)], -1)
    assert lower[:, :288].sum() == 288 and np.all(lower[300, :288])


def test_the_hub_is_symmetric_and_diagonally_dominant():
    A = CC.hub().A
    assert np.array_equal(A, A.T)
    assert np.all(np.diag(A) >= np.abs(A).sum(axis=1) - np.diag(A) + 0.5)


@pytest.mark.parametrize("name", [n for n in CC.EXACT if n != "dense1671"])
def test_host_factorisation_and_solves_are_exact(name):
    case = CC.exact(name)
    Ap = case.A[np.ix_(case.perm, case.perm)]
    L, bad, _ = CC.host_cholesky(Ap)
    assert bad == []
    assert np.array_equal(L, case.L0)
    X0, B = CC.solution(case, 2, 5)
    for x0, b in zip(X0, B):
        w = CC.host_solve(L, b[case.perm])
        assert np.array_equal(w, x0[case.perm])
    frozen = np.setdiff1d(np.arange(case.A.shape[0]), case.active)
    assert not X0[:, frozen].any() and not B[:, frozen].any()


PIVOT_CASES = [("dense807", 32), ("dense807", 64), ("stair", 32), ("stair", 64), ("components", 32), ("components", 64),
               ("components200", 32), ("components200", 64)]


@pytest.mark.parametrize("name,block", PIVOT_CASES)
def test_designed_pivots(name, block):
    case, places = CC.pivot_case(name, block)
    perm, heights = both_orders(case, block)
    assert np.array_equal(perm, case.perm)
    n = len(perm)
    assert places["first"] == 0 and places["end_of_block_0"] == block - 1 and places["start_of_block_2"] == 2 * block
    assert places["last"] == n - 1 and n % block != 0  # the last active row lies in the padded block
    if (name, block) in (("components", 32), ("components200", 64)):
        r = places["in_empty_run"]
        assert r // block in interior_zeros(heights) and not np.any(np.tril(case.pattern[np.ix_(perm, perm)], -1)[r])
    Ap = case.A[np.ix_(perm, perm)]
    L, bad, _ = CC.host_cholesky(Ap)
    assert bad == [] and np.array_equal(L, case.L0)
    assert np.array_equal(CC.host_cholesky_left(Ap)[0], L)  # the variants below are factored left-looking: quicker in numpy
    for place, r in places.items():
        assert case.L0[r, r] == 2. and not case.L0[r + 1:, r].any()
        # pivot r exactly 0, met after the updates of the columns before it (where there are any); nothing else goes bad
        A0 = CC.with_diagonal(case, [(r, -4.)])
        _, bad, pivots = CC.host_cholesky_left(A0[np.ix_(perm, perm)])
        assert bad == [r] and pivots[r] == 0. and np.all(pivots[:r] > 0.), place
        assert (A0[perm[r], perm[r]] > 0.) == bool(case.L0[r, :r].any()), place
        # pivot r exactly 1: a factorisation without a bad pivot, and still an exact solve
        A1 = CC.with_diagonal(case, [(r, -3.)])
        L1, bad, pivots = CC.host_cholesky_left(A1[np.ix_(perm, perm)])
        assert bad == [] and pivots[r] == 1., place
        x0 = CC.solution(case, 1, 9)[0][0]
        assert np.array_equal(CC.host_solve(L1, (A1 @ x0)[perm]), x0[perm]), place
        # + Inf on the diagonal: found at the same row, and no NaN comes of it
        Ainf = CC.with_diagonal(case, [(r, np.inf)])
        Linf, bad, _ = CC.host_cholesky_left(Ainf[np.ix_(perm, perm)])
        assert bad == [r] and np.all(np.isfinite(Linf)), place
    # two at once
    a, b = places["end_of_block_0"], places["last"]
    _, bad, _ = CC.host_cholesky_left(CC.with_diagonal(case, [(a, -4.), (b, -4.)])[np.ix_(perm, perm)])
    assert bad == [a, b]


def test_two_zero_pivots_of_components_lie_in_two_components():
    for name, block in (("components", 32), ("components200", 64)):
        case, places = CC.pivot_case(name, block)
        a, b = places["end_of_block_0"], places["last"]
        Sp = case.pattern[np.ix_(case.perm, case.perm)]
        # band(70, 1) comes first in the solver's order, band(150, 50) last, and nothing ties the two
        assert a < 70 and b >= len(case.perm) - 150 and not Sp[70:, :70].any() and not Sp[-150:, :-150].any()
