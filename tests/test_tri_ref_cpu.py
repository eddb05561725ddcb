"""tests/tri_ref.py, the numpy restatement of l3k_tri, pinned against dense definitions: ILU(0) reproduces A on its pattern and is
the exact LU where the pattern has no fill, SSOR equals its dense formula, the levels equal a brute-force longest path, the launch
plan of the grid is the one the issue of this feature states, and the restatement itself satisfies the bounds the device is held to."""
import numpy as np
import pytest

import tri_ref as R
from tri_ref import EPS, LD

PATTERNS = {
    "spd": lambda: R.spd_matrix(100),
    "band": lambda: R.band(120, 17),
    "grid": lambda: R.grid(9),
    "chains": lambda: R.chains(5),
}


def with_empty_rows(A, P, every=4):
    """rows every-th row emptied: their columns stay stored in the other rows"""
    P = P.copy()
    P[::every] = False
    return np.where(P, A, 0.0), P


@pytest.mark.parametrize("name", sorted(PATTERNS))
@pytest.mark.parametrize("dtype", [LD, np.float64])
def test_ilu0_reproduces_a_on_its_pattern(name, dtype):
    """(L U)_ij = a_ij on every stored (i, j): in longdouble to 1e-17 |L| |U|, in float64 inside factor_bound"""
    A, P = PATTERNS[name]()
    F, n_bad, _ = R.ilu0(A, P, dtype=dtype)
    err, bound = R.factor_bound(A, F, P)
    assert n_bad == 0 and np.isfinite(err[..., P]).all()
    if dtype is LD:
        assert (err[..., P] <= bound[..., P] * 1e-3 + 1e-300).all()
    else:
        assert (err[..., P] <= bound[..., P]).all()
        assert err[..., P].max() > 0


def test_ilu0_ignores_empty_rows_and_their_columns():
    A, P = with_empty_rows(*R.grid(8))
    F, n_bad, _ = R.ilu0(A, P, dtype=np.float64)
    B = R.block(P)
    assert n_bad == 0 and np.array_equal(F[P & ~B], A[P & ~B]) and (~B & P).any()
    err, bound = R.factor_bound(A, F, P)
    assert (err[B] <= bound[B]).all() and np.isnan(err[~B]).all()
    keep = R.active_rows(P)
    F2, _, _ = R.ilu0(A[np.ix_(keep, keep)], P[np.ix_(keep, keep)], dtype=np.float64)
    assert np.array_equal(F[np.ix_(keep, keep)], F2)  # the factor of the active block, as if the rest were not there


@pytest.mark.parametrize("make", [lambda: (R.spd_matrix(60)[0] + 0.3 * np.eye(60, k=1), R.tridiagonal_pattern(60)), lambda: R.band(90, 13)])
def test_ilu0_is_the_exact_lu_without_fill(make):
    A, P = make()
    F, _, _ = R.ilu0(A, P)
    Lm, U = R.lu_nopivot(A)
    assert np.abs(np.tril(F, -1) - np.tril(Lm, -1)).max() <= 1e-17 * np.abs(Lm).max()
    assert np.abs(np.triu(F) - U).max() <= 1e-16 * np.abs(U).max()
    assert np.array_equal(np.where(P, 0, Lm + U - np.eye(len(A))), np.zeros_like(A, dtype=LD))  # (no fill outside the pattern)


def test_thresholds_change_the_diagonal_before_the_factorisation():
    A, P = R.grid(6)
    A[7, 7] = -A[7, 7]
    T = R.thresholded(A, P, 0.5, 1.25)
    d = np.diag(A).astype(LD)
    assert np.array_equal(np.diag(T), np.where(d < 0, -0.5, 0.5) + LD(1.25) * d) and T[7, 7] == -8.3125 and T[0, 0] == 8.3125
    assert np.array_equal(T - np.diag(np.diag(T)), A - np.diag(np.diag(A)))
    F, _, _ = R.ilu0(A, P, 0.5, 1.25)
    assert np.array_equal(F, R.ilu0(T, P)[0])


def test_zero_pivot_becomes_one():
    A, P = np.ones((2, 2)), np.ones((2, 2), dtype=bool)
    F, n_bad, first = R.ilu0(A, P, dtype=np.float64)
    assert (n_bad, first) == (1, 1) and np.isfinite(F).all() and F[1, 1] == 1.0 and F[1, 0] == 1.0


@pytest.mark.parametrize("omega", [1.0, 1.3, 0.6])
def test_ssor_against_its_dense_formula(omega):
    A, P = R.grid(7)
    M = R.ssor_dense(A, omega)
    pre = R.Preconditioner(A, P, "sgs", omega)
    r = np.cos(np.arange(len(A)) * 0.7).astype(LD)
    z = pre(r)
    assert np.abs(M @ z - r).max() <= 1e-17 * np.abs(M).sum(1).max() * np.abs(z).max()
    if omega == 1.0:
        D = np.diag(np.diag(A)).astype(LD)
        assert np.abs(M - (D + np.tril(A, -1)) @ np.diag(1 / np.diag(D)) @ (D + np.triu(A, 1))).max() <= 1e-17 * np.abs(M).max()


def test_ilu0_apply_inverts_l_u():
    A, P = R.band(80, 9)
    pre = R.Preconditioner(A, P, "ilu0")
    r = np.sin(np.arange(80) * 0.3).astype(LD)
    assert np.abs(A.astype(LD) @ pre(r) - r).max() <= 1e-16 * np.abs(A).sum(1).max() * np.abs(pre(r)).max()  # (ILU(0) = LU here)


@pytest.mark.parametrize("kind", ["sgs", "ilu0"])
def test_float64_solves_satisfy_the_solve_bound(kind):
    A, P = with_empty_rows(*R.grid(9), every=5)
    pre = R.Preconditioner(A, P, kind, dtype=np.float64)
    r = np.cos(np.arange(len(A)) * 0.37)
    y = pre.lower(r)
    z = pre.upper(y)
    Tl, Tu, s = R.triangles(pre.F, P, kind)
    for T, out, rhs in ((Tl, y, r), (Tu, z, s * y.astype(LD))):
        err, bound = R.solve_bound(T, out, rhs, pre.active)
        assert (err <= bound).all() and err.max() > 0
    assert not y[~pre.active].any() and not z[~pre.active].any()


def longest_path(P, upper):
    """brute force: the longest chain of dependencies ending in every row, by relaxation until nothing changes"""
    B, a = R.block(P), R.active_rows(P)
    n = len(P)
    level = a.astype(np.int32)
    changed = True
    while changed:
        changed = False
        for i in range(n):
            for j in np.nonzero(B[i])[0]:
                if (j > i if upper else j < i) and level[i] < level[j] + 1:
                    level[i], changed = level[j] + 1, True
    return level


@pytest.mark.parametrize("upper", [False, True])
def test_levels_against_the_longest_path(upper):
    rng = np.random.default_rng(8)
    for name in sorted(PATTERNS):
        A, P = PATTERNS[name]()
        for Q in (P, with_empty_rows(A, P)[1], P & (rng.uniform(size=P.shape) < 0.6) | np.eye(len(P), dtype=bool)):
            level, n_levels = R.levels(Q, upper)
            assert np.array_equal(level, longest_path(Q, upper)) and n_levels == level.max()
            rows, ptr = R.rows_by_level(level)
            assert len(rows) == R.active_rows(Q).sum() and ptr[-1] == len(rows) and len(ptr) == n_levels + 1
            for lv in range(n_levels):
                mine = rows[ptr[lv]:ptr[lv + 1]]
                assert (level[mine] == lv + 1).all() and (np.diff(mine) > 0).all()


def test_designed_level_structures():
    assert R.levels(R.spd_matrix(100)[1])[1] == 100
    lv, nl = R.levels(R.grid(24)[1])
    sizes = np.bincount(lv)[1:]
    assert nl == 47 and sizes.max() == 24 and np.array_equal(sizes, np.concatenate([np.arange(1, 25), np.arange(23, 0, -1)]))
    assert np.array_equal(lv, R.levels(R.grid(24)[1], upper=True)[0][::-1])
    plan = R.launch_plan(lv, 1)
    assert len(plan) == 47 and sum(not f for _, _, f in plan) == 45 and plan[0] == (0, 1, True) and plan[-1] == (46, 47, True)
    assert R.launch_plan(lv, 1_000_000) == [(0, 47, True)]
    assert R.launch_plan(lv, 16) == [(0, 16, True)] + [(k, k + 1, False) for k in range(16, 31)] + [(31, 47, True)]
    assert [b - a for a, b, _ in R.launch_plan(R.levels(R.spd_matrix(5000)[1])[0], 64)] == [4096, 904]  # (the cap on a fused run)


def test_pcg_restatement_and_choose_tol():
    A, P = R.spd_matrix(100)
    xs = np.cos(0.3 * np.arange(100))
    b = A @ xs
    out = R.pcg(lambda v: A.astype(v.dtype) @ v, b, np.zeros(100), R.Preconditioner(A, P, "ilu0"), tol=1e-6)
    assert out["iterations"] == 1 and out["achieved_tol"] <= 1e-17  # (M = A)
    jac = R.pcg(lambda v: A.astype(v.dtype) @ v, b, np.zeros(100), lambda r: r / np.diag(A).astype(LD), tol=0.0, max_iters=12)
    tol, its = R.choose_tol(jac["history"], near=3)
    k = next(i for i, e in enumerate(jac["history"]) if e <= tol)
    assert its == k + 1 and R.choose_tol(jac["history"], near=3, also=[jac["history"]]) == (tol, its)
    with pytest.raises(AssertionError):
        R.choose_tol(jac["history"], near=3, also=[[2 * e for e in jac["history"]]])
    assert tol / jac["history"][k] >= 1.5 and jac["history"][k - 1] / tol >= 1.5 and min(jac["history"][:k]) >= 1.5 * tol
    assert np.abs(jac["x"] - xs).max() <= 1e-3
