"""The band Cholesky solver on the device on the designed systems of tests/chol_cases.py: envelopes with up to 26 blocks below the
diagonal (351 block pairs in one cholUpdateKernel launch), runs of H = 0 between non-empty block columns, heights that jump, and a
tall envelope that is almost empty; 70 columns at once; NaN in the triangle the solver must not read; pivots designed to be exactly
0, exactly 1 or +Inf at chosen columns of chosen blocks.

The exact cases carry no tolerance: their factors and solutions are small integers (tests/chol_cases.py explains why every
intermediate is exact in float64), so the device returns the prescribed solution bit for bit or the test fails.  The hub case has
real values and is held to the bars of tests/test_gpu_chol.py."""
import numpy as np
import pytest

import chol_cases as CC
import chol_ref as R
from l3ster_amd import capi, solve
from test_gpu_chol import SENTINEL, backward_bar, backward_error, ctx, dev, operator  # noqa: F401 (ctx is a fixture)

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def heights_of(case, block):
    return R.envelope(case.A.shape[0], *R.csr_from_dense(case.A, case.pattern)[:2], case.perm, block)


def frozen_rows(case):
    return np.setdiff1d(np.arange(case.A.shape[0]), case.active)


def start(case, n):
    """The x a solve starts from: distinct values, none of them a solution's"""
    return SENTINEL + np.arange(n)


def assert_exact_solve(chol, case, seed, tag):
    n = case.A.shape[0]
    X0, B = CC.solution(case, 1, seed)
    x_in = start(case, n)
    x = chol.solve(dev(B[0]), dev(x_in)).cpu().numpy()
    want = np.where(np.isin(np.arange(n), case.active), X0[0], x_in)
    wrong = np.nonzero(bits(x) != bits(want))[0]
    assert len(wrong) == 0, (tag, len(wrong), wrong[:5], x[wrong[:5]], want[wrong[:5]])


# ------------------------------------------------------------------------------------------------------------ a. exact solves
EXACT_RUNS = [(name, block) for name in CC.EXACT for block in (32, 64)]


@pytest.mark.parametrize("name,block", EXACT_RUNS)
def test_exact_solve(ctx, name, block):
    case = CC.exact(name)
    h = heights_of(case, block)
    chol = solve.CholeskySolver(operator(ctx, case.A, case.pattern), block=block)
    info = chol.info
    assert info.block == block and info.n == case.A.shape[0] and info.n_active == len(case.active)
    assert info.n_blocks == len(h) and info.max_height == h.max()
    chol.factor()
    info = chol.info
    assert info.factored == 1 and info.n_bad_pivots == 0 and info.first_bad_row == -1
    assert_exact_solve(chol, case, 21, (name, block))
    if name.endswith("_embedded"):
        assert len(frozen_rows(case)) == CC.EMBEDDED[name][1]  # (assert_exact_solve demanded the caller's bits on them)


def test_one_block_of_powers_of_two(ctx):
    """What the exact cases lean on: the device's f64 square roots of 1, 4 and 16 and its divisions by 1, 2 and 4 are exact.  A
    diagonal matrix with those entries in one block, solved for integers"""
    for block in (32, 64):
        d = np.tile([1., 4., 16.], block)[:block]
        chol = solve.CholeskySolver(operator(ctx, np.diag(d)), block=block).factor()
        x0 = np.arange(block) - 8.
        x = chol.solve(dev(d * x0 + 0.)).cpu().numpy()
        assert same_bits(x, x0 + 0.), (block, x, x0)


# ------------------------------------------------------------------------------------------------------------ b. many columns
PAD = 7


@pytest.mark.parametrize("name,block", [("stair", 32), ("stair", 64), ("dense807", 32), ("dense807", 64)])
def test_column_counts_grow_and_shrink_on_one_solver(ctx, name, block):
    case = CC.exact(name)
    n = case.A.shape[0]
    chol = solve.CholeskySolver(operator(ctx, case.A, case.pattern), block=block).factor()
    h_max = int(heights_of(case, block).max())
    assert chol.info.max_height == h_max and h_max >= (5 if name == "stair" else 12)  # scratch of [70][h_max * block] doubles
    for k, nc in enumerate((1, 37, 2, 70)):
        X0, B = CC.solution(case, nc, 300 + nc)
        # [nc + 1, n + PAD]: PAD entries behind every column and one more row behind the last column, all of them sentinels
        buf = np.full((nc + 1, n + PAD), SENTINEL) + np.arange((nc + 1) * (n + PAD)).reshape(nc + 1, -1)
        rhs = buf.copy()
        rhs[:nc, :n] = B
        forms = ("aliased", "separate") if k % 2 == 0 else ("separate", "aliased")
        for form in forms:
            Bd = dev(rhs)
            if form == "aliased":
                Xd = Bd
                chol.solve(Bd[:nc])  # b aliased to x
            else:
                Xd = dev(buf)
                chol.solve(Bd[:nc], Xd[:nc])
                assert same_bits(Bd.cpu().numpy(), rhs), (nc, form)  # b is read only
            X = Xd.cpu().numpy()
            for c in range(nc):
                wrong = np.nonzero(bits(X[c, :n]) != bits(X0[c]))[0]
                assert len(wrong) == 0, (nc, form, c, len(wrong), wrong[:5], X[c, wrong[:5]], X0[c, wrong[:5]])
            assert same_bits(X[:nc, n:], buf[:nc, n:]), (nc, form)
            assert same_bits(X[nc], buf[nc]), (nc, form)


# ------------------------------------------------------------------------------------------------------------ c. lower triangle only
@pytest.mark.parametrize("name", ["components", "stair"])
@pytest.mark.parametrize("block", [32, 64])
def test_the_other_triangle_is_never_read(ctx, block, name):
    case = CC.exact(name)
    n = case.A.shape[0]
    inv = R.inverse(n, case.perm)  # (tests/test_chol_cases_cpu.py: case.perm is what l3k_chol_order returns)
    op = operator(ctx, case.A, case.pattern)
    rp, ci = op.row_ptr.cpu().numpy(), op.col_ind.cpu().numpy()
    rows = np.repeat(np.arange(n), np.diff(rp))
    upper = inv[rows] < inv[ci]
    assert upper.sum() == (len(ci) - len(case.active)) // 2 > 0
    op.values[dev(upper, torch.bool)] = float("nan")
    assert torch.isnan(op.values).sum().item() == upper.sum()
    chol = solve.CholeskySolver(op, block=block).factor()
    assert chol.info.n_bad_pivots == 0
    assert_exact_solve(chol, case, 22, (name, block, "NaN above the diagonal of the ordered matrix"))


# ------------------------------------------------------------------------------------------------------------ d. hub
@pytest.mark.parametrize("block", [32, 64])
def test_hub_tall_and_almost_empty(ctx, block):
    case = CC.hub()
    A, n = case.A, case.A.shape[0]
    op = operator(ctx, A, case.pattern)
    b = np.random.default_rng(41).standard_normal(n)
    runs = []
    for _ in range(2):
        chol = solve.CholeskySolver(op, block=block).factor()
        assert chol.info.n_bad_pivots == 0 and chol.info.max_height == heights_of(case, block).max()
        runs.append(chol.solve(dev(b)).cpu().numpy())
    assert same_bits(runs[0], runs[1])
    x = runs[0]
    assert np.all(np.isfinite(x))
    x_np = np.linalg.solve(A, b)
    ours, lapack = backward_error(A, x, b), backward_error(A, x_np, b)
    forward = np.linalg.norm(x - x_np) / np.linalg.norm(x_np)
    kappa = np.linalg.cond(A, 2)
    print(f"hub NB {block}: n {n}, kappa_2 {kappa:.2e}, backward error {ours:.2e} (numpy.linalg.solve: {lapack:.2e}), forward {forward:.2e}, "
          f"bar {backward_bar(n):.2e}")
    assert ours <= backward_bar(n), (ours, backward_bar(n))
    assert forward <= kappa * backward_bar(n), (forward, kappa)


# ------------------------------------------------------------------------------------------------------------ e. designed pivots
def diagonal_slots(op):
    """Index into op.values of every row's diagonal entry (-1: the row stores none)"""
    rp, ci = op.row_ptr.cpu().numpy(), op.col_ind.cpu().numpy()
    rows = np.repeat(np.arange(op.n), np.diff(rp))
    at = np.full(op.n, -1, dtype=np.int64)
    at[rows[rows == ci]] = np.nonzero(rows == ci)[0]
    return at


def assert_refused(chol, case, rows, n_bad, tag):
    """factor() returns -2 with the first of the ordered rows `rows` in the caller's numbering and n_bad bad pivots in all; a
    following solve returns -1 and leaves x alone"""
    with pytest.raises(capi.L3KError, match="error -2: .*matrix is not positive definite"):
        chol.factor()
    info = chol.info
    assert info.factored == 0 and info.first_bad_row == case.perm[min(rows)], (tag, info)
    assert info.n_bad_pivots >= 1 and info.n_bad_pivots == n_bad, (tag, info)
    x_in = start(case, case.A.shape[0])
    x = dev(x_in)
    with pytest.raises(capi.L3KError, match="error -1"):
        chol.solve(dev(CC.solution(case, 1, 23)[1][0]), x)
    assert same_bits(x.cpu().numpy(), x_in), tag


PIVOT_RUNS = [("dense807", 32), ("dense807", 64), ("stair", 32), ("stair", 64), ("components", 32), ("components200", 64)]


@pytest.mark.parametrize("name,block", PIVOT_RUNS)
def test_designed_pivots(ctx, name, block):
    """tests/test_chol_cases_cpu.py factors the same variants on the host: lowering the diagonal entry of a designed row by 4 makes
    its pivot exactly 0 once the columns before it are eliminated, by 3 exactly 1, and no other pivot changes"""
    case, places = CC.pivot_case(name, block)
    assert set(places) >= {"first", "end_of_block_0", "start_of_block_2", "last"}
    assert ("in_empty_run" in places) == name.startswith("components")
    op = operator(ctx, case.A, case.pattern)
    slot = diagonal_slots(op)
    original = op.values.clone()
    chol = solve.CholeskySolver(op, block=block)
    for place, r in places.items():
        tag = (name, block, place, r)
        at = int(slot[case.perm[r]])
        keep = original[at].item()
        for value in (keep - 4., float("inf")):
            op.values[at] = value
            assert_refused(chol, case, [r], 1, tag + (value,))
        # exactly 1 is a good pivot: the matrix is A - 3 e e^T, and the solve of its system is exact too
        op.values[at] = keep - 3.
        chol.factor()
        assert chol.info.factored == 1 and chol.info.n_bad_pivots == 0 and chol.info.first_bad_row == -1, tag
        moved = case._replace(A=CC.with_diagonal(case, [(r, -3.)]))
        assert_exact_solve(chol, moved, 24, tag + ("pivot 1",))
        op.values[at] = keep
        assert torch.equal(op.values, original)
    if "in_empty_run" in places:
        # two zero pivots in two components: both counted, the one that comes first in the solver's order reported
        pair = [places["last"], places["end_of_block_0"]]
        for r in pair:
            op.values[int(slot[case.perm[r]])] -= 4.
        assert_refused(chol, case, pair, 2, (name, block, "two zero pivots", pair))
        op.values.copy_(original)
    chol.factor()
    assert chol.info.factored == 1 and chol.info.n_bad_pivots == 0 and chol.info.first_bad_row == -1
    assert_exact_solve(chol, case, 25, (name, block, "values restored"))
