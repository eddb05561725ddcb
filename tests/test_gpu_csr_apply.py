"""The device CSR operator (l3k_csr_create / _apply / _apply_energy / _diag / _dirichlet) against scipy where every order of
summation gives the same double, against the longdouble restatements of tests/csr_ref.py with the derived row-wise bound where
it does not, and the refusals of creation.  One matrix of 70 001 rows serves the module: more rows than any launch has groups
(1024 * 256 / 4 = 65 536), so every lanes-per-row route walks several rows per group."""
import numpy as np
import pytest
import torch

import csr_ref as R
from cg_ref import EPS, LD
from l3ster_amd import capi, system

pytestmark = pytest.mark.gpu
N = 70_001
LENGTHS = np.array([0, 1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 200, 1000])
WEIGHTS = np.array([6, 6, 6, 6, 6, 6, 6, 6, 4, 4, 4, 0.6, 0.1])  # (long rows are rare: the matrix stays at about 1.5 M entries)
LANES = [4, 16, 64, 0]
_M = {}


def dev(a, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


def matrix():
    """graph, integer and real values, numpy and device copies, one Context; built once"""
    if _M:
        return _M
    torch.cuda.set_device(0)
    rng = np.random.default_rng(11)
    lens = rng.choice(LENGTHS, size=N, p=WEIGHTS / WEIGHTS.sum())
    lens[0], lens[-1] = 1000, 0  # the first row is the longest, the last one is empty
    for L in LENGTHS:  # (every length occurs)
        assert (lens == L).any()
    row_ptr, col_ind = R.strided_graph(N, lens)
    _M.update(ctx=system.Context(0, torch.cuda.current_stream().cuda_stream), lens=lens, row_ptr=row_ptr, col_ind=col_ind,
              RP=torch.as_tensor(row_ptr, device="cuda"), CI=torch.as_tensor(col_ind, device="cuda"),
              ints=rng.integers(-8, 9, col_ind.size).astype(np.float64), reals=rng.standard_normal(col_ind.size), ops={})
    return _M


def operator(kind, lanes):
    m = matrix()
    if (kind, lanes) not in m["ops"]:
        m["ops"][kind, lanes] = system.CsrOperator(m["ctx"], m["RP"], m["CI"], dev(m[kind]), lanes)
    return m["ops"][kind, lanes]


def scipy_matrix(values):
    import scipy.sparse as sp
    m = matrix()
    return sp.csr_matrix((values, m["col_ind"], m["row_ptr"]), shape=(N, N))


# ------------------------------------------------------------------------------------------------ apply
@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("ncols", [1, 3, 5])
@pytest.mark.parametrize("alpha,beta", [(1.0, 0.0), (-0.5, 2.0), (0.0, 1.0)])
def test_apply_is_exact_on_integers(lanes, ncols, alpha, beta):
    """values and x are integers in [-8, 8]: every order of summation gives the same double, so the device equals scipy"""
    op = operator("ints", lanes)
    rng = np.random.default_rng(100 * ncols + lanes)
    ldx, ldy = N + 7, N + 13
    x = rng.integers(-8, 9, (ncols, ldx)).astype(np.float64)
    y0 = rng.integers(-8, 9, (ncols, ldy)).astype(np.float64)
    X = dev(x)
    Y = dev(y0) if beta != 0.0 else torch.full((ncols, ldy), float("nan"), dtype=torch.float64, device="cuda")
    op.apply(X, Y, alpha, beta)
    got = Y.cpu().numpy()
    A = scipy_matrix(matrix()["ints"])
    want = alpha * (A @ x[:, :N].T).T + (beta * y0[:, :N] if beta != 0.0 else 0.0)
    assert np.isfinite(got[:, :N]).all()  # (beta = 0: y is not read, its NaNs do not survive)
    assert torch.equal(torch.from_numpy(got[:, :N].copy()), torch.from_numpy(np.ascontiguousarray(want)))
    pad = got[:, N:]
    assert np.isnan(pad).all() if beta == 0.0 else np.array_equal(pad, y0[:, N:])  # nothing is written past row n


@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("ncols,alpha,beta", [(1, 1.0, 0.0), (3, -0.5, 2.0), (5, 1.25, -1.0)])
def test_apply_real_values_within_the_row_bound(lanes, ncols, alpha, beta):
    """|y_i - ref_i| <= (len_i + 3) EPS (|alpha| sum_j |a_ij x_j| + |beta y_i|) against the longdouble product"""
    m = matrix()
    op = operator("reals", lanes)
    rng = np.random.default_rng(7 + ncols)
    x, y0 = rng.standard_normal((ncols, N)), rng.standard_normal((ncols, N))
    Y = dev(y0)
    op.apply(dev(x), Y, alpha, beta)
    got = Y.cpu().numpy()
    for c in range(ncols):
        ax, absx = R.apply_ref(m["row_ptr"], m["col_ind"], m["reals"], x[c])
        ref = LD(alpha) * ax + LD(beta) * y0[c].astype(LD)
        bound = R.row_bound(m["lens"], abs(alpha) * absx + np.abs(beta * y0[c]))
        err = np.abs(got[c].astype(LD) - ref).astype(np.float64)
        worst = int(np.argmax(err - bound))
        print(f"lanes {lanes} column {c}: largest error / bound {np.max(err[bound > 0] / bound[bound > 0]):.3f}")
        assert (err <= bound).all(), (worst, err[worst], bound[worst])


@pytest.mark.parametrize("lanes", LANES)
def test_apply_and_energy_are_reproducible_and_energy_is_right(lanes):
    m = matrix()
    op = operator("reals", lanes)
    x = np.random.default_rng(21).standard_normal(N)
    X = dev(x)
    y1, y2, e1, e2 = (torch.full((N,), float("nan"), dtype=torch.float64, device="cuda") for _ in range(4))
    sentinel = torch.arange(10.0, 18.0, dtype=torch.float64, device="cuda")
    s1, s2 = sentinel.clone(), sentinel.clone()
    op.apply(X, y1)
    op.apply(X, y2)
    op.apply_energy(X, e1, s1)
    op.apply_energy(X, e2, s2)
    assert torch.equal(y1, y2) and torch.equal(e1, e2) and torch.equal(s1, s2)  # bit for bit
    assert torch.equal(y1, e1)  # the same sums in the same order
    keep = [0, 2, 3, 4, 5, 6, 7]
    assert torch.equal(s1[keep], sentinel[keep])  # only s[1] is written
    ax, absx = R.apply_ref(m["row_ptr"], m["col_ind"], m["reals"], x)
    assert (np.abs(e1.cpu().numpy().astype(LD) - ax).astype(np.float64) <= R.row_bound(m["lens"], absx)).all()
    want = np.sum(x.astype(LD) * ax)
    bound = (N + int(m["lens"].max()) + 3) * EPS * float(np.sum(np.abs(x).astype(LD) * absx))
    err = abs(float(LD(s1[1].item()) - want))
    print(f"lanes {lanes}: <x, A x> error {err:.3e}, bound {bound:.3e}")
    assert err <= bound


def test_info_agrees_with_numpy():
    m = matrix()
    lens = m["lens"]
    for lanes in LANES:
        i = operator("reals", lanes).info()
        assert (i.n, i.nnz, i.n_empty_rows, i.max_row_len) == (N, int(lens.sum()), int((lens == 0).sum()), 1000)
        assert i.mean_row_len == float(lens.sum()) / float((lens > 0).sum())
        assert i.lanes_per_row == lanes if lanes else i.lanes_per_row in (4, 16, 64)


def test_empty_operators_apply_as_beta_y():
    ctx = matrix()["ctx"]
    none_i, none_d = torch.zeros(0, dtype=torch.int32, device="cuda"), torch.zeros(0, dtype=torch.float64, device="cuda")
    zero = system.CsrOperator(ctx, torch.zeros(1, dtype=torch.int64, device="cuda"), none_i, none_d)
    assert (zero.info().n, zero.info().nnz) == (0, 0)
    zero.apply(torch.zeros((1, 0), dtype=torch.float64, device="cuda"), torch.zeros((1, 0), dtype=torch.float64, device="cuda"), 1.0, 2.0)
    for lanes in LANES:
        op = system.CsrOperator(ctx, torch.zeros(6, dtype=torch.int64, device="cuda"), none_i, none_d, lanes)
        i = op.info()
        assert (i.n, i.nnz, i.n_empty_rows, i.max_row_len, i.mean_row_len) == (5, 0, 5, 0, 0.0)
        x = dev(np.arange(5.0))
        y = dev(np.arange(1.0, 6.0))
        op.apply(x, y, 3.0, 2.0)
        assert torch.equal(y, dev(2.0 * np.arange(1.0, 6.0)))
        y = torch.full((5,), float("nan"), dtype=torch.float64, device="cuda")
        op.apply(x, y, 3.0, 0.0)
        assert torch.equal(y, torch.zeros_like(y))
        s = torch.arange(10.0, 18.0, dtype=torch.float64, device="cuda")
        op.apply_energy(x, y, s)
        assert s[1].item() == 0.0 and s[0].item() == 10.0 and not y.any()
        assert not op.diag().any() and not op.jacobi_inverse().any()


# ------------------------------------------------------------------------------------------------ diagonal
@pytest.mark.parametrize("damping,threshold", [(1.0, 0.25), (0.8, 1e-3), (1.0, 0.0)])
def test_diag_equals_the_restatement(damping, threshold):
    """One correctly rounded division per row: exact equality.  Rows without a stored diagonal give diag 0, empty rows minv 0.
    With threshold 0 a non-empty row without a diagonal is the formula's 1 / 0; that quotient is compared where it is finite."""
    m = matrix()
    op = operator("reals", 0)
    diag, minv = R.diag_ref(m["row_ptr"], m["col_ind"], m["reals"], damping, threshold)
    rows = R.row_of_entry(m["row_ptr"])
    stored = np.zeros(N, dtype=bool)
    stored[rows[m["col_ind"] == rows]] = True
    assert (~stored & (m["lens"] > 0)).sum() > 1000 and stored.sum() > 1000
    got_d, got_m = op.diag().cpu().numpy(), op.jacobi_inverse(damping, threshold).cpu().numpy()
    assert np.array_equal(got_d, diag) and not got_d[~stored].any()
    assert not got_m[m["lens"] == 0].any()
    finite = np.isfinite(minv)
    assert finite.all() or threshold == 0.0
    assert np.array_equal(got_m[finite], minv[finite])


# ------------------------------------------------------------------------------------------------ Dirichlet conditions
def dirichlet_case(ncols, seed=31):
    m = matrix()
    rng = np.random.default_rng(seed)
    rows = R.row_of_entry(m["row_ptr"])
    stored = np.zeros(N, dtype=bool)
    stored[rows[m["col_ind"] == rows]] = True
    mask = ((rng.random(N) < 0.2) & stored).astype(np.uint8)
    mask[0] = 1  # (the longest row as a Dirichlet row)
    return mask, stored, rng.standard_normal((ncols, N)), rng.standard_normal((ncols, N))


@pytest.mark.parametrize("lanes", [0, 4, 64])
@pytest.mark.parametrize("ncols", [1, 3])
def test_dirichlet_matches_the_restatement(lanes, ncols):
    m = matrix()
    mask, _, g, rhs = dirichlet_case(ncols)
    values = dev(m["reals"])
    op = system.CsrOperator(m["ctx"], m["RP"], m["CI"], values, lanes)
    G, F = dev(g), dev(rhs)
    op.dirichlet(dev(mask, torch.uint8), G if ncols > 1 else G[0], F if ncols > 1 else F[0])
    new, ref, absv = R.dirichlet_ref(m["row_ptr"], m["col_ind"], m["reals"], mask, g, rhs)
    assert torch.equal(values.cpu(), torch.from_numpy(new))  # bit for bit: old entries, zeros and ones
    err = np.abs(F.cpu().numpy().astype(LD) - ref).astype(np.float64)
    bound = R.row_bound(np.broadcast_to(m["lens"], err.shape), absv)
    assert (err <= bound).all()
    assert np.array_equal(F.cpu().numpy()[:, mask.astype(bool)], g[:, mask.astype(bool)])
    assert torch.equal(G, dev(g))


def test_dirichlet_refuses_a_masked_row_without_diagonal():
    m = matrix()
    mask, stored, g, rhs = dirichlet_case(1)
    bad = int(np.flatnonzero(~stored & (m["lens"] > 0))[5])
    empty = int(np.flatnonzero(m["lens"] == 0)[0])
    for row in (bad, empty):
        mk = mask.copy()
        mk[row] = 1
        values = dev(m["reals"])
        F = dev(rhs)
        op = system.CsrOperator(m["ctx"], m["RP"], m["CI"], values, 0)
        first = int(np.flatnonzero(mk.astype(bool) & ~stored)[0])
        with pytest.raises(capi.L3KError, match=f"libl3k error -1: l3k_csr_dirichlet: the Dirichlet row {first} has no stored diagonal"):
            op.dirichlet(dev(mk, torch.uint8), dev(g)[0], F[0])
        assert torch.equal(values, dev(m["reals"])) and torch.equal(F, dev(rhs))  # untouched


# ------------------------------------------------------------------------------------------------ creation
SIX_PTR = [0, 2, 3, 3, 5, 6, 8]
SIX_COL = [0, 3, 1, 2, 4, 3, 0, 5]


def six(row_ptr=SIX_PTR, col_ind=SIX_COL, lanes=0):
    ctx = matrix()["ctx"]
    return system.CsrOperator(ctx, torch.tensor(row_ptr, dtype=torch.int64, device="cuda"),
                              torch.tensor(col_ind, dtype=torch.int32, device="cuda"),
                              torch.ones(len(col_ind), dtype=torch.float64, device="cuda"), lanes)


def test_creation_refusals():
    """each on a six-row graph; the columns are only read once row_ptr has passed"""
    op = six()
    y = op.apply(torch.ones(6, dtype=torch.float64, device="cuda"), torch.empty(6, dtype=torch.float64, device="cuda"))
    assert y.tolist() == [2.0, 1.0, 0.0, 2.0, 1.0, 2.0]

    def edited(base, at, value):
        out = list(base)
        out[at] = value
        return out

    cases = [
        (dict(row_ptr=edited(SIX_PTR, 3, 2)), "row_ptr decreases at row 2"),
        (dict(row_ptr=edited(SIX_PTR, 0, 1)), r"row_ptr\[0\] is not 0"),
        (dict(col_ind=edited(SIX_COL, 1, 6)), r"row 0 has a column index outside \[0, n\)"),
        (dict(col_ind=edited(SIX_COL, 2, -1)), r"row 1 has a column index outside \[0, n\)"),
        (dict(col_ind=edited(SIX_COL, 4, 2)), "the column indices of row 3 are not strictly ascending"),
        (dict(col_ind=edited(SIX_COL, 6, 5)), "the column indices of row 5 are not strictly ascending"),
        (dict(lanes=8), "lanes_per_row = 8"),
    ]
    for kwargs, message in cases:
        with pytest.raises(capi.L3KError, match="libl3k error -1: l3k_csr_create: " + message):
            six(**kwargs)
    # both a bad row_ptr and a bad column: row_ptr is named, the columns were not looked at
    with pytest.raises(capi.L3KError, match="row_ptr decreases at row 2"):
        six(row_ptr=edited(SIX_PTR, 3, 2), col_ind=edited(SIX_COL, 1, 6))
    with pytest.raises(capi.L3KError, match="row_ptr\\[n\\] entries"):
        six(col_ind=SIX_COL + [1])
