"""The band Cholesky solver on the device (l3k_chol_*, solve.CholeskySolver, solve.direct_solve, l3k::Cholesky).

Bars (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., Thm 10.4, with the crude bound |L||L^T| <= n ||A||):
backward error ||b - A x||_2 / (||A||_2 ||x||_2) <= gamma_(3n+1) n with gamma_k = k u / (1 - k u), u = 2^-53, and forward error
against numpy.linalg.solve <= kappa_2(A) times that, kappa_2 computed by numpy.  n is the number of rows that take part (the
active rows), A the matrix on them.  Every synthetic case also measures numpy's own backward error; the largest of both are
printed (DESIGN.md 4.22 quotes them: 2.3e-16 against numpy's 2.1e-16)."""
import subprocess

import numpy as np
import pytest

import chol_ref as R
from l3ster_amd import capi, solve, system
from test_cpp_chol import build as build_shim

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

UNIT = 2.0 ** -53
U = 3
D2, ADI = system.KERNEL_DIFFUSION2D, system.KERNEL_ADIABATIC2D


def gamma(k):
    return k * UNIT / (1 - k * UNIT)


def backward_bar(n):
    return gamma(3 * n + 1) * n


def backward_error(A, x, b):
    return np.linalg.norm(b - A @ x) / (np.linalg.norm(A, 2) * np.linalg.norm(x))


@pytest.fixture(scope="module")
def ctx():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    torch.cuda.set_device(0)
    return system.Context(0, torch.cuda.current_stream().cuda_stream)


def dev(a, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def operator(ctx, A, pattern=None):
    row_ptr, col_ind, values = R.csr_from_dense(A, pattern)
    return system.CsrOperator(ctx, dev(row_ptr, torch.int64), dev(col_ind, torch.int32), dev(values))


def dense_of(op):
    rp, ci, v = op.row_ptr.cpu().numpy(), op.col_ind.cpu().numpy(), op.values.cpu().numpy()
    A = np.zeros((op.n, op.n))
    A[np.repeat(np.arange(op.n), np.diff(rp)), ci] = v
    return A


def spd_band(n, bw, rng):
    """B B^T + I, B lower triangular of half-bandwidth bw (scaled to keep the condition number modest): the matrix has exactly
    that band, so restricting it to the band changes nothing and it is positive definite by construction"""
    i, j = np.indices((n, n))
    B = np.where((i >= j) & (i - j <= bw), rng.standard_normal((n, n)), 0.) / np.sqrt(bw + 1.)
    A = B @ B.T + np.eye(n)
    return A, np.abs(i - j) <= bw


def scrambled(A, pattern, rng, n_empty=5):
    """A under a random symmetric permutation with n_empty empty rows (and columns) inserted: (matrix, pattern, active rows)"""
    n = A.shape[0] + n_empty
    q = rng.permutation(n)[:A.shape[0]]  # where the rows of A go, in random order
    A2, P2 = np.zeros((n, n)), np.zeros((n, n), dtype=bool)
    A2[np.ix_(q, q)] = A
    P2[np.ix_(q, q)] = pattern
    return A2, P2, np.sort(q)


SENTINEL = -123.456


def check_solve(ctx, A, pattern, active, rng, block, tag):
    """Creates, factors and solves on the device; asserts the two bars on the active rows and that x keeps its bits elsewhere.
    Returns (our backward error, numpy's)"""
    n, na = A.shape[0], len(active)
    op = operator(ctx, A, pattern)
    chol = solve.CholeskySolver(op, block=block)
    info = chol.info
    assert info.block == block and info.n == n and info.n_active == na and info.factored == 0
    chol.factor()
    assert chol.info.factored == 1 and chol.info.n_bad_pivots == 0 and chol.info.first_bad_row == -1
    b = rng.standard_normal(n)
    x0 = np.full(n, SENTINEL) + np.arange(n)
    x = chol.solve(dev(b), dev(x0)).cpu().numpy()
    frozen = np.setdiff1d(np.arange(n), active)
    assert np.array_equal(x[frozen].view(np.int64), x0[frozen].view(np.int64)), tag
    Aa, ba, xa = A[np.ix_(active, active)], b[active], x[active]
    assert np.all(np.isfinite(xa)), tag
    x_np = np.linalg.solve(Aa, ba)
    ours, lapack = backward_error(Aa, xa, ba), backward_error(Aa, x_np, ba)
    forward = np.linalg.norm(xa - x_np) / np.linalg.norm(x_np)
    kappa = np.linalg.cond(Aa, 2)
    assert ours <= backward_bar(na), (tag, ours, backward_bar(na))
    assert forward <= kappa * backward_bar(na), (tag, forward, kappa)
    return ours, lapack


def bandwidths(n, nb):
    return sorted({bw for bw in (0, 1, nb - 1, nb, nb + 1, 2 * nb + 3, n - 1) if 0 <= bw <= n - 1})


@pytest.mark.parametrize("size", ["1", "NB-1", "NB", "NB+1", "3NB+5"])
@pytest.mark.parametrize("block", [32, 64])
def test_synthetic_band_matrices(ctx, block, size):
    n = {"1": 1, "NB-1": block - 1, "NB": block, "NB+1": block + 1, "3NB+5": 3 * block + 5}[size]
    rng = np.random.default_rng(1000 * block + n)
    worst = [0., 0.]
    for bw in bandwidths(n, block):
        A, pattern = spd_band(n, bw, rng)
        plain = check_solve(ctx, A, pattern, np.arange(n), rng, block, (n, bw, "as generated"))
        mixed = check_solve(ctx, *scrambled(A, pattern, rng), rng, block, (n, bw, "permuted, empty rows"))
        worst = [max(worst[0], plain[0], mixed[0]), max(worst[1], plain[1], mixed[1])]
    print(f"NB {block} n {n}: largest backward error {worst[0]:.2e} (numpy.linalg.solve: {worst[1]:.2e}), bar {backward_bar(n):.2e}")


def thomas(lower, diag, upper, b):
    """Tridiagonal solve on the host: lower[i] = a(i, i-1), upper[i] = a(i, i+1)"""
    n = len(diag)
    c, d = np.zeros(n), np.zeros(n)
    c[0], d[0] = upper[0] / diag[0], b[0] / diag[0]
    for i in range(1, n):
        m = diag[i] - lower[i] * c[i - 1]
        c[i] = upper[i] / m
        d[i] = (b[i] - lower[i] * d[i - 1]) / m
    x = d.copy()
    for i in range(n - 2, -1, -1):
        x[i] = d[i] - c[i] * x[i + 1]
    return x


def test_one_long_chain(ctx):
    """A tridiagonal matrix of 300001 rows in its natural order: fill, gather and scatter past one grid (262144 threads) and
    several thousand block columns.  ||A||_2 >= max a_ii and kappa_2 >= max a_ii / min a_ii for a symmetric matrix, so using these
    in place of the true values only tightens the bars"""
    n = 300_001
    rng = np.random.default_rng(7)
    diag = 2.5 + rng.uniform(0., 1., n)
    off = -1. - 0.2 * rng.uniform(0., 1., n - 1)  # |off| <= 1.2: strictly diagonally dominant
    row_ptr = np.zeros(n + 1, dtype=np.int64)
    row_ptr[1:] = np.cumsum(np.r_[2, np.full(n - 2, 3), 2])
    col = np.stack([np.arange(n) - 1, np.arange(n), np.arange(n) + 1], axis=1).reshape(-1)[1:-1]
    val = np.stack([np.r_[0., off], diag, np.r_[off, 0.]], axis=1).reshape(-1)[1:-1]
    op = system.CsrOperator(ctx, dev(row_ptr, torch.int64), dev(col, torch.int32), dev(val))
    chol = solve.CholeskySolver(op)
    info = chol.info
    assert info.block == 32 and info.n_active == n and info.n_blocks == -(-n // 32) > 9000 and info.max_height == 1
    b = rng.standard_normal(n)
    x = chol.factor().solve(dev(b)).cpu().numpy()
    lower, upper = np.r_[0., off], np.r_[off, 0.]
    x_ref = thomas(lower, diag, upper, b)
    Ax = diag * x + lower * np.r_[0., x[:-1]] + upper * np.r_[x[1:], 0.]
    backward = np.linalg.norm(b - Ax) / (diag.max() * np.linalg.norm(x))
    forward = np.linalg.norm(x - x_ref) / np.linalg.norm(x_ref)
    print(f"chain n {n}: backward error {backward:.2e}, forward error against Thomas {forward:.2e}, bar {backward_bar(n):.2e}")
    assert backward <= backward_bar(n)
    assert forward <= diag.max() / diag.min() * backward_bar(n)


def scrambled_case(block, seed):
    rng = np.random.default_rng(seed)
    n = 3 * block + 5
    A, pattern = spd_band(n, 2 * block + 3, rng)
    return (*scrambled(A, pattern, rng), rng)


def test_two_runs_give_identical_bits(ctx):
    for block in (32, 64):
        A, pattern, active, rng = scrambled_case(block, 11)
        op = operator(ctx, A, pattern)
        b = dev(rng.standard_normal(A.shape[0]))
        runs = []
        for _ in range(2):
            chol = solve.CholeskySolver(op, block=block)
            runs.append(chol.factor().solve(b.clone()).cpu().numpy())
        again = chol.factor().solve(b.clone()).cpu().numpy()  # and a second factorisation on the same object
        assert np.array_equal(runs[0].view(np.int64), runs[1].view(np.int64))
        assert np.array_equal(runs[0].view(np.int64), again.view(np.int64))


def test_refactorisation_reads_the_new_values(ctx):
    block = 64
    A, pattern, active, rng = scrambled_case(block, 12)
    n = A.shape[0]
    op = operator(ctx, A, pattern)
    chol = solve.CholeskySolver(op, block=block).factor()
    b = rng.standard_normal(n)
    x_old = chol.solve(dev(b)).cpu().numpy()
    # rewrite the values in place: scale, and add to the diagonal
    rp, ci = op.row_ptr.cpu().numpy(), op.col_ind.cpu().numpy()
    on_diag = dev(np.repeat(np.arange(n), np.diff(rp)) == ci, torch.bool)
    op.values.mul_(3.0)
    op.values[on_diag] += 5.0
    A2 = 3.0 * A
    A2[active, active] += 5.0
    assert np.array_equal(dense_of(op), A2)
    x_new = chol.factor().solve(dev(b)).cpu().numpy()
    sub = np.ix_(active, active)
    bar = backward_bar(len(active))
    assert backward_error(A2[sub], x_new[active], b[active]) <= bar
    x_np = np.linalg.solve(A2[sub], b[active])
    assert np.linalg.norm(x_new[active] - x_np) / np.linalg.norm(x_np) <= np.linalg.cond(A2[sub], 2) * bar
    assert backward_error(A2[sub], x_old[active], b[active]) > bar


def test_columns_with_padding_and_aliasing(ctx):
    for block in (32, 64):
        A, pattern, active, rng = scrambled_case(block, 13)
        n = A.shape[0]
        chol = solve.CholeskySolver(operator(ctx, A, pattern), block=block).factor()
        B = dev(rng.standard_normal((3, n + 7)))
        singles = [chol.solve(B[c, :n].clone()) for c in range(3)]
        X = B.clone()
        assert chol.solve(X) is X  # b aliased to x, ld = n + 7 > n
        torch.cuda.synchronize()
        for c in range(3):
            assert torch.equal(X[c, :n].view(torch.int64), singles[c].view(torch.int64))
        assert torch.equal(X[:, n:], B[:, n:])
        out = torch.full((3, n + 7), SENTINEL, dtype=torch.float64, device="cuda")
        chol.solve(B, out)
        frozen = np.setdiff1d(np.arange(n), active)
        assert torch.equal(out[:, active], X[:, active]) and (out[:, frozen] == SENTINEL).all() and (out[:, n:] == SENTINEL).all()


def test_failures_are_clean_returns(ctx):
    block = 32
    A, pattern, active, rng = scrambled_case(block, 14)
    n = A.shape[0]
    op = operator(ctx, A, pattern)
    chol = solve.CholeskySolver(op, block=block)
    b = dev(rng.standard_normal(n))
    with pytest.raises(capi.L3KError, match="error -1"):
        chol.solve(b.clone())  # nothing factored yet
    row = int(active[len(active) // 2])
    rp, ci = op.row_ptr.cpu().numpy(), op.col_ind.cpu().numpy()
    at = int(rp[row] + np.searchsorted(ci[rp[row]:rp[row + 1]], row))
    keep = op.values[at].item()
    op.values[at] = -keep
    with pytest.raises(capi.L3KError, match="error -2: .*matrix is not positive definite"):
        chol.factor()
    info = chol.info
    assert info.factored == 0 and info.n_bad_pivots >= 1 and info.first_bad_row == row
    x = b.clone()
    with pytest.raises(capi.L3KError, match="error -1"):
        chol.solve(x)
    assert torch.equal(x, b)
    # a NaN is a bad pivot too, and makes no NaN of the rest of the factorisation's bookkeeping
    op.values[at] = float("nan")
    with pytest.raises(capi.L3KError, match="error -2"):
        chol.factor()
    assert chol.info.first_bad_row == row
    op.values[at] = keep
    x = chol.factor().solve(b.clone()).cpu().numpy()
    assert chol.info.factored == 1 and chol.info.n_bad_pivots == 0
    sub = np.ix_(active, active)
    assert backward_error(A[sub], x[active], b.cpu().numpy()[active]) <= backward_bar(len(active))
    # refusals at creation
    with pytest.raises(capi.L3KError, match="bytes"):
        solve.CholeskySolver(op, max_bytes=1)
    unsym = pattern.copy()
    i, j = active[0], active[-1]
    unsym[i, j], unsym[j, i] = True, False
    with pytest.raises(capi.L3KError, match="not structurally symmetric"):
        solve.CholeskySolver(operator(ctx, A, unsym))
    with pytest.raises(capi.L3KError, match="DistributedCsrOperator"):
        solve.CholeskySolver(object.__new__(system.DistributedCsrOperator))
    with pytest.raises(capi.L3KError, match="DistributedCsrOperator"):
        solve.direct_solve(object.__new__(system.DistributedCsrOperator), b, b.clone())


def test_empty_operator_and_operator_of_empty_rows(ctx):
    for n in (0, 3):
        op = system.CsrOperator(ctx, torch.zeros(n + 1, dtype=torch.int64, device="cuda"), torch.zeros(0, dtype=torch.int32, device="cuda"),
                                torch.zeros(0, dtype=torch.float64, device="cuda"))
        chol = solve.CholeskySolver(op).factor()
        assert chol.info.n_active == 0 and chol.info.n_blocks == 0 and chol.info.factor_bytes == 0
        x = torch.full((n,), SENTINEL, dtype=torch.float64, device="cuda")
        chol.solve(torch.ones(n, dtype=torch.float64, device="cuda"), x)
        assert (x == SENTINEL).all()


# ------------------------------------------------------------------------------------------------------------ mesh level
def diffusion2d(ctx, ne, p, condensation="none", sides=(2, 3), walls=(0, 1)):
    """tests/Diffusion2D.hpp as tests/test_gpu_quad_assembly.py sets it up: Dirichlet T = x on the left and right sides, Adiabatic2D
    on the bottom and top.  Returns (part, mesh, asm, operator, Dirichlet values)"""
    part = system.SquarePartition(ne, p)
    mesh = system.DeviceMesh(ctx, part, U, part.dirichlet_mask(U, sides=sides))
    n = part.n_local_nodes * U
    fe, fs = part.boundary_sides(list(sides))
    g = system.values_at_nodes(mesh, system.RESIDUAL_COORDX2D, [0], torch.zeros(n, dtype=torch.float64, device="cuda"), face_elem=fe,
                               face_side=fs)
    asm = system.AssembledSystem(mesh, condensation=condensation).begin()
    asm.add(system.MatrixFreeSystem(mesh, D2))
    if walls:
        asm.add(system.BoundaryTerm(mesh, ADI, *part.boundary_sides(list(walls))))
    return part, mesh, asm, asm.end(g[None, :]), g


def residual_through_apply(op, x, b):
    """||b - A x||_2 with A x formed by the device operator"""
    y = torch.zeros_like(x)
    op.apply(x, y)
    return (b - y).norm().item()


def test_full_2d_system(ctx):
    part, mesh, asm, op, _ = diffusion2d(ctx, 4, 2)
    n = op.n
    A = dense_of(op)
    x = torch.zeros(n, dtype=torch.float64, device="cuda")
    assert solve.direct_solve(op, asm.rhs[0], x) is x
    backward = residual_through_apply(op, x, asm.rhs[0]) / (np.linalg.norm(A, 2) * x.norm().item())
    x_np = np.linalg.solve(A, asm.rhs[0].cpu().numpy())
    forward = np.linalg.norm(x.cpu().numpy() - x_np) / np.linalg.norm(x_np)
    kappa = np.linalg.cond(A, 2)
    fields = x.view(-1, U).T.contiguous()
    err = np.linalg.norm(system.norm_l2(mesh, system.RESIDUAL_LINEAR2D_ERROR, fields))
    fe, fs = part.boundary_sides()
    berr = np.linalg.norm(system.norm_l2(mesh, system.RESIDUAL_LINEAR2D_ERROR, fields, face_elem=fe, face_side=fs))
    print(f"Diffusion2D 4 x 4, p 2: n {n}, kappa_2 {kappa:.2e}, backward {backward:.2e} (bar {backward_bar(n):.2e}), forward {forward:.2e}, "
          f"L2 error domain {err:.2e}, sides {berr:.2e}")
    assert backward <= backward_bar(n)
    assert forward <= kappa * backward_bar(n)
    assert err < 1e-8 and berr < 1e-8


def test_condensed_2d_system(ctx):
    p = 4
    _, _, asm_f, op_f, _ = diffusion2d(ctx, 4, p)
    _, _, asm_c, op_c, _ = diffusion2d(ctx, 4, p, condensation="element_boundary")
    n = op_f.n
    A = dense_of(op_f)
    kappa = np.linalg.cond(A, 2)
    x_f = solve.direct_solve(op_f, asm_f.rhs[0], torch.zeros(n, dtype=torch.float64, device="cuda"))
    internal = np.nonzero(np.diff(op_c.row_ptr.cpu().numpy()) == 0)[0]
    assert len(internal) == 16 * (p - 1) ** 2 * U
    x0 = SENTINEL + torch.arange(n, dtype=torch.float64, device="cuda")
    x_c = solve.direct_solve(op_c, asm_c.rhs[0], x0.clone())
    assert torch.equal(x_c[internal], x0[internal])  # the solver leaves the internal rows alone
    asm_c.recover(x_c)
    diff = (x_c - x_f).norm().item() / x_f.norm().item()
    print(f"condensed against full, p {p}: n {n}, {len(internal)} internal rows, kappa_2 {kappa:.2e}, relative difference {diff:.2e}, "
          f"bar {kappa * backward_bar(n):.2e}")
    assert diff <= kappa * backward_bar(n)
    backward = residual_through_apply(op_f, x_c, asm_f.rhs[0]) / (np.linalg.norm(A, 2) * x_c.norm().item())
    assert backward <= backward_bar(n)


def test_hex_system(ctx):
    U3 = 4
    part = system.CubePartition(2, 2, perturb=0.15)
    mask = part.dirichlet_mask(U3)
    mesh = system.DeviceMesh(ctx, part, U3, mask)
    n = part.n_local_nodes * U3
    g = dev(np.where(mask != 0, np.sin(np.arange(n) * 0.37), 0.0)[None, :])
    asm = system.AssembledSystem(mesh).begin()
    asm.add(system.MatrixFreeSystem(mesh, system.KERNEL_DIFFUSION3D, [0.7, 1.3]))
    asm.add(system.BoundaryTerm(mesh, system.KERNEL_ADIABATIC3D, *part.boundary_sides([1])))
    op = asm.end(g)
    A = dense_of(op)
    x = solve.direct_solve(op, asm.rhs[0], torch.zeros(n, dtype=torch.float64, device="cuda"))
    backward = residual_through_apply(op, x, asm.rhs[0]) / (np.linalg.norm(A, 2) * x.norm().item())
    x_np = np.linalg.solve(A, asm.rhs[0].cpu().numpy())
    forward = np.linalg.norm(x.cpu().numpy() - x_np) / np.linalg.norm(x_np)
    kappa = np.linalg.cond(A, 2)
    print(f"hexes 2^3, p 2: n {n}, kappa_2 {kappa:.2e}, backward {backward:.2e} (bar {backward_bar(n):.2e}), forward {forward:.2e}")
    assert backward <= backward_bar(n)
    assert forward <= kappa * backward_bar(n)


def test_cpp_mirror_matches_the_python_route_bit_for_bit(ctx, tmp_path):
    """tests/cpp/chol_shim.cpp: the condensed Diffusion2D system on 2 x 1 quads of order 4, Dirichlet T = x on all four sides (no entry
    of it has more than two addends, so the assembled values do not depend on the order of the scatter's atomics), through
    l3k::Cholesky; the same steps through solve.direct_solve on the same Dirichlet values"""
    part, mesh, asm, op, g = diffusion2d(ctx, (2, 1), 4, condensation="element_boundary", sides=(0, 1, 2, 3), walls=())
    n = op.n
    x = solve.direct_solve(op, asm.rhs[0], torch.zeros(n, dtype=torch.float64, device="cuda"))
    asm.recover(x)
    x_py = x.cpu().numpy()
    g_file, out = str(tmp_path / "dirichlet.bin"), str(tmp_path / "solution.bin")
    g.cpu().numpy().tofile(g_file)
    exe = build_shim(str(tmp_path / "chol_shim"))
    r = subprocess.run([exe, g_file, out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr
    x_cpp = np.fromfile(out, dtype=np.float64)
    assert x_cpp.shape == x_py.shape and np.abs(x_py).max() > 0
    assert np.array_equal(x_cpp.view(np.int64), x_py.view(np.int64)), np.abs(x_cpp - x_py).max()
