"""Restarted GMRES on the device (l3k_gmres_*, solve.gmres) against the longdouble restatement of tests/gmres_ref.py.

Every solve is held to the restatement run with the same options: iterations EQUAL, restarts equal, achieved_tol against an
independently computed |mask(b - A x)| / scale to 1e-12.  Equal, because every case asserts, on the CPU, how far the restatement's
estimates at the stopping step and at the step before lie from tol (margins()), and the device's estimates differ from the
restatement's by rounding only (1e-10 relative at the most: the two orthogonalise to 1e-16 and differ in summation order).  Where
the tolerance is this file's choice it is placed between two consecutive estimates that are a factor >= 2.25 apart, at their
geometric mean: both margins are then >= 1.5.  Where the case fixes the tolerance (1e-6 |b| on the reference's SPD matrix, 1e-10 |b|
on the non-symmetric tridiagonal and the matrix-free system) it stays as fixed; those systems converge by a factor 1.1 - 1.3 per step
near 1e-10, so margins of 1.5 do not exist there, and the margin each group has in the restatement is asserted instead: >= 1.2 on the
SPD matrix, >= 1.02 on the others -- two hundred million times the rounding.  check_every = 5 alone may run up to 4 steps on."""
import ctypes as C

import numpy as np
import pytest
import torch

import gmres_ref as G
from gmres_ref import EPS, LD
from l3ster_amd import capi, partition, solve, system

pytestmark = pytest.mark.gpu
_CTX, _TRI, _REF, _MF = [], {}, {}, {}
SCALING = {"none": 0, "initial": 1, "rhs": 2}


def ctx():
    if not _CTX:
        torch.cuda.set_device(0)
        _CTX.append(system.Context(0, torch.cuda.current_stream().cuda_stream))
    return _CTX[0]


def dev(a, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


class Tri:
    """a tridiagonal matrix as a CsrOperator and as a callable in any dtype; rows listed in `nan_rows` hold NaN on the device"""

    def __init__(self, lo, di, up, nan_rows=None):
        n = self.n = di.size
        self.lo, self.di, self.up = lo.copy(), di.copy(), up.copy()
        self.lo[0] = self.up[-1] = 0.0
        cols = np.stack([np.arange(n) - 1, np.arange(n), np.arange(n) + 1], axis=1)
        vals = np.stack([self.lo, self.di, self.up], axis=1)
        if nan_rows is not None:
            vals[nan_rows] = np.nan
        keep = (cols >= 0) & (cols < n)
        self.row_ptr = dev(np.concatenate([[0], np.cumsum(keep.sum(axis=1))]), torch.int64)
        self.col_ind, self.values = dev(cols[keep], torch.int32), dev(vals[keep])
        self.op = system.CsrOperator(ctx(), self.row_ptr, self.col_ind, self.values)

    def __call__(self, v):
        lo, di, up = (a.astype(v.dtype) for a in (self.lo, self.di, self.up))
        y = di * v
        y[1:] += lo[1:] * v[:-1]
        y[:-1] += up[:-1] * v[1:]
        return y


def tri(kind, n):
    """'spd': the reference's makeSPDMatrix (interior rows .5, 2, .5; the first and the last row are identity rows, and the rows next
    to them do not couple to them); c05 / c09: (-1 - c, 2.5 + 0.5 sin i, -1 + c); 'fast': (-0.6, 2.5 + 0.5 sin i, -0.2), whose
    estimates fall by more than 2.25 per step; '3I'"""
    if (kind, n) not in _TRI:
        i, one = np.arange(n), np.ones(n)
        if kind == "spd":
            lo, di, up = 0.5 * one, 2.0 * one, 0.5 * one
            di[[0, -1]] = 1.0
            lo[[1, -1]] = 0.0
            up[[0, -2]] = 0.0
        elif kind == "3I":
            lo, di, up = 0.0 * one, 3.0 * one, 0.0 * one
        elif kind == "fast":
            lo, di, up = -0.6 * one, 2.5 + 0.5 * np.sin(i), -0.2 * one
        else:
            c = {"c05": 0.5, "c09": 0.9}[kind]
            lo, di, up = (-1 - c) * one, 2.5 + 0.5 * np.sin(i), (-1 + c) * one
        _TRI[kind, n] = Tri(lo, di, up)
    return _TRI[kind, n]


def reference(key, T, b, x0, m, minv=None, live=None, **kw):
    """the longdouble restatement, once per key"""
    if key not in _REF:
        prec = None if minv is None else (lambda v: v * minv.astype(v.dtype))
        kw["residual_scaling"] = SCALING[kw.get("residual_scaling", "none")]
        _REF[key] = G.gmres(T, b, x0, m, prec=prec, live=live, dtype=LD, **kw)
    return _REF[key]


def margins(ref, tol, floor=1.5):
    below, above = G.stopping_margin(ref["history"], tol)
    print(f"margins (below, above): {below:.4f} {above:.4f}, asserted >= {floor}")
    assert below >= floor and above >= floor, (below, above)


def choose_tol(T, b, x0, m, minv, near, scaling="rhs", live=None):
    """a tolerance near step `near` of the restatement with both margins >= 1.5: the geometric mean of the first two consecutive
    estimates from there on that are a factor >= 2.25 apart"""
    h = G.gmres(T, b, x0, m, prec=None if minv is None else (lambda v: v * minv.astype(v.dtype)), live=live, tol=0.0,
                max_iters=near + 12, residual_scaling=SCALING[scaling], dtype=LD)["history"]
    k = next(j for j in range(near, len(h)) if h[j - 1] / h[j] >= 2.25)
    return float(np.sqrt(h[k - 1] * h[k]))


def true_residual(T, b, x, scale, live=None):
    r = b.astype(LD) - T(x.astype(LD))
    r = r if live is None else np.where(live, r, LD(0))
    return float(np.sqrt(np.sum(r * r)) / scale)


def scale_of(b, scaling, T=None, x0=None, live=None):
    if scaling == "rhs":
        return np.sqrt(np.sum(b.astype(LD) ** 2))
    if scaling == "initial":
        return LD(true_residual(T, b, x0, LD(1), live))
    return LD(1)


def held_to(res, ref, label, its_slack=0):
    print(f"{label}: device {res.num_iters} iterations, {res.restarts} restarts, achieved {res.tol:.3e}, estimate {res.estimate:.3e}, "
          f"orth_loss {res.orth_loss:.2e}; restatement {ref['iterations']} / {ref['restarts']} / {ref['achieved_tol']:.3e}")
    assert abs(res.num_iters - ref["iterations"]) <= its_slack and res.restarts == ref["restarts"]
    assert res.converged == ref["converged"] and bool(res.breakdown) == ref["breakdown"]
    assert res.orth_loss <= 1e-10


# ------------------------------------------------------------------------------------------------ the reference's SPD matrix
@pytest.mark.parametrize("m", [250, 10])
@pytest.mark.parametrize("jacobi", [False, True])
def test_reference_spd_matrix(jacobi, m):
    """makeSPDMatrix(100) of the reference's solver tests, two right-hand sides b = A x*, tol 1e-6 |b| (part of the case: the default of the reference's IterSolverOpts, which its solver tests use), without
    a preconditioner and with Jacobi; |x - x*|_inf <= 1e-5"""
    T, n = tri("spd", 100), 100
    rng = np.random.default_rng(5)
    xs = np.stack([np.cos(0.3 * np.arange(n)), rng.uniform(-1, 1, n)])
    B = np.stack([T(x) for x in xs])
    minv = 1.0 / T.di if jacobi else None
    X = torch.zeros((2, n), dtype=torch.float64, device="cuda")
    out = solve.gmres(T.op, dev(B), X, None if minv is None else dev(minv), tol=1e-6, residual_scaling="rhs", restart_length=m)
    assert len(out) == 2
    for c, res in enumerate(out):
        ref = reference(("spd", jacobi, m, c), T, B[c], np.zeros(n), min(m, n), minv, tol=1e-6, residual_scaling="rhs")
        margins(ref, 1e-6, 1.2)
        held_to(res, ref, f"SPD jacobi={jacobi} m={m} column {c}")
        x = X[c].cpu().numpy()
        assert res.converged and res.restarts == (0 if m == 250 else ref["restarts"])
        assert abs(res.tol - true_residual(T, B[c], x, scale_of(B[c], "rhs"))) <= 1e-12
        assert np.abs(x - xs[c]).max() <= 1e-5


# ------------------------------------------------------------------------------------------------ the case CG cannot serve
@pytest.mark.parametrize("m", [7, 30])
@pytest.mark.parametrize("kind", ["c05", "c09"])
@pytest.mark.parametrize("n", [1000, 300001])
def test_nonsymmetric_tridiagonal(n, kind, m):
    """(-1 - c, 2.5 + 0.5 sin i, -1 + c), Jacobi, tol 1e-10 |b| (part of the case), b = A x* with x*_i = cos(0.1 i).  n = 300001 is
    past one grid of 1024 x 256 rows: the threads of every vector kernel stride"""
    T = tri(kind, n)
    xs = np.cos(0.1 * np.arange(n))
    b, minv = T(xs), 1.0 / T.di
    x = torch.zeros(n, dtype=torch.float64, device="cuda")
    res = solve.gmres(T.op, dev(b), x, dev(minv), tol=1e-10, residual_scaling="rhs", restart_length=m)
    ref = reference(("tri", n, kind, m), T, b, np.zeros(n), m, minv, tol=1e-10, residual_scaling="rhs")
    margins(ref, 1e-10, 1.02)
    held_to(res, ref, f"tridiagonal n={n} {kind} m={m}")
    xh = x.cpu().numpy()
    assert res.converged and res.restarts >= 1
    assert abs(res.tol - true_residual(T, b, xh, scale_of(b, "rhs"))) <= 1e-12
    assert np.abs(xh - xs).max() <= 1e-7


# ------------------------------------------------------------------------------------------------ edge cases
def fast_case(n=1000):
    T = tri("fast", n)
    xs = np.sin(0.05 * np.arange(n)) + 0.3
    return T, T(xs), 1.0 / T.di, xs


def run(T, b, x0, minv, m, label, key, its_slack=0, live=None, **kw):
    x = dev(x0)
    res = solve.gmres(T.op, dev(b), x, None if minv is None else dev(minv), restart_length=m, throw_on_fail=False, **kw)
    rkw = {k: v for k, v in kw.items() if k != "check_every"}
    ref = reference(key, T, b, x0, m, minv, live=live, **rkw)
    held_to(res, ref, label, its_slack)
    xh = x.cpu().numpy()
    scale = scale_of(b, kw.get("residual_scaling", "none"), T, x0, live)
    assert np.isfinite(xh).all() and abs(res.tol - true_residual(T, b, xh, scale, live)) <= 1e-12
    return res, ref, xh


def test_restart_length_one():
    T, b, minv, xs = fast_case()
    tol = choose_tol(T, b, np.zeros(T.n), 1, minv, near=6)
    res, ref, _ = run(T, b, np.zeros(T.n), minv, 1, "GMRES(1)", "m1", tol=tol, residual_scaling="rhs")
    margins(ref, tol)
    assert res.converged and res.restarts == res.num_iters - 1 >= 5


def test_a_cycle_that_ends_exactly_at_m():
    T, b, minv, xs = fast_case()
    tol = choose_tol(T, b, np.zeros(T.n), 250, minv, near=8)
    full = reference("exact-full", T, b, np.zeros(T.n), 250, minv, tol=tol, residual_scaling="rhs")
    margins(full, tol)
    m = full["iterations"]
    res, ref, xh = run(T, b, np.zeros(T.n), minv, m, f"k reaches m = {m}", "exact-m", its_slack=0, tol=tol, residual_scaling="rhs")
    assert res.converged and res.num_iters == m and res.restarts == 0
    assert np.abs(xh - ref["x"].astype(np.float64)).max() <= 1e-12 * np.abs(xs).max()


def test_limits_hit():
    T, b, minv, xs = fast_case()
    # max_iters in the middle of the second cycle: x carries the partial cycle
    res, ref, xh = run(T, b, np.zeros(T.n), minv, 5, "max_iters mid-cycle", "mid", its_slack=0, tol=1e-14, residual_scaling="rhs", max_iters=7)
    assert not res.converged and res.num_iters == 7 and res.restarts == 1
    assert np.abs(xh - ref["x"].astype(np.float64)).max() <= 1e-12 * np.abs(xs).max()
    one = reference("mid-one-cycle", T, b, np.zeros(T.n), 5, minv, tol=1e-14, residual_scaling="rhs", max_iters=5)
    assert res.tol < 0.5 * one["achieved_tol"]  # (the two steps of the partial cycle are in x)
    # max_restarts
    res, ref, _ = run(T, b, np.zeros(T.n), minv, 3, "max_restarts", "restarts", its_slack=0, tol=1e-14, residual_scaling="rhs", max_restarts=1)
    assert not res.converged and res.num_iters == 6 and res.restarts == 1


def test_check_every_five():
    T, b, minv, xs = fast_case()
    tol = choose_tol(T, b, np.zeros(T.n), 250, minv, near=7)
    res, ref, _ = run(T, b, np.zeros(T.n), minv, 250, "check_every 5, one cycle", "ce5", its_slack=4, tol=tol, residual_scaling="rhs", check_every=5)
    margins(ref, tol)
    assert res.converged and ref["iterations"] <= res.num_iters <= ref["iterations"] + 4 and res.num_iters % 5 == 0
    # cycles of 7: a check at every multiple of 5 and at the end of every cycle, never a step beyond one
    x = torch.zeros(T.n, dtype=torch.float64, device="cuda")
    r7 = solve.gmres(T.op, dev(b), x, dev(minv), tol=1e-13, residual_scaling="rhs", restart_length=7, check_every=5)
    ref7 = reference("ce5-m7", T, b, np.zeros(T.n), 7, minv, tol=1e-13, residual_scaling="rhs")
    print(f"check_every 5, m 7: device {r7.num_iters} / {r7.restarts}, restatement {ref7['iterations']} / {ref7['restarts']}")
    assert r7.converged and ref7["iterations"] <= r7.num_iters <= ref7["iterations"] + 4 and r7.num_iters <= 7 * (r7.restarts + 1)
    assert abs(r7.tol - true_residual(T, b, x.cpu().numpy(), scale_of(b, "rhs"))) <= 1e-12


def test_nothing_to_do():
    T, b, minv, xs = fast_case()
    x = torch.zeros(T.n, dtype=torch.float64, device="cuda")
    res = solve.gmres(T.op, torch.zeros_like(x), x, dev(minv), tol=1e-12)
    assert res.converged and res.num_iters == 0 and res.restarts == 0 and res.tol == 0.0 and not x.any()
    # x0 is the solution already: b as the device's own A x0
    x0 = dev(xs)
    bd = torch.empty_like(x0)
    T.op.apply(x0, bd)
    res = solve.gmres(T.op, bd, x0, dev(minv), tol=1e-12, residual_scaling="rhs")
    assert res.converged and res.num_iters == 0 and res.restarts == 0 and res.tol == 0.0 and torch.equal(x0, dev(xs))


def test_breakdown_on_a_multiple_of_the_identity():
    T = tri("3I", 1000)
    b = np.cos(np.arange(1000.0))
    for minv in (None, np.full(1000, 1.0 / 3.0)):
        res, ref, xh = run(T, b, np.zeros(1000), minv, 10, "3 I", ("3I", minv is None), its_slack=0, tol=1e-12)
        assert res.converged and res.num_iters == 1 and res.breakdown and res.restarts == 0
        assert np.isfinite([res.tol, res.estimate, res.orth_loss]).all() and np.abs(xh - b / 3.0).max() <= 4 * EPS


# ------------------------------------------------------------------------------------------------ frozen rows
def test_frozen_rows_keep_x_and_the_rest_solves():
    """every 101st minv entry is 0 and the matrix holds NaN in those rows; x0 is random: x keeps its bits there"""
    n = 1000
    base = tri("fast", n)
    frozen = np.arange(n) % 101 == 0
    T = Tri(base.lo, base.di, base.up, nan_rows=frozen)
    live = ~frozen
    minv = np.where(live, 1.0 / T.di, 0.0)
    rng = np.random.default_rng(11)
    x0, b = rng.standard_normal(n), T(np.cos(0.1 * np.arange(n)))
    tol = choose_tol(T, b, x0, 5, minv, near=11, live=live)  # (in the third cycle of GMRES(5))
    res, ref, xh = run(T, b, x0, minv, 5, "frozen rows", "frozen", live=live, tol=tol, residual_scaling="rhs")
    margins(ref, tol)
    assert res.restarts >= 2
    assert res.converged and np.array_equal(xh[frozen].view(np.int64), x0[frozen].view(np.int64))
    assert np.abs(xh - ref["x"].astype(np.float64))[live].max() <= 1e-8


# ------------------------------------------------------------------------------------------------ matrix-free operators
def dense_by_apply(apply, n):
    A = np.empty((n, n))
    e, y = torch.zeros((1, n), dtype=torch.float64, device="cuda"), torch.empty((1, n), dtype=torch.float64, device="cuda")
    for j in range(n):
        e[0, j] = 1.0
        apply(e, y)
        A[:, j] = y[0].cpu().numpy()
        e[0, j] = 0.0
    return A


def rel_res(A, b, x):
    r = b.astype(LD) - A.astype(LD) @ x.astype(LD)
    return float(np.sqrt(np.sum(r * r)) / np.sqrt(np.sum(b.astype(LD) ** 2)))


def check_against_pcg(sys_, A, b, minv, preconds, label, m=40):
    """the GMRES solution equals the PCG solution of the same system to cond(A) (sum of the two residuals + n EPS)"""
    n, cond = b.numel(), float(np.linalg.cond(A))
    bh = b.cpu().numpy()
    for name, kw in [("Jacobi", dict(minv=minv))] + [(k, dict(precond=p)) for k, p in preconds]:
        xp, xg = torch.zeros_like(b), torch.zeros_like(b)
        rp = solve.pcg(sys_, b, xp, tol=1e-10, residual_scaling="rhs", **kw)
        rg = solve.gmres(sys_, b, xg, tol=1e-10, residual_scaling="rhs", restart_length=m, **kw)
        tp, tg = rel_res(A, bh, xp.cpu().numpy()), rel_res(A, bh, xg.cpu().numpy())
        diff = float((xg - xp).norm() / xp.norm())
        print(f"{label} {name}: PCG {rp.num_iters} iterations, GMRES({m}) {rg.num_iters} / {rg.restarts} restarts; true residuals {tp:.2e} "
              f"{tg:.2e}; |x_gmres - x_pcg| / |x_pcg| = {diff:.2e}, bound {cond * (tp + tg + n * EPS):.2e} (cond {cond:.2e})")
        assert rp.converged and rg.converged and abs(rg.tol - tg) <= 1e-12
        assert diff <= cond * (tp + tg + n * EPS)
        if name == "Jacobi":
            jac = rg
    return jac


def test_matrix_free_system_with_jacobi_chebyshev_and_pmultigrid():
    """CubePartition(2, 3, perturb=0.15), Diffusion3D, U = 4"""
    c, U, kid, kpar = ctx(), 4, system.KERNEL_DIFFUSION3D, [0.7, 1.3]
    fine, coarse = system.CubePartition(2, 3, perturb=0.15), system.CubePartition(2, 1, perturb=0.15)
    levels = []
    for part in (fine, coarse):
        mf = system.MatrixFreeSystem(system.DeviceMesh(c, part, U, part.dirichlet_mask(U)), kid, kpar)
        diag, rhs = mf.diag_rhs()
        levels.append((mf, solve.jacobi_inverse_native(c, diag), rhs))
    (mf, minv, rhs), (mc, minv_c, _) = levels
    n = fine.n_owned_nodes * U
    b = dev(np.sin(0.37 * np.arange(n)) + 0.1) * (minv != 0)
    cheb = solve.ChebyshevPreconditioner(mf, minv, degree=3)
    pmg = solve.PMultigrid([(mf, solve.ChebyshevPreconditioner(mf, minv, degree=3), None),
                            (mc, solve.ChebyshevPreconditioner(mc, minv_c, degree=3), system.match_elements(fine, coarse))])
    A = dense_by_apply(mf.apply, n)
    jac = check_against_pcg(mf, A, b, minv, [("Chebyshev(3)", cheb), ("p-multigrid 3 -> 1", pmg)], "matrix-free")
    # Jacobi against the restatement on the dense copy
    mh = minv.cpu().numpy()
    ref = G.gmres(lambda v: A.astype(v.dtype) @ v, b.cpu().numpy(), np.zeros(n), 40, prec=lambda v: v * mh.astype(v.dtype), live=mh != 0,
                  tol=1e-10, residual_scaling=2, dtype=LD)
    margins(ref, 1e-10, 1.02)
    held_to(jac, ref, "matrix-free Jacobi")
    # refusals on this system
    other = system.MatrixFreeSystem(mf.mesh, kid, kpar)
    x = torch.zeros_like(b)
    for p in (cheb, pmg):
        with pytest.raises(capi.L3KError, match="created for another system"):
            solve.gmres(other, b, x, precond=p)
    lib, res = capi.load(), capi.GmresResult()
    ws = solve.GmresWorkspace(c, n, 5)
    for entry, h in ((lib.l3k_gmres_solve_cheb, cheb._h), (lib.l3k_gmres_solve_pmg, pmg._h)):
        assert entry(ws._h, other._h, b.data_ptr(), x.data_ptr(), h, None, C.byref(res)) == -1
        assert "the preconditioner was created for another system" in lib.l3k_last_error().decode()
    assert lib.l3k_gmres_solve_pmg(ws._h, mf._h, b.data_ptr(), x.data_ptr(), None, None, C.byref(res)) == -1
    assert lib.l3k_last_error().decode() == "l3k_gmres_solve_pmg: null argument"
    assert not x.any()


def test_two_term_system():
    """the two-term sum of tests/test_gpu_multiterm.py::test_solve_against_the_assembled_system"""
    c, U, D3 = ctx(), 4, system.KERNEL_DIFFUSION3D
    part, k = system.CubePartition(3, 2, perturb=0.1), 10
    mask = part.dirichlet_mask(U, unknowns=(0,), sides=(0, 1))
    rows = system.DeviceMesh(c, part, U, mask)
    lo, hi = partition.element_subset(part, np.arange(0, k)), partition.element_subset(part, np.arange(k, part.n_elems))
    a = system.MatrixFreeSystem(system.DeviceMesh(c, lo, U, mask), D3, [0.7, 1.3])
    bt = system.MatrixFreeSystem(system.DeviceMesh(c, hi, U, mask), D3, [2.0, 0.5])
    S = system.MultiTermSystem(rows).add(a).add(bt).finalize()
    n = rows.n_owned_dofs
    diag, rhs = S.diag_rhs()
    minv = S.jacobi_inverse(diag)
    b = rhs[0].contiguous()
    if not b.any():
        b = dev(np.sin(0.37 * np.arange(n)) + 0.1) * (minv != 0)
    A = dense_by_apply(S.apply, n)
    # (GMRES(40) stagnates on this sum with Jacobi -- 1600 steps leave 1.1e-5 |b| -- so the reference's restart_length of 250 here)
    check_against_pcg(S, A, b, minv, [("Chebyshev(3)", solve.ChebyshevPreconditioner(S, minv, degree=3))], "two terms", m=250)
    pm = solve.PMultigrid.__new__(solve.PMultigrid)  # (a hierarchy cannot be made on a sum: the refusal comes before its handle is read)
    pm.system = S
    with pytest.raises(capi.L3KError, match="p-multigrid is not provided for a MultiTermSystem"):
        solve.gmres(S, b, torch.zeros_like(b), precond=pm)
    # a system that is not finalized is refused by the library
    open_ = system.MultiTermSystem(rows).add(a)
    lib, res, x = capi.load(), capi.GmresResult(), torch.zeros_like(b)
    ws = solve.GmresWorkspace(c, n, 5)
    assert lib.l3k_mfs_gmres_solve(ws._h, open_._h, b.data_ptr(), x.data_ptr(), None, None, C.byref(res)) == -1
    assert lib.l3k_last_error().decode() == "l3k_mfs_gmres_solve: call l3k_mfs_finalize first"


# ------------------------------------------------------------------------------------------------ reproducibility and refusals
def test_two_solves_give_equal_bits():
    T, n = tri("c09", 1000), 1000
    b, minv = dev(T(np.cos(0.1 * np.arange(n)))), dev(1.0 / T.di)
    ws = solve.GmresWorkspace(ctx(), n, 30)
    assert (ws.info.n, ws.info.ld, ws.info.restart_length) == (n, 1000, 30) and ws.info.bytes > 31 * 1000 * 8
    outs = []
    for w in (ws, ws, None):  # (the same workspace twice, then a fresh one)
        x = torch.zeros(n, dtype=torch.float64, device="cuda")
        r = solve.gmres(T.op, b, x, minv, tol=1e-10, residual_scaling="rhs", restart_length=30, workspace=w)
        outs.append((x, (r.tol, r.num_iters, r.restarts, r.estimate, r.orth_loss)))
    assert all(torch.equal(outs[0][0], o[0]) and outs[0][1] == o[1] for o in outs[1:])


def test_refusals():
    T, n = tri("fast", 1000), 1000
    c, lib, res = ctx(), capi.load(), capi.GmresResult()
    b, x = torch.ones(n, dtype=torch.float64, device="cuda"), torch.zeros(n + 8, dtype=torch.float64, device="cuda")
    h = C.c_void_p()

    def refused(rc, text):
        assert rc == -1 and text in lib.l3k_last_error().decode(), lib.l3k_last_error().decode()

    refused(lib.l3k_gmres_create(c._h, n, 0, 0, C.byref(h)), "restart_length = 0 must be at least 1")
    refused(lib.l3k_gmres_create(c._h, n, 30, 0, None), "l3k_gmres_create: null argument")
    refused(lib.l3k_gmres_create(c._h, 5000, 2047, 0, C.byref(h)), "l3k_gmres_create: restart_length = 2047 above 2046")
    refused(lib.l3k_gmres_create(c._h, n, 30, 1000, C.byref(h)), "bytes, above max_bytes = 1000")
    with pytest.raises(capi.L3KError, match="needs [0-9]+ bytes"):
        solve.GmresWorkspace(c, n, 30, max_bytes=1000)
    ws, small = solve.GmresWorkspace(c, n, 2000), solve.GmresWorkspace(c, n - 1, 5)
    assert ws.restart_length == n  # (lowered to n)
    refused(lib.l3k_csr_gmres_solve(small._h, T.op._h, b.data_ptr(), x.data_ptr(), None, None, C.byref(res)),
            "l3k_csr_gmres_solve: the workspace was created for n = 999, the operator has 1000 rows")
    refused(lib.l3k_csr_gmres_solve(ws._h, T.op._h, b.data_ptr(), b.data_ptr() + 8 * 10, None, None, C.byref(res)), "l3k_csr_gmres_solve: b and x overlap")
    refused(lib.l3k_csr_gmres_solve(ws._h, T.op._h, None, x.data_ptr(), None, None, C.byref(res)), "l3k_csr_gmres_solve: null argument")
    refused(lib.l3k_csr_gmres_solve(ws._h, T.op._h, b.data_ptr(), x.data_ptr(), None, None, None), "l3k_csr_gmres_solve: null argument")
    refused(lib.l3k_csr_gmres_solve_cheb(ws._h, T.op._h, b.data_ptr(), x.data_ptr(), None, None, C.byref(res)), "l3k_csr_gmres_solve_cheb: null argument")
    minv = dev(1.0 / T.di)
    cheb = solve.ChebyshevPreconditioner(T.op, minv, degree=2)
    twin = system.CsrOperator(c, T.row_ptr, T.col_ind, T.values)
    refused(lib.l3k_csr_gmres_solve_cheb(ws._h, twin._h, b.data_ptr(), x.data_ptr(), cheb._h, None, C.byref(res)),
            "l3k_csr_gmres_solve_cheb: the preconditioner was created for another system")
    with pytest.raises(capi.L3KError, match="the workspace was created for n = 999"):
        solve.gmres(T.op, b, x[:n], workspace=small)
    with pytest.raises(RuntimeError, match="Solver failed to converge"):
        solve.gmres(T.op, b, x[:n], minv, tol=1e-12, max_iters=2)
    assert not x[n:].any()
    # ... and the Chebyshev preconditioner on the right of a CSR operator solves
    xs = torch.zeros(n, dtype=torch.float64, device="cuda")
    r = solve.gmres(T.op, b, xs, precond=cheb, tol=1e-10, residual_scaling="rhs", workspace=ws)
    assert r.converged and abs(r.tol - true_residual(T, b.cpu().numpy(), xs.cpu().numpy(), scale_of(b.cpu().numpy(), "rhs"))) <= 1e-12


def test_ghost_nodes_are_refused():
    """an l3k_mf on one part of a partitioned mesh, and a sum over its rows: the single-rank message"""
    c = ctx()
    part = system.CubePartition(4, 2, (2, 1, 1), 1, perturb=0.1)
    assert part.n_ghost_nodes > 0
    mesh = system.DeviceMesh(c, part, 4, part.dirichlet_mask(4))
    gmf = system.MatrixFreeSystem(mesh, system.KERNEL_DIFFUSION3D, [1.0, 0.0])
    n = part.n_owned_nodes * 4
    b, x = torch.ones(n, dtype=torch.float64, device="cuda"), torch.zeros(n, dtype=torch.float64, device="cuda")
    with pytest.raises(capi.L3KError, match="libl3k error -1: l3k_gmres_solve is the single-rank solver; this mesh has ghost nodes"):
        solve.gmres(gmf, b, x, restart_length=5)
    S = system.MultiTermSystem(mesh).add(gmf).finalize()
    with pytest.raises(capi.L3KError, match="libl3k error -1: l3k_mfs_gmres_solve is the single-rank solver; this mesh has ghost nodes"):
        solve.gmres(S, b, x, restart_length=5)
    assert not x.any()
