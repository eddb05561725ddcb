"""CPU checks of restarted GMRES: the numpy restatement of tests/gmres_ref.py minimises the residual over the Krylov space (the
property that makes it GMRES), restarts and counts as include/l3k.h says; the header declares and the library exports the new
entry points; the Python layer refuses what it can refuse without a device."""
import os
import re
import types

import numpy as np
import pytest

import gmres_ref as G
from l3ster_amd import capi, solve

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["l3k_gmres_create", "l3k_gmres_info_get", "l3k_gmres_destroy", "l3k_gmres_solve", "l3k_gmres_solve_cheb", "l3k_gmres_solve_pmg",
       "l3k_csr_gmres_solve", "l3k_csr_gmres_solve_cheb", "l3k_mfs_gmres_solve", "l3k_mfs_gmres_solve_cheb", "l3k_gmres_multi_dot",
       "l3k_gmres_project", "l3k_gmres_combine"]


def matrix(n=60, seed=3):
    """random, non-symmetric, strictly diagonally dominant by rows (by 2 %)"""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((n, n))
    np.fill_diagonal(A, 0.0)
    A += np.diag(1.02 * np.abs(A).sum(axis=1) * np.where(rng.random(n) < 0.5, -1.0, 1.0))
    return A, rng.standard_normal(n), rng.standard_normal(n)


@pytest.mark.parametrize("dtype", [np.float64, np.longdouble])
@pytest.mark.parametrize("jacobi", [False, True])
@pytest.mark.parametrize("k", [1, 2, 3, 5])
def test_k_steps_minimise_the_residual_over_the_krylov_space(k, jacobi, dtype):
    """x_k = x_0 + M^-1 K c with K = [r_0, (A M^-1) r_0, ...]: the residual of the restatement after k steps of one cycle equals
    the least-squares minimum over c, to 1e-10 relative.  k stops at 5: a step divides the residual of this matrix by about 6 (the
    off-diagonal part has a spectral radius near sqrt(n), the diagonal is near 0.8 n), and the float64 evaluation of b - A x below
    carries a rounding of a few EPS |r_0|, which must stay under 1e-10 of the minimum: at k = 9 the minimum is 1e-7 |r_0| and the
    comparison measured 8e-10, the rounding of its own right-hand side"""
    A, b, x0 = matrix()
    minv = 1.0 / np.diag(A)
    prec = (lambda v: v * minv.astype(v.dtype)) if jacobi else None
    out = G.gmres(lambda v: A.astype(v.dtype) @ v, b, x0, m=k, prec=prec, tol=0.0, max_iters=k, max_restarts=0, dtype=dtype)
    assert out["iterations"] == k and out["restarts"] == 0 and not out["converged"] and not out["breakdown"]
    AM = A * minv[None, :] if jacobi else A
    r0 = b - A @ x0
    K = np.empty((A.shape[0], k))
    v = r0.copy()
    for j in range(k):
        # the Krylov space explicitly, column by column: (A M^-1) times the last column, made orthogonal to the columns before
        # by Householder QR (numpy.linalg.qr) -- the powers themselves lose the space to rounding: with them lstsq missed the
        # minimum by 8e-8 at k = 9, in float64 and in longdouble alike
        K[:, j] = np.linalg.qr(np.column_stack([K[:, :j], v]))[0][:, j]
        v = AM @ K[:, j]
    c = np.linalg.lstsq(AM @ K, r0, rcond=None)[0]
    best = np.linalg.norm(r0 - AM @ K @ c)
    got = np.linalg.norm(b - A @ np.asarray(out["x"], dtype=np.float64))
    assert abs(got - best) <= 1e-10 * best, (got, best)
    # the estimate of the recurrence is that residual, and achieved_tol is the explicit one
    assert abs(out["estimate"] - best) <= 1e-10 * best and abs(out["achieved_tol"] - best) <= 1e-10 * best
    assert out["orth_loss"] <= 64 * G.EPS


def test_restarts_limits_and_frozen_rows():
    A, b, x0 = matrix()
    n = A.shape[0]
    ap = lambda v: A.astype(v.dtype) @ v
    full = G.gmres(ap, b, x0, m=250, tol=1e-9, residual_scaling=2)
    short = G.gmres(ap, b, x0, m=4, tol=1e-9, residual_scaling=2)
    assert full["converged"] and full["restarts"] == 0 and full["iterations"] <= n
    assert short["converged"] and short["restarts"] >= 1 and short["iterations"] >= full["iterations"]
    for out in (full, short):
        true = np.linalg.norm(b - A @ out["x"]) / np.linalg.norm(b)
        assert abs(true - out["achieved_tol"]) <= 1e-13 and true <= 1e-9
    capped = G.gmres(ap, b, x0, m=4, tol=1e-9, residual_scaling=2, max_restarts=1)
    assert not capped["converged"] and capped["iterations"] == 8 and capped["restarts"] == 1
    mid = G.gmres(ap, b, x0, m=4, tol=1e-9, residual_scaling=2, max_iters=6)
    assert not mid["converged"] and mid["iterations"] == 6 and mid["restarts"] == 1
    assert abs(np.linalg.norm(b - A @ mid["x"]) / np.linalg.norm(b) - mid["achieved_tol"]) <= 1e-13
    zero = G.gmres(ap, np.zeros(n), np.zeros(n), m=4)
    assert zero["converged"] and zero["iterations"] == 0 and zero["restarts"] == 0
    ident = G.gmres(lambda v: 3 * v, b, x0, m=4, tol=1e-12)
    assert ident["converged"] and ident["iterations"] == 1 and ident["breakdown"] and np.isfinite(ident["x"]).all()
    # frozen rows: x keeps its bits, the live block is solved with the frozen x on the right-hand side
    live = np.arange(n) % 7 != 0
    minv = np.where(live, 1.0 / np.diag(A), 0.0)
    fr = G.gmres(ap, b, x0, m=250, prec=lambda v: v * minv.astype(v.dtype), live=live, tol=1e-10, residual_scaling=2)
    assert fr["converged"] and np.array_equal(fr["x"][~live], x0[~live])
    assert np.linalg.norm((b - A @ fr["x"])[live]) <= 1.0001e-10 * np.linalg.norm(b)


def test_header_declares_and_library_exports_the_new_entry_points():
    header = open(os.path.join(ROOT, "include", "l3k.h")).read()
    lib = capi.load()
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in capi.SIGNATURES and hasattr(lib, name), name
    for name in ("l3k_gmres", "l3k_gmres_opts", "l3k_gmres_result", "l3k_gmres_info"):
        assert re.search(r"\b" + name + r";", header), name
    assert "#define L3K_VERSION 101" in header and lib.l3k_version() == 101
    text = header[header.index("restarted GMRES"):]
    assert "solve/BelosSolvers.hpp:124-130" in text and "solve/SolverInterface.hpp:26-37" in text and "setLeftPrec" in text
    import ctypes as C
    assert C.sizeof(capi.GmresOpts) == 24 and C.sizeof(capi.GmresResult) == 40 and C.sizeof(capi.GmresInfo) == 32


def test_entry_points_refuse_null_arguments_without_a_device():
    import ctypes as C
    lib, res, out = capi.load(), capi.GmresResult(), C.c_void_p()
    assert lib.l3k_gmres_create(None, 10, 5, 0, C.byref(out)) == -1
    assert lib.l3k_last_error().decode() == "l3k_gmres_create: null argument"
    assert lib.l3k_gmres_info_get(None, None) == -1
    for name in NEW[3:10]:
        assert getattr(lib, name)(None, None, None, None, None, None, C.byref(res)) == -1
        assert lib.l3k_last_error().decode() == name + ": null argument"
    for name, extra in (("l3k_gmres_multi_dot", ()), ("l3k_gmres_project", (None,)), ("l3k_gmres_combine", ())):
        assert getattr(lib, name)(None, None, 8, 1, None, None, 4, None, *extra) == -1
        assert lib.l3k_last_error().decode() == name + ": null argument"
    assert lib.l3k_gmres_destroy(None) == 0


def test_python_refusals_that_need_no_device():
    sys_ = types.SimpleNamespace(mesh=types.SimpleNamespace(n_owned_dofs=8, ctx=None), _h=None)
    other = types.SimpleNamespace(mesh=types.SimpleNamespace(n_owned_dofs=8, ctx=None), _h=None)
    import torch
    b, x = torch.zeros(8, dtype=torch.float64), torch.zeros(8, dtype=torch.float64)
    prec = types.SimpleNamespace(system=other, _h=None)
    with pytest.raises(capi.L3KError, match="give minv or precond"):
        solve.gmres(sys_, b, x, minv=b, precond=prec)
    with pytest.raises(capi.L3KError, match="created for another system"):
        solve.gmres(sys_, b, x, precond=prec)
    with pytest.raises(capi.L3KError, match="restart_length = 0 must be at least 1"):
        solve.gmres(sys_, b, x, restart_length=0)
    with pytest.raises(capi.L3KError, match="one shape over the owned dofs"):
        solve.gmres(sys_, b, torch.zeros(9, dtype=torch.float64))
    with pytest.raises(capi.L3KError, match="one shape over the owned dofs"):
        solve.gmres(sys_, torch.zeros(16, dtype=torch.float64)[::2], x)
    with pytest.raises(capi.L3KError, match="must not share memory"):
        solve.gmres(sys_, b, b)
    with pytest.raises(capi.L3KError, match="minv must be a contiguous tensor"):
        solve.gmres(sys_, b, x, minv=torch.zeros(7, dtype=torch.float64))
    ws = types.SimpleNamespace(n=9, _h=None)
    with pytest.raises(capi.L3KError, match="the workspace was created for n = 9, the system has 8 rows"):
        solve.gmres(sys_, b, x, workspace=ws)
    with pytest.raises(capi.L3KError, match="restart_length = 0 must be at least 1"):
        solve.GmresWorkspace(None, 8, 0)
    with pytest.raises(capi.L3KError, match="n = 0 must be at least 1"):
        solve.GmresWorkspace(None, 0, 5)
    with pytest.raises(KeyError):
        solve.gmres(sys_, b, x, residual_scaling="other")
