"""The Chebyshev-Jacobi preconditioner on the CPU: solve.chebyshev_reference (the torch restatement of l3k_cheb_apply) against
the explicit polynomial in D^-1 A formed with numpy from the oracle's dense operator, solve.cg with a preconditioner callable,
and the new entry points of the C ABI without a device."""
import ctypes as C

import numpy as np
import pytest
import torch

import oracle_lib as O
from helpers import oracle_mesh
from l3ster_amd import capi, solve
from test_solve import setup_problem

COND = 30.0
_P = {}


def problem():
    """test_solve.setup_problem at (ne, p) = (3, 2): 1 372 dofs; the oracle's operator as a dense matrix (mf_apply on the
    identity), its diagonal and right-hand side, minv, and the extreme eigenvalue of D^-1 A."""
    if _P:
        return _P
    p, kpar = 2, [1.0, 0.0]
    part, mask, g, exact = setup_problem(3, p)
    om = oracle_mesh(part, p + 1, 4, np.arange(4), mask)
    diag, rhs = O.mf_diag_rhs(om, 0, 1, np.asfortranarray(g.T), kparams=kpar)
    n = len(diag)
    assert n == 1372
    A = np.ascontiguousarray(O.mf_apply(om, 0, np.eye(n), kparams=kpar))
    assert np.abs(A - A.T).max() <= 1e-12 * np.abs(A).max()
    A = 0.5 * (A + A.T)
    minv = solve.jacobi_inverse(torch.as_tensor(diag))
    d = minv.numpy()
    S = np.sqrt(d)[:, None] * A * np.sqrt(d)[None, :]  # D^-1/2 A D^-1/2: the spectrum of D^-1 A, symmetric
    lam = np.linalg.eigvalsh(S)
    assert lam[0] > 0
    At = torch.as_tensor(A)
    _P.update(A=A, At=At, minv=minv, b=torch.as_tensor(rhs[:, 0].copy()), exact=exact, n=n, lmax=float(lam[-1]),
              apply=lambda v, out: out.copy_(At @ v))
    return _P


def explicit_polynomial(A, minv, r, lmax, cond, degree):
    """z = (I - T_d((theta I - D^-1 A) / delta) / T_d(theta / delta)) A^-1 r, matrices formed explicitly"""
    n = len(r)
    lmin = lmax / cond
    theta, delta = (lmax + lmin) / 2, (lmax - lmin) / 2
    M = (theta * np.eye(n) - minv[:, None] * A) / delta
    T_prev, T, t_prev, t = np.eye(n), M, 1.0, theta / delta
    for _ in range(1, degree):
        T_prev, T = T, 2 * M @ T - T_prev
        t_prev, t = t, 2 * (theta / delta) * t - t_prev
    u = np.linalg.solve(A, r)
    return u - T @ u / t


@pytest.mark.parametrize("degree", [1, 2, 3, 4])
def test_reference_equals_the_explicit_polynomial(degree):
    P = problem()
    r = np.random.default_rng(11).standard_normal(P["n"])
    z = solve.chebyshev_reference(P["apply"], P["minv"], torch.as_tensor(r), P["lmax"], COND, degree).numpy()
    want = explicit_polynomial(P["A"], P["minv"].numpy(), r, P["lmax"], COND, degree)
    err = np.linalg.norm(z - want) / np.linalg.norm(want)
    print(f"degree {degree}: recurrence against the closed form {err:.3e}")
    assert err <= 1e-11


def test_degree_one_is_scaled_jacobi():
    P = problem()
    r = torch.as_tensor(np.random.default_rng(12).standard_normal(P["n"]))
    theta = (P["lmax"] + P["lmax"] / COND) / 2
    z = solve.chebyshev_reference(P["apply"], P["minv"], r, P["lmax"], COND, 1)
    assert (z - P["minv"] * r / theta).norm().item() <= 1e-15 * z.norm().item()
    c0, steps = solve.chebyshev_coefficients(P["lmax"], P["lmax"] / COND, 1)
    assert steps == [] and c0 == 1.0 / theta
    assert len(solve.chebyshev_coefficients(P["lmax"], P["lmax"] / COND, 5)[1]) == 4
    # frozen rows: zero, whatever A z holds there
    minv = P["minv"].clone()
    minv[::7] = 0.0

    def apply_nan(v, out):
        out.copy_(P["At"] @ v)
        out[::7] = float("nan")

    z = solve.chebyshev_reference(apply_nan, minv, r, P["lmax"], COND, 3)
    assert bool(torch.isfinite(z).all()) and float(z[::7].abs().max()) == 0.0 and float(z.abs().max()) > 0.0


def test_cg_with_a_preconditioner_callable_reaches_the_jacobi_solution():
    P = problem()
    xj = torch.zeros(P["n"], dtype=torch.float64)
    rj = solve.cg(P["apply"], P["b"], xj, P["minv"], tol=1e-11, residual_scaling="rhs")
    xc = torch.zeros(P["n"], dtype=torch.float64)
    rc = solve.cg(P["apply"], P["b"], xc, tol=1e-11, residual_scaling="rhs",
                  precond=lambda r: solve.chebyshev_reference(P["apply"], P["minv"], r, P["lmax"], COND, 3))
    print(f"iterations: Jacobi {rj.num_iters}, Chebyshev degree 3 {rc.num_iters}")
    assert rj.converged and rc.converged
    assert (xc - xj).norm().item() <= 1e-8 * xj.norm().item()
    assert np.abs(xc.numpy() - P["exact"]).max() < 1e-8
    assert rc.num_iters < rj.num_iters  # (a polynomial of degree 3 with the exact lambda_max: fewer outer iterations)
    with pytest.raises(ValueError, match="not both"):
        solve.cg(P["apply"], P["b"], xc, P["minv"], precond=lambda r: r)


def test_power_start_vector_is_the_documented_hash():
    """include/l3k.h: h = (uint32) i; h ^= h >> 16; h *= 0x7feb352d; h ^= h >> 15; h *= 0x846ca68b; h ^= h >> 16"""
    n = 70000
    h = np.arange(n, dtype=np.uint32)
    h ^= h >> np.uint32(16)
    h *= np.uint32(0x7FEB352D)
    h ^= h >> np.uint32(15)
    h *= np.uint32(0x846CA68B)
    h ^= h >> np.uint32(16)
    want = h.astype(np.float64) * 2.0 ** -31 - 1.0
    got = solve.power_start_vector(n).numpy()
    assert np.array_equal(got, want) and want.min() >= -1.0 and want.max() < 1.0 and abs(want.mean()) < 0.01


def test_new_entry_points_fail_loudly_without_a_device():
    """No handle can exist without a device (system.Context raises, test_cabi_cpu.py); the new entry points refuse null handles
    with -1 and a message instead of touching one."""
    lib = capi.load()
    out, info, res = C.c_void_p(), capi.ChebInfo(), capi.CgResult()
    calls = {
        "l3k_cheb_create": lambda: lib.l3k_cheb_create(None, None, None, C.byref(out)),
        "l3k_cheb_info_get": lambda: lib.l3k_cheb_info_get(None, C.byref(info)),
        "l3k_cheb_apply": lambda: lib.l3k_cheb_apply(None, None, None),
        "l3k_pcg_solve_cheb": lambda: lib.l3k_pcg_solve_cheb(None, None, None, None, None, C.byref(res)),
        "l3k_cheb_first": lambda: lib.l3k_cheb_first(None, None, None, 1.0, None, None, 0, None),
        "l3k_cheb_step": lambda: lib.l3k_cheb_step(None, None, None, None, 1.0, 1.0, None, None, 0, None),
        "l3k_cg_update_rx": lambda: lib.l3k_cg_update_rx(None, None, None, None, None, None, 0, None),
        "l3k_cg_update_p": lambda: lib.l3k_cg_update_p(None, None, None, 0, None),
    }
    for name, call in calls.items():
        assert call() == -1, name
        assert lib.l3k_last_error().decode() == f"{name}: null argument", name
        with pytest.raises(capi.L3KError, match=name):
            capi.check(call())
    assert out.value is None and lib.l3k_cheb_destroy(None) == 0
    if not torch.cuda.is_available():
        from l3ster_amd import system
        with pytest.raises(system.L3KError, match="no HIP device|no CPU fallback"):
            system.Context(0)
