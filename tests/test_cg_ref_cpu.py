"""Pins tests/cg_ref.py, the CPU restatements the PCG kernel tests compare the device with."""
import math
from fractions import Fraction

import numpy as np

import cg_ref as R


def test_longdouble_is_extended_or_sums_fall_back():
    assert R.HAVE_LD == (np.finfo(np.longdouble).eps < 1e-18)
    # either way the sums are good to far below float64's eps: 2^-30 + 1 - 1 over 1000 entries
    t = np.concatenate([[1.0], np.full(1000, 2.0 ** -30), [-1.0]])
    assert float(R._sum(t)) == 1000 * 2.0 ** -30


def test_dot_exact_against_fractions():
    rng = np.random.default_rng(11)
    u, v = R.rand24(rng, 1000, 3.0), R.rand24(rng, 1000, 1e3)
    u[::7] *= 2.0 ** 20  # a wide range of exponents, still 24 significant bits
    assert np.all(u.astype(np.float32).astype(np.float64) == u) and (u < 0).any() and (u > 0).any()
    exact = sum((Fraction(float(a)) * Fraction(float(b)) for a, b in zip(u, v)), Fraction(0))
    exact_abs = sum((abs(Fraction(float(a)) * Fraction(float(b))) for a, b in zip(u, v)), Fraction(0))
    got, got_abs = R.dot_exact(u, v)
    # correctly rounded: the nearest float64 of the exact rational sum
    assert got == float(exact) and got_abs == float(exact_abs)


def test_pcg_ref_solves_a_random_spd_system():
    rng = np.random.default_rng(5)
    n = 40
    Q = rng.standard_normal((n, n))
    A = Q @ Q.T + n * np.eye(n)
    b, x0 = rng.standard_normal(n), rng.standard_normal(n)
    minv = 1.0 / np.diag(A)
    want = np.linalg.solve(A, b)
    x, res, steps, init = R.pcg_ref(A, b, x0, minv, n)
    assert len(steps) == n
    assert np.abs(np.asarray(x, dtype=np.float64) - want).max() <= 1e-13 * np.abs(want).max()
    assert float(res) <= 1e-13 * np.linalg.norm(b)
    # the scalars are those of the recurrence: first step by hand
    r0 = b - A @ x0
    assert abs(float(init["rr"]) - r0 @ r0) <= 1e-14 * (r0 @ r0)
    assert abs(float(init["rz"]) - r0 @ (minv * r0)) <= 1e-14 * abs(r0 @ (minv * r0))
    p0 = minv * r0
    assert abs(float(steps[0]["alpha"]) - (r0 @ p0) / (p0 @ A @ p0)) <= 1e-14 * abs(float(steps[0]["alpha"]))
    # k steps stop after k steps, and no preconditioner is the identity
    x3, _, s3, _ = R.pcg_ref(A, b, x0, None, 3)
    x3b, _, _, _ = R.pcg_ref(A, b, x0, np.ones(n), 3)
    assert len(s3) == 3 and np.array_equal(x3, x3b) and not np.array_equal(x3, x)
    # the float64 run of the same recurrence stays within a few eps * cond of the longdouble one
    x64, _, _, _ = R.pcg_ref(A, b, x0, minv, 6, dtype=np.float64)
    xld, _, _, _ = R.pcg_ref(A, b, x0, minv, 6)
    assert x64.dtype == np.float64 and np.abs(x64 - np.asarray(xld, dtype=np.float64)).max() <= 1e-12 * np.abs(x64).max()


def test_frozen_row_rule_on_four_entries():
    b = np.array([3.0, 5.0, -2.0, 7.0])
    ax0 = np.array([1.0, 1.0, 1.0, 1.0])
    minv = np.array([0.5, 0.0, 2.0, 0.25])  # row 1 frozen
    i = R.cg_init_ref(ax0, b, minv)
    # r = (2, -, -3, 6); z = (1, 0, -6, 1.5)
    assert np.array_equal(np.asarray(i["z"], dtype=np.float64), [1.0, 0.0, -6.0, 1.5])
    assert float(i["rz"]) == 2.0 + 18.0 + 9.0 and float(i["rr"]) == 4.0 + 9.0 + 36.0  # the frozen row's 4^2 is left out
    assert float(i["terms"][1]) == 0.0
    z = np.array([1.0, 0.0, -6.0, 1.5])
    ap = np.array([2.0, 100.0, 1.0, -4.0])
    u = R.cg_update_z_ref(z, ap, minv, 3.0, 6.0)  # alpha = 0.5
    assert u["alpha"] == 0.5
    assert np.array_equal(np.asarray(u["z"], dtype=np.float64), [1.0 - 0.5, 0.0, -6.0 - 1.0, 1.5 + 0.5])
    rz, rr, arz, arr = R.residual_sums_ref(np.asarray(u["z"], dtype=np.float64), minv)
    # r = z / minv = (1, -, -3.5, 8)
    assert float(rz) == 0.5 + 24.5 + 16.0 and float(rr) == 1.0 + 12.25 + 64.0 and float(arz) == float(rz) and float(arr) == float(rr)
    px = R.cg_update_px_ref(np.array([1.0, 0.0, 2.0, 4.0]), np.array([9.0, 8.0, 7.0, 6.0]), z, 2.0, 4.0, 1.0)  # alpha = beta = 0.5
    assert np.array_equal(np.asarray(px["x"], dtype=np.float64), [9.5, 8.0, 8.0, 8.0])
    assert np.array_equal(np.asarray(px["p"], dtype=np.float64), [1.5, 0.0, -5.0, 3.5])
    # no preconditioner: minv = None is minv = 1
    a, o = R.cg_init_ref(ax0, b, None), R.cg_init_ref(ax0, b, np.ones(4))
    assert np.array_equal(a["z"], o["z"]) and a["rz"] == o["rz"] == a["rr"]
    # the frozen row in the dense recurrence: x keeps x0 there
    A = np.diag([2.0, 3.0, 4.0, 5.0]) + 0.1
    x, res, steps, _ = R.pcg_ref(A, b, np.array([0.0, 0.7, 0.0, 0.0]), np.array([0.5, 0.0, 0.25, 0.2]), 4)
    assert float(x[1]) == 0.7
    free = [0, 2, 3]
    want = np.linalg.solve(A[np.ix_(free, free)], b[free] - A[free, 1] * 0.7)
    assert np.abs(np.asarray(x, dtype=np.float64)[free] - want).max() < 1e-14 and float(res) < 1e-14


def test_jacobi_inverse_ref():
    d = np.array([2.0, -4.0, 1e-9, 0.0, -1e-9])
    assert np.array_equal(R.jacobi_inverse_ref(d, 0.5, 1e-3), [0.25, -0.125, 500.0, 500.0, -500.0])
    assert np.array_equal(R.jacobi_inverse_ref(d[:2], 0.0, 0.0), [0.0, -0.0])
    assert math.isinf(R.jacobi_inverse_ref(np.array([0.0]))[0])
