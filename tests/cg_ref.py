"""Plain high-precision restatements of the Jacobi-PCG vector kernels (include/l3k.h, "Jacobi-preconditioned conjugate
gradients"): what l3k_cg_init, l3k_cg_update_z, l3k_cg_update_px, l3k_jacobi_inverse and l3k_pcg_solve compute, written
element by element with numpy on the CPU.  No GPU, no libl3k.  tests/test_cg_ref_cpu.py pins these helpers,
tests/test_gpu_cg_kernels.py and tests/test_solve.py compare the device with them.

Precision: element-wise work and sums run in numpy.longdouble (x87 extended: eps = 2^-63; numpy.sum is pairwise, its
error is about 20 * 2^-64 relative to sum |terms|).  Where longdouble is no wider than that (HAVE_LD False) the sums take
the other exact route: the terms rounded to float64 and added with math.fsum (correctly rounded sum of its arguments).
dot_exact is exact on every platform for inputs of at most 24 significant bits (rand24).
"""
import math

import numpy as np

LD = np.longdouble
HAVE_LD = bool(np.finfo(LD).eps < 1e-18)
EPS = float(np.finfo(np.float64).eps)  # 2^-52


def rand24(rng, n, scale=1.0):
    """n mixed-sign float64 values with at most 24 significant bits (float32 draws): products of two are exact in float64"""
    return (rng.standard_normal(n).astype(np.float32) * np.float32(scale)).astype(np.float64)


def _sum(terms):
    terms = np.asarray(terms)
    if HAVE_LD:
        return np.sum(terms.astype(LD))
    return LD(math.fsum(np.asarray(terms, dtype=np.float64).tolist()))


def dot_exact(u, v):
    """(<u, v>, sum |u_i v_i|) as floats: every product is exact in float64 for 24-bit inputs, math.fsum rounds the exact
    sum once."""
    prod = np.asarray(u, dtype=np.float64) * np.asarray(v, dtype=np.float64)
    return math.fsum(prod.tolist()), math.fsum(np.abs(prod).tolist())


def _minv(minv, n):
    if minv is None:
        return np.ones(n, dtype=LD), np.zeros(n, dtype=bool)
    m = np.asarray(minv, dtype=np.float64)
    return m.astype(LD), m == 0.0


def residual_sums_ref(z, minv):
    """<r, z> and <r, r> with r = z / minv, frozen rows (minv == 0) left out: (rz, rr, sum |r z|, sum r^2)"""
    z = np.asarray(z, dtype=np.float64).astype(LD)
    m, frozen = _minv(minv, z.size)
    r = np.where(frozen, LD(0), z / np.where(frozen, LD(1), m))
    return _sum(r * z), _sum(r * r), _sum(np.abs(r * z)), _sum(r * r)


def cg_init_ref(ax0, b, minv):
    """l3k_cg_init: r = b - A x0 (0 on frozen rows), z = minv r, p = z, s[2] = <r, z>, s[3] = <r, r>.
    Returns dict(z, rz, rr, abs_rz, abs_rr, terms) with terms_i = |minv_i b_i| + |minv_i (A x0)_i| (the entry's formula)."""
    ax0, b = np.asarray(ax0, dtype=np.float64).astype(LD), np.asarray(b, dtype=np.float64).astype(LD)
    m, frozen = _minv(minv, b.size)
    r = np.where(frozen, LD(0), b - ax0)
    z = m * r
    return dict(z=z, rz=_sum(r * z), rr=_sum(r * r), abs_rz=_sum(np.abs(r * z)), abs_rr=_sum(r * r),
                terms=np.where(frozen, LD(0), np.abs(m * b) + np.abs(m * ax0)))


def cg_update_z_ref(z, ap, minv, s0, s1):
    """l3k_cg_update_z: alpha = s[0] / s[1] (one float64 division, as on the device); z -= alpha minv Ap.
    Returns dict(z, alpha, terms) with terms_i = |z_i| + |alpha minv_i ap_i|; the sums come from residual_sums_ref."""
    alpha = np.float64(s0) / np.float64(s1)
    z, ap = np.asarray(z, dtype=np.float64).astype(LD), np.asarray(ap, dtype=np.float64).astype(LD)
    m, _ = _minv(minv, z.size)
    t = LD(alpha) * (m * ap)
    return dict(z=z - t, alpha=float(alpha), terms=np.abs(z) + np.abs(t))


def cg_update_px_ref(p, x, z, s0, s1, s2):
    """l3k_cg_update_px: alpha = s[0] / s[1], beta = s[2] / s[0] (float64 divisions); x += alpha p; p = z + beta p.
    Returns dict(x, p, alpha, beta, terms_x, terms_p)."""
    alpha, beta = np.float64(s0) / np.float64(s1), np.float64(s2) / np.float64(s0)
    p, x, z = (np.asarray(a, dtype=np.float64).astype(LD) for a in (p, x, z))
    return dict(x=x + LD(alpha) * p, p=z + LD(beta) * p, alpha=float(alpha), beta=float(beta),
                terms_x=np.abs(x) + np.abs(LD(alpha) * p), terms_p=np.abs(z) + np.abs(LD(beta) * p))


def jacobi_inverse_ref(d, damping=1.0, threshold=0.0):
    """l3k_jacobi_inverse: sign(d) damping / max(|d|, threshold), sign(0) = +1.  One division per entry, which IEEE float64
    rounds correctly: the float64 quotient IS the reference (a longdouble quotient rounded again could differ in the last
    bit), so this one returns float64."""
    d = np.asarray(d, dtype=np.float64)
    a = np.abs(d)
    with np.errstate(divide="ignore"):
        return np.where(d < 0, -np.float64(damping), np.float64(damping)) / np.where(a > threshold, a, np.float64(threshold))


def pcg_ref(A, b, x0, minv, k, dtype=LD):
    """k steps of Hestenes-Stiefel PCG on the dense matrix A, every operation in `dtype` (longdouble: the reference;
    float64: the same recurrence at working precision, to measure what float64 alone costs).  Rows with minv == 0 are
    frozen: z = p = 0, x keeps x0, the row is left out of <r, r>.  Stops early when <r, r> reaches 0.
    Returns (x, res, steps, init): res = ||b - A x|| recomputed from x over the rows that are not frozen; steps[j] =
    dict(alpha, beta, pap, rz, rr) of step j + 1 (rz = <r, z> and rr = <r, r> after the step); init = dict(rz, rr) before
    the first step."""
    A, b, x = np.asarray(A).astype(dtype), np.asarray(b).astype(dtype), np.asarray(x0).astype(dtype).copy()
    n = b.size
    if minv is None:
        m, frozen = np.ones(n, dtype=dtype), np.zeros(n, dtype=bool)
    else:
        m, frozen = np.asarray(minv).astype(dtype), np.asarray(minv) == 0
    zero = dtype(0)

    def dot(u, v):
        return np.sum(u * v) if (dtype is not LD or HAVE_LD) else LD(math.fsum((u * v).astype(np.float64).tolist()))

    r = np.where(frozen, zero, b - A @ x)
    z = m * r
    p = z.copy()
    rz = dot(r, z)
    init = dict(rz=rz, rr=dot(r, r))
    steps = []
    for _ in range(k):
        if dot(r, r) == 0:
            break
        ap = A @ p
        pap = dot(p, ap)
        alpha = rz / pap
        x = x + alpha * p
        r = np.where(frozen, zero, r - alpha * ap)
        z = m * r
        rz_new = dot(r, z)
        beta = rz_new / rz
        p = z + beta * p
        rz = rz_new
        steps.append(dict(alpha=alpha, beta=beta, pap=pap, rz=rz, rr=dot(r, r)))
    true_r = np.where(frozen, zero, b - A @ x)
    return x, np.sqrt(dot(true_r, true_r)), steps, init
