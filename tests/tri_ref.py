"""The triangular preconditioners of l3k_tri (include/l3k.h) restated in numpy and longdouble: the levels of the two solves, row-wise
IKJ ILU(0) with the two thresholds, SSOR, the two triangular solves of each kind, PCG with a preconditioner given as a callable, and
the two derived bounds the device is held to.  No GPU and no libl3k in here.

A matrix is a dense array A[..., n, n] (leading dimensions: a batch of matrices of ONE pattern) with a boolean pattern P[n, n] of
the stored entries; a row is ACTIVE if it stores an entry, and entries in the column of an inactive row are outside the block the
factorisation and the solves work on."""
import numpy as np

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)


def active_rows(P):
    return P.any(axis=1)


def block(P):
    """the pattern restricted to the active principal block"""
    a = active_rows(P)
    return P & a[:, None] & a[None, :]


def levels(P, upper=False):
    """level[i] = 1 + max level[j] over the stored active j < i (upper: j > i, rows walked downwards), 1 without one, 0 on an
    inactive row; returns (level, n_levels)"""
    n, a, B = P.shape[0], active_rows(P), block(P)
    level = np.zeros(n, dtype=np.int32)
    for i in (range(n - 1, -1, -1) if upper else range(n)):
        if a[i]:
            dep = B[i, i + 1:] if upper else B[i, :i]
            lv = level[i + 1:] if upper else level[:i]
            level[i] = 1 + (lv[dep].max() if dep.any() else 0)
    return level, int(level.max()) if n else 0


def rows_by_level(level):
    """the active rows level by level, ascending within a level, and the first position of every level"""
    order = np.argsort(level, kind="stable")
    order = order[level[order] > 0]
    return order.astype(np.int32), np.concatenate([[0], np.cumsum(np.bincount(level[level > 0], minlength=level.max() + 1)[1:])])


def launch_plan(level, fuse_rows, max_fused_levels=4096):
    """[(first level, one past the last, fused)]: consecutive levels of at most fuse_rows rows form one fused launch of at most
    max_fused_levels levels, every wider level is a launch of its own"""
    sizes = np.bincount(level[level > 0], minlength=int(level.max()) + 1)[1:]
    plan = []
    for lv, s in enumerate(sizes):
        narrow = s <= fuse_rows
        if narrow and plan and plan[-1][2] and lv - plan[-1][0] < max_fused_levels:
            plan[-1][1] = lv + 1
        else:
            plan.append([lv, lv + 1, narrow])
    return [tuple(p) for p in plan]


def thresholded(A, P, absolute=0.0, relative=1.0, dtype=LD):
    """a_ii <- sign(a_ii) * absolute + relative * a_ii on the active rows (sign(0) = +1)"""
    F = np.array(A, dtype=dtype)
    i = np.nonzero(active_rows(P))[0]
    d = F[..., i, i]
    F[..., i, i] = np.where(d < 0, -dtype(absolute), dtype(absolute)) + dtype(relative) * d
    return F


def ilu0(A, P, absolute=0.0, relative=1.0, dtype=LD):
    """Row-wise IKJ: for row i, every stored active k < i ascending: l_ik = a_ik / u_kk; for every stored active j > k of row k
    that row i stores: a_ij -= l_ik u_kj.  A pivot that is zero or not finite becomes 1.  Returns (F, n_bad, first_bad): l below
    the diagonal, u on and above, A's values outside the active block"""
    n, a, B = P.shape[0], active_rows(P), block(P)
    F = thresholded(A, P, absolute, relative, dtype)
    n_bad, first_bad = 0, -1
    cols = np.arange(n)
    for i in np.nonzero(a)[0]:
        for k in np.nonzero(B[i, :i])[0]:
            lik = F[..., i, k] / F[..., k, k]
            F[..., i, k] = lik
            js = np.nonzero(B[k] & B[i] & (cols > k))[0]
            F[..., i, js] -= lik[..., None] * F[..., k, js]
        piv = F[..., i, i]
        bad = (piv == 0) | ~np.isfinite(piv)
        if np.any(bad):
            n_bad += int(np.sum(bad))
            first_bad = i if first_bad < 0 else first_bad
            F[..., i, i] = np.where(bad, dtype(1), piv)
    return F, n_bad, first_bad


def triangles(M, P, kind, omega=1.0, dtype=LD):
    """(T_lower, T_upper, s): the matrices of the two solves on the active block -- 'ilu0': I + strict lower of the factor M, its
    upper triangle, s = 1; 'sgs': D / omega + L and D / omega + U of A = M, and s = ((2 - omega) / omega) diag(A), the scaling of the
    right-hand side of the upper solve.  Inactive rows and columns are zero"""
    B = block(P)
    M = np.where(B, np.asarray(M, dtype=dtype), dtype(0))
    n = P.shape[0]
    a = active_rows(P).astype(dtype)
    d = np.einsum("...ii->...i", M)
    eye = np.eye(n, dtype=dtype)
    if kind == "ilu0":
        return np.tril(M, -1) + eye * a, np.triu(M), np.ones(M.shape[:-1], dtype=dtype) * a
    w = dtype(omega)
    D = eye * (d / w)[..., None, :]
    return np.tril(M, -1) + D, np.triu(M, 1) + D, (dtype(2) - w) / w * d


def solve_tri(T, r, upper, active):
    """T z = r by substitution on the active rows, z = 0 elsewhere"""
    n = T.shape[-1]
    z = np.zeros(np.broadcast_shapes(T.shape[:-2], r.shape[:-1]) + (n,), dtype=T.dtype)
    for i in (range(n - 1, -1, -1) if upper else range(n)):
        if active[i]:
            s = (T[..., i, i + 1:] * z[..., i + 1:]).sum(-1) if upper else (T[..., i, :i] * z[..., :i]).sum(-1)
            z[..., i] = (r[..., i] - s) / T[..., i, i]
    return z


class Preconditioner:
    """z = M^-1 r as l3k_tri_apply defines it, in `dtype`: lower(r), upper(y) and __call__ = upper(lower(r))"""

    def __init__(self, A, P, kind, omega=1.0, absolute=0.0, relative=1.0, dtype=LD):
        self.kind, self.active, self.dtype = kind, active_rows(P), dtype
        self.n_bad, self.first_bad = 0, -1
        if kind == "ilu0":
            self.F, self.n_bad, self.first_bad = ilu0(A, P, absolute, relative, dtype)
        else:
            self.F = np.array(A, dtype=dtype)
        self.Tl, self.Tu, self.s = triangles(self.F, P, kind, omega, dtype)

    def lower(self, r):
        return solve_tri(self.Tl, np.asarray(r, dtype=self.dtype), False, self.active)

    def upper(self, y):
        return solve_tri(self.Tu, self.s * np.asarray(y, dtype=self.dtype), True, self.active)

    def __call__(self, r):
        return self.upper(self.lower(r))


def ssor_dense(A, omega=1.0):
    """M = (D / w + L) (w / (2 - w)) D^-1 (D / w + U) from its formula, dense, every row active"""
    A = np.asarray(A, dtype=LD)
    w, D = LD(omega), np.diag(np.diag(A))
    return (D / w + np.tril(A, -1)) @ (w / (LD(2) - w) * np.diag(1 / np.diag(A))) @ (D / w + np.triu(A, 1))


def lu_nopivot(A, dtype=LD):
    """dense LU without pivoting, L unit lower: (L, U)"""
    U = np.array(A, dtype=dtype)
    n = U.shape[0]
    Lm = np.eye(n, dtype=dtype)
    for k in range(n - 1):
        Lm[k + 1:, k] = U[k + 1:, k] / U[k, k]
        U[k + 1:] -= Lm[k + 1:, k, None] * U[k]
        U[k + 1:, k] = 0
    return Lm, U


# ------------------------------------------------------------------------------------------------ the bounds
def factor_bound(A, F, P):
    """For every stored (i, j) of the active block, with l and u taken from F (the device's factor, or the restatement's) and the
    sums formed in longdouble: err = |a_ij - sum_k l_ik u_kj| and bound = (m_ij + 3) EPS sum_k |l_ik| |u_kj| -- k over the pattern
    intersection, the unit diagonal of L included, m_ij the number of terms.  That is the first-order backward error of Gaussian
    elimination in any order of summation (Higham, Accuracy and Stability, Theorem 9.3, with gamma_m <= (m + 3) EPS to first
    order and three roundings to spare for the thresholded diagonal); contraction to FMA only removes roundings.  A: the matrix
    that was factored, thresholds applied.  Returns (err, bound), both NaN outside the block"""
    B = block(P)
    n = P.shape[0]
    Tl, Tu, _ = triangles(F, P, "ilu0")
    Pl, Pu = np.tril(B, -1) | (np.eye(n, dtype=bool) & B), np.triu(B)
    m = Pl.astype(np.float64) @ Pu.astype(np.float64)
    S, Sabs = np.zeros(Tl.shape, dtype=LD), np.zeros(Tl.shape, dtype=LD)
    for i in np.nonzero(active_rows(P))[0]:
        ks = np.nonzero(Pl[i])[0]
        S[..., i, :] = np.einsum("...k,...kj->...j", Tl[..., i, ks], Tu[..., ks, :])
        Sabs[..., i, :] = np.einsum("...k,...kj->...j", np.abs(Tl[..., i, ks]), np.abs(Tu[..., ks, :]))
    err = np.where(B, np.abs(np.asarray(A, dtype=LD) - S), np.nan)
    return err, np.where(B, (m + 3) * EPS * Sabs, np.nan)


def solve_bound(T, z, r, active):
    """For every active row: err = |r_i - (T z)_i| with T z in longdouble from the solver's z, bound = (len_i + 3) EPS sum_j
    |t_ij| |z_j|, len_i the entries of row i of T: a sum of len_i - 1 products, one subtraction from r_i and the division by (or
    the multiplication with the rounded reciprocal of) t_ii."""
    T, z, r = np.asarray(T, dtype=LD), np.asarray(z, dtype=LD), np.asarray(r, dtype=LD)
    err = np.abs(r - np.einsum("...ij,...j->...i", T, z))
    bound = ((T != 0).sum(-1) + 3) * EPS * np.einsum("...ij,...j->...i", np.abs(T), np.abs(z))
    return np.where(active, err, 0), np.where(active, bound, 0)


# ------------------------------------------------------------------------------------------------ PCG
def pcg(apply, b, x0, prec, live=None, tol=1e-6, max_iters=10_000, residual_scaling=2, dtype=LD):
    """The loop of l3k_csr_pcg_solve_tri (pcgSolvePrecond): Hestenes-Stiefel PCG that keeps r, the frozen rows (live == False) keep
    x and carry r = 0, the residual of the recurrence decides.  residual_scaling 0: none, 2: |b|.  Returns dict(x, iterations,
    converged, achieved_tol, history): history[k] = the scaled residual after step k + 1"""
    T = dtype
    b, x = np.asarray(b, dtype=T), np.array(x0, dtype=T)
    live = np.ones(b.size, dtype=bool) if live is None else np.asarray(live, dtype=bool)
    zero = T(0)
    r = np.where(live, b - apply(x), zero)
    scale = T(1)
    if residual_scaling == 2:
        bb = np.sqrt(np.sum(b * b))
        scale = bb if bb > 1e-300 else T(1e-300)
    res, it, history = np.sqrt(np.sum(r * r)) / scale, 0, []
    if res > tol and max_iters > 0:
        z = np.where(live, prec(r), zero)
        p, rz = z.copy(), np.sum(r * z)
        while True:
            ap = apply(p)
            alpha = rz / np.sum(p * ap)
            x = np.where(live, x + alpha * p, x)
            r = np.where(live, r - alpha * ap, zero)
            res = np.sqrt(np.sum(r * r)) / scale
            it += 1
            history.append(float(res))
            if res <= tol or it >= max_iters:
                break
            z = np.where(live, prec(r), zero)
            rz_new = np.sum(r * z)
            p = z + (rz_new / rz) * p
            rz = rz_new
    return dict(x=x, iterations=it, converged=bool(res <= tol), achieved_tol=float(res), history=history)


def choose_tol(history, near=2, also=()):
    """a tolerance with both stopping margins >= 1.5: the geometric mean of the first two consecutive entries of `history`, from
    step `near` on, that are a factor >= 2.25 apart (the method of tests/test_gpu_gmres.py), with every earlier entry a factor >= 1.5
    above it as well (the residuals of PCG do not fall monotonically).  `also`: further histories of the same iteration -- the same
    restatement in float64, say -- that must stop at the same step with the same margins: a tolerance at which rounding in the
    working precision cannot move the count.  Returns (tol, iterations)"""
    for j in range(max(near, 1), len(history)):
        tol = float(np.sqrt(history[j - 1] * history[j]))
        if all(len(h) > j and h[j] * 1.5 <= tol and min(h[:j]) >= 1.5 * tol for h in (history, *also)):
            return tol, j + 1
    raise AssertionError("no two consecutive residuals a factor 2.25 apart")


# ------------------------------------------------------------------------------------------------ the designed matrices
def to_csr(A, P):
    """(row_ptr int64, col_ind int32, values float64) of the stored entries"""
    rows, cols = np.nonzero(P)
    return (np.concatenate([[0], np.cumsum(P.sum(axis=1))]).astype(np.int64), cols.astype(np.int32),
            np.ascontiguousarray(np.asarray(A, dtype=np.float64)[rows, cols]))


def from_csr(row_ptr, col_ind, values, dtype=np.float64):
    n = len(row_ptr) - 1
    rows = np.repeat(np.arange(n), np.diff(row_ptr))
    A, P = np.zeros((n, n), dtype=dtype), np.zeros((n, n), dtype=bool)
    A[rows, col_ind] = values
    P[rows, col_ind] = True
    return A, P


def tridiagonal_pattern(n):
    i = np.arange(n)
    return np.abs(i[:, None] - i[None, :]) <= 1


def spd_matrix(n=100):
    """the reference's makeSPDMatrix: tridiagonal [.5 2 .5], identity end rows, the zeroed couplings stored"""
    A = 2.0 * np.eye(n) + 0.5 * np.eye(n, k=1) + 0.5 * np.eye(n, k=-1)
    A[0], A[-1] = 0.0, 0.0
    A[0, 0] = A[-1, -1] = 1.0
    A[1, 0] = A[-2, -1] = 0.0
    return A, tridiagonal_pattern(n)


def chains(n_chains, seed=3):
    """n_chains independent chains of 3 rows: B[n_chains, 3, 3] of tridiagonal pattern, random, strictly diagonally dominant, not
    symmetric.  Row 3 c + q of the whole matrix is row q of block c: 3 levels of n_chains rows each way"""
    rng = np.random.default_rng(seed)
    P = tridiagonal_pattern(3)
    B = np.where(P, rng.uniform(-1.0, 1.0, (n_chains, 3, 3)), 0.0)
    q = np.arange(3)
    B[:, q, q] = (np.abs(B).sum(-1) - np.abs(B[:, q, q]) + rng.uniform(0.5, 1.5, (n_chains, 3))) * np.where(rng.uniform(size=(n_chains, 3)) < 0.25, -1, 1)
    return B, P


def chains_csr(B, P):
    nc = B.shape[0]
    r, c = np.nonzero(P)
    per_row = P.sum(axis=1)
    row_ptr = np.concatenate([[0], np.cumsum(np.tile(per_row, nc))]).astype(np.int64)
    col_ind = (3 * np.arange(nc)[:, None] + c[None, :]).reshape(-1).astype(np.int32)
    return row_ptr, col_ind, np.ascontiguousarray(B[:, r, c].reshape(-1))


def band(n=400, half_width=70, seed=4):
    """a full band, random, strictly diagonally dominant, not symmetric"""
    rng = np.random.default_rng(seed)
    i = np.arange(n)
    P = np.abs(i[:, None] - i[None, :]) <= half_width
    A = np.where(P, rng.uniform(-1.0, 1.0, (n, n)), 0.0)
    A[i, i] = np.abs(A).sum(-1) - np.abs(A[i, i]) + rng.uniform(0.5, 1.5, n)
    return A, P


def grid(m=24):
    """upwind convection-diffusion on m x m points in natural order: diagonal 6.25, west -2.5, east -1, south -1.75, north -1"""
    n = m * m
    A, P = np.zeros((n, n)), np.zeros((n, n), dtype=bool)
    for y in range(m):
        for x in range(m):
            i = y * m + x
            for dx, dy, v in ((0, 0, 6.25), (-1, 0, -2.5), (1, 0, -1.0), (0, -1, -1.75), (0, 1, -1.0)):
                if 0 <= x + dx < m and 0 <= y + dy < m:
                    A[i, i + dy * m + dx], P[i, i + dy * m + dx] = v, True
    return A, P
