"""The collective GMRES of a partitioned system (include/l3k.h: l3k_gmres_solve_dist, l3k_csr_dist_gmres_solve) restated in numpy, and
a partitioned non-symmetric chain to run it on.  No GPU, no libl3k.

The arithmetic is that of tests/gmres_ref.py with the dot products of a partitioned run: every rank sums over its OWNED rows, the
ranks' sums are added in ascending rank order (l3k_halo_allreduce_sum_n), and every step after a reducing pass -- the Hessenberg
column, the rotations, the breakdown test, the stopping rules -- reads the reduced values.  The operator and the preconditioner are
callables on whole vectors: what a rank's rows of A x are does not depend on the partition beyond rounding.

The chain is the tridiagonal (-1 - c, 2.5 + 0.5 sin i, -1 + c) of tests/test_gpu_gmres.py::test_nonsymmetric_tridiagonal in the
SUB-ASSEMBLED form of DESIGN.md 4.20: link i joins the rows i and i + 1 and belongs to the owner of row i; a rank holds the 2 x 2
blocks of its links over [owned | ghost], so the last link of a rank reaches into a ghost copy of the next rank's first row, and
that ghost row is export-added to its owner.  A row's diagonal is split in halves between its two links (the end rows have one)."""
import types

import numpy as np

from csr_dist_ref import ExchangeLists
from gmres_ref import LD


def rank_slices(offsets):
    return [slice(int(a), int(b)) for a, b in zip(offsets[:-1], offsets[1:])]


def gmres(apply, offsets, b, x0, m, prec=None, live=None, tol=1e-6, max_iters=10_000, residual_scaling=0, max_restarts=39,
          dtype=np.float64):
    """gmres_ref.gmres with partitioned dot products; offsets: the first row of every rank and the number of rows.  Returns its dict."""
    T = dtype
    parts = rank_slices(offsets)
    b = np.asarray(b, dtype=T)
    x = np.array(x0, dtype=T)
    n = b.size
    live = np.ones(n, dtype=bool) if live is None else np.asarray(live, dtype=bool)
    prec = prec or (lambda v: v)
    zero = T(0)

    def dot(u, v):
        acc = None
        for p in parts:  # (ascending rank order; a rank without rows brings 0)
            s = np.sum(u[p] * v[p], dtype=T)
            acc = s if acc is None else acc + s
        return acc

    def dots(Vk, w):
        acc = None
        for p in parts:
            s = Vk[:, p] @ w[p]
            acc = s if acc is None else acc + s
        return acc

    it, cycles, breakdown, orth_loss, scale, est = 0, 0, False, 0.0, T(1), None
    history = []
    while True:
        r = np.where(live, b - apply(x), zero)
        beta = np.sqrt(dot(r, r))
        if cycles == 0:
            if residual_scaling == 1:
                scale = beta if beta > 0 else T(1)
            elif residual_scaling == 2:
                bb = np.sqrt(dot(b, b))
                scale = bb if bb > 1e-300 else T(1e-300)
            est = beta / scale
        res = beta / scale
        if res <= tol or it >= max_iters or cycles > max_restarts or not beta > 0:
            break
        steps = min(m, max_iters - it)
        V = np.zeros((steps + 1, n), dtype=T)
        H = np.zeros((steps + 1, steps), dtype=T)
        cs, sn, g = np.zeros(steps, dtype=T), np.zeros(steps, dtype=T), np.zeros(steps + 1, dtype=T)
        V[0], g[0] = r / beta, beta
        kv = 0
        for k in range(steps):
            w = np.where(live, apply(prec(V[k])), zero)
            Vk = V[:k + 1]
            h1 = dots(Vk, w)
            w = w - h1 @ Vk
            h2 = dots(Vk, w)
            w = w - h2 @ Vk
            t, nu = dots(Vk, w), np.sqrt(dot(w, w))
            col = np.zeros(k + 2, dtype=T)
            col[:k + 1] = h1 + h2
            bd = not nu > T(2.0 ** -52) * np.sqrt(np.sum(col[:k + 1] ** 2))
            for j in range(k):
                a, c = col[j], col[j + 1]
                col[j], col[j + 1] = cs[j] * a + sn[j] * c, cs[j] * c - sn[j] * a
            a = col[k]
            rr = np.hypot(a, nu)
            cs[k], sn[k] = (a / rr, nu / rr) if rr > 0 else (T(1), zero)
            col[k], col[k + 1] = rr, zero
            H[:k + 2, k] = col
            g[k + 1], g[k] = -sn[k] * g[k], cs[k] * g[k]
            est = abs(g[k + 1]) / scale
            history.append(float(est))
            kv = k + 1
            if bd:
                breakdown = True
                break
            orth_loss = max(orth_loss, float(np.max(np.abs(t)) / nu))
            if est <= tol:
                break
            if k + 1 < steps:
                V[k + 1] = w / nu
        it += kv
        y = np.zeros(kv, dtype=T)
        for j in range(kv - 1, -1, -1):
            y[j] = (g[j] - H[j, j + 1:kv] @ y[j + 1:]) / H[j, j] if H[j, j] != 0 else zero
        x = np.where(live, x + prec(y @ V[:kv]), x)
        cycles += 1
    return dict(x=x, iterations=it, restarts=max(cycles - 1, 0), converged=bool(res <= tol), breakdown=breakdown,
                achieved_tol=float(res), estimate=float(est), orth_loss=orth_loss, history=history)


def pcg(apply, b, minv, tol, max_iters, dtype=LD):
    """Jacobi-PCG as l3k_pcg_solve runs it (residual_scaling rhs), for the statement that it does not solve a non-symmetric system:
    (converged, iterations, the true |b - A x| / |b|, x)"""
    T = dtype
    b, minv = np.asarray(b, dtype=T), np.asarray(minv, dtype=T)
    x = np.zeros_like(b)
    r = b.copy()
    z = minv * r
    p = z.copy()
    rz, scale = np.sum(r * z), np.sqrt(np.sum(b * b))
    it = 0
    with np.errstate(all="ignore"):
        while it < max_iters and not np.sqrt(np.sum(r * r)) / scale <= tol:
            ap = apply(p)
            alpha = rz / np.sum(p * ap)
            x, r = x + alpha * p, r - alpha * ap
            z = minv * r
            rz, old = np.sum(r * z), rz
            p = z + (rz / old) * p
            it += 1
        true = b - apply(x)
        res = float(np.sqrt(np.sum(true * true)) / scale)
    return bool(res <= tol), it, res, x


def tridiagonal(n, c):
    """(lo, di, up) of the whole chain: row i holds lo[i] at column i - 1, di[i], up[i] at column i + 1"""
    one = np.ones(n)
    lo, di, up = (-1 - c) * one, 2.5 + 0.5 * np.sin(np.arange(n)), (-1 + c) * one
    lo[0] = up[-1] = 0.0
    return lo, di, up


def tri_apply(lo, di, up):
    def apply(v):
        l, d, u = (a.astype(v.dtype) for a in (lo, di, up))
        y = d * v
        y[1:] += l[1:] * v[:-1]
        y[:-1] += u[:-1] * v[1:]
        return y
    return apply


def chain(n, c, n_owned):
    """The chain of n rows over len(n_owned) ranks that own n_owned[r] consecutive rows (0: a rank that owns nothing).  Returns a
    namespace: world, n, c, offsets, lo / di / up of the whole matrix, ranks[r] with n_owned, n_ghost, part (ExchangeLists, one dof per
    node), row_ptr / col_ind / values of the local matrix over [owned | ghost] (columns ascending), gid [n_local]."""
    assert sum(n_owned) == n and n >= 2
    world = len(n_owned)
    offsets = np.concatenate([[0], np.cumsum(n_owned)]).astype(np.int64)
    lo, di, up = tridiagonal(n, c)
    left = np.where(np.arange(n) == n - 1, 0.0, np.where(np.arange(n) == 0, 1.0, 0.5)) * di  # the share of d_i in link i
    right = di - left  # ... in link i - 1 (0.5 d_i + 0.5 d_i = d_i exactly)
    holders = [r for r in range(world) if n_owned[r] > 0]
    ranks = []
    for r in range(world):
        s, e = int(offsets[r]), int(offsets[r + 1])
        prev = max([q for q in holders if q < r], default=None) if e > s else None
        nxt = min([q for q in holders if q > r], default=None) if e > s else None
        no, ng = e - s, int(nxt is not None)
        rows, cols, vals = [], [], []
        for i in range(s, e):  # link i: rows i and i + 1 (local: i - s; row e is the ghost, local no)
            if i + 1 >= n:
                continue
            a, bq = i - s, i + 1 - s
            rows += [a, a, bq, bq]
            cols += [a, bq, a, bq]
            vals += [left[i], up[i], lo[i + 1], right[i + 1]]
        nl = no + ng
        dense = {}
        for i, j, v in zip(rows, cols, vals):
            dense[i, j] = dense.get((i, j), 0.0) + v
        keys = sorted(dense)
        row_ptr = np.zeros(nl + 1, dtype=np.int64)
        for i, _ in keys:
            row_ptr[i + 1] += 1
        row_ptr = np.cumsum(row_ptr)
        nbr, send, ranges = [], [], []
        if prev is not None:  # it holds a ghost copy of this rank's first row
            nbr.append(prev), send.append(np.array([0], dtype=np.int32)), ranges.append((0, 0))
        if nxt is not None:
            nbr.append(nxt), send.append(np.zeros(0, dtype=np.int32)), ranges.append((0, 1))
        ranks.append(types.SimpleNamespace(
            n_owned=no, n_ghost=ng, part=ExchangeLists(nbr, send, ranges), row_ptr=row_ptr,
            col_ind=np.array([j for _, j in keys], dtype=np.int32), values=np.array([dense[k] for k in keys], dtype=np.float64),
            gid=np.concatenate([np.arange(s, e), [e] if ng else []]).astype(np.int64)))
    return types.SimpleNamespace(world=world, n=n, c=c, offsets=offsets, lo=lo, di=di, up=up, ranks=ranks)


def summed_diagonals(case):
    """sum_r R_r^T A_r R_r of a chain as (lo, di, up, the number of stored entries off the three diagonals)"""
    lo, di, up, off = np.zeros(case.n), np.zeros(case.n), np.zeros(case.n), 0
    for k in case.ranks:
        for i in range(k.n_owned + k.n_ghost):
            for p in range(k.row_ptr[i], k.row_ptr[i + 1]):
                gi, gj, v = k.gid[i], k.gid[k.col_ind[p]], k.values[p]
                if gj == gi - 1:
                    lo[gi] += v
                elif gj == gi:
                    di[gi] += v
                elif gj == gi + 1:
                    up[gi] += v
                else:
                    off += 1
    return lo, di, up, off


def frozen_rows(case, rank=1, every=101, seed=11):
    """(live, x0, minv) of the frozen-row case on a chain: every `every`-th owned row of `rank` is frozen (minv = 0 there), x0 is
    random so that the frozen rows hold something to keep"""
    live = np.ones(case.n, dtype=bool)
    s, e = int(case.offsets[rank]), int(case.offsets[rank + 1])
    live[s:e] = np.arange(e - s) % every != 0
    return live, np.random.default_rng(seed).standard_normal(case.n), np.where(live, 1.0 / case.di, 0.0)


def choose_tol(history, near):
    """choose_tol of tests/test_gpu_gmres.py on a history: the geometric mean of the first two consecutive estimates from step `near`
    on that are a factor >= 2.25 apart (both stopping margins are then >= 1.5), or None if there is no such pair"""
    k = next((j for j in range(max(near, 1), len(history)) if history[j - 1] / history[j] >= 2.25), None)
    return None if k is None else float(np.sqrt(history[k - 1] * history[k]))
