"""Restarted GMRES(m) as l3k_gmres_solve runs it (include/l3k.h), restated in numpy: right preconditioning, classical Gram-Schmidt
with one re-orthogonalisation, Givens rotations, the same stopping rules and counters.  dtype = np.float64 or np.longdouble; the
operator and the preconditioner are callables on whole vectors, `live` is the boolean mask of the rows the iteration may change
(None: all).  check_every is 1 here: the device never stops earlier than this restatement, and at most check_every - 1 steps later."""
import numpy as np

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)


def gmres(apply, b, x0, m, prec=None, live=None, tol=1e-6, max_iters=10_000, residual_scaling=0, max_restarts=39, dtype=np.float64):
    """Returns a dict: x, iterations, restarts, converged, breakdown, achieved_tol, estimate, orth_loss, and `history`, the
    estimate after every Arnoldi step (scaled as tol)."""
    T = dtype
    b = np.asarray(b, dtype=T)
    x = np.array(x0, dtype=T)
    n = b.size
    live = np.ones(n, dtype=bool) if live is None else np.asarray(live, dtype=bool)
    prec = prec or (lambda v: v)
    zero = T(0)
    it, cycles, breakdown, orth_loss, scale, est = 0, 0, False, 0.0, T(1), None
    history = []
    while True:
        r = np.where(live, b - apply(x), zero)
        beta = np.sqrt(np.sum(r * r))
        if cycles == 0:
            if residual_scaling == 1:
                scale = beta if beta > 0 else T(1)
            elif residual_scaling == 2:
                bb = np.sqrt(np.sum(b * b))
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
            h1 = Vk @ w
            w = w - h1 @ Vk
            h2 = Vk @ w
            w = w - h2 @ Vk
            t, nu = Vk @ w, np.sqrt(np.sum(w * w))
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


def stopping_margin(history, tol):
    """(tol / estimate at the first step whose estimate is <= tol, the estimate of the step before / tol): both must be >= 1.5 for
    an iteration count to be held to +-1 honestly.  `history` must come from a run with that tol, of ONE cycle or of several: the
    step before is the one before in the same list"""
    k = next(i for i, e in enumerate(history) if e <= tol)
    return tol / max(history[k], 1e-300), (history[k - 1] / tol if k else float("inf"))
