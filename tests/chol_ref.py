"""numpy restatement of the band Cholesky solver (l3k_chol_*): the rule of its reverse Cuthill-McKee ordering, the monotone block
envelope, and a block-envelope factorisation and solve.  Written from the rules stated in include/l3k.h, not from the library's
code: the tests demand identical permutations and heights from both."""
import numpy as np


def active_rows(row_ptr):
    return np.nonzero(np.diff(row_ptr) > 0)[0]


def first_unsymmetric_pair(n, row_ptr, col_ind):
    """The first stored (i, j), in row-major order, without a stored (j, i); None if the graph is structurally symmetric"""
    rows = [set(col_ind[row_ptr[i]:row_ptr[i + 1]].tolist()) for i in range(n)]
    for i in range(n):
        for j in col_ind[row_ptr[i]:row_ptr[i + 1]].tolist():
            if i not in rows[j]:
                return i, j
    return None


def _levels(adj, root, numbered):
    seen = {root}
    levels = [[root]]
    while True:
        nxt = []
        for v in levels[-1]:
            for w in adj[v]:
                if w not in seen and not numbered[w]:
                    seen.add(w)
                    nxt.append(w)
        if not nxt:
            return levels
        levels.append(nxt)


def rcm(n, row_ptr, col_ind):
    """perm (perm[new] = old) over the active rows: Cuthill-McKee component by component in ascending order of the components'
    lowest rows, each from a pseudo-peripheral node, neighbours by ascending (degree, index); the whole order reversed"""
    adj = [[int(j) for j in col_ind[row_ptr[i]:row_ptr[i + 1]] if j != i] for i in range(n)]
    deg = [len(a) for a in adj]
    key = lambda v: (deg[v], v)
    numbered = [False] * n
    order = []
    for s in range(n):
        if numbered[s] or row_ptr[s + 1] == row_ptr[s]:
            continue
        r = s
        lv = _levels(adj, r, numbered)
        while True:
            c = min(lv[-1], key=key)
            if c == r:
                break
            lv2 = _levels(adj, c, numbered)
            if len(lv2) <= len(lv):
                break
            r, lv = c, lv2
        head = len(order)
        order.append(r)
        numbered[r] = True
        while head < len(order):
            v = order[head]
            head += 1
            for w in sorted((w for w in adj[v] if not numbered[w]), key=key):
                numbered[w] = True
                order.append(w)
    return np.array(order[::-1], dtype=np.int32)


def choose_block(n, row_ptr, col_ind, perm):
    inv = inverse(n, perm)
    rows = np.repeat(np.arange(n), np.diff(row_ptr))
    reach = int(np.max(inv[rows] - inv[col_ind])) if len(col_ind) else 0
    return 64 if reach >= 64 else 32


def inverse(n, perm):
    inv = np.full(n, -1, dtype=np.int64)
    inv[perm] = np.arange(len(perm))
    return inv


def envelope(n, row_ptr, col_ind, perm, nb):
    """H(K) of the ceil(n_active / nb) block columns: the smallest heights that hold the permuted lower triangle with K + H(K)
    non-decreasing"""
    inv = inverse(n, perm)
    nblk = (len(perm) + nb - 1) // nb
    raw = np.zeros(nblk, dtype=np.int64)
    rows = np.repeat(np.arange(n), np.diff(row_ptr))
    bi, bj = inv[rows] // nb, inv[col_ind] // nb
    low = bi > bj
    np.maximum.at(raw, bj[low], (bi - bj)[low])
    end = np.maximum.accumulate(np.arange(nblk) + raw) if nblk else raw
    return (end - np.arange(nblk)).astype(np.int32)


def symbolic(n, row_ptr, col_ind, block=0):
    """(perm, heights, nb, factor bytes) as l3k_chol_order returns them"""
    perm = rcm(n, row_ptr, col_ind)
    nb = block or choose_block(n, row_ptr, col_ind, perm)
    h = envelope(n, row_ptr, col_ind, perm, nb)
    return perm, h, nb, int((len(h) + h.sum()) * nb * nb * 8)


def in_envelope(heights, nb, pi, pj):
    """Is the entry (pi, pj), pi >= pj, of the permuted matrix inside the block envelope?"""
    return pi // nb - pj // nb <= heights[pj // nb]


def envelope_mask(heights, nb):
    """Boolean [m, m] (m = blocks * nb): the lower-triangle entries the storage holds"""
    nblk = len(heights)
    m = nblk * nb
    mask = np.zeros((m, m), dtype=bool)
    for k in range(nblk):
        mask[k * nb:(k + 1 + heights[k]) * nb, k * nb:(k + 1) * nb] = True
    return mask & np.tril(np.ones((m, m), dtype=bool))


def block_cholesky(Ap, heights, nb):
    """Right-looking block Cholesky of the dense symmetric positive definite Ap [m, m] (already permuted and padded with identity to
    m = blocks * nb) that touches only blocks inside the envelope; returns the dense lower factor, exactly 0 outside the envelope"""
    nblk = len(heights)
    L = np.tril(Ap).astype(np.float64) * envelope_mask(heights, nb)
    blk = lambda i, j: (slice(i * nb, (i + 1) * nb), slice(j * nb, (j + 1) * nb))
    for k in range(nblk):
        h = int(heights[k])
        Lkk = np.linalg.cholesky(np.tril(L[blk(k, k)]) + np.tril(L[blk(k, k)], -1).T)
        L[blk(k, k)] = Lkk
        for i in range(k + 1, k + h + 1):
            L[blk(i, k)] = np.linalg.solve(Lkk, L[blk(i, k)].T).T
        for j in range(k + 1, k + h + 1):
            for i in range(j, k + h + 1):
                upd = L[blk(i, k)] @ L[blk(j, k)].T
                L[blk(i, j)] -= np.tril(upd) if i == j else upd
    return L


def solve(n, row_ptr, col_ind, values, b, x0, block=0):
    """x with A x = b on the active rows and x0 elsewhere, by the block-envelope factorisation of the ordered matrix"""
    perm, h, nb, _ = symbolic(n, row_ptr, col_ind, block)
    m = len(h) * nb
    A = np.zeros((n, n))
    rows = np.repeat(np.arange(n), np.diff(row_ptr))
    A[rows, col_ind] = values
    Ap = np.eye(m)
    Ap[:len(perm), :len(perm)] = A[np.ix_(perm, perm)]
    L = block_cholesky(Ap, h, nb)
    w = np.zeros(m)
    w[:len(perm)] = b[perm]
    w = np.linalg.solve(L.T, np.linalg.solve(L, w))
    x = np.array(x0, dtype=np.float64)
    x[perm] = w[:len(perm)]
    return x


def csr_from_dense(A, pattern=None):
    """(row_ptr int64, col_ind int32, values) of the entries of A where pattern (default: A != 0) is set"""
    pattern = (A != 0) if pattern is None else pattern
    n = A.shape[0]
    row_ptr = np.zeros(n + 1, dtype=np.int64)
    row_ptr[1:] = np.cumsum(pattern.sum(axis=1))
    r, c = np.nonzero(pattern)
    return row_ptr, c.astype(np.int32), A[r, c].astype(np.float64)
