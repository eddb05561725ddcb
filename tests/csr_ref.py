"""Plain numpy restatements of the device CSR operator (include/l3k.h, "device CSR operator"): what l3k_csr_apply,
l3k_csr_diag and l3k_csr_dirichlet compute, with the sums in numpy.longdouble (cg_ref.LD), and the row-wise error bound the
device results are held to.  No GPU, no libl3k.  tests/test_csr_ref_cpu.py pins these helpers against the dense definitions,
tests/test_gpu_csr_apply.py and tests/test_gpu_csr_solve.py compare the device with them.

The format is that of l3k_assembled_scatter: row_ptr int64 [n + 1], col_ind int32 strictly ascending within a row, values."""
import numpy as np

from cg_ref import EPS, LD


def row_of_entry(row_ptr):
    """the row of every stored entry"""
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    return np.repeat(np.arange(row_ptr.size - 1, dtype=np.int64), np.diff(row_ptr))


def row_sums(row_ptr, terms):
    """sum of `terms` (one per stored entry, any dtype) over each row; 0 on an empty row"""
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    out = np.zeros(row_ptr.size - 1, dtype=terms.dtype)
    live = np.flatnonzero(np.diff(row_ptr) > 0)
    if live.size:  # (reduceat sums from one start to the next: the starts of the non-empty rows partition the entries)
        out[live] = np.add.reduceat(terms, row_ptr[live])
    return out


def apply_ref(row_ptr, col_ind, values, x):
    """(A x, sum_j |a_ij x_j|) per row, in longdouble"""
    prod = np.asarray(values, dtype=np.float64).astype(LD) * np.asarray(x, dtype=np.float64).astype(LD)[np.asarray(col_ind)]
    return row_sums(row_ptr, prod), row_sums(row_ptr, np.abs(prod))


def row_bound(lens, abs_terms):
    """The first-order bound of a float64 sum of len_i products in ANY order, plus the scaling and the update of y:
    (len_i + 3) EPS * (sum of the absolute values of what is added in row i).  Derived, not measured: every partial sum of m
    terms carries at most m - 1 roundings of relative size EPS / 2, each product one more, alpha * and + beta y two more."""
    return (np.asarray(lens, dtype=np.float64) + 3.0) * EPS * np.asarray(abs_terms, dtype=np.float64)


def diag_ref(row_ptr, col_ind, values, damping=1.0, threshold=0.0):
    """l3k_csr_diag: (diag, minv) in float64.  diag_i = a_ii, 0 where the row stores none; minv_i = sign(a_ii) damping /
    max(|a_ii|, threshold) with sign(0) = +1 (one correctly rounded division: the float64 quotient IS the reference, as in
    cg_ref.jacobi_inverse_ref) on every non-empty row, 0 on an empty one."""
    row_ptr, col_ind = np.asarray(row_ptr, dtype=np.int64), np.asarray(col_ind, dtype=np.int64)
    n = row_ptr.size - 1
    rows = row_of_entry(row_ptr)
    diag = np.zeros(n)
    on = col_ind == rows
    diag[rows[on]] = np.asarray(values, dtype=np.float64)[on]
    a = np.abs(diag)
    with np.errstate(divide="ignore"):
        minv = np.where(diag < 0, -np.float64(damping), np.float64(damping)) / np.where(a > threshold, a, np.float64(threshold))
    return diag, np.where(np.diff(row_ptr) > 0, minv, 0.0)


def dirichlet_ref(row_ptr, col_ind, values, mask, g, rhs):
    """l3k_csr_dirichlet (DirichletBCAlgebraic::apply): g, rhs [ncols, n].  Returns (values', rhs' in longdouble, abs) with
    abs[c, i] = |rhs_i| + sum over the masked columns j of |a_ij g_j| on the free rows (what the row-wise bound multiplies)
    and 0 on the masked ones, whose rhs is a copy.  values' holds the old entries, zeros and ones only.  ValueError if a
    masked row stores no diagonal entry."""
    row_ptr, col_ind = np.asarray(row_ptr, dtype=np.int64), np.asarray(col_ind, dtype=np.int64)
    values, mask = np.asarray(values, dtype=np.float64), np.asarray(mask).astype(bool)
    g, rhs = np.atleast_2d(np.asarray(g, dtype=np.float64)), np.atleast_2d(np.asarray(rhs, dtype=np.float64))
    rows = row_of_entry(row_ptr)
    has_diag = np.zeros(mask.size, dtype=bool)
    has_diag[rows[col_ind == rows]] = True
    if (mask & ~has_diag).any():
        raise ValueError(f"Dirichlet row {int(np.flatnonzero(mask & ~has_diag)[0])} has no stored diagonal entry")
    in_masked_row, in_masked_col = mask[rows], mask[col_ind]
    new = np.where(in_masked_row, (col_ind == rows).astype(np.float64), np.where(in_masked_col, 0.0, values))
    out, absv = np.empty(rhs.shape, dtype=LD), np.empty(rhs.shape, dtype=LD)
    lift = ~in_masked_row & in_masked_col
    for c in range(rhs.shape[0]):
        prod = np.where(lift, values.astype(LD) * g[c].astype(LD)[col_ind], LD(0))
        out[c] = np.where(mask, g[c].astype(LD), rhs[c].astype(LD) - row_sums(row_ptr, prod))
        absv[c] = np.where(mask, LD(0), np.abs(rhs[c]).astype(LD) + row_sums(row_ptr, np.abs(prod)))
    return new, out, absv


def strided_graph(n, lens, no_diag_every=3):
    """A CSR graph with the given row lengths whose rows are arithmetic progressions of columns (strictly ascending, inside
    [0, n)) drawn deterministically from the row index.  A non-empty row i holds its diagonal unless i % no_diag_every == 1,
    where the diagonal's place is taken by a neighbouring column.  Returns (row_ptr int64, col_ind int32)."""
    lens = np.asarray(lens, dtype=np.int64)
    assert lens.size == n and lens.max() <= n // 4
    i = np.arange(n, dtype=np.int64)
    # the diagonal sits at position k of the row, in proportion to where the row sits in the matrix
    k = np.where(lens > 1, (i * np.maximum(lens - 1, 0)) // max(n - 1, 1), 0)
    big = np.int64(n)
    room = np.minimum(np.where(k > 0, i // np.maximum(k, 1), big), np.where(k < lens - 1, (n - 1 - i) // np.maximum(lens - 1 - k, 1), big))
    h = (i * 2654435761 + 12345) % 1000003  # a fixed scramble of the row index
    stride = 2 + h % np.maximum(np.minimum(room, 97) - 1, 1)
    stride = np.where(room >= 2, np.minimum(stride, room), 1)
    row_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    rows = np.repeat(i, lens)
    pos = np.arange(row_ptr[-1], dtype=np.int64) - row_ptr[rows]
    cols = i[rows] + (pos - k[rows]) * stride[rows]
    moved = (pos == k[rows]) & (rows % no_diag_every == 1) & (stride[rows] >= 2)
    cols = np.where(moved, np.where(rows + 1 < n, cols + 1, cols - 1), cols)
    assert cols.min() >= 0 and cols.max() < n
    return row_ptr, cols.astype(np.int32)
