"""l3k_tri_levels (include/l3k.h), the host half of the triangular preconditioners -- no context, no GPU -- on designed graphs,
held equal to the numpy restatement of tests/tri_ref.py."""
import ctypes as C

import numpy as np
import pytest

import tri_ref as R
from l3ster_amd import capi


def lib_levels(row_ptr, col_ind, upper):
    lib = capi.load()
    n = len(row_ptr) - 1
    row_ptr, col_ind = np.ascontiguousarray(row_ptr, dtype=np.int64), np.ascontiguousarray(col_ind, dtype=np.int32)
    level, n_levels = np.full(max(n, 1), -7, dtype=np.int32), C.c_int64(-1)
    capi.check(lib.l3k_tri_levels(n, row_ptr.ctypes.data_as(capi.c_int64_p), col_ind.ctypes.data_as(capi.c_int32_p), int(upper),
                                  level.ctypes.data_as(capi.c_int32_p), C.byref(n_levels)))
    return level[:n], n_levels.value


def independent_chains():
    """chains of lengths 1 .. 6 whose rows are interleaved: row r of chain c is c + 6 r; the 15 rows left over store their diagonal alone"""
    n = 36
    P = np.eye(n, dtype=bool)
    for c in range(6):
        for r in range(1, c + 1):
            P[c + 6 * r, c + 6 * (r - 1)] = P[c + 6 * (r - 1), c + 6 * r] = True
    return P


def with_empty_rows(P):
    P = P.copy()
    P[[0, 5, 6, 17, len(P) - 1]] = False  # (their columns stay stored in the other rows)
    return P


GRAPHS = {
    "chain": lambda: R.tridiagonal_pattern(100),
    "independent chains": independent_chains,
    "blocks of three": lambda: np.kron(np.eye(40, dtype=int), R.tridiagonal_pattern(3).astype(int)).astype(bool),
    "grid": lambda: R.grid(24)[1],
    "grid with empty rows": lambda: with_empty_rows(R.grid(9)[1]),
    "chain with empty rows": lambda: with_empty_rows(R.tridiagonal_pattern(30)),
    "lower only": lambda: np.tril(R.grid(7)[1]),
    "nothing stored": lambda: np.zeros((4, 4), dtype=bool),
}


@pytest.mark.parametrize("upper", [False, True])
@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_levels_equal_the_restatement(name, upper):
    P = GRAPHS[name]()
    row_ptr, col_ind, _ = R.to_csr(P, P)
    level, n_levels = lib_levels(row_ptr, col_ind, upper)
    ref, ref_n = R.levels(P, upper)
    assert np.array_equal(level, ref) and n_levels == ref_n
    assert ((level == 0) == ~R.active_rows(P)).all()


def test_designed_counts():
    for upper in (False, True):
        level, n_levels = lib_levels(*R.to_csr(*(GRAPHS["chain"](),) * 2)[:2], upper)
        assert n_levels == 100 and np.array_equal(level, np.arange(100, 0, -1) if upper else np.arange(1, 101))
        level, n_levels = lib_levels(*R.to_csr(*(GRAPHS["independent chains"](),) * 2)[:2], upper)
        assert n_levels == 6 and np.bincount(level).tolist() == [0, 6 + 15, 5, 4, 3, 2, 1]
        level, n_levels = lib_levels(*R.to_csr(*(GRAPHS["grid"](),) * 2)[:2], upper)
        assert n_levels == 47 and np.bincount(level)[1:].max() == 24
    level, n_levels = lib_levels(*R.to_csr(*(GRAPHS["lower only"](),) * 2)[:2], True)
    assert n_levels == 1 and (level == 1).all()
    # a row whose only neighbours below it are empty rows starts a chain
    P = with_empty_rows(R.tridiagonal_pattern(30))
    level, _ = lib_levels(*R.to_csr(P, P)[:2], False)
    assert level[1] == 1 and level[7] == 1 and level[18] == 1 and level[6] == 0 and level[16] == 10


def test_refusals():
    lib = capi.load()
    n_levels, level = C.c_int64(), np.zeros(4, dtype=np.int32)
    lp = level.ctypes.data_as(capi.c_int32_p)

    def call(row_ptr, col_ind, out=lp, nl=C.byref(n_levels)):
        rp, ci = np.asarray(row_ptr, dtype=np.int64), np.asarray(col_ind, dtype=np.int32)
        return lib.l3k_tri_levels(len(rp) - 1, rp.ctypes.data_as(capi.c_int64_p), ci.ctypes.data_as(capi.c_int32_p), 0, out, nl)

    for args, text in ((([0, 1, 2], [0, 1], lp, None), "l3k_tri_levels: null argument"),
                       (([0, 1, 2], [0, 1], None), "l3k_tri_levels: null argument"),
                       (([1, 1, 2], [0, 1]), "l3k_tri_levels: row_ptr[0] is not 0"),
                       (([0, 2, 1], [0, 1]), "l3k_tri_levels: row_ptr decreases at row 1"),
                       (([0, 2, 3], [1, 0, 1]), "l3k_tri_levels: the columns of row 0 are not strictly ascending inside [0, n)"),
                       (([0, 1, 2], [0, 2]), "l3k_tri_levels: the columns of row 1 are not strictly ascending inside [0, n)")):
        assert call(*args) == -1 and lib.l3k_last_error().decode() == text, lib.l3k_last_error().decode()
    assert call([0, 1, 2], [0, 1]) == 0 and n_levels.value == 1
