"""Pins tests/csr_dist_ref.py: the synthetic partitioned systems are valid (graphs, exchange lists), the restatements of the
distributed apply, diagonal and Dirichlet step agree with the dense definitions on small cases (the dense sum of the ranks'
matrices, asm_dist_ref.dirichlet_owner_rule, asm_dist_ref.row_classes), and the full-size case has the structure
tests/test_gpu_csr_dist_kernels.py relies on: lists longer than a launch has row groups, several tiles per block of the
compaction, every row length in every class, the empty and ghost-only rows, class changes at tile and chunk boundaries.
No GPU, no libl3k."""
import numpy as np
import pytest

import asm_dist_ref as AD
import csr_dist_ref as D
import csr_ref as R
from cg_ref import EPS, LD

LD_NOISE = 64 * 2.0 ** -64
_SMALL = {}


def small_case():
    if not _SMALL:
        _SMALL["case"] = D.split_case(2, [dict(n_owned=90, n_border=30, ghosts={1: 25}, pin={3: D.BORDER, 4: D.INTERIOR}),
                                          dict(n_owned=70, n_border=20, ghosts={0: 20})], seed=3)
    return _SMALL["case"]


CASES = [small_case, D.tiny_case]
ALL_CASES = CASES + [D.full_case]


def dense_local(k, values):
    return AD.dense_of(k.row_ptr, k.col_ind, values, k.n_owned + k.n_ghost)


def dense_sum(case, of):
    """sum_r R_r^T of(rank r) R_r over the global dofs, in longdouble (two ranks may store the same entry)"""
    A = np.zeros((case.n_global, case.n_global), dtype=LD)
    for k in case.ranks:
        A[np.ix_(k.gid, k.gid)] += of(k)
    return A


# ------------------------------------------------------------------------------------------------------------ the cases
@pytest.mark.parametrize("make", ALL_CASES)
def test_graphs_and_exchange_lists_are_valid(make):
    case = make()
    for r, k in enumerate(case.ranks):
        n = k.n_owned + k.n_ghost
        assert k.row_ptr.dtype == np.int64 and k.col_ind.dtype == np.int32 and k.row_ptr.size == n + 1
        assert k.row_ptr[0] == 0 and np.array_equal(np.diff(k.row_ptr), k.lens) and k.row_ptr[-1] == k.col_ind.size
        assert k.col_ind.min() >= 0 and k.col_ind.max() < n
        inner = np.ones(k.col_ind.size, dtype=bool)
        inner[k.row_ptr[:-1][k.lens > 0]] = False  # the first entry of a row has no predecessor in it
        assert (np.diff(k.col_ind.astype(np.int64))[inner[1:]] > 0).all()  # strictly ascending within a row
        for v in (k.ints, k.reals):
            assert v.dtype == np.float64 and v.size == k.col_ind.size
        assert np.array_equal(k.ints, np.round(k.ints)) and np.abs(k.ints).max() == 8
        # the exchange lists: no rank is its own neighbour, the ranges tile the ghosts in neighbour order, and what a neighbour
        # sends is, entry by entry, what this rank's range of ghosts are copies of
        p = k.part
        assert r not in p.nbr_rank and len(set(p.nbr_rank)) == len(p.nbr_rank) == len(p.send_nodes) == len(p.ghost_ranges)
        cursor = 0
        for q, (g0, g1) in zip(p.nbr_rank, p.ghost_ranges):
            assert g0 == cursor and g1 >= g0
            cursor = g1
            assert (k.ghost_owner[g0:g1] == q).all()
            back = case.ranks[q].part
            assert np.array_equal(back.send_nodes[back.nbr_rank.index(r)], k.ghost_index[g0:g1])
        assert cursor == k.n_ghost
        for q, send in zip(p.nbr_rank, p.send_nodes):
            assert send.dtype == np.int32 and (send.size == 0 or (send.min() >= 0 and send.max() < k.n_owned))
            assert np.unique(send).size == send.size  # every ghost dof is a distinct owned dof of its owner
        assert np.unique(k.gid).size == n
        assert np.array_equal(k.gid[:k.n_owned], case.offsets[r] + np.arange(k.n_owned))


@pytest.mark.parametrize("make", ALL_CASES)
def test_row_classes_are_the_chosen_ones(make):
    for k in make().ranks:
        interior, border, ghost = D.row_classes(k)
        assert np.array_equal(interior, np.flatnonzero(k.cls == D.INTERIOR)) and np.array_equal(border, np.flatnonzero(k.cls == D.BORDER))
        assert np.array_equal(ghost, np.arange(k.n_owned, k.n_owned + k.n_ghost))
        last = k.col_ind[np.maximum(k.row_ptr[1:] - 1, 0)]  # the device's rule: the last column decides
        assert np.array_equal(border, np.flatnonzero((k.lens[:k.n_owned] > 0) & (last[:k.n_owned] >= k.n_owned)))


def test_chunk_is_the_compactions():
    assert [D.chunk_of(n) for n in (1, 256, 257, 262_144, 262_145, 524_288, 524_289)] == [256, 256, 256, 256, 512, 512, 768]


# ------------------------------------------------------------------------------------------- restatements against dense
@pytest.mark.parametrize("make", CASES)
@pytest.mark.parametrize("values", ["ints", "reals"])
@pytest.mark.parametrize("alpha,beta,ncols", [(1.0, 0.0, 1), (-0.5, 2.0, 3)])
def test_apply_dist_ref_vs_the_dense_sum_of_ranks(make, values, alpha, beta, ncols):
    case = make()
    rng = np.random.default_rng(17)
    x = [rng.standard_normal((ncols, k.n_owned + 7)) for k in case.ranks]  # (padded: only the owned rows are read)
    y0 = [rng.standard_normal((ncols, k.n_owned + 13)) for k in case.ranks]
    out = D.apply_dist_ref(case, x, alpha, beta, y0, values)
    A = dense_sum(case, lambda k: dense_local(k, getattr(k, values)))
    absA = dense_sum(case, lambda k: np.abs(dense_local(k, getattr(k, values))))
    count = dense_sum(case, lambda k: dense_local(k, np.ones(k.col_ind.size))).sum(axis=1)
    xg = np.concatenate([v[:, :k.n_owned] for v, k in zip(x, case.ranks)], axis=1)
    yg = np.concatenate([v[:, :k.n_owned] for v, k in zip(y0, case.ranks)], axis=1)
    want = LD(alpha) * (A @ xg.astype(LD).T).T + LD(beta) * yg.astype(LD)
    want_abs = abs(alpha) * (absA @ np.abs(xg).T).T + np.abs(beta * yg)
    for r, (k, (y, absy, n_terms)) in enumerate(zip(case.ranks, out)):
        assert y.dtype == LD and y.shape == (ncols, k.n_owned)
        assert np.abs(y - D.owned(case, r, want)).max() <= LD_NOISE * max(1.0, float(absy.max()))
        assert np.allclose(np.asarray(absy, dtype=np.float64), np.asarray(D.owned(case, r, want_abs), dtype=np.float64), rtol=1e-13, atol=0)
        assert np.array_equal(n_terms, np.asarray(D.owned(case, r, count), dtype=np.int64))  # the ghost copies' entries are counted
        # a float64 evaluation in another order (columns backwards, the sharers' rows added one after the other) is inside the bound
        bound = D.row_bound_dist(n_terms, k.n_exports, absy)
        got = np.zeros((ncols, k.n_owned))
        got += alpha * (dense_local(k, getattr(k, values))[:k.n_owned, ::-1] @ D.local_vector(case, r, x)[:, ::-1].T).T
        if beta != 0.0:
            got += beta * y0[r][:, :k.n_owned]
        for q, kq in enumerate(case.ranks):
            mine = np.flatnonzero(kq.ghost_owner == r)
            if mine.size:
                share = alpha * (dense_local(kq, getattr(kq, values))[kq.n_owned + mine][:, ::-1] @ D.local_vector(case, q, x)[:, ::-1].T).T
                got[:, kq.ghost_index[mine]] += share
        assert (np.abs(got.astype(LD) - y) <= bound).all()
    assert sum(int(k.n_exports.sum()) for k in case.ranks) == sum(k.n_ghost for k in case.ranks)


def test_row_bound_dist_hand_values():
    assert D.row_bound_dist([5], [2], [1.0])[0] == 10 * EPS and D.row_bound_dist([0], [0], [3.0])[0] == 3 * EPS * 3.0
    assert np.array_equal(D.row_bound_dist([7, 1000], [0, 0], [2.0, 1.0]), R.row_bound([7, 1000], [2.0, 1.0]))  # no sharer: row_bound


@pytest.mark.parametrize("make", CASES)
@pytest.mark.parametrize("damping,threshold", [(1.0, 0.0), (0.8, 1e-3)])
def test_diag_dist_ref_vs_the_dense_sum_of_ranks(make, damping, threshold):
    case = make()
    diag = np.diag(dense_sum(case, lambda k: dense_local(k, k.reals)))
    absd = np.diag(dense_sum(case, lambda k: np.abs(dense_local(k, k.reals))))
    for r, (k, d) in enumerate(zip(case.ranks, D.diag_dist_ref(case, damping, threshold))):
        assert np.abs(d.diag - D.owned(case, r, diag)).max() <= LD_NOISE * max(1.0, float(d.abs.max()))
        assert np.allclose(np.asarray(d.abs, dtype=np.float64), np.asarray(D.owned(case, r, absd), dtype=np.float64), rtol=1e-14, atol=0)
        exact = d.n_contrib <= 1
        assert exact.any() and (~exact).any() and np.array_equal(d.diag[exact], D.owned(case, r, diag)[exact])
        for i in range(k.n_owned):
            if k.lens[i] == 0:
                assert d.minv[i] == 0.0  # frozen, whatever the neighbours contribute
            else:
                v = np.float64(d.diag[i])
                with np.errstate(divide="ignore"):
                    assert d.minv[i] == (-damping if v < 0 else damping) / np.float64(max(abs(v), threshold))


@pytest.mark.parametrize("make", CASES)
@pytest.mark.parametrize("ncols", [1, 3])
def test_dirichlet_owner_ref_vs_the_dense_owner_rule(make, ncols):
    for k in make().ranks:
        n = k.n_owned + k.n_ghost
        A = dense_local(k, k.reals)
        stored = dense_local(k, np.ones(k.col_ind.size)) > 0
        rng = np.random.default_rng(23)
        mask = (rng.random(n) < 0.3) & (np.diag(stored) | (np.arange(n) >= k.n_owned))
        assert mask[:k.n_owned].any() and (mask[k.n_owned:] & ~np.diag(stored)[k.n_owned:]).any() and (~mask).any()
        g, rhs = rng.standard_normal((ncols, n)), rng.standard_normal((ncols, n))
        new, out, absv = D.dirichlet_owner_ref(k.row_ptr, k.col_ind, k.reals, mask.astype(np.uint8), g, rhs, k.n_owned)
        A2, rhs2 = AD.dirichlet_owner_rule(A, rhs, mask, g, k.n_owned)
        assert np.array_equal(dense_local(k, new), A2)
        assert set(np.unique(new)) <= set(np.unique(k.reals)) | {0.0, 1.0}
        assert out.dtype == LD and (np.abs(out - rhs2.astype(LD)) <= R.row_bound(np.broadcast_to(k.lens, out.shape), absv)).all()
        assert np.array_equal(out[:, mask].astype(np.float64), rhs2[:, mask]) and not absv[:, mask].any()
        assert not out[:, np.flatnonzero(mask[k.n_owned:]) + k.n_owned].any()  # a flagged ghost row: rhs 0
        free = np.flatnonzero(~mask)
        want_abs = np.abs(rhs[:, free]) + (np.abs(A[np.ix_(free, np.flatnonzero(mask))]) @ np.abs(g[:, mask]).T).T
        assert np.allclose(np.asarray(absv[:, free], dtype=np.float64), want_abs, rtol=1e-13, atol=0)
        # the refusal names the smallest flagged owned row without a stored diagonal; a ghost row needs none
        bad = np.flatnonzero(~np.diag(stored)[:k.n_owned])
        if bad.size >= 2:
            mk = mask.copy()
            mk[bad[-1]] = mk[bad[1]] = True
            with pytest.raises(ValueError, match=f"owned Dirichlet row {bad[1]} has no stored diagonal"):
                D.dirichlet_owner_ref(k.row_ptr, k.col_ind, k.reals, mk, g, rhs, k.n_owned)


# ----------------------------------------------------------------------------------------- the structure of the full-size case
GROUPS_AT_4_LANES = D.MAX_BLOCKS * D.BLOCK // 4  # 65 536: the most row groups a launch has
THREADS_OF_A_LAUNCH = D.MAX_BLOCKS * D.BLOCK  # 262 144


def test_full_case_runs_every_loop_more_than_once():
    case = D.full_case()
    assert case.world == 2
    k = case.ranks[0]
    interior, border, ghost = D.row_classes(k)
    ni = interior.size
    assert min(ni // 2, ni - ni // 2, border.size, ghost.size) > GROUPS_AT_4_LANES  # (the apply splits the interior list at ni / 2)
    n = k.n_owned + k.n_ghost
    chunk = D.chunk_of(n)
    assert n > THREADS_OF_A_LAUNCH and chunk > D.BLOCK and (n + chunk - 1) // chunk > 2  # several tiles per block, many blocks
    assert k.n_owned > THREADS_OF_A_LAUNCH  # the one-thread-per-owned-row kernels (minv, the Dirichlet check) stride too
    assert n % chunk != 0 and n % D.BLOCK != 0  # the last block and its last tile are partial
    k1 = case.ranks[1]
    assert k1.n_owned >= k.n_ghost and k1.n_ghost >= 2000 and all(x.size > 0 for x in D.row_classes(k1))


def test_full_case_has_every_row_length_in_every_class():
    k = D.full_case().ranks[0]
    assert abs(k.lens.mean() - 8.0) < 1.5
    for name, rows in zip(("interior", "border", "ghost"), D.row_classes(k)):
        for L in D.LENGTHS:
            assert (k.lens[rows] == L).any() or (name == "border" and L == 0), (name, L)  # (an empty owned row is interior)


def test_full_case_row_class_edges():
    case = D.full_case()
    k = case.ranks[0]
    no, n = k.n_owned, k.n_owned + k.n_ghost
    interior, border, ghost = D.row_classes(k)
    first_col = k.col_ind[np.minimum(k.row_ptr[:-1], k.col_ind.size - 1)]
    ghost_only = border[first_col[border] >= no]
    assert (k.lens[interior] == 0).sum() > 1000 and (k.lens[ghost] == 0).sum() > 1000 and ghost_only.size > 1000
    assert (k.lens[ghost_only] > 1).any()
    cls = np.full(n, D.GHOST)
    cls[interior], cls[border] = D.INTERIOR, D.BORDER
    chunk = D.chunk_of(n)
    assert cls[255] != cls[256] and cls[256] != cls[257]  # at a tile boundary, either side
    assert cls[chunk - 1] != cls[chunk] and cls[chunk + D.BLOCK - 1] != cls[chunk + D.BLOCK]  # at a chunk boundary and at the tile boundary inside a chunk
    assert no % chunk == 0 and cls[no - 1] == D.BORDER  # owned / ghost changes at a chunk boundary
    assert cls[n - 1] == D.GHOST and k.lens[n - 1] > 0  # the last local row: the list entry that "names itself again"
    # empty owned rows whose ghost copy on the other rank stores a diagonal (the frozen-row rule), both ways
    for r, q in ((0, 1), (1, 0)):
        kr, kq = case.ranks[r], case.ranks[q]
        dq = R.diag_ref(kq.row_ptr, kq.col_ind, kq.reals)[0][kq.n_owned:]
        assert ((kr.lens[kq.ghost_index] == 0) & (dq != 0)).sum() > 10
    # rows that receive an export and rows that do not, on both ranks
    assert all((kr.n_exports == 1).any() and (kr.n_exports == 0).any() for kr in case.ranks)


def test_tiny_case_has_the_empty_lists_and_two_exporters():
    case = D.tiny_case()
    assert case.world == 3 and sum(k.n_owned + k.n_ghost for k in case.ranks) < 1000
    sizes = [[x.size for x in D.row_classes(k)] for k in case.ranks]
    assert any(s[0] == 0 and s[1] > 0 for s in sizes)  # a rank without interior rows
    assert any(s[1] == 0 and s[2] > 0 for s in sizes)  # a rank with ghost rows and no border rows
    assert all(s[2] > 0 for s in sizes)
    assert any((k.n_exports == 2).any() for k in case.ranks)  # an owned row with two exporters
    assert any(g0 == g1 for k in case.ranks for g0, g1 in k.part.ghost_ranges)  # a neighbour that only receives
