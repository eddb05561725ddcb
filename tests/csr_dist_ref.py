"""Synthetic partitioned systems in the sub-assembled form A = sum_r R_r^T A_r R_r and plain numpy restatements of
what the distributed CSR operator computes on them (include/l3k.h: l3k_csr_dist_*, l3k_csr_dirichlet_dist), with the sums in
numpy.longdouble, and the row-wise error bound the device results are held to.  No GPU, no libl3k.  Built on tests/csr_ref.py (the
single-rank restatements and strided_graph) and tests/asm_dist_ref.py (row_classes, dirichlet_owner_rule);
tests/test_csr_dist_ref_cpu.py pins these helpers against dense definitions and asserts the structure of the two cases,
tests/test_gpu_csr_dist_kernels.py compares the device with them.

A case is a list of ranks.  Rank r owns the dofs [0, n_owned) of its local numbering [owned | ghost]; a ghost dof is a copy of an
owned dof of another rank.  The local matrix A_r is any CSR matrix over the local dofs -- nothing here is a mesh: the test chooses
the class of every owned row (interior: every column owned; border: some ghost column), the row lengths and where the classes
change."""
import types

import numpy as np

import asm_dist_ref as AD
import csr_ref as R
from cg_ref import EPS, LD

LENGTHS = np.array([0, 1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 200, 1000])  # (those of tests/test_gpu_csr_apply.py)
WEIGHTS = np.array([6, 8, 8, 8, 8, 4, 4, 4, 0.5, 0.5, 0.5, 0.1, 0.02])  # mean length 8.4
INTERIOR, BORDER, GHOST = 0, 1, 2
BLOCK, MAX_BLOCKS = 256, 1024  # threads of a block and the cap on the blocks of a launch (cg_threads, cg_blocks)


def chunk_of(n):
    """rows per block of the ordered compaction, as buildRowLists (csrc/api_csr_dist.hip) computes it: the rows are dealt to at most
    MAX_BLOCKS blocks in chunks that are a multiple of BLOCK"""
    per = (n + MAX_BLOCKS - 1) // MAX_BLOCKS
    return (per + BLOCK - 1) // BLOCK * BLOCK


class ExchangeLists:
    """what distributed.NativeHalo reads of a partition: nbr_rank, send_nodes (per neighbour: the owned dofs it holds copies of, in
    the order of its ghost range), ghost_ranges (per neighbour: its slice of this rank's ghosts; contiguous in neighbour order)"""

    def __init__(self, nbr_rank, send_nodes, ghost_ranges):
        self.nbr_rank, self.send_nodes, self.ghost_ranges = nbr_rank, send_nodes, ghost_ranges


def _draw_lengths(rng, count, cap, allow_empty):
    ok = (LENGTHS <= cap) & (allow_empty | (LENGTHS > 0))
    return rng.choice(LENGTHS[ok], size=count, p=WEIGHTS[ok] / WEIGHTS[ok].sum()), LENGTHS[ok]


def _scramble(i, salt):
    return (np.asarray(i, dtype=np.int64) * 2654435761 + salt) % 1000003


def split_case(world, sizes, seed):
    """A synthetic partitioned system.  sizes[r]: dict(n_owned, n_border, ghosts={owner rank: count}, pin={owned row: class}) -- rank r
    owns n_owned dofs of which n_border rows are border rows, and holds `count` ghost copies of distinct owned dofs of every listed
    owner; `pin` fixes the class of single owned rows ahead of the draw.  Returns a namespace with world, offsets (the first global
    dof of every rank, rank-major) and ranks[r]: n_owned, n_ghost, ghost_owner / ghost_index [n_ghost] (the owner of every ghost and
    its index there), part (ExchangeLists, dofs_per_node = 1), row_ptr / col_ind (columns strictly ascending), ints (integers in
    [-8, 8]) / reals (standard normal) for that graph, lens, gid [n_local] (the global dof of every local dof).

    Owned rows: strided_graph(n_owned, .) gives the owned columns; a border row gets ascending ghost columns appended (about one
    border row in seven has ghost columns ONLY).  Ghost rows: strided_graph(n_local, .) over all local dofs.  Every length that fits
    is planted once in the first rows of every class; the last local row is a non-empty ghost row.  No rank is its own neighbour."""
    rng = np.random.default_rng(seed)
    n_owned = [int(s["n_owned"]) for s in sizes]
    ranks = [types.SimpleNamespace(n_owned=n_owned[r]) for r in range(world)]
    # ---- ghosts: distinct owned dofs of their owners, in neighbour (= owner) order, in a drawn order within an owner
    for r, s in enumerate(sizes):
        owners = sorted(s.get("ghosts", {}))
        assert r not in owners and all(0 <= q < world for q in owners)
        picks = [rng.choice(n_owned[q], size=s["ghosts"][q], replace=False).astype(np.int64) for q in owners]
        ranks[r].ghost_owner = np.concatenate([np.full(p.size, q, dtype=np.int64) for q, p in zip(owners, picks)] + [np.zeros(0, np.int64)])
        ranks[r].ghost_index = np.concatenate(picks + [np.zeros(0, np.int64)])
        ranks[r].n_ghost = int(ranks[r].ghost_index.size)
    for r in range(world):
        nbrs = sorted(set(ranks[r].ghost_owner.tolist()) | {q for q in range(world) if (ranks[q].ghost_owner == r).any()})
        send, ranges, cursor = [], [], 0
        for q in nbrs:
            send.append(ranks[q].ghost_index[ranks[q].ghost_owner == r].astype(np.int32))
            k = int((ranks[r].ghost_owner == q).sum())
            ranges.append((cursor, cursor + k))
            cursor += k
        ranks[r].part = ExchangeLists(nbrs, send, ranges)
    offsets = np.concatenate([[0], np.cumsum(n_owned)]).astype(np.int64)
    # ---- the local matrices
    for r, s in enumerate(sizes):
        k = ranks[r]
        no, ng = k.n_owned, k.n_ghost
        n = no + ng
        cls = np.full(no, -1, dtype=np.int64)
        for row, c in s.get("pin", {}).items():
            cls[row] = c
        want_border = int(s["n_border"]) - int((cls == BORDER).sum())
        free = np.flatnonzero(cls < 0)
        assert 0 <= want_border <= free.size and (ng > 0 or s["n_border"] == 0)
        cls[free] = INTERIOR
        cls[rng.choice(free, size=want_border, replace=False)] = BORDER
        lens = np.zeros(n, dtype=np.int64)
        for c, rows, cap in ((INTERIOR, np.flatnonzero(cls == INTERIOR), no // 4), (BORDER, np.flatnonzero(cls == BORDER), min(no // 4, ng)),
                             (GHOST, np.arange(no, n), n // 4)):
            if rows.size:
                lens[rows], fit = _draw_lengths(rng, rows.size, cap, c != BORDER)
                lens[rows[:fit.size]] = fit[:rows.size]  # (every length that fits, once)
        if ng:
            lens[n - 1] = max(lens[n - 1], 3)
        # border rows: how many of the columns are ghosts (at least one; all of them in about one row in seven)
        border = np.flatnonzero(cls == BORDER)
        lg = np.zeros(no, dtype=np.int64)
        if border.size:
            share = np.where(rng.random(border.size) < 1 / 7, 1.0, rng.random(border.size))
            lg[border] = np.clip(np.ceil(share * lens[border]).astype(np.int64), 1, np.minimum(lens[border], ng))
            lg[border[:2]] = lens[border[:2]]  # (the first two border rows hold ghost columns only, whatever was drawn)
        lo = lens[:no] - lg
        rp_o, ci_o = R.strided_graph(no, lo) if no else (np.zeros(1, np.int64), np.zeros(0, np.int32))
        # the ghost columns of a border row: an arithmetic progression inside [n_owned, n)
        i = np.arange(no, dtype=np.int64)
        stride = 1 + _scramble(i, 777) % np.maximum(np.minimum((max(ng, 1) - 1) // np.maximum(lg - 1, 1), 97), 1)
        start = _scramble(i, 4242) % np.maximum(ng - stride * np.maximum(lg - 1, 0), 1)
        row_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        col_ind = np.empty(row_ptr[-1], dtype=np.int32)
        rows_o = np.repeat(i, lo)
        col_ind[row_ptr[rows_o] + (np.arange(rows_o.size) - rp_o[rows_o])] = ci_o
        rows_g = np.repeat(i, lg)
        pos = np.arange(rows_g.size) - (np.cumsum(lg) - lg)[rows_g]
        col_ind[row_ptr[rows_g] + lo[rows_g] + pos] = no + start[rows_g] + pos * stride[rows_g]
        if ng:  # the ghost rows: columns over all local dofs
            full = lens.copy()
            full[:no] = 0
            col_ind[row_ptr[no]:] = R.strided_graph(n, full)[1]
        k.row_ptr, k.col_ind, k.lens, k.cls = row_ptr, col_ind, lens, cls
        k.ints = rng.integers(-8, 9, col_ind.size).astype(np.float64)
        k.reals = rng.standard_normal(col_ind.size)
        k.gid = np.concatenate([offsets[r] + np.arange(no), offsets[k.ghost_owner] + k.ghost_index]).astype(np.int64)
    case = types.SimpleNamespace(world=world, ranks=ranks, offsets=offsets, n_global=int(offsets[-1]))
    # per owned row: the stored entries of the row and of its ghost copies, and the number of ghost copies (= export-adds)
    terms, exports = np.zeros(case.n_global, dtype=np.int64), np.zeros(case.n_global, dtype=np.int64)
    for k in ranks:
        terms[k.gid] += k.lens  # (the local dofs of a rank are distinct global dofs)
        exports[k.gid[k.n_owned:]] += 1
    for r, k in enumerate(ranks):
        k.n_terms, k.n_exports = terms[offsets[r]:offsets[r + 1]], exports[offsets[r]:offsets[r + 1]]
    return case


def owned(case, r, whole):
    """rank r's owned rows of a [..., n_global] array"""
    return whole[..., case.offsets[r]:case.offsets[r + 1]]


def local_vector(case, r, x_owned_by_rank):
    """[ncols, n_local]: rank r's owned rows followed by the imported ghosts"""
    k = case.ranks[r]
    x = np.atleast_2d(x_owned_by_rank[r])[:, :k.n_owned]
    ghosts = [np.atleast_2d(x_owned_by_rank[q])[:, k.ghost_index[k.ghost_owner == q]] for q in case.ranks[r].part.nbr_rank]
    return np.concatenate([x] + ghosts, axis=1)  # (ghosts are grouped by owner in neighbour order)


def apply_dist_ref(case, x_owned_by_rank, alpha, beta, y0_by_rank, values="reals"):
    """The owned rows of alpha A x + beta y0 with A = sum_r R_r^T A_r R_r, in longdouble.  x, y0: per rank [ncols, >= n_owned] (y0 is
    not read where beta == 0).  Returns per rank (y [ncols, n_owned], abs [ncols, n_owned]: |alpha| * the sum of |a_ij x_j| over the
    row and its ghost copies + |beta y0_i|, n_terms [n_owned]: the stored entries of the row and of its ghost copies on other
    ranks); ranks[r].n_exports counts those copies."""
    ncols = np.atleast_2d(x_owned_by_rank[0]).shape[0]
    ax, absx = np.zeros((ncols, case.n_global), dtype=LD), np.zeros((ncols, case.n_global), dtype=LD)
    for r, k in enumerate(case.ranks):
        xl = local_vector(case, r, x_owned_by_rank)
        for c in range(ncols):
            t, a = R.apply_ref(k.row_ptr, k.col_ind, getattr(k, values), xl[c])
            ax[c, k.gid] += t
            absx[c, k.gid] += a
    out = []
    for r, k in enumerate(case.ranks):
        y, a = LD(alpha) * owned(case, r, ax), abs(LD(alpha)) * owned(case, r, absx)
        if beta != 0.0:
            y0 = np.atleast_2d(y0_by_rank[r])[:, :k.n_owned].astype(LD)
            y, a = y + LD(beta) * y0, a + np.abs(LD(beta) * y0)
        out.append((y, a, k.n_terms))
    return out


def row_bound_dist(n_terms, n_exports, abs_terms):
    """csr_ref.row_bound for a row that is summed on several ranks.  Derived, not measured: the owner sums its own len_i products,
    every sharer the len of its ghost copy, in any order; each sharer scales by alpha (one rounding) and each export-add rounds
    once; the owner's alpha * and + beta y are the 3 of row_bound.  No partial result carries more than (all lengths + number of
    export-adds + 3) roundings, each of relative size EPS / 2, on terms whose absolute values sum to abs_terms."""
    return R.row_bound(np.asarray(n_terms, dtype=np.float64) + np.asarray(n_exports, dtype=np.float64), abs_terms)


def minv_of(diag, non_empty, damping, threshold):
    """l3k_csr_dist_diag's minv from a float64 diagonal: sign(a_ii) damping / max(|a_ii|, threshold) with sign(0) = +1 (one correctly
    rounded division, as csr_ref.diag_ref) where the row is non-empty IN THE LOCAL MATRIX of its owner, 0 elsewhere: the frozen-row
    rule looks at the owner's row only, even where a neighbour's ghost copy of the row contributes a diagonal"""
    diag = np.asarray(diag, dtype=np.float64)
    a = np.abs(diag)
    with np.errstate(divide="ignore"):
        minv = np.where(diag < 0, -np.float64(damping), np.float64(damping)) / np.where(a > threshold, a, np.float64(threshold))
    return np.where(non_empty, minv, 0.0)


def diag_dist_ref(case, damping=1.0, threshold=0.0, values="reals"):
    """l3k_csr_dist_diag.  Per rank a namespace: diag [n_owned] longdouble (the stored a_ii of the owner's row plus those of the
    ghost copies' rows), abs (the sum of their absolute values), n_contrib (how many of them are non-zero: with at most one the
    float64 result is exact), n_exports (the adds), minv (minv_of the float64 rounding of diag: exact where n_contrib <= 1)."""
    total, absd = np.zeros(case.n_global, dtype=LD), np.zeros(case.n_global, dtype=LD)
    contrib = np.zeros(case.n_global, dtype=np.int64)
    for k in case.ranks:
        d = R.diag_ref(k.row_ptr, k.col_ind, getattr(k, values))[0]
        total[k.gid] += d.astype(LD)
        absd[k.gid] += np.abs(d).astype(LD)
        contrib[k.gid] += d != 0
    out = []
    for r, k in enumerate(case.ranks):
        d = owned(case, r, total)
        out.append(types.SimpleNamespace(diag=d, abs=owned(case, r, absd), n_contrib=owned(case, r, contrib), n_exports=k.n_exports,
                                         minv=minv_of(d.astype(np.float64), k.lens[:k.n_owned] > 0, damping, threshold)))
    return out


def diag_bound(n_exports, abs_terms):
    """one rounding per export-add, each at most EPS / 2 relative to a partial sum that is at most abs_terms (1 + EPS)^k: EPS where
    EPS / 2 would do to first order, as in csr_ref.row_bound"""
    return np.asarray(n_exports, dtype=np.float64) * EPS * np.asarray(abs_terms, dtype=np.float64)


def dirichlet_owner_ref(row_ptr, col_ind, values, mask, g, rhs, n_owned):
    """l3k_csr_dirichlet_dist on one rank, the sparse form of asm_dist_ref.dirichlet_owner_rule: mask [n], g and rhs [ncols, n] over
    the LOCAL dofs.  A flagged owned row becomes the identity row with rhs = g, a flagged ghost row an all-zero row with rhs = 0, a
    free row gives rhs_i -= a_ij g_j over its flagged columns, which are zeroed.  Returns (values', rhs' in longdouble, abs) with
    abs as in csr_ref.dirichlet_ref (0 on the flagged rows, whose rhs is a copy or 0).  ValueError naming the smallest flagged
    OWNED row that stores no diagonal entry (a flagged ghost row needs none)."""
    row_ptr, col_ind = np.asarray(row_ptr, dtype=np.int64), np.asarray(col_ind, dtype=np.int64)
    values, mask = np.asarray(values, dtype=np.float64), np.asarray(mask).astype(bool)
    g, rhs = np.atleast_2d(np.asarray(g, dtype=np.float64)), np.atleast_2d(np.asarray(rhs, dtype=np.float64))
    rows = R.row_of_entry(row_ptr)
    is_owned = np.arange(mask.size) < n_owned
    has_diag = np.zeros(mask.size, dtype=bool)
    has_diag[rows[col_ind == rows]] = True
    bad = mask & is_owned & ~has_diag
    if bad.any():
        raise ValueError(f"owned Dirichlet row {int(np.flatnonzero(bad)[0])} has no stored diagonal entry")
    in_masked_row, in_masked_col = mask[rows], mask[col_ind]
    new = np.where(in_masked_row, ((col_ind == rows) & is_owned[rows]).astype(np.float64), np.where(in_masked_col, 0.0, values))
    out, absv = np.empty(rhs.shape, dtype=LD), np.empty(rhs.shape, dtype=LD)
    lift = ~in_masked_row & in_masked_col
    for c in range(rhs.shape[0]):
        prod = np.where(lift, values.astype(LD) * g[c].astype(LD)[col_ind], LD(0))
        out[c] = np.where(mask, np.where(is_owned, g[c].astype(LD), LD(0)), rhs[c].astype(LD) - R.row_sums(row_ptr, prod))
        absv[c] = np.where(mask, LD(0), np.abs(rhs[c]).astype(LD) + R.row_sums(row_ptr, np.abs(prod)))
    return new, out, absv


def row_classes(k):
    """(interior, border, ghost) of a rank of a case: asm_dist_ref.row_classes"""
    return AD.row_classes(k.row_ptr, k.col_ind, k.n_owned)


# ------------------------------------------------------------------------------------------------------------- the two cases
FULL_OWNED, FULL_BORDER, FULL_GHOST = 514 * 512, 66_000, 66_001  # rank 0: 197 168 interior rows; n_local = 329 169, chunk 512
_CASES = {}


def full_case():
    """World of two.  Rank 0: every row list (and each half of the interior list) is longer than the 65 536 groups a launch has at
    4 lanes per row, n_owned exceeds the 262 144 threads of a launch, n_local makes the compaction's chunk 512 (two tiles per
    block); the classes change at rows 255/256/257 and 511/512, and the ghost rows begin at a chunk boundary.  Rank 1 is small: it
    owns the dofs rank 0 holds copies of and has 3 000 ghosts of its own."""
    if "full" not in _CASES:
        assert chunk_of(FULL_OWNED + FULL_GHOST) == 512 and FULL_OWNED % 512 == 0
        pin = {255: INTERIOR, 256: BORDER, 257: INTERIOR, 510: BORDER, 511: INTERIOR, 512: BORDER, 513: BORDER, 767: BORDER, 768: INTERIOR,
               FULL_OWNED - 1: BORDER}
        _CASES["full"] = split_case(2, [dict(n_owned=FULL_OWNED, n_border=FULL_BORDER, ghosts={1: FULL_GHOST}, pin=pin),
                                        dict(n_owned=70_001, n_border=2_500, ghosts={0: 3_000})], seed=2024)
    return _CASES["full"]


def tiny_case():
    """World of three, a few hundred rows.  Rank 1 has ghost rows but no border rows, rank 2 has no interior rows, ranks 1 and 2
    both hold copies of some dofs of rank 0 (two exporters into one row); rank 1 sends to rank 2 and receives nothing from it."""
    if "tiny" not in _CASES:
        _CASES["tiny"] = split_case(3, [dict(n_owned=120, n_border=50, ghosts={1: 20, 2: 15}), dict(n_owned=150, n_border=0, ghosts={0: 40}),
                                        dict(n_owned=40, n_border=40, ghosts={0: 35, 1: 10})], seed=7)
    return _CASES["tiny"]
