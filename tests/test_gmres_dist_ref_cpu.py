"""tests/gmres_dist_ref.py pinned on the CPU: the partitioned restatement against tests/gmres_ref.py on the summed matrix, the
structure of the partitioned chain, what tests/test_gpu_gmres_dist.py relies on (the stopping margins of the restatement, the failure
of PCG on the chain), and the new names of the C interface.  No GPU."""
import os
import re

import numpy as np
import pytest

import gmres_dist_ref as GD
import gmres_ref as G
from gmres_ref import LD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, C09 = 3000, 0.9
SPLITS = {"three": [1000, 1100, 900], "empty": [1500, 0, 1500]}
NEW_NAMES = ("l3k_halo_reduce_reserve", "l3k_halo_allreduce_sum_n", "l3k_gmres_create_dist", "l3k_gmres_solve_dist",
             "l3k_csr_dist_gmres_solve")
_RUNS = {}


def system_of(split):
    case = GD.chain(N, C09, SPLITS[split])
    A = GD.tri_apply(case.lo, case.di, case.up)
    xs = np.cos(0.1 * np.arange(N))
    return case, A, A(xs), 1.0 / case.di, xs


def run(split, m, dtype=LD):
    if (split, m, dtype) not in _RUNS:
        case, A, b, minv, _ = system_of(split)
        _RUNS[split, m, dtype] = GD.gmres(A, case.offsets, b, np.zeros(N), m, prec=lambda v: v * minv.astype(v.dtype), tol=1e-10,
                                          residual_scaling=2, dtype=dtype)
    return _RUNS[split, m, dtype]


@pytest.mark.parametrize("split", list(SPLITS))
def test_chain_structure(split):
    case = GD.chain(N, C09, SPLITS[split])
    lo, di, up, off = GD.summed_diagonals(case)
    want = GD.tridiagonal(N, C09)
    assert off == 0 and all(np.array_equal(a, b) for a, b in zip((lo, di, up), want))  # (the halves of a diagonal add up exactly)
    holders = [r for r, k in enumerate(case.ranks) if k.n_owned]
    for r, k in enumerate(case.ranks):
        nl = k.n_owned + k.n_ghost
        assert k.row_ptr.size == nl + 1 and k.row_ptr[-1] == k.col_ind.size == k.values.size and k.gid.size == nl
        assert all(np.all(np.diff(k.col_ind[a:b]) > 0) for a, b in zip(k.row_ptr[:-1], k.row_ptr[1:]))
        assert k.col_ind.size == 0 or (k.col_ind.min() >= 0 and k.col_ind.max() < nl)
        if k.n_owned == 0:
            assert nl == 0 and k.part.nbr_rank == [] and k.row_ptr.tolist() == [0]
            continue
        i = holders.index(r)
        assert k.n_ghost == (i + 1 < len(holders)) and r not in k.part.nbr_rank
        assert k.part.nbr_rank == ([holders[i - 1]] if i else []) + ([holders[i + 1]] if k.n_ghost else [])
        # the exchange lists mirror each other: what a neighbour holds as its ghost is this rank's first row
        for nb, send, (g0, g1) in zip(k.part.nbr_rank, k.part.send_nodes, k.part.ghost_ranges):
            other = case.ranks[nb]
            j = other.part.nbr_rank.index(r)
            assert len(send) == other.part.ghost_ranges[j][1] - other.part.ghost_ranges[j][0]
            assert g1 - g0 == len(other.part.send_nodes[j])
            assert all(case.offsets[r] + s == other.gid[other.n_owned + q] for q, s in enumerate(send))
        if k.n_ghost:  # the ghost row is stored: it is export-added to its owner
            assert k.row_ptr[nl] - k.row_ptr[nl - 1] == 2
    small = GD.chain(7, 0.5, [3, 0, 4])
    dense = np.zeros((7, 7))
    for k in small.ranks:
        for i in range(k.n_owned + k.n_ghost):
            for p in range(k.row_ptr[i], k.row_ptr[i + 1]):
                dense[k.gid[i], k.gid[k.col_ind[p]]] += k.values[p]
    lo, di, up = GD.tridiagonal(7, 0.5)
    assert np.array_equal(dense, np.diag(di) + np.diag(lo[1:], -1) + np.diag(up[:-1], 1))


@pytest.mark.parametrize("m", [5, 30, 300])
def test_restatement_against_gmres_ref(m):
    """one rank: the same bits as gmres_ref in float64.  Three ranks: the same iteration in longdouble -- counts equal, the
    estimates of the first cycle within 1e-12 (the sums differ in their last bits only)"""
    case, A, b, minv, xs = system_of("three")
    prec = lambda v: v * minv.astype(v.dtype)
    kw = dict(prec=prec, tol=1e-10, residual_scaling=2)
    one = GD.gmres(A, np.array([0, N]), b, np.zeros(N), m, dtype=np.float64, **kw)
    ref64 = G.gmres(A, b, np.zeros(N), m, dtype=np.float64, **kw)
    assert one["history"] == ref64["history"] and np.array_equal(one["x"], ref64["x"])
    assert all(one[k] == ref64[k] for k in ("iterations", "restarts", "converged", "breakdown", "achieved_tol", "estimate", "orth_loss"))
    three, ref = run("three", m), G.gmres(A, b, np.zeros(N), m, dtype=LD, **kw)
    assert (three["iterations"], three["restarts"], three["converged"]) == (ref["iterations"], ref["restarts"], True)
    first = min(m, len(ref["history"]))
    assert np.allclose(three["history"][:first], ref["history"][:first], rtol=1e-12, atol=0)
    assert np.abs(three["x"] - xs).max() <= 1e-7
    empty = run("empty", m)
    assert (empty["iterations"], empty["restarts"]) == (ref["iterations"], ref["restarts"])


@pytest.mark.parametrize("split", list(SPLITS))
@pytest.mark.parametrize("m", [5, 30, 300])
def test_stopping_margins_of_the_chain(split, m):
    """What the GPU test may hold the device to.  At tol 1e-10 the chain converges by 1.1 - 1.3 per step: both margins are >= 1.02 --
    two hundred million times the 1e-10 by which the device's estimates differ from the restatement's -- and below the 1.5 of
    gmres_ref.stopping_margin's rule for a count within 1.  No two consecutive estimates of the first cycle are 2.25 apart, so no tolerance of this
    chain has both margins >= 1.5 (choose_tol finds none): the count is also asserted at the margins the chain has, 1.02."""
    ref = run(split, m)
    below, above = G.stopping_margin(ref["history"], 1e-10)
    print(f"{split} m={m}: {ref['iterations']} iterations, {ref['restarts']} restarts, margins {below:.4f} {above:.4f}")
    assert ref["converged"] and min(below, above) >= 1.02
    h = ref["history"][:m]
    assert GD.choose_tol(h, 1) is None and max(h[j - 1] / h[j] for j in range(1, len(h))) < 2.25


def test_stopping_margins_of_the_frozen_rows_case():
    """the case of tests/test_gpu_gmres_dist.py::test_frozen_rows_keep_x_and_the_rest_solves: GMRES(30) with Jacobi from a random x0,
    11 rows of rank 1 frozen.  Its margins at 1e-10 are 1.25 and 1.012: the device's count is held within 1 at a floor of 1.01"""
    case, A, b, _, xs = system_of("three")
    live, x0, minv = GD.frozen_rows(case)
    ref = GD.gmres(A, case.offsets, b, x0, 30, prec=lambda v: v * minv.astype(v.dtype), live=live, tol=1e-10, residual_scaling=2, dtype=LD)
    below, above = G.stopping_margin(ref["history"], 1e-10)
    print(f"frozen rows: {ref['iterations']} iterations, {ref['restarts']} restarts, margins {below:.4f} {above:.4f}")
    assert ref["converged"] and int((~live).sum()) == 11 and min(below, above) >= 1.01
    assert np.array_equal(ref["x"][~live].astype(np.float64), x0[~live])


def test_pcg_is_not_the_answer_on_the_chain():
    """Jacobi-PCG on the non-symmetric chain, given the operator applies of the GMRES(30) solve (one per step, one per cycle head):
    it is not near the tolerance"""
    case, A, b, minv, _ = system_of("three")
    ref = run("three", 30)
    applies = ref["iterations"] + ref["restarts"] + 2
    converged, its, res, _ = GD.pcg(A, b, minv, 1e-10, applies)
    print(f"PCG after {its} iterations: |b - A x| / |b| = {res:.3e}; GMRES(30) took {applies} applies")
    assert not converged and its == applies and not res <= 1e-3


def test_new_names_are_declared_and_bound():
    from l3ster_amd import capi
    header = open(os.path.join(ROOT, "include", "l3k.h")).read()
    for name in NEW_NAMES:
        assert re.search(r"^int\s+" + name + r"\(", header, re.M), name
        assert name in capi.SIGNATURES, name
    from l3ster_amd import solve
    from l3ster_amd.distributed import NativeHalo
    assert callable(solve.gmres_distributed) and callable(NativeHalo.allreduce_n) and callable(NativeHalo.reduce_reserve)
