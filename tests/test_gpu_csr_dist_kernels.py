"""The kernels of the distributed CSR operator (device/csr_dist.hpp behind l3k_csr_dist_create / _apply / _diag and
l3k_csr_dirichlet_dist) on SYNTHETIC partitioned matrices, where tests/test_gpu_asm_dist.py drives them through small meshes only:
row lists longer than a launch has row groups (1024 * 256 / 4 = 65 536), so that every group of every lanes-per-row route walks
several rows and the rolling prefetch of the next list entry runs; more local rows than 262 144, so that a block of the ordered
compaction scans several tiles; row lengths 0 ... 1000 in every class; empty owned rows, empty ghost rows, owned rows with ghost
columns only; class changes at tile and chunk boundaries (tests/csr_dist_ref.py builds the cases, tests/test_csr_dist_ref_cpu.py
asserts this structure).  A tiny world of three covers empty lists and two exporters into one row.

The ranks are threads of this process on one GPU with the library's in-process transport, as in tests/test_gpu_asm_dist.py.  A rank
body only computes and stores; every assertion runs afterwards in the main thread.  One run per (case, value kind, lanes) serves
all tests.  No tolerance here is measured: integer data must come out bit-equal to the longdouble restatement (every order of
summation gives the same double), real data within the derived row-wise bound of csr_dist_ref.row_bound_dist."""
import numpy as np
import pytest
import torch

import csr_dist_ref as D
import csr_ref as R
from cg_ref import LD
from l3ster_amd import capi, system
from l3ster_amd.distributed import InprocGroup, NativeHalo
from test_gpu_asm_dist import rank_context, run_ranks

pytestmark = pytest.mark.gpu
LANES = [4, 16, 64, 0]
CASES = {"full": D.full_case, "tiny": D.tiny_case}
# (alpha, beta, ncols), applied one after another through the SAME operator, each with its own x: the widest first, so that the
# export buffer is allocated once; (1, 0, 1) -> (0, 1, 1) and the two (-0.5, 2, 3) are consecutive with the same ncols -- a ghost
# row that did not store would hand the previous apply's value to its owner
APPLIES = {"ints": [(1.0, 0.0, 5), (1.0, 0.0, 1), (0.0, 1.0, 1), (-0.5, 2.0, 3), (-0.5, 2.0, 3)],
           "reals": [(1.25, -1.0, 5), (1.0, 0.0, 1), (-0.5, 2.0, 3)]}
DIAGS = [(1.0, 0.25), (0.8, 1e-3), (1.0, 0.0)]  # (damping, threshold)
PAD_X, PAD_Y = 7, 13
_INPUTS, _REFS, _RUNS, _MAIN = {}, {}, {}, {}


@pytest.fixture(scope="module", autouse=True)
def release_the_runs():
    """the cached inputs, references and results (a few hundred MB on the host) go when the module is done"""
    yield
    for cache in (_INPUTS, _REFS, _RUNS, _MAIN):
        cache.clear()


def dev(a, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


def host(t):
    return t.detach().cpu().numpy().copy()


def nans(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float64, device="cuda")


def inputs(name, kind):
    """per apply: (x by rank [ncols, n_owned + 7], y0 by rank [ncols, n_owned + 13]); integers in [-8, 8] or standard normal"""
    if (name, kind) not in _INPUTS:
        case, rng = CASES[name](), np.random.default_rng(41 + len(name) + len(kind))
        draw = (lambda *s: rng.integers(-8, 9, s).astype(np.float64)) if kind == "ints" else (lambda *s: rng.standard_normal(s))
        _INPUTS[name, kind] = [([draw(nc, k.n_owned + PAD_X) for k in case.ranks], [draw(nc, k.n_owned + PAD_Y) for k in case.ranks])
                               for _, _, nc in APPLIES[kind]]
    return _INPUTS[name, kind]


def reference(name, kind, idx):
    """apply_dist_ref of apply idx: computed once, shared by the lanes values"""
    if (name, kind, idx) not in _REFS:
        (alpha, beta, _), (x, y0) = APPLIES[kind][idx], inputs(name, kind)[idx]
        _REFS[name, kind, idx] = D.apply_dist_ref(CASES[name](), x, alpha, beta, y0, kind)
    return _REFS[name, kind, idx]


def run(name, kind, lanes):
    """every rank's script, once per (case, value kind, lanes): what each rank left, by rank"""
    key = (name, kind, lanes)
    if key in _RUNS:
        return _RUNS[key]
    case, data = CASES[name](), inputs(name, kind)
    group, out = InprocGroup(case.world), {}

    def body(rank):
        k, d = case.ranks[rank], {}
        no, ng = k.n_owned, k.n_ghost
        c = rank_context()
        local = system.CsrOperator(c, dev(k.row_ptr, torch.int64), dev(k.col_ind, torch.int32), dev(getattr(k, kind)), lanes)
        op = system.DistributedCsrOperator(local, NativeHalo(c, k.part, 1, rank, case.world, transport=group))
        i = op.info
        d["counts"] = (op.n, i.n_owned, i.n_ghost, i.n_interior_rows, i.n_border_rows, i.n_ghost_rows)
        d["lists"] = tuple(host(t) for t in (i.interior_rows, i.border_rows, i.ghost_rows))
        d["lanes"] = local.info().lanes_per_row
        d["apply"] = []
        for (alpha, beta, nc), (x, y0) in zip(APPLIES[kind], data):
            Y = dev(y0[rank]) if beta != 0.0 else nans(nc, no + PAD_Y)
            op.apply(dev(x[rank]), Y, alpha, beta)
            d["apply"].append(host(Y))
        # the last apply once more: bit for bit the same
        (alpha, beta, nc), (x, y0) = APPLIES[kind][-1], data[-1]
        d["again"] = host(op.apply(dev(x[rank]), dev(y0[rank]), alpha, beta))
        # the single-rank operator of the local matrix on [x_owned | imported ghosts], with the coefficients of apply 1 (1, 0, 1)
        X = dev(data[1][0][rank])
        Xl = torch.cat([X[:, :no], op.import_ghosts(X)[:, :ng]], dim=1).contiguous()
        d["local"] = host(local.apply(Xl, nans(1, no + ng), 1.0, 0.0))[:, :no]
        d["diag"] = host(op.diag())
        d["minv"] = [host(op.jacobi_inverse(*dt)) for dt in DIAGS]
        out[rank] = d

    run_ranks(case.world, body)
    _RUNS[key] = out
    return out


# ------------------------------------------------------------------------------------------------------------- row lists
@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("name", list(CASES))
def test_row_lists_equal_the_restatement(name, lanes):
    """the ordered compaction: counts and the three ascending lists, the same for every lanes value (tiny: empty lists)"""
    case, out, first = CASES[name](), run(name, "ints", lanes), run(name, "ints", LANES[0])
    for r, k in enumerate(case.ranks):
        want = D.row_classes(k)
        assert out[r]["counts"] == (k.n_owned, k.n_owned, k.n_ghost, want[0].size, want[1].size, want[2].size)
        for got, exp, ref in zip(out[r]["lists"], want, first[r]["lists"]):
            assert got.dtype == np.int32 and np.array_equal(got, exp) and np.array_equal(got, ref)
        assert out[r]["lanes"] == lanes if lanes else out[r]["lanes"] in (4, 16, 64)


# ----------------------------------------------------------------------------------------------------------------- apply
@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("idx", range(len(APPLIES["ints"])))
@pytest.mark.parametrize("name", list(CASES))
def test_apply_is_exact_on_integers(name, idx, lanes):
    """values, x and y0 are integers in [-8, 8] (alpha, beta: powers of two): the device equals the longdouble restatement bit for
    bit on every owned row of every rank, writes nothing past row n_owned, and leaves no NaN of y behind where beta = 0.  An apply
    that follows one of the same width also shows that every entry of the export buffer was stored again (empty ghost rows)."""
    case, out = CASES[name](), run(name, "ints", lanes)
    (alpha, beta, nc), (x, y0) = APPLIES["ints"][idx], inputs(name, "ints")[idx]
    for r, (k, (want, _, _)) in enumerate(zip(case.ranks, reference(name, "ints", idx))):
        got = out[r]["apply"][idx]
        assert got.shape == (nc, k.n_owned + PAD_Y)
        assert np.isfinite(got[:, :k.n_owned]).all()
        assert np.array_equal(got[:, :k.n_owned], want.astype(np.float64)), (r, int(np.flatnonzero((got[:, :k.n_owned] != want).any(axis=0))[0]))
        pad = got[:, k.n_owned:]
        assert np.isnan(pad).all() if beta == 0.0 else np.array_equal(pad, y0[r][:, k.n_owned:])


@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("idx", range(len(APPLIES["reals"])))
def test_apply_real_values_within_the_derived_bound(idx, lanes):
    """|y_i - ref_i| <= (len_i + the lengths of the ghost copies + the export-adds + 3) EPS (|alpha| sum |a_ij x_j| + |beta y_i|)"""
    case, out = D.full_case(), run("full", "reals", lanes)
    worst = 0.0
    for r, (k, (ref, absv, n_terms)) in enumerate(zip(case.ranks, reference("full", "reals", idx))):
        got = out[r]["apply"][idx][:, :k.n_owned]
        bound = D.row_bound_dist(n_terms, k.n_exports, absv)
        err = np.abs(got.astype(LD) - ref).astype(np.float64)
        worst = max(worst, float(np.max(err[bound > 0] / bound[bound > 0])))
        at = np.unravel_index(int(np.argmax(err - bound)), err.shape)
        assert np.isfinite(got).all() and (err <= bound).all(), (r, at, err[at], bound[at])
    print(f"lanes {lanes} apply {APPLIES['reals'][idx]}: largest error / bound {worst:.3f}")


@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("kind", ["ints", "reals"])
def test_apply_is_reproducible_and_rows_without_an_export_are_the_local_operators(kind, lanes):
    """two identical applies give the same bits; an owned row no neighbour holds a copy of gets exactly what CsrOperator(local matrix)
    gives on [x_owned | imported ghosts]: same lanes, same order, same butterfly"""
    case, out = D.full_case(), run("full", kind, lanes)
    for r, k in enumerate(case.ranks):
        assert np.array_equal(out[r]["again"], out[r]["apply"][-1])
        alone = k.n_exports == 0
        assert alone.sum() > 1000 and (~alone).sum() > 1000
        assert APPLIES[kind][1] == (1.0, 0.0, 1)
        got, local = out[r]["apply"][1][:, :k.n_owned], out[r]["local"]
        assert np.isfinite(local).all() and np.array_equal(got[:, alone], local[:, alone])
        if kind == "reals":
            assert (got[:, ~alone] != local[:, ~alone]).any()  # (the other rows did receive something)


@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("ncols", [1, 5])
def test_world_of_one_is_the_csr_operator_bit_for_bit(ncols, lanes):
    """the 70 001-row matrix of tests/test_gpu_csr_apply.py behind a halo without neighbours: one interior list in one launch, more
    rows than groups at 4 lanes"""
    from test_gpu_csr_apply import N, matrix, operator
    m = matrix()
    local = operator("reals", lanes)
    op = system.DistributedCsrOperator(local, NativeHalo(m["ctx"], D.ExchangeLists([], [], []), 1, 0, 1, transport=InprocGroup(1)))
    i = op.info
    assert (op.n, i.n_owned, i.n_ghost, i.n_interior_rows, i.n_border_rows, i.n_ghost_rows) == (N, N, 0, N, 0, 0)
    assert torch.equal(i.interior_rows.cpu(), torch.arange(N, dtype=torch.int32))
    rng = np.random.default_rng(3 + ncols)
    x, y0 = rng.standard_normal((ncols, N + PAD_X)), rng.standard_normal((ncols, N + PAD_Y))
    for alpha, beta in ((1.0, 0.0), (-0.5, 2.0)):
        Y, Z = (dev(y0) if beta != 0.0 else nans(ncols, N + PAD_Y) for _ in range(2))
        op.apply(dev(x), Y, alpha, beta)
        local.apply(dev(x), Z, alpha, beta)
        assert torch.isfinite(Y[:, :N]).all() and torch.equal(Y[:, :N], Z[:, :N])
        assert torch.isnan(Y[:, N:]).all() if beta == 0.0 else torch.equal(Y[:, N:], dev(y0)[:, N:])
    assert torch.equal(op.diag(), local.diag()) and torch.equal(op.jacobi_inverse(0.8, 1e-3), local.jacobi_inverse(0.8, 1e-3))


# -------------------------------------------------------------------------------------------------------- diagonal, minv
@pytest.mark.parametrize("which", range(len(DIAGS)))
@pytest.mark.parametrize("name,kind,lanes", [("full", "reals", 0), ("full", "ints", 4), ("tiny", "reals", 16), ("tiny", "ints", 64)])
def test_diag_and_minv(name, kind, lanes, which):
    """diag: the owner's stored a_ii plus the export-added ones of the ghost copies -- bit-equal where at most one of them is not 0
    (and everywhere on integers), within one rounding per add elsewhere; minv: the correctly rounded quotient of the DEVICE diagonal,
    0 on an owned row that is empty in the owner's local matrix even where a neighbour's ghost row contributes a diagonal"""
    case, out = CASES[name](), run(name, kind, lanes)
    damping, threshold = DIAGS[which]
    frozen_with_diag = 0
    for r, (k, ref) in enumerate(zip(case.ranks, D.diag_dist_ref(case, damping, threshold, kind))):
        got, got_m = out[r]["diag"], out[r]["minv"][which]
        assert got.shape == got_m.shape == (k.n_owned,)
        exact = (ref.n_contrib <= 1) | (kind == "ints")
        assert np.array_equal(got[exact], ref.diag[exact].astype(np.float64))
        assert (np.abs(got.astype(LD) - ref.diag).astype(np.float64) <= D.diag_bound(ref.n_exports, ref.abs)).all()
        non_empty = k.lens[:k.n_owned] > 0
        assert np.array_equal(got_m, D.minv_of(got, non_empty, damping, threshold))  # (inf where the formula is 1 / 0)
        assert np.array_equal(got_m[exact], ref.minv[exact])
        assert not got_m[~non_empty].any() and (np.isfinite(got_m).all() or threshold == 0.0)
        frozen_with_diag += int((~non_empty & (got != 0)).sum())
    assert frozen_with_diag > 0  # the empty-local-row rule met a non-zero summed diagonal


# ---------------------------------------------------------------------------------- Dirichlet conditions with the owner rule
def main_rank0():
    """rank 0's local matrix of the full case on the main thread's context (l3k_csr_dirichlet_dist is rank-local)"""
    if not _MAIN:
        torch.cuda.set_device(0)
        k = D.full_case().ranks[0]
        rows = R.row_of_entry(k.row_ptr)
        stored = np.zeros(k.lens.size, dtype=bool)
        stored[rows[k.col_ind == rows]] = True
        _MAIN.update(k=k, ctx=rank_context(), RP=dev(k.row_ptr, torch.int64), CI=dev(k.col_ind, torch.int32), stored=stored, cases={})
    return _MAIN


def dirichlet_case(ncols):
    """mask over owned and ghost rows (a flagged owned row stores its diagonal, a flagged ghost row need not), g, rhs and the
    restatement; built once per ncols"""
    m = main_rank0()
    if ncols not in m["cases"]:
        k, n = m["k"], m["k"].lens.size
        rng = np.random.default_rng(31 + ncols)
        mask = (rng.random(n) < 0.2) & (m["stored"] | (np.arange(n) >= k.n_owned))
        mask[np.flatnonzero(m["stored"] & (k.lens == 1000))[:2]] = True  # (long rows as Dirichlet rows, owned or ghost)
        g, rhs = rng.standard_normal((ncols, n + 5)), rng.standard_normal((ncols, n + 3))
        m["cases"][ncols] = (mask.astype(np.uint8), g, rhs,
                             D.dirichlet_owner_ref(k.row_ptr, k.col_ind, k.reals, mask, g[:, :n], rhs[:, :n], k.n_owned))
    return m["cases"][ncols]


@pytest.mark.parametrize("lanes", [0, 4, 64])
@pytest.mark.parametrize("ncols", [1, 3])
def test_dirichlet_local_matches_the_restatement(ncols, lanes):
    m = main_rank0()
    k, n = m["k"], m["k"].lens.size
    mask, g, rhs, (new, ref, absv) = dirichlet_case(ncols)
    flagged = mask.astype(bool)
    ghost = np.arange(n) >= k.n_owned
    assert (flagged & ghost).sum() > 1000 and (flagged & ghost & ~m["stored"]).sum() > 100 and (flagged & ~ghost).sum() > 1000
    values, G, F, M = dev(k.reals), dev(g), dev(rhs), dev(mask, torch.uint8)
    op = system.CsrOperator(m["ctx"], m["RP"], m["CI"], values, lanes)
    op.dirichlet_local(M, G, F, k.n_owned)
    got_v, got_f = host(values), host(F)
    assert np.array_equal(got_v, new)  # bit for bit: old entries, zeros and ones
    err = np.abs(got_f[:, :n].astype(LD) - ref).astype(np.float64)
    bound = R.row_bound(np.broadcast_to(k.lens, err.shape), absv)
    print(f"lanes {lanes} ncols {ncols}: largest error / bound {np.max(err[bound > 0] / bound[bound > 0]):.3f}")
    assert (err <= bound).all()
    assert np.array_equal(got_f[:, :n][:, flagged & ~ghost], g[:, :n][:, flagged & ~ghost])  # owned: the prescribed value
    assert not got_f[:, :n][:, flagged & ghost].any()  # ghost: rhs 0 ...
    assert not got_v[flagged[R.row_of_entry(k.row_ptr)] & (R.row_of_entry(k.row_ptr) >= k.n_owned)].any()  # ... and an all-zero row
    assert np.array_equal(got_f[:, n:], rhs[:, n:]) and torch.equal(G, dev(g)) and torch.equal(M, dev(mask, torch.uint8))


def test_dirichlet_local_refuses_an_owned_row_without_diagonal():
    """several offenders in different blocks, below and past the 262 144 threads of the check's launch: the smallest one is named
    and nothing is changed; a flagged ghost row without a diagonal is no offence (the test above flags hundreds)"""
    m = main_rank0()
    k, n = m["k"], m["k"].lens.size
    mask, g, rhs, _ = dirichlet_case(1)
    bad = np.flatnonzero(~m["stored"][:k.n_owned])
    past = D.MAX_BLOCKS * D.BLOCK
    assert k.n_owned > past + 600
    pick = lambda lo: int(bad[bad >= lo][0])
    empty_past = int(np.flatnonzero((k.lens[:k.n_owned] == 0) & (np.arange(k.n_owned) >= past + 500))[0])
    for rows in ([pick(70_003), pick(150_000), pick(past + 300)], [pick(past + 300), empty_past, pick(k.n_owned - 50)], [empty_past]):
        mk = mask.copy()
        mk[rows] = 1
        values, F = dev(k.reals), dev(rhs)
        op = system.CsrOperator(m["ctx"], m["RP"], m["CI"], values, 0)
        message = f"libl3k error -1: l3k_csr_dirichlet_dist: the owned Dirichlet row {min(rows)} has no stored diagonal"
        with pytest.raises(capi.L3KError, match=message):
            op.dirichlet_local(dev(mk, torch.uint8), dev(g), F, k.n_owned)
        assert torch.equal(values, dev(k.reals)) and torch.equal(F, dev(rhs))  # bitwise unchanged
