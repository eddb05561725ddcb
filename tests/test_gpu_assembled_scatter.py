"""GPU tests of the assembled path's hand-off from element systems to the caller's CSR matrix (csrc/api_assembled.hip and
l3k_assemble_global in csrc/api.hip; the reference's scatterLocalSystem / assembleGlobalSystem, algsys/ScatterLocalSystem.hpp:24-54,
AssembleGlobalSystem.hpp:20-53) on three routes:

  node_rows  l3k_assembled_scatter, assembledScatterKernel<U>: one wave per (element, row node), one search per entry shared by the
             node's U rows after a check
  per_entry  the same call with l3k_tuning::scatter_per_entry: assembledScatterPerEntryKernel, one search per entry
  global     l3k_assemble_global: element systems formed on one stream and scattered on a second one, through
             assembledScatterTiledKernel<U, N1> where the tiled assembly kernel exists (U <= 4, order <= 7), else through node_rows

The reference is the scatter-add restated on the host (HostScatter): for every element e and local (i, j) the value K_e[i, j] goes to
row = elem_nodes[e, i // U] * dpn + field_inds[i % U], col likewise, summed with scipy's coo -> csr and placed into the graph by a
search over sorted (row, col) keys: no device index computation takes part.  The sums are accumulated in long double so that the
reference carries no summation error of its own.

node_rows and per_entry get K, F of l3k_local_assemble (pinned entry by entry against the oracle in test_gpu_assembly.py) and add
the very same numbers in another order.  A sum of t terms in any order differs from the exact sum by at most (t - 1) 2^-53 S, S the
sum of the terms' magnitudes (one rounding of at most 2^-53 |partial sum| <= 2^-53 S per addition): that is the bound asserted for
every CSR value and every rhs entry, t and S taken from the host scatter (t <= 8 on a hex mesh; a non-zero start value is one more
term).  One term gives a bound of zero: the value itself.  Route global forms K_e in the tiled layout, equal to the row-major one to
rounding: the project's stated tolerance, 1e-12 max|A_ref| (values) and 1e-12 max(1, max|rhs_ref|), and at orders
<= 4 the same against the oracle's element systems.  On every route a position without a contribution keeps its start value bit for
bit, and the number of entries outside the graph equals the host's count."""
import os

import numpy as np
import pytest

import oracle_lib as O
from helpers import HEX, SingleElementMesh, csr_graph
from l3ster_amd import system

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

LD = np.longdouble
ROUNDOFF = LD(2.0) ** -53
ROUTES = ("node_rows", "per_entry", "global")
DIFF, MASS, ADVEC, DIVCURL = system.KERNEL_DIFFUSION3D, system.KERNEL_MASS3D, system.KERNEL_ADVECTION3D, system.KERNEL_DIVCURL3D


@pytest.fixture(scope="module")
def ctx():
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return system.Context(0, torch.cuda.current_stream().cuda_stream)


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


class Ref:
    """Per position (CSR value or rhs entry): exact sum incl. the start value, sum of magnitudes, number of terms, whether any
    element contributes, and the contributions alone (the scale of the global route's tolerance)."""

    def __init__(self, init):
        self.init = init
        self.sum, self.abs = init.astype(LD), np.abs(init).astype(LD)
        self.terms = (init != 0).astype(np.int64)
        self.touched = np.zeros(init.shape, bool)
        self.contrib = np.zeros(init.shape)
        self.missing = 0


class HostScatter:
    """The scatter-add of K [count, Nd, Nd] and F [count, R, Nd] (elements first .. first + count of `part`) on the host."""

    def __init__(self, part, dpn, field_inds, K, F, first=0):
        import scipy.sparse as sp
        assert np.finfo(LD).nmant >= 63, "the reference accumulates in the x87 extended format"
        count, Nd = K.shape[0], K.shape[1]
        U = len(field_inds)
        en = part.elem_nodes[first:first + count].astype(np.int64)
        dofs = np.empty((count, Nd), np.int64)
        for i in range(Nd):
            dofs[:, i] = en[:, i // U] * dpn + int(field_inds[i % U])
        self.n = n = part.n_local_nodes * dpn
        rows, cols = np.repeat(dofs, Nd, axis=1).ravel(), np.tile(dofs, (1, Nd)).ravel()

        def summed(v):
            M = sp.coo_matrix((v, (rows, cols)), shape=(n, n)).tocsr()
            M.sort_indices()
            return M

        A, S, N = summed(K.reshape(-1).astype(LD)), summed(np.abs(K).reshape(-1).astype(LD)), summed(np.ones(rows.size, np.int64))
        assert A.data.dtype == LD and np.array_equal(A.indptr, N.indptr) and np.array_equal(A.indices, N.indices)
        assert np.array_equal(S.indptr, N.indptr) and np.array_equal(S.indices, N.indices) and int(N.data.sum()) == rows.size
        self.row = np.repeat(np.arange(n, dtype=np.int64), np.diff(N.indptr))
        self.col = N.indices.astype(np.int64)
        self.sum, self.abs, self.cnt = A.data, S.data, N.data
        self.F = None
        if F is not None:
            R = F.shape[1]
            r_idx = np.tile(np.repeat(np.arange(R), Nd), count)
            d_idx = np.repeat(dofs, R, axis=0).ravel()

            def summed_rhs(v):
                return sp.coo_matrix((v, (r_idx, d_idx)), shape=(R, n)).toarray()

            self.F = (summed_rhs(F.reshape(-1).astype(LD)), summed_rhs(np.abs(F).reshape(-1).astype(LD)),
                      summed_rhs(np.ones(d_idx.size, np.int64)))
            assert self.F[0].dtype == LD and int(self.F[2].sum()) == d_idx.size

    def onto_graph(self, row_ptr, col_ind, init, mask=None):
        """Reference for `values` started at `init`; with a mask: skip_dirichlet (entries of masked rows or columns are left out,
        they do not count as missing either)."""
        n = self.n
        gkey = np.repeat(np.arange(n, dtype=np.int64), np.diff(row_ptr)) * n + col_ind.astype(np.int64)
        assert np.all(np.diff(gkey) > 0) and gkey.size == init.size
        live = np.ones(self.row.size, bool) if mask is None else ~(mask[self.row] | mask[self.col])
        at = np.searchsorted(gkey, self.row * n + self.col)
        hit = gkey[np.minimum(at, gkey.size - 1)] == self.row * n + self.col
        put, pos = live & hit, at[live & hit]
        ref = Ref(init)
        ref.sum[pos] += self.sum[put]
        ref.abs[pos] += self.abs[put]
        ref.terms[pos] += self.cnt[put]
        ref.touched[pos] = True
        ref.contrib[pos] = self.sum[put].astype(np.float64)
        ref.missing = int(self.cnt[live & ~hit].sum())
        return ref

    def onto_rhs(self, init, mask=None):
        """Reference for rhs [R, ldr] started at `init` (ldr >= n: the columns behind n are padding)."""
        n = self.n
        live = np.ones(n, bool) if mask is None else ~mask
        ref = Ref(init)
        ref.sum[:, :n] += np.where(live, self.F[0], 0)
        ref.abs[:, :n] += np.where(live, self.F[1], 0)
        ref.terms[:, :n] += np.where(live, self.F[2], 0)
        ref.touched[:, :n] = live[None, :] & (self.F[2] > 0)
        ref.contrib[:, :n] = np.where(live, self.F[0], 0).astype(np.float64)
        return ref


def assert_placed(got, ref, what):
    still = ~ref.touched
    assert np.array_equal(bits(got)[still], bits(ref.init)[still]), f"{what}: a position without a contribution changed"


def assert_same_terms(got, ref, what):
    """routes that add the numbers the reference adds: the summation bound of the module's docstring"""
    assert_placed(got, ref, what)
    several = ref.terms > 1  # (most positions hold one term, a bound of zero: compared as float64, which holds that term exactly)
    wrong = np.nonzero(got[~several] != ref.sum[~several].astype(np.float64))[0]
    assert wrong.size == 0, f"{what}: {wrong.size} positions with a single term differ from it, first {np.argwhere(~several)[wrong[0]]}"
    err = np.abs(got[several].astype(LD) - ref.sum[several])
    bound = (ref.terms[several] - 1) * ROUNDOFF * ref.abs[several]
    if (bound > 0).any():
        ratio = float((err[bound > 0] / bound[bound > 0]).max())
        print(f"{what}: max err {float(err.max()):.3e}, max err / bound {ratio:.3f}, max terms {int(ref.terms.max())}")
    bad = err > bound
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} positions over (t - 1) 2^-53 S, first at {np.argwhere(several)[np.nonzero(bad)[0][0]]}"


def assert_to_rounding(got, ref, floor, what):
    """route global: the stated fp64 tolerance relative to the largest reference entry"""
    assert_placed(got, ref, what)
    scale = max(floor, float(np.abs(ref.contrib).max())) if ref.contrib.size else floor
    err = float(np.abs(got.astype(LD) - ref.sum).max()) if got.size else 0.0
    print(f"{what}: max err {err:.3e}, tolerance {1e-12 * scale:.3e}")
    assert err <= 1e-12 * scale, f"{what}: {err:.3e} > {1e-12 * scale:.3e}"


def pattern(shape):
    """a non-zero start: multiples of 1/8 in [-0.75, 0.875], none of them zero"""
    k = np.arange(int(np.prod(shape)), dtype=np.int64) % 13 - 6
    return (np.where(k == 0, 7, k) / 8.0).reshape(shape)


class Case:
    """One mesh + kernel: the element systems of l3k_local_assemble, their host scatter, and at orders <= 4 the oracle's element
    systems scattered the same way.  check() runs routes on one graph and asserts everything the module's docstring lists."""

    def __init__(self, ctx, part, kid, kpar=None, opts=(1, 0, 0), dpn=None, field_inds=None, mask=None, fields=None, oracle_kid=None):
        info = system.kernel_info(kid)
        self.ctx, self.part, self.U = ctx, part, info["n_unknowns"]
        self.p = p = part.order
        self.dpn = self.U if dpn is None else dpn
        self.fi = list(range(self.U)) if field_inds is None else list(field_inds)
        self.mask = None if mask is None else np.asarray(mask).astype(bool)
        self.mf = system.MatrixFreeSystem(system.DeviceMesh(ctx, part, self.dpn, mask), kid, kpar, asm_opts=opts,
                                          field_inds=None if field_inds is None else self.fi)
        if fields is not None:
            self.mf.set_fields(dev(fields))
        self.Nd = (p + 1) ** 3 * self.U
        self.Kd, self.Fd, _ = self.mf.local_assemble()
        torch.cuda.synchronize()
        self.host = HostScatter(part, self.dpn, self.fi, self.Kd.cpu().numpy(), self.Fd.cpu().numpy())
        self.n = self.host.n
        self.oracle = None
        if p <= 4 and oracle_kid is not None:
            nq = system.n_qps1d(p, *opts[:2])
            Ko, Fo = np.empty((part.n_elems, self.Nd, self.Nd)), np.empty((part.n_elems, 1, self.Nd))
            for e in range(part.n_elems):
                nf = None if fields is None else fields[:, part.elem_nodes[e]].T
                Ko[e], F_ref = O.assemble_local(oracle_kid, p, nq, 1, part.elem_verts[e], nf, kpar)
                Fo[e] = F_ref.T
            self.oracle = HostScatter(part, self.dpn, self.fi, Ko, Fo)

    def graph(self, drop=None):
        return csr_graph(self.part, self.dpn, self.fi, drop)[:2]

    def global_calls(self):
        """l3k_assemble_global in two calls: all elements but the last with room for one element per buffer (from the third
        sub-batch on a buffer is re-used behind its `consumed` event), then the last one with the default workspace"""
        ne = self.part.n_elems
        one = 2 * 8 * (self.Nd * self.Nd + self.Nd)
        return [(0, ne, 0)] if ne == 1 else [(0, ne - 1, one), (ne - 1, 1, 0)]

    def run(self, route, RP, CI, vals0, rhs0, skip):
        vals, rhs = dev(vals0), None if rhs0 is None else dev(rhs0)
        if route == "global":
            miss = sum(self.mf.assemble_global(RP, CI, vals, rhs, first=f, count=c, skip_dirichlet=skip, workspace_bytes=ws)
                       for f, c, ws in self.global_calls())
        else:
            with self.ctx.tuning(scatter_per_entry=int(route == "per_entry")):
                miss = self.mf.assembled_scatter(self.Kd, None if rhs is None else self.Fd, RP, CI, vals, rhs, skip_dirichlet=skip)
        torch.cuda.synchronize()
        return vals.cpu().numpy(), None if rhs is None else rhs.cpu().numpy(), miss

    def check(self, routes=ROUTES, skips=(False,), drop=None, start=np.zeros, pad=0, missing=None, tag=""):
        """Returns {(route, skip): (values, rhs, n_missing)}.  `missing`: None = whatever the host counts, 0 / "some" = the host's
        count must be zero / positive as well (a guard of the test's own graph)."""
        row_ptr, col_ind = self.graph(drop)
        RP, CI = torch.as_tensor(row_ptr, device="cuda"), torch.as_tensor(col_ind, device="cuda")
        vals0, rhs0 = start(col_ind.size), start((1, self.n + pad))
        out = {}
        for skip in skips:
            mask = self.mask if skip else None
            assert not skip or mask is not None
            ref_v, ref_r = self.host.onto_graph(row_ptr, col_ind, vals0, mask), self.host.onto_rhs(rhs0, mask)
            assert ref_v.touched.any() and ref_r.touched.any()
            if missing == 0:
                assert ref_v.missing == 0
            elif missing == "some":
                assert ref_v.missing > 0
            for route in routes:
                what = f"{tag} order {self.p} U {self.U} {route} skip {int(skip)}"
                vals, rhs, miss = out[(route, skip)] = self.run(route, RP, CI, vals0, rhs0, skip)
                assert miss == ref_v.missing, f"{what}: n_missing {miss}, the host counts {ref_v.missing}"
                if route == "global":
                    assert_to_rounding(vals, ref_v, 0.0, what + " values")
                    assert_to_rounding(rhs, ref_r, 1.0, what + " rhs")
                    if self.oracle is not None:
                        assert_to_rounding(vals, self.oracle.onto_graph(row_ptr, col_ind, vals0, mask), 0.0, what + " values vs oracle")
                        assert_to_rounding(rhs, self.oracle.onto_rhs(rhs0, mask), 1.0, what + " rhs vs oracle")
                else:
                    assert_same_terms(vals, ref_v, what + " values")
                    assert_same_terms(rhs, ref_r, what + " rhs")
        return out


# ---------------------------------------------------------------------------------------------- orders and numbers of unknowns
@pytest.mark.parametrize("p", [1, 5, 6, 7])
def test_orders_1_5_6_7(ctx, p):
    """assembledScatterTiledKernel<4, N1> for N1 = 2, 6, 7, 8 (and the other two kernels at those orders): order 1 has Nd = 32 < 64,
    half of every wave idle; order 6 is the north-star shape.  With and without skip_dirichlet (unknown 0 on all sides)."""
    part = system.CubePartition((2, 2, 1) if p == 1 else (2, 1, 1), p, perturb=0.15)
    case = Case(ctx, part, DIFF, [0.7, 1.3], mask=part.dirichlet_mask(4), oracle_kid=O.KERNEL_DIFFUSION3D)
    case.check(skips=(False, True), missing=0)


def test_one_unknown(ctx):
    """U = 1: Advection3D with its three fields set, order 2"""
    part = system.CubePartition((2, 2, 2), 2, perturb=0.15)
    fields = np.random.default_rng(2).uniform(-1, 1, (3, part.n_local_nodes))
    case = Case(ctx, part, ADVEC, [0.05], mask=part.dirichlet_mask(1), fields=fields, oracle_kid=O.KERNEL_ADVECTION3D)
    case.check(skips=(False, True), missing=0)


@pytest.mark.parametrize("p", [2, 4])
def test_three_unknowns(ctx, p):
    """U = 3: DivCurl3D"""
    part = system.CubePartition((2, 2, 1), p, perturb=0.15)
    case = Case(ctx, part, DIVCURL, [0.6], mask=part.dirichlet_mask(3), oracle_kid=O.KERNEL_DIVCURL3D)
    case.check(skips=(False, True), missing=0)


NS3D_SOURCE_FILE = "ns3d.hpp"


@pytest.mark.parametrize("which", ["order8", "u7"])
def test_shapes_without_the_tiled_scatter(ctx, which):
    """Order 8 and U = 7 (the NS3D plugin, compiled as in test_gpu_condensation.py: one plugin library for the suite) take the
    `tiled == 0` branch of l3k_assemble_global: row-major element systems between the streams, scattered by node_rows; global agrees
    with l3k_assembled_scatter within the global route's tolerance."""
    if which == "order8":
        case = Case(ctx, SingleElementMesh(8, HEX), DIFF, [0.7, 1.3])
        skips = (False,)
    else:
        from l3ster_amd import plugin
        src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "kernels", NS3D_SOURCE_FILE)).read()
        kid = plugin.compile_kernel("NS3D", src, 1013, shapes=[(2, 4, 1), (4, 8, 1), (6, 12, 1)])  # (as test_ns3d_plugin.py: one library)
        part = system.CubePartition((2, 2, 1), 2, perturb=0.15)
        fields = np.random.default_rng(3).uniform(0.5, 1.0, (7, part.n_local_nodes))
        case = Case(ctx, part, kid, None, opts=(1, 1, 0), mask=part.dirichlet_mask(7, unknowns=(0, 1, 2)), fields=fields,
                    oracle_kid=O.KERNEL_NS3D)
        skips = (False, True)
    out = case.check(routes=("global", "node_rows"), skips=skips, missing=0)
    for skip in skips:
        (vg, rg, _), (vn, rn, _) = out[("global", skip)], out[("node_rows", skip)]
        assert np.abs(vg - vn).max() <= 1e-12 * np.abs(vn).max()
        assert np.abs(rg - rn).max() <= 1e-12 * max(1.0, np.abs(rn).max())


# ------------------------------------------------------------------------------------------------- subsets of the node's dofs
@pytest.mark.parametrize("p", [2, 4])
def test_four_of_six_node_dofs_unsorted(ctx, p):
    """Diffusion3D on the dofs [4, 0, 5, 2] of 6 per node: row / col = node * dpn + field_inds[u], a node's columns not ascending in
    j; graph over the kernel's dofs only (the other rows are empty), values and rhs started from a non-zero pattern, rhs with three
    columns of padding; Dirichlet mask on field 4."""
    dpn, fi = 6, [4, 0, 5, 2]
    part = system.CubePartition((3, 2, 2) if p == 2 else 2, p, perturb=0.15)
    case = Case(ctx, part, DIFF, [0.7, 1.3], dpn=dpn, field_inds=fi, mask=part.dirichlet_mask(dpn, unknowns=(4,)), oracle_kid=O.KERNEL_DIFFUSION3D)
    row_ptr, _ = case.graph()
    assert all(np.all(np.diff(row_ptr)[k::dpn] == 0) for k in (1, 3))
    out = case.check(skips=(False, True), start=pattern, pad=3, missing=0)
    for (route, skip), (_, rhs, _) in out.items():  # (spelled out: dofs outside field_inds and the padding keep the pattern)
        start = pattern(rhs.shape)
        for k in (1, 3):
            assert np.array_equal(rhs[:, k:case.n:dpn], start[:, k:case.n:dpn]), (route, skip)
        assert np.array_equal(rhs[:, case.n:], start[:, case.n:]), (route, skip)


def test_two_of_five_node_dofs_unsorted(ctx):
    """Mass3D on the dofs [3, 1] of 5 per node, as above; Dirichlet mask on field 3."""
    dpn, fi = 5, [3, 1]
    part = system.CubePartition(2, 2, perturb=0.15)
    case = Case(ctx, part, MASS, None, dpn=dpn, field_inds=fi, mask=part.dirichlet_mask(dpn, unknowns=(3,)), oracle_kid=O.KERNEL_MASS3D)
    out = case.check(skips=(False, True), start=pattern, pad=3, missing=0)
    for (route, skip), (_, rhs, _) in out.items():
        start = pattern(rhs.shape)
        for k in (0, 2, 4):
            assert np.array_equal(rhs[:, k:case.n:dpn], start[:, k:case.n:dpn]), (route, skip)
        assert np.array_equal(rhs[:, case.n:], start[:, case.n:]), (route, skip)


# ----------------------------------------------------------------------------- graphs on which the shared search must fall back
@pytest.mark.parametrize("p", [2, 4])
def test_graphs_where_the_shared_search_falls_back(ctx, p):
    """The position found in the searched row of a node (u = 0 in node_rows, the first live row in the tiled kernel) is re-used for
    the node's other rows after a check; here the rows of a node differ:
    (a) Dirichlet rows trimmed to the diagonal, Dirichlet columns removed from the free rows, skip_dirichlet: nothing is missing;
    (b) the same graph without skip_dirichlet: on every boundary node the searched row is the odd one, the entries outside the graph
        are counted exactly;
    (c) every second entry removed from the u = 0 row of three interior nodes: the searched row is the sparse one;
    (d) every second entry removed from one u = 2 row only.
    n_missing of all three routes equals the host's count, the surviving entries are the reference's."""
    part = system.CubePartition(3 if p == 2 else 2, p, perturb=0.15)
    mask = part.dirichlet_mask(4).astype(bool)
    case = Case(ctx, part, DIFF, [0.7, 1.3], mask=mask, oracle_kid=O.KERNEL_DIFFUSION3D)
    inner = np.nonzero(part.node_boundary == 0)[0].astype(np.int64)
    assert inner.size >= 3

    def trimmed(r, c):
        return (mask[r] | mask[c]) & (r != c)

    def every_second_of(rows_hit):
        def drop(r, c):
            out = np.zeros(r.size, bool)
            for row in rows_hit:
                idx = np.nonzero(r == row)[0]
                assert idx.size > 2
                out[idx[::2]] = True
            return out
        return drop

    case.check(skips=(True,), drop=trimmed, missing=0, tag="(a)")
    case.check(skips=(False,), drop=trimmed, missing="some", tag="(b)")
    case.check(skips=(False,), drop=every_second_of(inner[[0, inner.size // 2, -1]] * 4), missing="some", tag="(c)")
    case.check(skips=(False,), drop=every_second_of([inner[inner.size // 2] * 4 + 2]), missing="some", tag="(d)")


# ------------------------------------------------------------------------------------------------------------------ two ranks
@pytest.mark.parametrize("p", [2, 4])
def test_two_ranks_sum_to_the_single_rank_matrix(ctx, p):
    """Each rank of a 2 x 1 x 1 partition assembles into its own local graph, ghost rows included (local rows past
    n_owned_nodes * dpn, element nodes in the ghost range); in the numbering of node_grid_id the two matrices and right-hand sides add
    up to those of the unpartitioned mesh (the host scatter of its element systems)."""
    import scipy.sparse as sp
    U = 4
    single = system.CubePartition((4, 2, 2), p, perturb=0.15)
    whole = Case(ctx, single, DIFF, [0.7, 1.3], mask=single.dirichlet_mask(U))
    ng = int(single.node_grid_id.max()) + 1
    assert ng == single.n_local_nodes == (4 * p + 1) * (2 * p + 1) ** 2

    def in_grid_numbering(part, row_ptr, col_ind, vals, rhs):
        gid = part.node_grid_id.astype(np.int64)
        to_grid = (gid[:, None] * U + np.arange(U)[None, :]).ravel()
        rows = np.repeat(np.arange(row_ptr.size - 1), np.diff(row_ptr))
        A = sp.coo_matrix((vals, (to_grid[rows], to_grid[col_ind])), shape=(ng * U, ng * U)).tocsr()
        return A, np.bincount(to_grid, weights=rhs[0], minlength=ng * U)

    ranks = []
    for r in (0, 1):
        part = system.CubePartition((4, 2, 2), p, parts=(2, 1, 1), rank=r, perturb=0.15)
        assert part.n_elems == 8
        ranks.append(Case(ctx, part, DIFF, [0.7, 1.3], mask=part.dirichlet_mask(U)))
    assert sum(c.part.n_ghost_nodes for c in ranks) > 0
    outs = [c.check(routes=("global", "node_rows"), skips=(False, True), missing=0, tag=f"rank {r}") for r, c in enumerate(ranks)]
    rp_w, ci_w = whole.graph()
    for skip in (False, True):
        mask = whole.mask if skip else None
        ref_v = whole.host.onto_graph(rp_w, ci_w, np.zeros(ci_w.size), mask)
        ref_r = whole.host.onto_rhs(np.zeros((1, whole.n)), mask)
        A_ref, rhs_ref = in_grid_numbering(single, rp_w, ci_w, ref_v.contrib, ref_r.contrib)
        for route in ("global", "node_rows"):
            A, rhs = 0, 0
            for c, out in zip(ranks, outs):
                vals, rhs_loc, _ = out[(route, skip)]
                rp, ci = c.graph()
                ghost_rows = slice(rp[c.part.n_owned_nodes * U], None)
                assert c.part.n_ghost_nodes == 0 or np.abs(vals[ghost_rows]).max() > 0
                A_r, rhs_r = in_grid_numbering(c.part, rp, ci, vals, rhs_loc)
                A, rhs = A + A_r, rhs + rhs_r
            D = (A - A_ref).tocsr()
            err, scale = float(np.abs(D.data).max()) if D.nnz else 0.0, float(np.abs(A_ref.data).max())
            print(f"two ranks order {p} {route} skip {int(skip)}: values {err:.3e} (tolerance {1e-12 * scale:.3e})")
            assert err <= 1e-12 * scale
            assert np.abs(rhs - rhs_ref).max() <= 1e-12 * max(1.0, np.abs(rhs_ref).max())


# -------------------------------------------------------------------------------------------------------------- small API edges
def test_api_edges(ctx):
    """assemble_global without a right-hand side; count = 0 leaves the values alone and returns 0; a leading dimension of rhs below
    the number of local dofs is refused before anything is written; l3k_assembled_scatter with first > 0 on a middle slice."""
    import ctypes as C
    part = system.CubePartition((3, 2, 2), 2, perturb=0.15)
    case = Case(ctx, part, DIFF, [0.7, 1.3], mask=part.dirichlet_mask(4))
    mf, n = case.mf, case.n
    row_ptr, col_ind = case.graph()
    RP, CI = torch.as_tensor(row_ptr, device="cuda"), torch.as_tensor(col_ind, device="cuda")
    vals0, rhs0 = pattern(col_ind.size), pattern((1, n))
    # rhs = None
    vals = dev(vals0)
    assert mf.assemble_global(RP, CI, vals, None) == 0
    torch.cuda.synchronize()
    assert_to_rounding(vals.cpu().numpy(), case.host.onto_graph(row_ptr, col_ind, vals0), 0.0, "global without rhs")
    # count = 0
    vals, rhs = dev(vals0), dev(rhs0)
    assert mf.assemble_global(RP, CI, vals, rhs, first=3, count=0) == 0
    miss = C.c_int64(7)
    P = lambda t: C.c_void_p(t.data_ptr())
    assert system.capi.load().l3k_assembled_scatter(mf._h, 3, 0, P(case.Kd), P(case.Fd), P(RP), P(CI), P(vals), P(rhs), n, 0, C.byref(miss)) == 0
    assert miss.value == 0
    torch.cuda.synchronize()
    assert np.array_equal(bits(vals.cpu().numpy()), bits(vals0)) and np.array_equal(bits(rhs.cpu().numpy()), bits(rhs0))
    # ldr < n
    short = dev(pattern((1, n - 1)))
    with pytest.raises(system.L3KError, match="leading dimension"):
        mf.assemble_global(RP, CI, vals, short)
    with pytest.raises(system.L3KError, match="leading dimension"):
        mf.assembled_scatter(case.Kd, case.Fd, RP, CI, vals, short)
    torch.cuda.synchronize()
    assert np.array_equal(bits(vals.cpu().numpy()), bits(vals0)) and np.array_equal(bits(short.cpu().numpy()), bits(pattern((1, n - 1))))
    # a middle slice
    first, count = 4, 5
    K, F, _ = mf.local_assemble(first, count)
    host = HostScatter(part, 4, range(4), K.cpu().numpy(), F.cpu().numpy(), first=first)
    for route in ("node_rows", "per_entry"):
        vals, rhs = dev(vals0), dev(rhs0)
        with ctx.tuning(scatter_per_entry=int(route == "per_entry")):
            assert mf.assembled_scatter(K, F, RP, CI, vals, rhs, first=first) == 0
        torch.cuda.synchronize()
        ref_v = host.onto_graph(row_ptr, col_ind, vals0)
        assert not ref_v.touched.all()
        assert_same_terms(vals.cpu().numpy(), ref_v, f"middle slice {route} values")
        assert_same_terms(rhs.cpu().numpy(), host.onto_rhs(rhs0), f"middle slice {route} rhs")
