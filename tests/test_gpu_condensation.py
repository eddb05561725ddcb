"""GPU tests of static condensation (the reference's CondensationPolicy::ElementBoundary, StaticCondensationManager.hpp):
l3k_condense_local against a numpy Schur complement of the oracle's element systems, l3k_condense_global against a dense
Schur complement of the oracle-assembled global matrix, a condensed solve + l3k_condensed_recover against the full assembled
solve, other shapes (a U = 7 plugin, order 8) and the error paths; recovery with three right-hand sides per element against numpy,
strict sub-ranges of condense_local / recover_internal against slices of the full range, and a mesh on which some elements fail their
pivot while their neighbours do not."""
import numpy as np
import pytest

import oracle_lib as O
from helpers import HEX, SingleElementMesh, cube_with_inverted_element
from l3ster_amd import system

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return system.Context(0, torch.cuda.current_stream().cuda_stream)


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")


def split_dofs(p, U):
    primary, internal = system.element_node_split(p)
    return (primary[:, None] * U + np.arange(U)).ravel(), (internal[:, None] * U + np.arange(U)).ravel()


def schur(K, F, p, U):
    """S = K_bb - K_bi K_ii^-1 K_ib, g = F_b - K_bi K_ii^-1 F_i (F [Nd, R]) and cond_2(K_ii)"""
    b, i = split_dofs(p, U)
    if len(i) == 0:
        return K.copy(), F.copy(), 1.0
    Kii = K[np.ix_(i, i)]
    X = np.linalg.solve(Kii, np.concatenate([K[np.ix_(i, b)], F[i]], axis=1))
    return K[np.ix_(b, b)] - K[np.ix_(b, i)] @ X[:, :len(b)], F[b] - K[np.ix_(b, i)] @ X[:, len(b):], np.linalg.cond(Kii)


def tol(cond, K):
    return max(1e-12, 100 * cond * 2.0 ** -52) * np.abs(K).max()


LOCAL_CASES = [
    # kid, ne, p, value_order, R, kparams
    (system.KERNEL_DIFFUSION3D, 2, 1, 1, 1, [0.7, 1.3]),
    (system.KERNEL_DIFFUSION3D, 2, 2, 1, 2, [0.7, 1.3]),
    (system.KERNEL_DIFFUSION3D, (2, 1, 1), 3, 2, 3, [1.0, 0.5]),
    (system.KERNEL_DIFFUSION3D, (2, 1, 1), 4, 1, 1, [1.0, 1.0]),
    (system.KERNEL_DIFFUSION3D, (2, 1, 1), 6, 1, 1, [0.7, 1.3]),
    (system.KERNEL_DIFFUSION3D_VAR, (2, 1, 1), 3, 2, 2, None),
    (system.KERNEL_ADVDIFF3D, 2, 2, 1, 2, [0.7, 1.3, 0.5]),
]


@pytest.mark.parametrize("kid,ne,p,vo,R,kpar", LOCAL_CASES)
def test_condense_local_vs_numpy(ctx, kid, ne, p, vo, R, kpar):
    info = system.kernel_info(kid)
    U, NF = info["n_unknowns"], info["n_fields"]
    part = system.CubePartition(ne, p, perturb=0.15)
    nq = system.n_qps1d(p, vo)
    mesh = system.DeviceMesh(ctx, part, U)
    mf = system.MatrixFreeSystem(mesh, kid, kpar, asm_opts=(vo, 0, 0), n_rhs=R)
    fields = np.random.default_rng(2).uniform(-1, 1, (NF, part.n_local_nodes)) if NF else None
    if NF:
        mf.set_fields(dev(fields))
    S, G = mf.condense_local()
    S2, G2 = mf.condense_local()
    torch.cuda.synchronize()
    assert torch.equal(S, S2) and torch.equal(G, G2)  # bitwise reproducible
    assert torch.equal(S, S.transpose(1, 2))  # bitwise symmetric
    S, G = S.cpu().numpy(), G.cpu().numpy()
    if p == 1:
        K, Fe, _ = mf.local_assemble()
        assert np.array_equal(S, K.cpu().numpy()) and np.array_equal(G, Fe.cpu().numpy())
    for e in range(part.n_elems):
        nf = fields[:, part.elem_nodes[e]].T if NF else None
        K_ref, F_ref = O.assemble_local(kid, p, nq, R, part.elem_verts[e], nf, kpar)
        S_ref, g_ref, cond = schur(K_ref, F_ref, p, U)
        assert np.abs(S[e] - S_ref).max() <= tol(cond, K_ref)
        assert np.abs(G[e].T - g_ref).max() <= max(1e-12, 100 * cond * 2.0 ** -52) * max(1.0, np.abs(F_ref).max(), np.abs(K_ref).max())


def _global_ref(kid, p, nq, R, kpar, part, U, skip_mask=None):
    """dense Schur complement of the oracle-assembled global matrix over all internal dofs -> (S over all dofs, rhs, b, i)"""
    n = part.n_local_nodes * U
    A, rhs = np.zeros((n, n)), np.zeros((n, R))
    for e in range(part.n_elems):
        K, F = O.assemble_local(kid, p, nq, R, part.elem_verts[e], None, kpar)
        dofs = (part.elem_nodes[e].astype(np.int64)[:, None] * U + np.arange(U)).ravel()
        if skip_mask is not None:  # the rows / columns of Dirichlet dofs left out, as skip_dirichlet does
            keep = ~skip_mask[dofs].astype(bool)
            K = K * keep[:, None] * keep[None, :]
            F = F * keep[:, None]
        A[np.ix_(dofs, dofs)] += K
        rhs[dofs] += F
    _, internal = system.element_node_split(p)
    i = np.unique((part.elem_nodes[:, internal].astype(np.int64)[:, :, None] * U + np.arange(U)).ravel())
    b = np.setdiff1d(np.arange(n), i)
    full = np.zeros((n, n))
    g = np.zeros((n, R))
    if len(i):
        X = np.linalg.solve(A[np.ix_(i, i)], np.concatenate([A[np.ix_(i, b)], rhs[i]], axis=1))
        full[np.ix_(b, b)] = A[np.ix_(b, b)] - A[np.ix_(b, i)] @ X[:, :len(b)]
        g[b] = rhs[b] - A[np.ix_(b, i)] @ X[:, len(b):]
    return full, g, A, np.linalg.cond(A[np.ix_(i, i)]) if len(i) else 1.0


@pytest.mark.parametrize("ne,p", [(3, 2), (2, 4)])
def test_condense_global_vs_dense_schur(ctx, ne, p):
    import scipy.sparse as sp
    kid, U, R, kpar, vo = system.KERNEL_DIFFUSION3D, 4, 1, [0.7, 1.3], 1
    part = system.CubePartition(ne, p, perturb=0.15)
    nq = system.n_qps1d(p, vo)
    mask = part.dirichlet_mask(U)
    mesh = system.DeviceMesh(ctx, part, U, mask)
    mf = system.MatrixFreeSystem(mesh, kid, kpar, asm_opts=(vo, 0, 0), n_rhs=R)
    row_ptr, col_ind = system.condensed_graph(part.elem_nodes, p, U, np.arange(U))
    n = part.n_local_nodes * U
    RP, CI = torch.as_tensor(row_ptr, device="cuda"), torch.as_tensor(col_ind, device="cuda")
    Nd = (p + 1) ** 3 * U
    small = 2 * 3 * 8 * (Nd * Nd + Nd * R + 32 * Nd)  # about three elements per half: several sub-batches

    def run(skip):
        vals = torch.zeros(len(col_ind), dtype=torch.float64, device="cuda")
        rhs = torch.zeros((R, n), dtype=torch.float64, device="cuda")
        half = part.n_elems // 2
        assert mf.condense_global(RP, CI, vals, rhs, first=0, count=half, skip_dirichlet=skip, workspace_bytes=small) == 0
        assert mf.condense_global(RP, CI, vals, rhs, first=half, skip_dirichlet=skip) == 0
        torch.cuda.synchronize()
        return sp.csr_matrix((vals.cpu().numpy(), col_ind, row_ptr), shape=(n, n)).toarray(), rhs.cpu().numpy()

    for skip in (False, True):
        Sg, rhs = run(skip)
        S_ref, g_ref, A, cond = _global_ref(kid, p, nq, R, kpar, part, U, mask if skip else None)
        t = max(1e-12, 100 * cond * 2.0 ** -52) * np.abs(A).max()
        assert np.abs(Sg - S_ref).max() <= t
        assert np.abs(rhs.T - g_ref).max() <= t
        if not skip:
            Sg_plain, rhs_plain = Sg, rhs
    # the same as condense_local + condensed_graph scattered on the host
    S, G = mf.condense_local()
    S, G = S.cpu().numpy(), G.cpu().numpy()
    primary, _ = system.element_node_split(p)
    A_h, r_h = np.zeros((n, n)), np.zeros((n, R))
    for e in range(part.n_elems):
        bd = (part.elem_nodes[e, primary].astype(np.int64)[:, None] * U + np.arange(U)).ravel()
        A_h[np.ix_(bd, bd)] += S[e]
        r_h[bd] += G[e].T
    assert np.abs(A_h - Sg_plain).max() <= 1e-13 * np.abs(A_h).max()
    assert np.abs(r_h - rhs_plain.T).max() <= 1e-13 * max(1.0, np.abs(r_h).max())
    # graphs that lack entries: they are skipped and counted, once per (element, primary dof i, primary dof j) that lands on one
    # (no pivot fails here).  Every second entry removed from (1) the fourth non-empty row, (2) the u = 0 row of a node inside a
    # face between two elements: the row the node's one search runs in is then the sparse one, and the guesses it hands to the
    # rows u > 0 miss (device/csr_scatter.hpp), as in case (c) of test_graphs_where_the_shared_search_falls_back
    elem_dofs = (part.elem_nodes[:, primary].astype(np.int64)[:, :, None] * U + np.arange(U)).reshape(part.n_elems, -1)
    shared_by = np.bincount(part.elem_nodes[:, primary].ravel(), minlength=part.n_local_nodes)
    face_nodes = np.flatnonzero((shared_by == 2) & (part.node_boundary == 0))
    assert face_nodes.size > 0
    for thinned_row in (int(np.flatnonzero(np.diff(row_ptr))[3]), int(face_nodes[face_nodes.size // 2]) * U):
        keep = np.ones(len(col_ind), bool)
        keep[row_ptr[thinned_row]:row_ptr[thinned_row + 1]][::2] = False
        assert (~keep).sum() > 1
        rp2 = np.concatenate([[0], np.cumsum(keep)])[row_ptr].astype(np.int64)
        vals2 = torch.zeros(int(keep.sum()), dtype=torch.float64, device="cuda")
        missing = mf.condense_global(torch.as_tensor(rp2, device="cuda"), torch.as_tensor(col_ind[keep], device="cuda"), vals2)
        torch.cuda.synchronize()
        dropped = np.zeros((n, n), bool)
        dropped[thinned_row, col_ind[row_ptr[thinned_row]:row_ptr[thinned_row + 1]][::2]] = True
        assert missing == sum(int(dropped[np.ix_(d, d)].sum()) for d in elem_dofs), thinned_row
        A2 = sp.csr_matrix((vals2.cpu().numpy(), col_ind[keep], rp2), shape=(n, n)).toarray()
        assert np.abs(np.where(dropped, 0.0, Sg_plain) - A2).max() <= 1e-13 * np.abs(Sg_plain).max(), thinned_row


@pytest.mark.parametrize("ne,p", [(3, 2), (2, 4)])
def test_condensed_solve_and_recovery_match_full_solve(ctx, ne, p):
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla
    kid, U, R, kpar, vo = system.KERNEL_DIFFUSION3D, 4, 1, [0.7, 1.3], 1
    part = system.CubePartition(ne, p, perturb=0.15)
    mask = part.dirichlet_mask(U)
    mesh = system.DeviceMesh(ctx, part, U, mask)
    mf = system.MatrixFreeSystem(mesh, kid, kpar, asm_opts=(vo, 0, 0), n_rhs=R)
    n = part.n_local_nodes * U
    dmask = np.asarray(mask).astype(bool).ravel()[:n]
    gvals = np.where(dmask, np.sin(np.arange(n) * 0.37), 0.0)  # Dirichlet values

    def solve(row_ptr, col_ind, assemble):
        RP, CI = torch.as_tensor(row_ptr, device="cuda"), torch.as_tensor(col_ind, device="cuda")
        vals = torch.zeros(len(col_ind), dtype=torch.float64, device="cuda")
        rhs = torch.zeros((R, n), dtype=torch.float64, device="cuda")
        assert assemble(RP, CI, vals, rhs) == 0
        torch.cuda.synchronize()
        A = sp.csr_matrix((vals.cpu().numpy(), col_ind, row_ptr), shape=(n, n))
        f = rhs.cpu().numpy()[0] - A @ gvals  # Dirichlet columns eliminated on the host
        live = np.flatnonzero((np.diff(row_ptr) > 0) & ~dmask)
        x = gvals.copy()
        x[live] = spla.spsolve(A[live][:, live].tocsc(), f[live])
        return x

    x_full = solve(*_full_graph(part, U), lambda RP, CI, v, r: mf.assemble_global(RP, CI, v, r))
    x_c = solve(*system.condensed_graph(part.elem_nodes, p, U, np.arange(U)), lambda RP, CI, v, r: mf.condense_global(RP, CI, v, r))
    _, internal = system.element_node_split(p)
    i = np.unique((part.elem_nodes[:, internal].astype(np.int64)[:, :, None] * U + np.arange(U)).ravel())
    X = dev(np.where(np.isin(np.arange(n), i), np.nan, x_c)[None, :])  # (internal entries must all be overwritten)
    X2 = X.clone()
    mf.recover_internal(X)
    mf.recover_internal(X2)
    torch.cuda.synchronize()
    assert torch.equal(X, X2)  # bitwise reproducible
    x = X.cpu().numpy()[0]
    assert np.isfinite(x).all()
    assert np.linalg.norm(x - x_full) <= 1e-9 * np.linalg.norm(x_full)


def _full_graph(part, U):
    import scipy.sparse as sp
    dofs = (part.elem_nodes.astype(np.int64)[:, :, None] * U + np.arange(U)).reshape(part.n_elems, -1)
    nd = dofs.shape[1]
    n = part.n_local_nodes * U
    G = sp.coo_matrix((np.ones(part.n_elems * nd * nd), (np.repeat(dofs, nd, axis=1).ravel(), np.tile(dofs, (1, nd)).ravel())),
                      shape=(n, n)).tocsr()
    G.sort_indices()
    return G.indptr.astype(np.int64), G.indices.astype(np.int32)


NS3D_SOURCE_FILE = "ns3d.hpp"
ZERO_SOURCE = """
struct ZeroOperator
{
    static constexpr l3k::KernelParams params{.dimension = 3, .n_equations = 1, .n_unknowns = 1};

    template < typename In, typename Out >
    L3K_HD void operator()(const In&, Out& out) const
    {
        auto& [operators, rhs] = out;
        rhs[0]                 = 1.;
    }
};
"""


def test_plugin_u7_and_order8_vs_numpy(ctx):
    import os
    from l3ster_amd import plugin
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "kernels", NS3D_SOURCE_FILE)).read()
    kid = plugin.compile_kernel("NS3D", src, 1013, shapes=[(2, 4, 1), (4, 8, 1), (6, 12, 1)])  # (as test_ns3d_plugin.py: one library)
    cases = [(kid, 2, (1, 1, 0), system.CubePartition((2, 1, 1), 2, perturb=0.1)),
             (system.KERNEL_DIFFUSION3D, 8, (1, 0, 0), SingleElementMesh(8, HEX))]
    for k, p, opts, part in cases:
        info = system.kernel_info(k)
        U, NF = info["n_unknowns"], info["n_fields"]
        mesh = system.DeviceMesh(ctx, part, U)
        mf = system.MatrixFreeSystem(mesh, k, None if NF else [0.7, 1.3], asm_opts=opts)
        if NF:
            mf.set_fields(dev(np.random.default_rng(3).uniform(0.5, 1.0, (NF, part.n_local_nodes))))
        K, Fe, _ = mf.local_assemble()
        S, G = mf.condense_local()
        torch.cuda.synchronize()
        assert torch.equal(S, S.transpose(1, 2))
        K, Fe, S, G = K.cpu().numpy(), Fe.cpu().numpy(), S.cpu().numpy(), G.cpu().numpy()
        for e in range(part.n_elems):
            S_ref, g_ref, cond = schur(K[e], Fe[e].T, p, U)
            assert np.abs(S[e] - S_ref).max() <= tol(cond, K[e]), (k, p)
            assert np.abs(G[e].T - g_ref).max() <= tol(cond, K[e]) + 1e-12 * np.abs(Fe[e]).max(), (k, p)


def test_errors(ctx):
    import ctypes as C
    lib = system.capi.load()
    # quads
    quad = system.SquarePartition(3, 2)
    qmf = system.MatrixFreeSystem(system.DeviceMesh(ctx, quad, 3), system.KERNEL_DIFFUSION2D)
    buf = torch.zeros(1 << 16, dtype=torch.float64, device="cuda")
    idx32 = torch.zeros(16, dtype=torch.int32, device="cuda")
    idx64 = torch.zeros(16, dtype=torch.int64, device="cuda")
    bp = C.c_void_p(buf.data_ptr())
    for rc in (lib.l3k_condense_local(qmf._h, 0, 1, bp, None),
               lib.l3k_condense_global(qmf._h, 0, 1, C.c_void_p(idx64.data_ptr()), C.c_void_p(idx32.data_ptr()), bp, None, 0, 0, 0, None),
               lib.l3k_condensed_recover(qmf._h, 0, 1, bp, 1 << 16)):
        assert rc < 0 and "quads" in lib.l3k_last_error().decode()
    # ranges and null arguments
    part = system.CubePartition(2, 2)
    mf = system.MatrixFreeSystem(system.DeviceMesh(ctx, part, 4), system.KERNEL_DIFFUSION3D, [1.0, 1.0])
    with pytest.raises(system.L3KError, match="outside"):
        mf.condense_local(first=5, count=4)
    with pytest.raises(system.L3KError, match="outside"):
        mf.recover_internal(torch.zeros((1, part.n_local_nodes * 4), dtype=torch.float64, device="cuda"), first=-1, count=1)
    assert lib.l3k_condense_global(mf._h, 0, 1, None, None, bp, None, 0, 0, 0, None) == -1
    assert lib.l3k_condensed_recover(mf._h, 0, 1, None, 1 << 16) == -1
    assert lib.l3k_condense_local(None, 0, 1, bp, None) == -1
    # a degenerate element: the existing message
    bad = HEX.copy()
    bad[[0, 1]] = bad[[1, 0]]
    dmf = system.MatrixFreeSystem(system.DeviceMesh(ctx, SingleElementMesh(2, bad), 4), system.KERNEL_DIFFUSION3D)
    with pytest.raises(system.L3KError, match="degenerate"):
        dmf.condense_local()
    # K_e = 0: the pivot error, and no NaN in the global system
    from l3ster_amd import plugin
    zid = plugin.compile_kernel("ZeroOperator", ZERO_SOURCE, 1077, shapes=[(2, 3, 1)])
    part = system.CubePartition(2, 2)
    zmf = system.MatrixFreeSystem(system.DeviceMesh(ctx, part, 1), zid)
    rp, ci = system.condensed_graph(part.elem_nodes, 2, 1, [0])
    vals = torch.zeros(len(ci), dtype=torch.float64, device="cuda")
    rhs = torch.zeros((1, part.n_local_nodes), dtype=torch.float64, device="cuda")
    with pytest.raises(system.L3KError, match="non-positive pivot in the element-internal block"):
        zmf.condense_global(torch.as_tensor(rp, device="cuda"), torch.as_tensor(ci, device="cuda"), vals, rhs)
    torch.cuda.synchronize()
    assert torch.isfinite(vals).all() and torch.isfinite(rhs).all()
    with pytest.raises(system.L3KError, match="non-positive pivot"):
        zmf.condense_local()


# Diffusion3D (k = 0.7) with a source per right-hand side: the built-in kernel fills column 0 only
SOURCES = (1.0, -2.5, 0.75)
SOURCES_SOURCE = """
struct Diffusion3DSources
{
    static constexpr l3k::KernelParams params{.dimension = 3, .n_equations = 7, .n_unknowns = 4};

    template < typename In, typename Out >
    L3K_HD void operator()(const In&, Out& out) const
    {
        constexpr double k = 0.7, s[3] = {%r, %r, %r};
        auto& [operators, rhs] = out;
        auto& [A0, Ax, Ay, Az] = operators;
        Ax(0, 1) = -k;
        Ay(0, 2) = -k;
        Az(0, 3) = -k;
        for (int r = 0; r < rhs.cols() && r < 3; ++r)
            rhs(0, r) = s[r];
        A0(1, 1) = -1.;
        Ax(1, 0) = 1.;
        A0(2, 2) = -1.;
        Ay(2, 0) = 1.;
        A0(3, 3) = -1.;
        Az(3, 0) = 1.;
        Ay(4, 3) = 1.;
        Az(4, 2) = -1.;
        Ax(5, 3) = -1.;
        Az(5, 1) = 1.;
        Ax(6, 2) = 1.;
        Ay(6, 1) = -1.;
    }
};
""" % SOURCES


@pytest.fixture(scope="module")
def sources_kid():
    from l3ster_amd import plugin
    return plugin.compile_kernel("Diffusion3DSources", SOURCES_SOURCE, 1078, shapes=[(2, 3, 3), (3, 4, 3), (4, 5, 3)])


def _sources_case(ctx, kid, p, ne=(3, 2, 1)):
    """the three-column system on a perturbed mesh, X [3, n] with three different random columns on the primary dofs and NaN on the
    internal ones, and the internal dofs' indices"""
    U, R = 4, 3
    part = system.CubePartition(ne, p, perturb=0.15)
    mf = system.MatrixFreeSystem(system.DeviceMesh(ctx, part, U), kid, asm_opts=(1, 0, 0), n_rhs=R)
    n = part.n_local_nodes * U
    _, internal = system.element_node_split(p)
    i_all = np.unique((part.elem_nodes[:, internal].astype(np.int64)[:, :, None] * U + np.arange(U)).ravel())
    x = np.random.default_rng(p).uniform(-1, 1, (R, n))
    x[:, i_all] = np.nan
    return part, mf, x, i_all


@pytest.mark.parametrize("p", [2, 3, 4])
def test_recover_three_columns_vs_numpy(ctx, sources_kid, p):
    """l3k_condensed_recover with R = 3, per element and column against solve(K_ii, F_i - K_ib x_b) of the oracle's element systems
    (F_e is linear in the source: column r is SOURCES[r] times the oracle's F_e for s = 1).  The 4 (p - 1)^3 internal dofs are a single
    partial panel of 4 (p = 2), exactly one panel of 32 (p = 3), three panels and a partial one of 12 (p = 4).  The columns have
    different x_b and different F: a value kept in the kernel's xs[] from one column to the next shows.  Bound: the relative error of
    a Cholesky solve grows with cond(K_ii) eps -- the factor of tol(), the bound the Schur complement is held to, on the scale of
    the solution."""
    U, R = 4, 3
    part, mf, x, i_all = _sources_case(ctx, sources_kid, p)
    nq = system.n_qps1d(p, 1)
    assert len(i_all) == part.n_elems * 4 * (p - 1) ** 3
    X = dev(x)
    X2 = X.clone()
    mf.recover_internal(X)
    mf.recover_internal(X2)
    torch.cuda.synchronize()
    assert torch.equal(X, X2)  # bitwise reproducible (no NaN is left: every internal dof is overwritten)
    got = X.cpu().numpy()
    assert np.isfinite(got).all()
    prim = np.setdiff1d(np.arange(x.shape[1]), i_all)
    assert np.array_equal(got[:, prim], x[:, prim])  # the primary dofs are read only
    b, i = split_dofs(p, U)
    for e in range(part.n_elems):
        K_ref, F1 = O.assemble_local(system.KERNEL_DIFFUSION3D, p, nq, 1, part.elem_verts[e], None, [0.7, 1.0])
        F_ref = F1[:, :1] * np.asarray(SOURCES)[None, :]
        dofs = (part.elem_nodes[e].astype(np.int64)[:, None] * U + np.arange(U)).ravel()
        Kii = K_ref[np.ix_(i, i)]
        x_ref = np.linalg.solve(Kii, F_ref[i] - K_ref[np.ix_(i, b)] @ x[:, dofs[b]].T)  # [Ni, R]
        assert np.abs(x_ref[:, 0] - x_ref[:, 1]).max() > 1e-3 and np.abs(x_ref[:, 1] - x_ref[:, 2]).max() > 1e-3
        bound = tol(np.linalg.cond(Kii), np.append(x_ref.ravel(), 1.0))
        for r in range(R):
            assert np.abs(got[r, dofs[i]] - x_ref[:, r]).max() <= bound, (e, r)


@pytest.mark.parametrize("p", [3, 4])
def test_sub_ranges_equal_slices_of_the_full_range(ctx, sources_kid, p):
    """condense_local(first, count) and recover_internal(first=, count=) over a strict sub-range: bit for bit the slices of the
    full-range call; recovery leaves the internal dofs of the elements outside the range alone"""
    U = 4
    part, mf, x, i_all = _sources_case(ctx, sources_kid, p)
    first, count = 2, 3
    assert 0 < first and first + count < part.n_elems
    S, G = mf.condense_local()
    Ss, Gs = mf.condense_local(first=first, count=count)
    torch.cuda.synchronize()
    assert Ss.shape[0] == count and Gs.shape[0] == count
    assert torch.equal(Ss, S[first:first + count]) and torch.equal(Gs, G[first:first + count])
    X_full, X_sub = dev(x), dev(x)
    mf.recover_internal(X_full)
    mf.recover_internal(X_sub, first=first, count=count)
    torch.cuda.synchronize()
    full, sub = X_full.cpu().numpy(), X_sub.cpu().numpy()
    _, internal = system.element_node_split(p)
    in_range = np.zeros(x.shape[1], bool)
    in_range[(part.elem_nodes[first:first + count][:, internal].astype(np.int64)[:, :, None] * U + np.arange(U)).ravel()] = True
    outside = np.setdiff1d(i_all, np.flatnonzero(in_range))
    assert len(outside) == (part.n_elems - count) * 4 * (p - 1) ** 3
    assert np.isnan(sub[:, outside]).all()  # untouched
    assert np.isfinite(full).all() and np.array_equal(sub[:, in_range], full[:, in_range])
    prim = np.setdiff1d(np.arange(x.shape[1]), i_all)
    assert np.array_equal(sub[:, prim], x[:, prim])


# grad u . grad v + u v with the source 1 where x >= 0.34, nothing (K_e = 0, F_e = 0) where x < 0.34
HALF_SPACE_X = 0.34
HALF_SPACE_SOURCE = """
struct HalfSpaceOperator
{
    static constexpr l3k::KernelParams params{.dimension = 3, .n_equations = 4, .n_unknowns = 1};

    template < typename In, typename Out >
    L3K_HD void operator()(const In& in, Out& out) const
    {
        auto& [operators, rhs] = out;
        auto& [A0, Ax, Ay, Az] = operators;
        if (in.point.space.x() < %r)
            return;
        Ax(0, 0) = 1.;
        Ay(1, 0) = 1.;
        Az(2, 0) = 1.;
        A0(3, 0) = 1.;
        rhs[3]   = 1.;
    }
};
""" % HALF_SPACE_X


def test_one_failing_column_of_elements_among_healthy_ones(ctx):
    """An operator that vanishes on the elements of the first of three element layers in x (all their quadrature points have
    x < 1/3 < 0.34 < the first quadrature point of the next layer, 1/3 + 0.113 / 3): those elements stop at their first pivot,
    l3k_condense_global reports it, and the global system holds the healthy elements' contributions only -- finite, exactly zero in
    the rows and columns that only failed elements touch, the dense Schur complement of the healthy elements elsewhere.  The
    reference element systems are the tensor products of the oracle's 1-D tables on the (undistorted) box elements."""
    import scipy.sparse as sp
    from l3ster_amd import plugin
    p, U, R = 2, 1, 1
    kid = plugin.compile_kernel("HalfSpaceOperator", HALF_SPACE_SOURCE, 1079, shapes=[(2, 3, 1)])
    ne = (3, 2, 2)
    part = system.CubePartition(ne, p)
    nq = system.n_qps1d(p, 1)
    centre_x = part.elem_verts[:, :, 0].mean(axis=1)
    failed = centre_x < 1 / 3
    assert failed.sum() == 4 and (~failed).sum() == 8
    assert part.elem_verts[failed][:, :, 0].max() < HALF_SPACE_X < 1 / 3 + (1 - np.sqrt(0.6)) / 6
    mf = system.MatrixFreeSystem(system.DeviceMesh(ctx, part, U), kid)
    n = part.n_local_nodes
    rp, ci = system.condensed_graph(part.elem_nodes, p, U, [0])
    vals = torch.zeros(len(ci), dtype=torch.float64, device="cuda")
    rhs = torch.zeros((R, n), dtype=torch.float64, device="cuda")
    with pytest.raises(system.L3KError, match="non-positive pivot in the element-internal block"):
        mf.condense_global(torch.as_tensor(rp, device="cuda"), torch.as_tensor(ci, device="cuda"), vals, rhs)
    torch.cuda.synchronize()
    assert torch.isfinite(vals).all() and torch.isfinite(rhs).all()
    Sg = sp.csr_matrix((vals.cpu().numpy(), ci, rp), shape=(n, n)).toarray()
    g = rhs.cpu().numpy()[0]
    # the element systems of a box with edges h: 1-D mass and stiffness matrices from the oracle's basis and Gauss rule
    I1, D1 = O.basis_1d(p, nq)
    _, w = O.gl_rule(nq)
    M1, S1, m1 = (I1 * w) @ I1.T, (D1 * w) @ D1.T, I1 @ w
    k3 = lambda az, ay, ax: np.kron(az, np.kron(ay, ax))  # node ix + n iy + n^2 iz
    h = 1.0 / np.asarray(ne)
    jac = np.prod(h / 2)
    K_box = jac * (k3(M1, M1, S1) * (2 / h[0]) ** 2 + k3(M1, S1, M1) * (2 / h[1]) ** 2 + k3(S1, M1, M1) * (2 / h[2]) ** 2 + k3(M1, M1, M1))
    F_box = jac * np.kron(m1, np.kron(m1, m1))
    A, f = np.zeros((n, n)), np.zeros(n)
    for e in np.flatnonzero(~failed):
        assert np.allclose(np.ptp(part.elem_verts[e], axis=0), h)
        d = part.elem_nodes[e].astype(np.int64)
        A[np.ix_(d, d)] += K_box
        f[d] += F_box
    _, internal = system.element_node_split(p)
    i = np.unique(part.elem_nodes[~failed][:, internal].astype(np.int64).ravel())
    touched = np.zeros(n, bool)
    touched[part.elem_nodes[~failed].ravel()] = True
    only_failed = ~touched
    assert only_failed.sum() > 0 and len(i) == 8
    b = np.setdiff1d(np.flatnonzero(touched), i)
    S_ref, g_ref = np.zeros((n, n)), np.zeros(n)
    X = np.linalg.solve(A[np.ix_(i, i)], np.concatenate([A[np.ix_(i, b)], f[i, None]], axis=1))
    S_ref[np.ix_(b, b)] = A[np.ix_(b, b)] - A[np.ix_(b, i)] @ X[:, :len(b)]
    g_ref[b] = f[b] - A[np.ix_(b, i)] @ X[:, -1]
    assert not Sg[only_failed].any() and not Sg[:, only_failed].any() and not g[only_failed].any()  # exactly zero
    assert np.abs(Sg[np.ix_(b, b)]).max() > 0.01
    t = max(1e-12, 100 * np.linalg.cond(A[np.ix_(i, i)]) * 2.0 ** -52) * np.abs(A).max()  # (test_condense_global_vs_dense_schur)
    assert np.abs(Sg - S_ref).max() <= t
    assert np.abs(g - g_ref).max() <= t
    # the local route names the same error
    with pytest.raises(system.L3KError, match="non-positive pivot"):
        mf.condense_local()


def test_condense_global_after_a_degenerate_sub_batch(ctx):
    """l3k_condense_global leaves nothing behind when a call fails: 27 elements, about three per half, element 20 -- sub-batch 6 --
    degenerate.  The sums of the clean range [0, 18) before and after the failing call, through the same two halves, agree to the
    rounding of the atomic adds (1e-12 of the largest value), and no entry misses the graph."""
    U, p, R = 4, 2, 1
    part = cube_with_inverted_element()
    mf = system.MatrixFreeSystem(system.DeviceMesh(ctx, part, U), system.KERNEL_DIFFUSION3D)
    row_ptr, col_ind = system.condensed_graph(part.elem_nodes, p, U, np.arange(U))
    n = part.n_local_nodes * U
    RP, CI = torch.as_tensor(row_ptr, device="cuda"), torch.as_tensor(col_ind, device="cuda")
    Nd = (p + 1) ** 3 * U
    small = 2 * 3 * 8 * (Nd * Nd + Nd * R + 32 * Nd)

    def run(count):
        vals = torch.zeros(len(col_ind), dtype=torch.float64, device="cuda")
        rhs = torch.zeros((R, n), dtype=torch.float64, device="cuda")
        missing = mf.condense_global(RP, CI, vals, rhs, first=0, count=count, workspace_bytes=small)
        torch.cuda.synchronize()
        return vals, rhs, missing

    v0, r0, m0 = run(18)
    with pytest.raises(system.L3KError, match="degenerate"):
        run(part.n_elems)
    v1, r1, m1 = run(18)
    assert m0 == 0 and m1 == 0
    assert float(v0.abs().amax()) > 0
    assert float((v1 - v0).abs().amax()) <= 1e-12 * float(v0.abs().amax())
    assert float((r1 - r0).abs().amax()) <= 1e-12 * max(1.0, float(r0.abs().amax()))
