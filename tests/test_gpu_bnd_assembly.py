"""Boundary equation kernels in the assembled and condensed paths on the device (hexes): the side element matrices of
l3k_bnd_local_assemble against the oracle's assembleLocalSystem on a side, the standalone global sum against the matrix-free
boundary term, the switch l3k_mf_assemble_boundary at element and mesh level, and three solves (matrix-free, assembled, condensed)
of one problem with a Robin wall.

Tolerances: entrywise 1e-12 max|K| against the oracle at element level, relative L2 <= 1e-11 at mesh level.  The
solves agree within the perturbation bound of test_gpu_csr_solve.py, ||x - y|| / ||y|| <= cond(A) (res(x) + res(y) + n EPS), every
residual taken in the dense copy of the assembled system with the switch on."""
import ctypes as C

import numpy as np
import pytest
import torch

import helpers
import oracle_lib as O
from cg_ref import EPS, LD
from l3ster_amd import solve, system

pytestmark = pytest.mark.gpu
U = 4
DIFF, DIFF_PAR = system.KERNEL_DIFFUSION3D, [0.7, 1.3]
HEXM = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [0, 0, 1], [1, 0, 1.5], [0, 1, 1.5], [1, 1, 2]], float)
KERNELS = {  # device id, oracle id, non-default parameters
    "robin": (system.KERNEL_ROBIN3D, O.KERNEL_ROBIN3D, [2.0, 0.7]),
    "normalflux": (system.KERNEL_NORMALFLUX3D, O.KERNEL_NORMALFLUX3D, [2.0, 0.7, 0.3]),
    "robinpoint": (system.KERNEL_ROBINPOINT3D, O.KERNEL_ROBINPOINT3D, [1.5, 0.4]),
    "adiabatic": (system.KERNEL_ADIABATIC3D, O.KERNEL_ADIABATIC3D, None),
}


@pytest.fixture(scope="module")
def ctx():
    torch.cuda.set_device(0)
    return system.Context(0, torch.cuda.current_stream().cuda_stream)


def dev(a, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(np.asarray(b)))


def check_side_systems(K, F, sides, okid, p, nq, R, verts_of, kp, t=0.0):
    """K [n, Nd, Nd], F [n, R, Nd] (numpy) against the oracle on (verts_of(i), sides[i]); returns the largest errors / scale"""
    worst = 0.0
    for i, s in enumerate(sides):
        K_ref, F_ref = O.assemble_local_side(int(s), okid, p, nq, R, verts_of(i), None, kp, time=t)
        ek, ef = np.abs(K[i] - K_ref).max() / np.abs(K_ref).max(), np.abs(F[i].T - F_ref).max() / max(1.0, np.abs(F_ref).max())
        worst = max(worst, ek, ef)
        assert ek <= 1e-12, (i, s, ek)
        assert ef <= 1e-12, (i, s, ef)
    return worst


# ------------------------------------------------------------------------------------------- 1. one element against the oracle
ONE_ELEMENT = [(k, p, vo, R, range(6)) for k, p, vo, R in [
    ("robin", 1, 1, 1), ("robin", 2, 1, 1), ("robin", 2, 1, 2), ("robin", 3, 2, 1), ("robin", 4, 1, 1),
    ("normalflux", 2, 1, 1), ("normalflux", 2, 1, 2), ("normalflux", 3, 2, 1), ("normalflux", 4, 1, 1),
    ("robinpoint", 2, 1, 1), ("robinpoint", 4, 1, 1)]] + [("adiabatic", 6, 1, 1, (1, 4))]


@pytest.mark.parametrize("hexname", ["K1", "mapping"])
@pytest.mark.parametrize("kernel,p,vo,R,sides", ONE_ELEMENT, ids=[f"{k}-p{p}-vo{vo}-R{R}" for k, p, vo, R, _ in ONE_ELEMENT])
def test_one_element_vs_oracle(ctx, kernel, p, vo, R, sides, hexname):
    verts = helpers.HEX if hexname == "K1" else HEXM
    kid, okid, kp = KERNELS[kernel]
    t = 0.3 if kernel == "robinpoint" else 0.0
    nq = system.n_qps1d(p, vo, 0)
    assert (p, nq) in {(1, 2), (2, 3), (3, 7), (4, 5), (6, 7)}
    sides = list(sides)
    mesh = system.DeviceMesh(ctx, helpers.SingleElementMesh(p, verts), U)
    term = system.BoundaryTerm(mesh, kid, [0] * len(sides), sides, kernel_params=kp, asm_opts=(vo, 0, 0), n_rhs=R)
    term.set_time(t)
    K, F = term.local_assemble()
    K2, F2 = term.local_assemble()
    torch.cuda.synchronize()
    Nd = (p + 1) ** 3 * U
    assert K.shape == (len(sides), Nd, Nd) and F.shape == (len(sides), R, Nd)
    assert torch.equal(K, K.transpose(1, 2))  # bitwise symmetric
    assert torch.equal(K, K2) and torch.equal(F, F2)  # a second call gives the same bits
    Kh, Fh = K.cpu().numpy(), F.cpu().numpy()
    assert all(np.array_equal(Kh[i], Kh[i].T) for i in range(len(sides)))
    worst = check_side_systems(Kh, Fh, sides, okid, p, nq, R, lambda i: verts, kp, t)
    print(f"{kernel} p {p} nq {nq} R {R} on {hexname}: worst entrywise error / scale {worst:.2e}")
    # either output may be left out, and the other one keeps its bits
    K3, none = term.local_assemble(want_F=False)
    none2, F3 = term.local_assemble(want_K=False)
    assert none is None and none2 is None and torch.equal(K3, K) and torch.equal(F3, F)


# ------------------------------------------------------------------------------------------- 2. sub-ranges, order of the list
def test_subranges_and_list_order(ctx):
    p, nq = 2, 3
    part = system.CubePartition((3, 2, 2), p, perturb=0.15)
    fe, fs = part.boundary_sides()
    perm = np.random.default_rng(5).permutation(len(fe))
    fe, fs = fe[perm], fs[perm]
    assert (np.diff(fe) < 0).any() and len(fe) == 32
    kid, okid, kp = KERNELS["normalflux"]
    term = system.BoundaryTerm(system.DeviceMesh(ctx, part, U), kid, fe, fs, kernel_params=kp)
    K, F = term.local_assemble()
    Ks, Fs = term.local_assemble(first=5, count=7)
    torch.cuda.synchronize()
    assert torch.equal(Ks, K[5:12]) and torch.equal(Fs, F[5:12])
    check_side_systems(K.cpu().numpy(), F.cpu().numpy(), fs, okid, p, nq, 1, lambda i: part.elem_verts[fe[i]], kp)
    Ke, Fe = term.local_assemble(first=len(fe), count=0)
    assert Ke.shape[0] == 0 and Fe.shape[0] == 0


# ------------------------------------------------------------------------------------------- 3. the standalone global sum
def dense_of(row_ptr, col_ind, vals, n):
    import scipy.sparse as sp
    return sp.csr_matrix((vals.cpu().numpy(), col_ind.cpu().numpy(), row_ptr.cpu().numpy()), shape=(n, n)).toarray()


def split_apply(term, part, X):
    """term.apply on a local vector X (ncols, n_local_dofs): owned rows | ghost rows"""
    no = part.n_owned_nodes * U
    Y = torch.zeros_like(X)
    for c in range(X.shape[0]):  # (the term has one right-hand side: column by column)
        x, y = X[c:c + 1], Y[c:c + 1]
        if part.n_ghost_nodes:
            term.apply(x[:, :no], y[:, :no], XG=x[:, no:], YG=y[:, no:])
        else:
            term.apply(x, y)
    return Y


@pytest.mark.parametrize("p,parts", [(2, (1, 1, 1)), (4, (1, 1, 1)), (2, (2, 1, 1))])
def test_standalone_global_sum_vs_matrix_free_term(ctx, p, parts):
    nq = p + 1
    part = system.CubePartition((3, 2, 2), p, parts=parts, rank=parts[0] - 1, perturb=0.15)  # (the last rank has the ghosts)
    assert (part.n_ghost_nodes > 0) == (parts != (1, 1, 1))
    mask = part.dirichlet_mask(U, unknowns=(0,), sides=(2, 5))
    mesh = system.DeviceMesh(ctx, part, U, mask)
    mf = system.MatrixFreeSystem(mesh, DIFF, DIFF_PAR)
    g = mf.sparsity_graph()
    n = part.n_local_nodes * U
    assert g.n == n
    fe, fs = part.boundary_sides()
    perm = np.random.default_rng(6).permutation(len(fe))
    fe, fs = fe[perm], fs[perm]
    kid, okid, kp = KERNELS["normalflux"]
    term = system.BoundaryTerm(mesh, kid, fe, fs, kernel_params=kp)
    vals = torch.zeros(g.col_ind.numel(), dtype=torch.float64, device="cuda")
    rhs = torch.zeros((1, n), dtype=torch.float64, device="cuda")
    assert term.assemble_global(g.row_ptr, g.col_ind, vals, rhs, skip_dirichlet=True) == 0  # n_missing
    op = system.CsrOperator(ctx, g.row_ptr, g.col_ind, vals)
    X = dev(np.random.default_rng(7).standard_normal((2, n)))
    Yc = torch.empty_like(X)
    op.apply(X, Yc)
    Ym = split_apply(term, part, X)
    torch.cuda.synchronize()
    err = rel(Yc.cpu().numpy(), Ym.cpu().numpy())
    print(f"p {p} parts {parts}: CSR of the side systems against the matrix-free term {err:.2e}")
    assert err <= 1e-11
    # the rhs against the term's own (no Dirichlet values) on the free dofs
    no = part.n_owned_nodes * U
    diag, r2 = torch.zeros(n, dtype=torch.float64, device="cuda"), torch.zeros((1, n), dtype=torch.float64, device="cuda")
    if part.n_ghost_nodes:
        term.diag_rhs(diag[:no], r2[:, :no], diag_ghost=diag[no:], rhs_ghost=r2[:, no:])
    else:
        term.diag_rhs(diag, r2)
    free = mask == 0
    assert rel(rhs.cpu().numpy()[0][free], r2.cpu().numpy()[0][free]) <= 1e-11
    assert not rhs.cpu().numpy()[0][~free].any()
    assert rel(op.diag().cpu().numpy()[free], diag.cpu().numpy()[free]) <= 1e-11
    # a sub-range plus the rest is the whole (additive), in two calls and with a small workspace (several sub-batches)
    v2 = torch.zeros_like(vals)
    Nd = (p + 1) ** 3 * U
    small = 2 * 3 * 8 * (Nd * Nd + Nd + nq * nq * 17)  # three sides per half
    cut = len(fe) // 3
    assert cut > 3
    assert term.assemble_global(g.row_ptr, g.col_ind, v2, None, first=0, count=cut, skip_dirichlet=True, workspace_bytes=small) == 0
    assert term.assemble_global(g.row_ptr, g.col_ind, v2, None, first=cut, skip_dirichlet=True, workspace_bytes=small) == 0
    assert float((v2 - vals).abs().max()) <= 1e-12 * float(vals.abs().max())
    if p == 2:
        # all entries: the dense matrix against the host sum of the oracle's K_s over the listed sides
        v3 = torch.zeros_like(vals)
        assert term.assemble_global(g.row_ptr, g.col_ind, v3, None, skip_dirichlet=False) == 0
        A = dense_of(g.row_ptr, g.col_ind, v3, n)
        A_ref = np.zeros((n, n))
        for e, s in zip(fe, fs):
            K_ref, _ = O.assemble_local_side(int(s), okid, p, nq, 1, part.elem_verts[e], None, kp)
            dofs = (part.elem_nodes[e].astype(np.int64)[:, None] * U + np.arange(U)).ravel()
            A_ref[np.ix_(dofs, dofs)] += K_ref
        assert rel(A, A_ref) <= 1e-11
        # a graph without the rows of one node: its entries are counted, the others summed
        drop_node = int(part.elem_nodes[fe[0]][0])
        row_ptr, col_ind, _ = helpers.csr_graph(part, U, range(U), drop=lambda r, c: (r // U == drop_node) | (c // U == drop_node))
        RP, CI = dev(row_ptr, torch.int64), dev(col_ind, torch.int32)
        v4 = torch.zeros(len(col_ind), dtype=torch.float64, device="cuda")
        nm = term.assemble_global(RP, CI, v4, None)
        Nd, want = 27 * U, 0
        for e in fe:  # per side: the entries of the rows and columns of the dropped node's dofs
            k = U * int((part.elem_nodes[e] == drop_node).sum())
            want += Nd * Nd - (Nd - k) * (Nd - k)
        assert nm == want > 0


# ------------------------------------------------------------------------------------------- 4. the switch, element level
def two_terms(mesh, part, p, n_rhs=1):
    """Robin3D on the cube sides 0-3 and NormalFlux3D on 4-5 (order 1: Robin3D on all six), with their oracle descriptions"""
    kid_r, okid_r, kp_r = KERNELS["robin"]
    kid_n, okid_n, kp_n = KERNELS["normalflux"]
    if p == 1:
        lists = [(kid_r, okid_r, kp_r, part.boundary_sides(range(6)))]
    else:
        lists = [(kid_r, okid_r, kp_r, part.boundary_sides([0, 1, 2, 3])), (kid_n, okid_n, kp_n, part.boundary_sides([4, 5]))]
    terms = [system.BoundaryTerm(mesh, kid, fe, fs, kernel_params=kp, n_rhs=n_rhs) for kid, _, kp, (fe, fs) in lists]
    return terms, lists


def oracle_element_systems(part, p, lists, R=1):
    nq = p + 1
    out = []
    for e in range(part.n_elems):
        K, F = O.assemble_local(O.KERNEL_DIFFUSION3D, p, nq, R, part.elem_verts[e], None, DIFF_PAR)
        for _, okid, kp, (fe, fs) in lists:
            for s in fs[fe == e]:
                Ks, Fs = O.assemble_local_side(int(s), okid, p, nq, R, part.elem_verts[e], None, kp)
                K, F = K + Ks, F + Fs
        out.append((K, F))
    return out


def schur(K, F, p):
    """S = K_bb - K_bi K_ii^-1 K_ib, g = F_b - K_bi K_ii^-1 F_i (F [Nd, R]) and cond_2(K_ii), as test_gpu_condensation.py"""
    primary, internal = system.element_node_split(p)
    b, i = (primary[:, None] * U + np.arange(U)).ravel(), (internal[:, None] * U + np.arange(U)).ravel()
    if len(i) == 0:
        return K.copy(), F.copy(), 1.0
    Kii = K[np.ix_(i, i)]
    X = np.linalg.solve(Kii, np.concatenate([K[np.ix_(i, b)], F[i]], axis=1))
    return K[np.ix_(b, b)] - K[np.ix_(b, i)] @ X[:, :len(b)], F[b] - K[np.ix_(b, i)] @ X[:, len(b):], np.linalg.cond(Kii)


def schur_tol(cond, K):
    return max(1e-12, 100 * cond * 2.0 ** -52) * np.abs(K).max()


@pytest.mark.parametrize("p", [1, 2, 4])
def test_switch_element_level(ctx, p):
    part = system.CubePartition(2, p, perturb=0.15)
    mesh = system.DeviceMesh(ctx, part, U)
    mf, bare = system.MatrixFreeSystem(mesh, DIFF, DIFF_PAR), system.MatrixFreeSystem(mesh, DIFF, DIFF_PAR)
    terms, lists = two_terms(mesh, part, p)
    assert all(sum(int((fe == e).sum()) for _, _, _, (fe, _) in lists) == 3 for e in range(part.n_elems))  # corner elements
    for t in terms:
        mf.attach_boundary(t)
    K0, F0, _ = mf.local_assemble()  # switch off, terms attached: the system without terms, bit for bit
    Kb, Fb, _ = bare.local_assemble()
    assert torch.equal(K0, Kb) and torch.equal(F0, Fb)
    mf.assemble_boundary()
    K, F, _ = mf.local_assemble()
    K2, F2, _ = mf.local_assemble()
    torch.cuda.synchronize()
    assert torch.equal(K, K2) and torch.equal(F, F2)
    assert torch.equal(K, K.transpose(1, 2))
    Ks, Fs, _ = mf.local_assemble(first=3, count=4)
    assert torch.equal(Ks, K[3:7]) and torch.equal(Fs, F[3:7])
    Kh, Fh = K.cpu().numpy(), F.cpu().numpy()
    ref = oracle_element_systems(part, p, lists)
    worst = 0.0
    for e, (K_ref, F_ref) in enumerate(ref):
        ek, ef = np.abs(Kh[e] - K_ref).max() / np.abs(K_ref).max(), np.abs(Fh[e].T - F_ref).max() / max(1.0, np.abs(F_ref).max())
        worst = max(worst, ek, ef)
        assert ek <= 1e-12 and ef <= 1e-12, (e, ek, ef)
    assert float((K - K0).abs().max()) > 1e-3 * float(K0.abs().max())
    print(f"p {p}: K_e + sum K_s against the oracle, worst entrywise error / scale {worst:.2e}")
    # condensation forms its element systems through the same call
    S, G = mf.condense_local()
    S2, G2 = mf.condense_local()
    torch.cuda.synchronize()
    assert torch.equal(S, S2) and torch.equal(G, G2) and torch.equal(S, S.transpose(1, 2))
    S, G = S.cpu().numpy(), G.cpu().numpy()
    for e in range(part.n_elems):
        S_ref, g_ref, cond = schur(Kh[e], Fh[e].T, p)
        assert np.abs(S[e] - S_ref).max() <= schur_tol(cond, Kh[e])
        assert np.abs(G[e].T - g_ref).max() <= max(1e-12, 100 * cond * 2.0 ** -52) * max(1.0, np.abs(Fh[e]).max(), np.abs(Kh[e]).max())
    mf.assemble_boundary(False)
    K3, F3, _ = mf.local_assemble()
    assert torch.equal(K3, Kb) and torch.equal(F3, Fb)


def test_switch_leaves_interior_elements_alone(ctx):
    p = 2
    part = system.CubePartition(3, p, perturb=0.15)
    mesh = system.DeviceMesh(ctx, part, U)
    mf = system.MatrixFreeSystem(mesh, DIFF, DIFF_PAR)
    terms, lists = two_terms(mesh, part, p)
    for t in terms:
        mf.attach_boundary(t)
    K0, F0, _ = mf.local_assemble()
    mf.assemble_boundary()
    K, F, _ = mf.local_assemble()
    interior = np.flatnonzero(part.elem_boundary == 0)
    assert len(interior) == 1
    e = int(interior[0])
    assert torch.equal(K[e], K0[e]) and torch.equal(F[e], F0[e])
    touched = [i for i in range(part.n_elems) if not torch.equal(K[i], K0[i])]
    assert touched == [i for i in range(part.n_elems) if i != e]


# ------------------------------------------------------------------------------------------- 5. the switch, mesh level
@pytest.mark.parametrize("p", [2, 4])
def test_switch_mesh_level(ctx, p):
    part = system.CubePartition((3, 2, 2), p, perturb=0.15)
    mask = part.dirichlet_mask(U, unknowns=(0,), sides=(4, 5))
    mesh = system.DeviceMesh(ctx, part, U, mask)
    mf, bare = system.MatrixFreeSystem(mesh, DIFF, DIFF_PAR), system.MatrixFreeSystem(mesh, DIFF, DIFF_PAR)
    terms, _ = two_terms(mesh, part, p)
    for t in terms:
        mf.attach_boundary(t)
    g = mf.sparsity_graph()
    n = g.n
    free = dev(mask == 0, torch.bool)
    x = dev(np.random.default_rng(p).standard_normal(n))
    out = {}
    for on, other in ((True, mf), (False, bare)):
        mf.assemble_boundary(on)
        vals = torch.zeros(g.col_ind.numel(), dtype=torch.float64, device="cuda")
        assert mf.assemble_global(g.row_ptr, g.col_ind, vals, None, skip_dirichlet=True) == 0
        op = system.CsrOperator(ctx, g.row_ptr, g.col_ind, vals)
        y_csr, y_mf = torch.empty_like(x), torch.empty_like(x)
        op.apply(x, y_csr)
        other.apply(x[None, :], y_mf[None, :])
        err = float((y_mf[free] - y_csr[free]).norm() / y_mf[free].norm())
        diag, _ = other.diag_rhs(None)
        derr = float((op.diag()[free] - diag[free]).norm() / diag[free].norm())
        print(f"p {p} switch {'on' if on else 'off'}: CSR apply against the matrix-free one {err:.2e}, diagonal {derr:.2e}")
        assert err <= 1e-11 and derr <= 1e-11
        out[on] = y_csr
    assert float((out[True] - out[False]).norm() / out[False].norm()) > 1e-3  # the terms are in the assembled operator


# ------------------------------------------------------------------------------------------- 6. end to end
def true_residual(A, b, x):
    r = b.astype(LD) - A.astype(LD) @ x.astype(LD)
    return float(np.sqrt(np.sum(r * r)) / np.sqrt(np.sum(b.astype(LD) ** 2)))


def robin_problem(ctx, ne, p, robin_sides):
    part = system.CubePartition(ne, p, perturb=0.15)
    mask = part.dirichlet_mask(U, unknowns=(0,), sides=(4, 5))
    mesh = system.DeviceMesh(ctx, part, U, mask)
    mf = system.MatrixFreeSystem(mesh, DIFF, DIFF_PAR)
    fe, fs = robin_sides(part)
    mf.attach_boundary(system.BoundaryTerm(mesh, system.KERNEL_ROBIN3D, fe, fs, kernel_params=[2.0, 1.0]))
    n = part.n_local_nodes * U
    dmask = mask.astype(bool)
    g = np.where(dmask, np.sin(np.arange(n) * 0.37), 0.0)
    return part, mf, n, dmask, dev(dmask.astype(np.uint8), torch.uint8), dev(g[None, :])


def solve_matrix_free(ctx, mf, G, max_iters=20000, must_converge=True):
    diag, rhs = mf.diag_rhs(G)
    x = torch.zeros_like(rhs[0])
    res = solve.pcg(mf, rhs[0].contiguous(), x, solve.jacobi_inverse_native(ctx, diag), tol=1e-12, residual_scaling="rhs",
                    max_iters=max_iters, throw_on_fail=must_converge)
    assert res.converged or not must_converge
    return x.cpu().numpy()


def solve_assembled(ctx, mf, n, M, G, max_iters=20000, must_converge=True):
    g = mf.sparsity_graph()
    vals = torch.zeros(g.col_ind.numel(), dtype=torch.float64, device="cuda")
    rhs = torch.zeros((1, n), dtype=torch.float64, device="cuda")
    assert mf.assemble_global(g.row_ptr, g.col_ind, vals, rhs) == 0
    op = system.CsrOperator(ctx, g.row_ptr, g.col_ind, vals)
    op.dirichlet(M, G, rhs)
    x = torch.zeros(n, dtype=torch.float64, device="cuda")
    res = solve.pcg(op, rhs[0], x, op.jacobi_inverse(), tol=1e-12, residual_scaling="rhs", max_iters=max_iters, throw_on_fail=must_converge)
    assert res.converged or not must_converge
    return x.cpu().numpy(), dense_of(g.row_ptr, g.col_ind, vals, n), rhs[0].cpu().numpy()


def solve_condensed(ctx, mf, n, M, G):
    g = mf.sparsity_graph("condensed")
    vals = torch.zeros(g.col_ind.numel(), dtype=torch.float64, device="cuda")
    rhs = torch.zeros((1, n), dtype=torch.float64, device="cuda")
    assert mf.condense_global(g.row_ptr, g.col_ind, vals, rhs) == 0
    op = system.CsrOperator(ctx, g.row_ptr, g.col_ind, vals)
    op.dirichlet(M, G, rhs)
    X = torch.zeros((1, n), dtype=torch.float64, device="cuda")
    res = solve.pcg(op, rhs[0], X[0], op.jacobi_inverse(), tol=1e-12, residual_scaling="rhs", max_iters=20000)
    assert res.converged
    mf.recover_internal(X)
    torch.cuda.synchronize()
    return X.cpu().numpy()[0]


@pytest.mark.parametrize("ne,p", [(3, 2), (2, 4)])
def test_three_solves_agree(ctx, ne, p):
    part, mf, n, dmask, M, G = robin_problem(ctx, ne, p, lambda part: part.boundary_sides([0, 1, 2, 3]))
    x_mf = solve_matrix_free(ctx, mf, G)
    x_off, _, _ = solve_assembled(ctx, mf, n, M, G)  # switch off: the assembled operator lacks the Robin term
    mf.assemble_boundary()
    x_asm, A, b = solve_assembled(ctx, mf, n, M, G)
    x_cond = solve_condensed(ctx, mf, n, M, G)
    assert np.abs(A - A.T).max() <= 1e-12 * np.abs(A).max()
    cond = float(np.linalg.cond(A))
    sols = {"matrix-free": x_mf, "assembled": x_asm, "condensed": x_cond}
    res = {k: true_residual(A, b, v) for k, v in sols.items()}
    names = list(sols)
    for i in range(3):
        for j in range(i + 1, 3):
            a, c = names[i], names[j]
            err, bound = rel(sols[a], sols[c]), cond * (res[a] + res[c] + n * EPS)
            print(f"ne {ne} p {p}: {a} against {c} {err:.3e}, bound {bound:.3e} (cond {cond:.3e}, residuals {res[a]:.2e} {res[c]:.2e})")
            assert err <= bound
    off = rel(x_off, x_mf)
    print(f"switch off: assembled against matrix-free {off:.3e}")
    assert off > 100 * cond * (res["matrix-free"] + res["assembled"] + n * EPS)


def test_order_6_assembled_vs_matrix_free(ctx):
    """Nd = 1372: the accumulating store over 21 full tiles and a remainder of 28 per side, one Robin side per element.  The
    element systems against the oracle, the assembled operator against the matrix-free one, and the two solves.  The Jacobi PCG
    needs tens of thousands of iterations on this system (two order-6 elements, Dirichlet values on one unknown of two faces), so
    the solves stop at 40 000 iterations and the bound takes the true residuals they reached."""
    p = 6
    sides = (np.array([0, 1]), np.array([1, 3], dtype=np.uint8))
    part, mf, n, dmask, M, G = robin_problem(ctx, (2, 1, 1), p, lambda part: sides)
    K0, _, _ = mf.local_assemble(want_F=False)
    mf.assemble_boundary()
    K, F, _ = mf.local_assemble()
    K2, F2, _ = mf.local_assemble()
    assert torch.equal(K, K.transpose(1, 2)) and torch.equal(K, K2) and torch.equal(F, F2)
    assert all(not torch.equal(K[e], K0[e]) for e in range(2))
    lists = [(None, O.KERNEL_ROBIN3D, [2.0, 1.0], sides)]
    for e, (K_ref, F_ref) in enumerate(oracle_element_systems(part, p, lists)):
        ek = np.abs(K[e].cpu().numpy() - K_ref).max() / np.abs(K_ref).max()
        ef = np.abs(F[e].cpu().numpy().T - F_ref).max() / max(1.0, np.abs(F_ref).max())
        print(f"order 6 element {e}: K_e + K_s against the oracle {ek:.2e}, F {ef:.2e}")
        assert ek <= 1e-12 and ef <= 1e-12
    # the assembled operator against the matrix-free one on the free dofs
    g = mf.sparsity_graph()
    vals = torch.zeros(g.col_ind.numel(), dtype=torch.float64, device="cuda")
    assert mf.assemble_global(g.row_ptr, g.col_ind, vals, None, skip_dirichlet=True) == 0
    op = system.CsrOperator(ctx, g.row_ptr, g.col_ind, vals)
    x = dev(np.random.default_rng(6).standard_normal(n))
    y_csr, y_mf = torch.empty_like(x), torch.empty_like(x)
    op.apply(x, y_csr)
    mf.apply(x[None, :], y_mf[None, :])
    free = dev(~dmask, torch.bool)
    err = float((y_mf[free] - y_csr[free]).norm() / y_mf[free].norm())
    print(f"order 6: CSR apply against the matrix-free one {err:.2e}")
    assert err <= 1e-11
    # the two solves
    x_mf = solve_matrix_free(ctx, mf, G, max_iters=40000, must_converge=False)
    x_asm, A, b = solve_assembled(ctx, mf, n, M, G, max_iters=40000, must_converge=False)
    cond = float(np.linalg.cond(A))
    r_mf, r_asm = true_residual(A, b, x_mf), true_residual(A, b, x_asm)
    err, bound = rel(x_asm, x_mf), cond * (r_mf + r_asm + n * EPS)
    print(f"order 6: assembled against matrix-free {err:.3e}, bound {bound:.3e} (cond {cond:.3e}, residuals {r_mf:.2e} {r_asm:.2e})")
    assert err <= bound


# ------------------------------------------------------------------------------------------- 7. plugin
PLUGIN_SRC = """
struct RobinTwicePlugin {
    static constexpr l3k::KernelParams params{.dimension = 3, .n_equations = 1, .n_unknowns = 4};
    double h = 1., t_inf = 0.;
    template <typename In, typename Out> L3K_HD void operator()(const In& in, Out& out) const {
        const auto& normal     = in.normal;
        auto& [operators, rhs] = out;
        auto& [A0, A1, A2, A3] = operators;
        A0(0, 0) = 2. * h;
        A0(0, 1) = normal[0];
        A0(0, 2) = normal[1];
        A0(0, 3) = normal[2];
        rhs[0]   = 2. * h * t_inf;
    }
};"""


def test_plugin_boundary_kernel(ctx):
    from l3ster_amd import plugin
    kid = plugin.compile_kernel("RobinTwicePlugin", PLUGIN_SRC, kernel_id=1420, shapes=[(2, 3, 1)], kind="boundary")
    part = system.CubePartition((2, 1, 1), 2, perturb=0.15)
    mesh = system.DeviceMesh(ctx, part, U)
    fe, fs = part.boundary_sides()
    Kp, Fp = system.BoundaryTerm(mesh, kid, fe, fs, kernel_params=[0.75, 0.4]).local_assemble()
    Kr, Fr = system.BoundaryTerm(mesh, system.KERNEL_ROBIN3D, fe, fs, kernel_params=[1.5, 0.4]).local_assemble()
    assert float((Kp - Kr).abs().max()) <= 1e-13 * float(Kr.abs().max()) and float(Kr.abs().max()) > 0
    assert float((Fp - Fr).abs().max()) <= 1e-13 * float(Fr.abs().max()) and float(Fr.abs().max()) > 0


# ------------------------------------------------------------------------------------------- 8. refusals
def test_refusals(ctx):
    lib = system.capi.load()
    last = lambda: lib.l3k_last_error().decode()
    buf = torch.zeros(1 << 16, dtype=torch.float64, device="cuda")
    bp = C.c_void_p(buf.data_ptr())
    # ---- quads
    qpart = system.SquarePartition((3, 2), 2)
    qmesh = system.DeviceMesh(ctx, qpart, 3)
    qfe, qfs = qpart.boundary_sides()
    qterm = system.BoundaryTerm(qmesh, system.KERNEL_ADIABATIC2D, qfe, qfs)
    qmf = system.MatrixFreeSystem(qmesh, system.KERNEL_DIFFUSION2D)
    missing = C.c_int64(0)
    for name, rc in (("l3k_bnd_local_assemble", lib.l3k_bnd_local_assemble(qterm._h, 0, 1, bp, bp)),
                     ("l3k_bnd_assemble_global", lib.l3k_bnd_assemble_global(qterm._h, 0, 1, bp, bp, bp, bp, 1 << 16, 0, 0, C.byref(missing))),
                     ("l3k_mf_assemble_boundary", lib.l3k_mf_assemble_boundary(qmf._h, 1))):
        assert rc == -1, name
    assert last().startswith("l3k_mf_assemble_boundary: quads (dim = 2) are not supported here")
    assert lib.l3k_bnd_local_assemble(qterm._h, 0, 1, bp, bp) == -1 and last().startswith("l3k_bnd_local_assemble: quads (dim = 2)")
    assert lib.l3k_bnd_assemble_global(qterm._h, 0, 1, bp, bp, bp, bp, 1 << 16, 0, 0, None) == -1
    assert last().startswith("l3k_bnd_assemble_global: quads (dim = 2)")
    assert not buf.any()
    # ---- a hex system with one dof per node more than the kernel's unknowns
    p = 2
    part = system.CubePartition(2, p, perturb=0.1)
    mesh = system.DeviceMesh(ctx, part, 5)
    fe, fs = part.boundary_sides()
    kid, _, kp = KERNELS["robin"]
    good = system.BoundaryTerm(mesh, kid, fe, fs, kernel_params=kp, field_inds=[0, 1, 2, 3])
    shifted = system.BoundaryTerm(mesh, kid, fe, fs, kernel_params=kp, field_inds=[1, 2, 3, 4])
    two_cols = system.BoundaryTerm(mesh, kid, fe, fs, kernel_params=kp, field_inds=[0, 1, 2, 3], n_rhs=2)
    mf = system.MatrixFreeSystem(mesh, DIFF, DIFF_PAR, field_inds=[0, 1, 2, 3])
    with pytest.raises(system.L3KError, match="boundary term has n_rhs = 2, system has 1"):
        mf.attach_boundary(two_cols)  # (a term with another n_rhs cannot be attached at all)
    mf.attach_boundary(good)
    mf.assemble_boundary()
    K_ok, F_ok, _ = mf.local_assemble()
    # out-of-range sides
    n_f = len(fe)
    for first, count in ((0, n_f + 1), (-1, 2), (n_f, 1), (3, -1)):
        assert lib.l3k_bnd_local_assemble(good._h, first, count, bp, bp) == -1
        assert last() == f"l3k_bnd_local_assemble: side range [{first}, {first + count}) outside [0, {n_f})"
        assert lib.l3k_bnd_assemble_global(good._h, first, count, bp, bp, bp, None, 0, 0, 0, None) == -1
        assert last() == f"l3k_bnd_assemble_global: side range [{first}, {first + count}) outside [0, {n_f})"
    # small ldr, missing graph arrays
    g = mf.sparsity_graph()
    vals = torch.zeros(g.col_ind.numel(), dtype=torch.float64, device="cuda")
    rhs = torch.zeros((1, g.n), dtype=torch.float64, device="cuda")
    args = lambda rp, ci, v, r, ldr: (good._h, 0, n_f, C.c_void_p(rp), C.c_void_p(ci), C.c_void_p(v), C.c_void_p(r), ldr, 0, 0, None)
    RP, CI, V, R = g.row_ptr.data_ptr(), g.col_ind.data_ptr(), vals.data_ptr(), rhs.data_ptr()
    assert lib.l3k_bnd_assemble_global(*args(RP, CI, V, R, g.n - 1)) == -1
    assert last() == "l3k_bnd_assemble_global: rhs leading dimension smaller than the number of local dofs"
    for a in (args(0, CI, V, R, g.n), args(RP, 0, V, R, g.n), args(RP, CI, 0, R, g.n)):
        assert lib.l3k_bnd_assemble_global(*a) == -1
        assert last() == "l3k_bnd_assemble_global: null argument (row_ptr, col_ind and values are needed)"
    assert not vals.any() and not rhs.any()
    assert good.assemble_global(g.row_ptr, g.col_ind, vals, rhs) == 0 and vals.any() and rhs.any()  # a valid call still works
    # checksum with the switch on, the tiled layout with the switch on
    Nd = 27 * 4
    cs = torch.zeros(part.n_elems, dtype=torch.float64, device="cuda")
    assert lib.l3k_local_assemble(mf._h, 0, part.n_elems, None, None, C.c_void_p(cs.data_ptr())) == -1
    assert last().startswith("l3k_local_assemble: no checksum with l3k_mf_assemble_boundary on")
    Kt = torch.zeros(part.n_elems * Nd * Nd, dtype=torch.float64, device="cuda")
    assert lib.l3k_local_assemble_tiled(mf._h, 0, part.n_elems, C.c_void_p(Kt.data_ptr())) == -1
    assert last().startswith("l3k_local_assemble_tiled: not with l3k_mf_assemble_boundary on")
    assert not cs.any() and not Kt.any()
    K2, F2, _ = mf.local_assemble()
    assert torch.equal(K2, K_ok) and torch.equal(F2, F_ok)
    # a term on other dofs than the system's
    mf.attach_boundary(shifted)
    with pytest.raises(system.L3KError, match=r"l3k_local_assemble: attached boundary term 1 has field_inds\[0\] = 1, the system has 0"):
        mf.local_assemble()
    with pytest.raises(system.L3KError, match=r"l3k_assemble_global: attached boundary term 1 has field_inds\[0\] = 1, the system has 0"):
        mf.assemble_global(g.row_ptr, g.col_ind, torch.zeros_like(vals), None)
    with pytest.raises(system.L3KError, match=r"l3k_local_assemble: attached boundary term 1 has field_inds"):
        mf.condense_local()
    mf.assemble_boundary(False)  # off: the calls ignore the terms again
    K3, _, cs3 = mf.local_assemble(want_F=False, want_checksum=True)
    assert cs3 is not None and mf.local_assemble_tiled().shape[0] == part.n_elems
    # a shape without an assembly launcher: none is registered for this (order, nq)
    odd = system.BoundaryTerm(mesh, kid, fe, fs, kernel_params=kp, asm_opts=(2, 0, 0), field_inds=[0, 1, 2, 3])
    with pytest.raises(system.L3KError, match="l3k_bnd_local_assemble: no device instantiation for boundary kernel"):
        odd.local_assemble()
