"""Static condensation of the element-internal dofs on quad meshes inside the assembled system (l3k_asm_create_condensed,
system.AssembledSystem(condensation="element_boundary"); the reference's StaticCondensationManager< ElementBoundary >).

References: what the library already provides and tests -- MatrixFreeSystem.element_systems, BoundaryTerm.side_systems and the full
AssembledSystem -- plus the numpy restatement of quad_condense_ref.py.

Tolerances: A = max(1e-12, 100 cond_2(K_ii) 2^-52) max|K_e| at element level (test_gpu_condensation.py), B = the same expression with
the global K_ii and max|A| at mesh level, 1e-13 max|A| for the reordering of at most four atomic addends (test_gpu_quad_assembly.py),
the reference's 1e-8 end to end."""
import ctypes as C
import gc
import os
import shutil
import subprocess
import weakref

import numpy as np
import pytest

import quad_condense_ref as QC
import quad_side_ref as QS
from l3ster_amd import capi, solve, system
from test_gpu_quad_assembly import SOURCE_SRC, dense_of, dev

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

U = 3
D2, ADI = system.KERNEL_DIFFUSION2D, system.KERNEL_ADIABATIC2D
EB = "element_boundary"
EPS = 2.0 ** -52
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MASS_SRC = """
struct QuadCondMass {
    static constexpr l3k::KernelParams params{.dimension = 2, .n_equations = 1, .n_unknowns = 1};
    template <typename In, typename Out> L3K_HD void operator()(const In& in, Out& out) const {
        auto& [operators, rhs] = out;
        auto& [A0, Ax, Ay] = operators;
        A0(0, 0) = 1.;
        for (int r = 0; r < rhs.cols(); ++r)
            rhs(0, r) = 1. + r + in.point.space.x();
    }
};"""


@pytest.fixture(scope="module")
def ctx():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    torch.cuda.set_device(0)
    return system.Context(0, torch.cuda.current_stream().cuda_stream)


@pytest.fixture(scope="module")
def source_id():
    from l3ster_amd import plugin
    return plugin.compile_kernel("QuadCondSource", SOURCE_SRC.replace("QuadAsmSource", "QuadCondSource"), kernel_id=1351,
                                 shapes=[(p, p + 1, R) for p in (1, 2, 3, 4, 6) for R in (1, 2)])


@pytest.fixture(scope="module")
def wall_id():
    from l3ster_amd import plugin
    return plugin.compile_kernel("QuadCondWall", QS.PLUGIN_SRC.replace("QuadWallPlugin", "QuadCondWall"), kernel_id=1352,
                                 shapes=[(2, 3, 2), (4, 5, 2)], kind="boundary")


@pytest.fixture(scope="module")
def mass_id():
    from l3ster_amd import plugin
    return plugin.compile_kernel("QuadCondMass", MASS_SRC, kernel_id=1353, shapes=[(2, 3, 2), (6, 7, 1)])


def condensed(mesh, **kw):
    return system.AssembledSystem(mesh, condensation=EB, **kw)


def assemble(asm, *terms, dirichlet_vals=None):
    asm.begin()
    for t in terms:
        asm.add(t)
    return asm.end(dirichlet_vals)


def factor(cond):
    return max(1e-12, 100 * cond * EPS)


# ------------------------------------------------------------------------------------------------------ 1. element level
@pytest.mark.parametrize("R", [1, 2])
@pytest.mark.parametrize("p", [1, 2, 3, 4, 6])
def test_schur_updates_vs_numpy(ctx, source_id, p, R):
    """W_e = K_bi K_ii^-1 K_ib and w_e = K_bi K_ii^-1 F_i of every element against numpy on the device's own element systems"""
    part = system.SquarePartition((3, 2), p, perturb=0.15)
    mesh = system.DeviceMesh(ctx, part, U)
    mf = system.MatrixFreeSystem(mesh, source_id, n_rhs=R)
    mf.set_time(0.3)
    asm = condensed(mesh, n_rhs=R)
    assemble(asm, mf)
    W, w = asm.schur_updates()
    Ws, ws = asm.schur_updates(first=1, count=4)
    assemble(asm, mf)
    W2, w2 = asm.schur_updates()
    torch.cuda.synchronize()
    Nb = 4 * p * U
    assert W.shape == (part.n_elems, Nb, Nb) and w.shape == (part.n_elems, R, Nb)
    assert torch.equal(W, W.transpose(1, 2))           # bitwise symmetric
    assert torch.equal(W, W2) and torch.equal(w, w2)   # the same bits on a second assembly (domain term only)
    assert torch.equal(Ws, W[1:5]) and torch.equal(ws, w[1:5])
    if p == 1:
        assert not W.any().item() and not w.any().item()
        return
    K, F = mf.element_systems()
    K, F, Wh, wh = K.cpu().numpy(), F.cpu().numpy(), W.cpu().numpy(), w.cpu().numpy()
    pe, ie = QC.dof_split(p, U)
    worst = 0.0
    for e in range(part.n_elems):
        W_ref, w_ref, cond = QC.schur_parts(K[e], F[e].T, pe, ie)
        eW, ew = np.abs(Wh[e] - W_ref).max(), np.abs(wh[e].T - w_ref).max()
        worst = max(worst, eW / QC.tol(cond, K[e]))
        assert eW <= QC.tol(cond, K[e]), (e, eW, cond)
        assert ew <= factor(cond) * max(1.0, np.abs(F[e]).max(), np.abs(K[e]).max()), (e, ew, cond)
    print(f"p {p} R {R}: worst |W - W_numpy| / tolerance A = {worst:.2e}")


def test_slots_above_the_lds_bound_are_eliminated_in_global_memory(ctx, mass_id):
    """Order 6 with four fields: 100 internal rows of 197 doubles = 154 KiB per element, above the 128 KiB a workgroup takes: the
    in-place route of the same kernel.  Updates against numpy, and recovery against the element solves"""
    p, Us = 6, 4
    part = system.SquarePartition((3, 2), p, perturb=0.15)
    mesh = system.DeviceMesh(ctx, part, Us)
    terms = [(system.MatrixFreeSystem(mesh, D2, field_inds=[0, 1, 2]), [0, 1, 2]), (system.MatrixFreeSystem(mesh, mass_id, field_inds=[3]), [3])]
    asm = condensed(mesh)
    assemble(asm, *[t for t, _ in terms])
    Nis, Nbs = (p - 1) ** 2 * Us, 4 * p * Us
    assert asm.cond_info.store_bytes // part.n_elems == 8 * Nis * (Nis + Nbs + 1) > 128 * 1024
    W, w = asm.schur_updates()
    assert torch.equal(W, W.transpose(1, 2))
    NN = (p + 1) ** 2
    pe, ie = QC.dof_split(p, Us)
    rng = np.random.default_rng(6)
    x = rng.uniform(-1, 1, (1, asm.n))
    X = dev(x)
    asm.recover(X)
    Xh = X.cpu().numpy()
    for e in range(part.n_elems):
        Ksum, Fsum = np.zeros((NN * Us, NN * Us)), np.zeros((NN * Us, 1))
        for term, fields in terms:
            K, F = term.element_systems(e, 1)
            Ke, Fe = QC.embed(K[0].cpu().numpy(), F[0].cpu().numpy().T, NN, fields, range(Us))
            Ksum += Ke
            Fsum += Fe
        W_ref, w_ref, cond = QC.schur_parts(Ksum, Fsum, pe, ie)
        assert np.abs(W[e].cpu().numpy() - W_ref).max() <= QC.tol(cond, Ksum), (e, cond)
        assert np.abs(w[e].cpu().numpy().T - w_ref).max() <= factor(cond) * max(1.0, np.abs(Fsum).max(), np.abs(Ksum).max()), (e, cond)
        d = (part.elem_nodes[e].astype(np.int64)[:, None] * Us + np.arange(Us)[None, :]).reshape(-1)
        x_i = QC.recover(Ksum, Fsum, pe, ie, x[:, d[pe]].T)
        assert np.abs(Xh[:, d[ie]].T - x_i).max() <= factor(cond) * max(1.0, np.abs(x_i).max()), (e, cond)


# ----------------------------------------------------------------------------------------------- 2. sides into the store
@pytest.mark.parametrize("p", [2, 4])
def test_side_systems_reach_the_store(ctx, source_id, wall_id, p):
    """Every element receives its domain system and up to five side systems, several of them in one sub-batch: the updates are
    those of K_e + sum K_s"""
    R = 2
    part = system.SquarePartition((3, 2), p, perturb=0.15)
    mesh = system.DeviceMesh(ctx, part, U)
    mf = system.MatrixFreeSystem(mesh, source_id, n_rhs=R)
    mf.set_time(0.3)
    fe, fs = np.repeat(np.arange(part.n_elems), 4), np.tile(np.arange(4), part.n_elems).astype(np.uint8)
    wall_fields = [2, 1]
    wall = system.BoundaryTerm(mesh, wall_id, fe, fs, field_inds=wall_fields, n_rhs=R)
    wall.set_fields(dev(np.random.default_rng(p).uniform(0.5, 1.5, (1, part.n_local_nodes))))
    wall.set_time(0.4)
    ae, as_ = part.boundary_sides([0, 1])
    adi = system.BoundaryTerm(mesh, ADI, ae, as_, n_rhs=R)
    asm = condensed(mesh, n_rhs=R)
    assemble(asm, mf, wall, adi)
    assert asm.info.n_missing == 0
    W, w = asm.schur_updates()
    torch.cuda.synchronize()
    assert torch.equal(W, W.transpose(1, 2))
    NN = (p + 1) ** 2
    K, F = (t.cpu().numpy() for t in mf.element_systems())
    Kw, Fw = (t.cpu().numpy() for t in wall.side_systems())
    Ka, Fa = (t.cpu().numpy() for t in adi.side_systems())
    Ksum, Fsum = K.copy(), np.transpose(F, (0, 2, 1)).copy()
    for i, e in enumerate(fe):
        Ke, Fe = QC.embed(Kw[i], Fw[i].T, NN, wall_fields, range(U))
        Ksum[e] += Ke
        Fsum[e] += Fe
    for i, e in enumerate(ae):
        Ksum[e] += Ka[i]
        Fsum[e] += Fa[i].T
    pe, ie = QC.dof_split(p, U)
    Wh, wh = W.cpu().numpy(), w.cpu().numpy()
    reach = 0.0
    for e in range(part.n_elems):
        W_ref, w_ref, cond = QC.schur_parts(Ksum[e], Fsum[e], pe, ie)
        reach = max(reach, np.abs(Ksum[e] - K[e])[np.ix_(ie, ie)].max())
        assert np.abs(Wh[e] - W_ref).max() <= QC.tol(cond, Ksum[e]), (e, cond)
        assert np.abs(wh[e].T - w_ref).max() <= factor(cond) * max(1.0, np.abs(Fsum[e]).max(), np.abs(Ksum[e]).max()), (e, cond)
    assert reach > 0  # the wall plugin's derivative operators reach the internal nodes


# ------------------------------------------------------------------------------------------------ 3. mesh level, no mask
@pytest.mark.parametrize("p", [2, 3])
def test_condensed_system_is_the_dense_schur_complement(ctx, source_id, p):
    part = system.SquarePartition((5, 4), p, perturb=0.15)
    mesh = system.DeviceMesh(ctx, part, U)  # no Dirichlet mask
    mf = system.MatrixFreeSystem(mesh, source_id)
    mf.set_time(0.3)
    bnd = system.BoundaryTerm(mesh, ADI, *part.boundary_sides([0, 3]))
    full, cond_sys = system.AssembledSystem(mesh), condensed(mesh)
    assemble(full, mf, bnd)
    assemble(cond_sys, mf, bnd)
    assert cond_sys.info.n_missing == 0 and cond_sys.info.state == "closed"
    A, f = dense_of(full), full.rhs.cpu().numpy().T
    prim, inner = QC.mesh_split(part, U, range(U))
    S, g, cond = QC.schur_complement(A, f, prim, inner)
    C_, c_ = dense_of(cond_sys), cond_sys.rhs.cpu().numpy().T
    t = factor(cond) * np.abs(A).max()
    eS, eg = np.abs(C_[np.ix_(prim, prim)] - S).max(), np.abs(c_[prim] - g).max()
    print(f"p {p}: |C - S| = {eS:.2e}, |c - g| = {eg:.2e}, tolerance B = {t:.2e} (cond K_ii = {cond:.2e})")
    assert eS <= t and eg <= t
    # the rows of internal dofs are empty, and nothing else is stored in their columns
    rp = cond_sys.row_ptr.cpu().numpy()
    assert np.all(np.diff(rp)[inner] == 0) and np.all(np.diff(rp)[prim] > 0)
    assert not C_[:, inner].any() and not c_[inner].any()
    assert cond_sys.nnz < full.nnz
    ci = cond_sys.cond_info
    Nis, Nbs = (p - 1) ** 2 * U, 4 * p * U
    assert (ci.condensed, ci.n_primary_nodes, ci.n_internal_nodes, ci.n_elems, ci.n_failed) == (1, 4 * p, (p - 1) ** 2, part.n_elems, 0)
    assert ci.store_bytes == 8 * part.n_elems * Nis * (Nis + Nbs + 1)
    fi = full.cond_info
    assert (fi.condensed, fi.store_bytes, fi.n_elems) == (0, 0, 0)


def test_order_one_has_nothing_to_condense(ctx, source_id):
    part = system.SquarePartition((5, 4), 1, perturb=0.15)
    mesh = system.DeviceMesh(ctx, part, U)
    mf = system.MatrixFreeSystem(mesh, source_id)
    bnd = system.BoundaryTerm(mesh, ADI, *part.boundary_sides([0, 3]))
    full, cond_sys = system.AssembledSystem(mesh), condensed(mesh)
    assemble(full, mf, bnd)
    assemble(cond_sys, mf, bnd)
    assert torch.equal(full.row_ptr, cond_sys.row_ptr) and torch.equal(full.col_ind, cond_sys.col_ind)
    scale = full.values.abs().max().item()
    assert scale > 0 and (full.values - cond_sys.values).abs().max().item() <= 1e-13 * scale
    assert (full.rhs - cond_sys.rhs).abs().max().item() <= 1e-13 * max(scale, full.rhs.abs().max().item())
    assert cond_sys.cond_info.store_bytes == 0
    x = torch.ones((1, full.n), dtype=torch.float64, device="cuda")
    assert torch.equal(cond_sys.recover(x.clone()), x)


# ----------------------------------------------------------------------------------------------------- 4. sub-batches
def test_sub_batches(ctx):
    p = 3
    part = system.SquarePartition((7, 5), p, perturb=0.15)
    mesh = system.DeviceMesh(ctx, part, U)
    mf, bnd = system.MatrixFreeSystem(mesh, D2), system.BoundaryTerm(mesh, ADI, *part.boundary_sides([1, 2]))
    Nd = (p + 1) ** 2 * U
    workspace = 2 * 10 * 8 * Nd * Nd  # two halves of at most ten element matrices
    assert -(-part.n_elems // (workspace // 2 // (8 * Nd * Nd))) >= 3  # at least three sub-batches of element systems
    small, default = condensed(mesh, workspace_bytes=workspace), condensed(mesh)
    assemble(small, mf, bnd)
    assemble(default, mf, bnd)
    assert small.info.n_missing == 0 and default.info.n_missing == 0
    assert torch.equal(small.col_ind, default.col_ind) and torch.equal(small.row_ptr, default.row_ptr)
    scale = default.values.abs().max().item()
    assert scale > 0 and (small.values - default.values).abs().max().item() <= 1e-13 * scale
    Ws, _ = small.schur_updates()
    Wd, _ = default.schur_updates()
    assert Wd.abs().max().item() > 0 and (Ws - Wd).abs().max().item() <= 1e-13 * scale


# ------------------------------------------------------------------------------- 5. solve and recover = the full solve
def dirichlet_problem(ctx, part, kid):
    mask = part.dirichlet_mask(U, sides=(2, 3))
    mesh = system.DeviceMesh(ctx, part, U, mask)
    mf = system.MatrixFreeSystem(mesh, kid)
    mf.set_time(0.3)
    bnd = system.BoundaryTerm(mesh, ADI, *part.boundary_sides([0, 1]))
    n = part.n_local_nodes * U
    g = dev(np.where(mask.reshape(-1) != 0, 0.5 + np.sin(np.arange(n) * 0.37), 0.0)[None, :])
    return mesh, mf, bnd, g, n


def pcg_solve(asm, op, tol):
    x = torch.zeros(asm.n, dtype=torch.float64, device="cuda")
    res = solve.pcg(op, asm.rhs[0], x, op.jacobi_inverse(), tol=tol, residual_scaling="rhs", max_iters=50000)
    return x, res


@pytest.mark.parametrize("p", [2, 4, 6])
def test_solve_and_recover_equal_the_full_solve(ctx, source_id, p):
    """Jacobi PCG at 1e-12 on the condensed operator, then recover, against the PCG solution of the full system; the bar 1e-8 max|x|
    is set by the solver tolerance, not by the elimination.  Measured on one MI355X (difference / max|x|; iterations condensed /
    full): order 2: 2.3e-13, 122 / 139; order 4: 3.3e-11, 312 / 484; order 6: 2.6e-11, 610 / 1005."""
    part = system.SquarePartition((4, 3), p, perturb=0.15)
    mesh, mf, bnd, g, n = dirichlet_problem(ctx, part, source_id)
    full, cond_sys = system.AssembledSystem(mesh), condensed(mesh)
    x_f, res_f = pcg_solve(full, assemble(full, mf, bnd, dirichlet_vals=g), 1e-12)
    x_c, res_c = pcg_solve(cond_sys, assemble(cond_sys, mf, bnd, dirichlet_vals=g), 1e-12)
    assert res_f.converged and res_c.converged
    prim, inner = QC.mesh_split(part, U, range(U))
    assert not x_c[dev(inner, torch.int64)].any().item()  # the PCG leaves the empty rows alone
    before = x_c.clone()
    again = x_c.clone()
    cond_sys.recover(x_c)
    cond_sys.recover(again)
    torch.cuda.synchronize()
    assert torch.equal(again, x_c)                                                        # the same bits on every call
    assert torch.equal(x_c[dev(prim, torch.int64)], before[dev(prim, torch.int64)])       # the primary entries are untouched
    assert x_c[dev(inner, torch.int64)].abs().max().item() > 0
    diff, scale = (x_c - x_f).abs().max().item(), x_f.abs().max().item()
    print(f"p {p}: max|x_condensed - x_full| / max|x| = {diff / scale:.2e}; iterations condensed {res_c.num_iters}, full {res_f.num_iters}")
    assert diff <= 1e-8 * scale


# -------------------------------------------------------------------- 6. the reference's Diffusion2D test with condensation
@pytest.mark.parametrize("ne,p", [(4, 2), (3, 4)])
def test_diffusion2d_condensed_end_to_end(ctx, ne, p):
    """tests/Diffusion2D.hpp with CondensationPolicy::ElementBoundary: Dirichlet T = x on the left and right sides, Adiabatic2D on the
    bottom and top, Jacobi PCG at 1e-10 on the condensed matrix, recoverSolution; L2 errors against T = x, q = (1, 0) below 1e-8"""
    part = system.SquarePartition(ne, p)
    mask = part.dirichlet_mask(U, sides=(2, 3))
    mesh = system.DeviceMesh(ctx, part, U, mask)
    mf, bnd = system.MatrixFreeSystem(mesh, D2), system.BoundaryTerm(mesh, ADI, *part.boundary_sides([0, 1]))
    n = part.n_local_nodes * U
    g = system.values_at_nodes(mesh, system.RESIDUAL_COORDX2D, [0], torch.zeros(n, dtype=torch.float64, device="cuda"),
                               face_elem=part.boundary_sides([2, 3])[0], face_side=part.boundary_sides([2, 3])[1])
    asm = condensed(mesh)
    op = assemble(asm, mf, bnd, dirichlet_vals=g[None, :])
    assert asm.info.n_missing == 0 and asm.cond_info.n_failed == 0
    sol = torch.zeros(n, dtype=torch.float64, device="cuda")
    res = solve.pcg(op, asm.rhs[0], sol, op.jacobi_inverse(), tol=1e-10, residual_scaling="rhs", max_iters=20000)
    assert res.converged
    asm.recover(sol)
    fields = sol.view(-1, U).T.contiguous()
    err = np.linalg.norm(system.norm_l2(mesh, system.RESIDUAL_LINEAR2D_ERROR, fields))
    fe, fs = part.boundary_sides()
    berr = np.linalg.norm(system.norm_l2(mesh, system.RESIDUAL_LINEAR2D_ERROR, fields, face_elem=fe, face_side=fs))
    print(f"{ne} x {ne} order {p}: {res.num_iters} iterations; L2 error domain {err:.2e}, sides {berr:.2e}")
    assert err < 1e-8 and berr < 1e-8


# ------------------------------------------------------------------ 7. two right-hand-side columns and a field subset
def subset_problem(ctx, wall_id, mass_id, definite):
    p, R, dpn, sys_fields = 2, 2, 5, [0, 1, 2, 4]
    part = system.SquarePartition((3, 2), p, perturb=0.15)
    mesh = system.DeviceMesh(ctx, part, dpn)
    terms = [(system.MatrixFreeSystem(mesh, D2, field_inds=[2, 0, 1], n_rhs=R), [2, 0, 1])]
    if definite:
        wall = system.BoundaryTerm(mesh, wall_id, *part.boundary_sides(), field_inds=[4, 1], n_rhs=R)
        wall.set_fields(dev(np.random.default_rng(7).uniform(0.5, 1.5, (1, part.n_local_nodes))))
        wall.set_time(0.4)
        terms += [(wall, [4, 1]), (system.MatrixFreeSystem(mesh, mass_id, field_inds=[4], n_rhs=R), [4])]
    return part, mesh, terms, sys_fields, R, dpn


def test_two_rhs_columns_and_a_field_subset(ctx, wall_id, mass_id):
    part, mesh, terms, sys_fields, R, dpn = subset_problem(ctx, wall_id, mass_id, True)
    p, Us, NN = part.order, len(sys_fields), (part.order + 1) ** 2
    asm = condensed(mesh, field_inds=sys_fields, n_rhs=R)
    full = system.AssembledSystem(mesh, field_inds=sys_fields, n_rhs=R)
    assemble(asm, *[t for t, _ in terms])
    assemble(full, *[t for t, _ in terms])
    assert asm.info.n_missing == 0 and asm.cond_info.n_failed == 0
    # element level: the updates of the sum of the embedded local systems
    Ksum, Fsum = np.zeros((part.n_elems, NN * Us, NN * Us)), np.zeros((part.n_elems, NN * Us, R))
    for term, fields in terms:
        if isinstance(term, system.BoundaryTerm):
            K, F = (t.cpu().numpy() for t in term.side_systems())
            elems = part.boundary_sides()[0]
        else:
            K, F = (t.cpu().numpy() for t in term.element_systems())
            elems = np.arange(part.n_elems)
        for i, e in enumerate(elems):
            Ke, Fe = QC.embed(K[i], F[i].T, NN, fields, sys_fields)
            Ksum[e] += Ke
            Fsum[e] += Fe
    W, w = asm.schur_updates()
    assert W.shape == (part.n_elems, 4 * p * Us, 4 * p * Us) and w.shape == (part.n_elems, R, 4 * p * Us)
    assert torch.equal(W, W.transpose(1, 2))
    pe, ie = QC.dof_split(p, Us)
    for e in range(part.n_elems):
        W_ref, w_ref, cond = QC.schur_parts(Ksum[e], Fsum[e], pe, ie)
        assert np.abs(W[e].cpu().numpy() - W_ref).max() <= QC.tol(cond, Ksum[e]), e
        assert np.abs(w[e].cpu().numpy().T - w_ref).max() <= factor(cond) * max(1.0, np.abs(Fsum[e]).max(), np.abs(Ksum[e]).max()), e
    # mesh level: the dense Schur complement of the full system, both columns
    A, f = dense_of(full), full.rhs.cpu().numpy().T
    prim, inner = QC.mesh_split(part, dpn, sys_fields)
    S, g, cond = QC.schur_complement(A, f, prim, inner)
    C_, c_ = dense_of(asm), asm.rhs.cpu().numpy().T
    assert np.abs(C_[np.ix_(prim, prim)] - S).max() <= factor(cond) * np.abs(A).max()
    assert np.abs(c_[prim] - g).max() <= factor(cond) * np.abs(A).max()
    assert np.abs(g[:, 0] - g[:, 1]).max() > 0
    # recovery of both columns from the exact primary values
    x = np.zeros((R, asm.n))
    x[:, prim] = np.linalg.solve(S, g).T
    X = dev(x)
    asm.recover(X)
    x_i = QC.recover(A, f, prim, inner, x[:, prim].T)
    assert np.abs(X.cpu().numpy()[:, inner].T - x_i).max() <= factor(cond) * max(1.0, np.abs(x_i).max())
    untouched = np.setdiff1d(np.arange(asm.n), inner)
    assert np.array_equal(X.cpu().numpy()[:, untouched], x[:, untouched])


def test_a_field_without_internal_contributions_fails_the_pivot_test(ctx, wall_id, mass_id):
    part, mesh, terms, sys_fields, R, _ = subset_problem(ctx, wall_id, mass_id, False)
    asm = condensed(mesh, field_inds=sys_fields, n_rhs=R)
    asm.begin().add(terms[0][0])
    with pytest.raises(system.L3KError, match="error -2: .*non-positive pivot in the element-internal block"):
        asm.end()
    assert asm.cond_info.n_failed == part.n_elems and asm.info.state == "open"


# --------------------------------------------------------------------------------------------------------- 8. a time loop
def test_time_loop(ctx, source_id):
    p = 4
    part = system.SquarePartition((4, 3), p, perturb=0.15)
    mesh, mf, bnd, g, n = dirichlet_problem(ctx, part, source_id)
    asm = condensed(mesh)
    x, res = pcg_solve(asm, assemble(asm, mf, bnd, dirichlet_vals=g), 1e-10)
    asm.recover(x)
    first_rhs = asm.rhs.clone()
    mf.set_time(0.9)
    x2, res2 = pcg_solve(asm, assemble(asm, mf, bnd, dirichlet_vals=g), 1e-10)
    asm.recover(x2)
    fresh = condensed(mesh)
    x3, res3 = pcg_solve(fresh, assemble(fresh, mf, bnd, dirichlet_vals=g), 1e-10)
    fresh.recover(x3)
    assert res.converged and res2.converged and res3.converged
    assert (asm.rhs - first_rhs).abs().max().item() > 0  # the source depends on the time
    scale = fresh.values.abs().max().item()
    assert (asm.values - fresh.values).abs().max().item() <= 1e-13 * scale
    assert (asm.rhs - fresh.rhs).abs().max().item() <= 1e-13 * max(scale, fresh.rhs.abs().max().item())
    (W, w), (Wf, wf) = asm.schur_updates(), fresh.schur_updates()
    assert (W - Wf).abs().max().item() <= 1e-13 * scale
    assert (w - wf).abs().max().item() <= 1e-13 * max(scale, wf.abs().max().item())
    assert (x2 - x3).abs().max().item() <= 1e-8 * x3.abs().max().item()  # (two PCG runs at 1e-10)


# ------------------------------------------------------------------------------------------------ 9. states and refusals
def test_states_and_refusals(ctx):
    p = 3
    part = system.SquarePartition((3, 2), p, perturb=0.1)
    mesh = system.DeviceMesh(ctx, part, U, part.dirichlet_mask(U, sides=(2, 3)))
    mf, bnd = system.MatrixFreeSystem(mesh, D2), system.BoundaryTerm(mesh, ADI, *part.boundary_sides([0, 1]))
    with pytest.raises(system.L3KError, match="condensation"):
        system.AssembledSystem(mesh, condensation="elements")
    with pytest.raises(system.L3KError, match="hex mesh.*l3k_condense_global"):
        condensed(system.DeviceMesh(ctx, system.CubePartition(2, 2), 4))
    ghosted = system.DeviceMesh(ctx, system.CubePartition(2, 2, parts=(2, 1, 1), rank=1), 4)  # (rank 1 holds the ghost nodes)
    with pytest.raises(system.L3KError, match="partitioned"):
        condensed(ghosted)
    with pytest.raises(system.L3KError, match="field_inds"):
        condensed(system.DeviceMesh(ctx, part, 5), field_inds=[2, 1])
    asm = condensed(mesh)
    x = torch.zeros((1, asm.n), dtype=torch.float64, device="cuda")
    with pytest.raises(system.L3KError, match="not closed"):
        asm.recover(x)  # a new system
    with pytest.raises(system.L3KError, match="not closed"):
        asm.schur_updates()
    asm.begin().add(mf)
    with pytest.raises(system.L3KError, match="not closed"):
        asm.recover(x)  # an open system
    with pytest.raises(system.L3KError, match="not closed"):
        asm.schur_updates()
    asm.add(bnd).end()
    lib = capi.load()
    assert lib.l3k_asm_recover(asm._h, C.c_void_p(x.data_ptr()), asm.n - 1) == -1
    assert "leading dimension" in lib.l3k_last_error().decode()
    for first, count in ((4, 3), (-1, 2), (0, part.n_elems + 1)):
        with pytest.raises(system.L3KError, match="range"):
            asm.schur_updates(first, count)
    with pytest.raises(system.L3KError, match="not open"):
        asm.add(mf)  # closed
    plain = system.AssembledSystem(mesh)
    plain.begin().add(mf).add(bnd).end()
    with pytest.raises(system.L3KError, match="not condensed"):
        plain.recover(x)
    with pytest.raises(system.L3KError, match="not condensed"):
        plain.schur_updates()
    # a mask flag on an element-internal dof: l3k_csr_dirichlet refuses the row without a diagonal, the system stays open
    _, inner = system.element_node_split(p, dim=2)
    mask = part.dirichlet_mask(U, sides=(2, 3)).reshape(-1).copy()
    mask[int(part.elem_nodes[2, inner[1]]) * U] = 1
    flagged = system.DeviceMesh(ctx, part, U, mask)
    fmf, fbnd = system.MatrixFreeSystem(flagged, D2), system.BoundaryTerm(flagged, ADI, *part.boundary_sides([0, 1]))
    fasm = condensed(flagged)
    fasm.begin().add(fmf).add(fbnd)
    with pytest.raises(system.L3KError, match="no stored diagonal"):
        fasm.end()
    assert fasm.info.state == "open"
    with pytest.raises(system.L3KError, match="eliminated"):
        fasm.add(fmf)  # the store is factored: begin starts over
    with pytest.raises(system.L3KError, match="eliminated"):
        fasm.end()
    fasm.begin().add(fmf)
    assert fasm.info.state == "open"


def test_a_dropped_condensed_system_is_destroyed(ctx):
    part = system.SquarePartition((3, 2), 3)
    mesh = system.DeviceMesh(ctx, part, U)
    mf, bnd = system.MatrixFreeSystem(mesh, D2), system.BoundaryTerm(mesh, ADI, *part.boundary_sides([0]))
    asm = condensed(mesh)
    op = assemble(asm, mf, bnd)
    assert asm.cond_info.store_bytes > 0
    views = (asm.row_ptr, asm.col_ind, asm.values, asm.rhs)
    alive = weakref.ref(asm)
    del asm
    gc.collect()
    assert alive() is not None and views[2].data_ptr() == op.values.data_ptr()
    del op
    gc.collect()
    assert alive() is not None  # the views alone hold it
    del views
    gc.collect()
    assert alive() is None


# --------------------------------------------------------------------------------------------------- 10. pivot failure
def test_pivot_failure_leaves_no_nan(ctx, wall_id, mass_id):
    part, mesh, terms, sys_fields, R, _ = subset_problem(ctx, wall_id, mass_id, False)
    asm = condensed(mesh, field_inds=sys_fields, n_rhs=R)
    asm.begin().add(terms[0][0])
    lib = capi.load()
    assert lib.l3k_asm_end(asm._h, None, 0) == -2
    assert "non-positive pivot in the element-internal block" in lib.l3k_last_error().decode()
    assert asm.cond_info.n_failed == part.n_elems and asm.info.state == "open"
    assert torch.isfinite(asm.values).all().item() and torch.isfinite(asm.rhs).all().item()
    assert asm.values.abs().max().item() > 0  # the primary blocks are there, no update was subtracted
    asm.begin()
    assert asm.cond_info.n_failed == 0


def test_degenerate_quad(ctx):
    part = system.SquarePartition((3, 2), 2, perturb=0.1)
    verts = part.elem_verts.copy()
    verts[4, [0, 1]] = verts[4, [1, 0]]
    part.elem_verts = verts
    mesh = system.DeviceMesh(ctx, part, U)
    asm = condensed(mesh).begin()
    with pytest.raises(system.L3KError, match="error -2: Encountered degenerate element"):
        asm.add(system.MatrixFreeSystem(mesh, D2))


# ------------------------------------------------------------------------------------------------------ 11. C++ mirror
def test_cpp_mirror_agrees_with_the_python_route(ctx, tmp_path):
    """tests/cpp/quad_condense_shim.cpp: l3k::AssembledSystem with Condensation::ElementBoundary assembles, solves and recovers
    the Diffusion2D problem on 2 x 2 quads of order 3 and writes its solution; the same steps through system.AssembledSystem"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe, out = str(tmp_path / "quad_condense_shim"), str(tmp_path / "solution.bin")
    cmd = [hipcc, "-std=c++20", "-O1", "--offload-arch=gfx950", f"-I{ROOT}/include", os.path.join(ROOT, "tests", "cpp", "quad_condense_shim.cpp"),
           f"-L{ROOT}/l3ster_amd/lib", "-ll3k", f"-Wl,-rpath,{ROOT}/l3ster_amd/lib", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe, out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr
    x_cpp = np.fromfile(out, dtype=np.float64)
    p = 3
    part = system.SquarePartition(2, p)
    mask = part.dirichlet_mask(U, sides=(2, 3))
    mesh = system.DeviceMesh(ctx, part, U, mask)
    mf, bnd = system.MatrixFreeSystem(mesh, D2), system.BoundaryTerm(mesh, ADI, *part.boundary_sides([0, 1]))
    n = part.n_local_nodes * U
    g = system.values_at_nodes(mesh, system.RESIDUAL_COORDX2D, [0], torch.zeros(n, dtype=torch.float64, device="cuda"),
                               face_elem=part.boundary_sides([2, 3])[0], face_side=part.boundary_sides([2, 3])[1])
    asm = condensed(mesh)
    op = assemble(asm, mf, bnd, dirichlet_vals=g[None, :])
    sol = torch.zeros(n, dtype=torch.float64, device="cuda")
    res = solve.pcg(op, asm.rhs[0], sol, op.jacobi_inverse(), tol=1e-13, residual_scaling="rhs", max_iters=20000)
    assert res.converged
    asm.recover(sol)
    x_py = sol.cpu().numpy()
    assert x_cpp.shape == x_py.shape
    diff = np.abs(x_cpp - x_py).max()
    print(f"C++ mirror against the Python route: max difference {diff:.2e}")
    assert diff <= 1e-13 * max(1.0, np.abs(x_py).max())
