"""The assembled path on quadrilateral meshes and the assembled system as one object (l3k_asm_*, system.AssembledSystem): element
systems of quads against the goldens, the oracle and the numpy restatement of quad_asm_ref.py, side systems, the CSR system as the
sum of the local systems, sub-batches, the assembled operator against the matrix-free one, the reference's
Diffusion2DAssembledTest end to end, hexes through the same object, and the states and refusals.

Tolerances: entrywise 1e-12 max|K_e| at element level, relative L2 <= 1e-11 at mesh level, the reference's 1e-8
end to end."""
import numpy as np
import pytest

import oracle_lib as O
import quad_asm_ref as QA
import quad_side_ref as QS
from helpers import rel_err
from l3ster_amd import solve, system
from test_gpu_quad import SingleQuad
from test_oracle_boundary import QUAD

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

U = 3
D2, D2V, ADI = system.KERNEL_DIFFUSION2D, system.KERNEL_DIFFUSION2D_VAR, system.KERNEL_ADIABATIC2D
ORACLE_ID = {D2: O.KERNEL_DIFFUSION2D, D2V: O.KERNEL_DIFFUSION2D_VAR}


@pytest.fixture(scope="module")
def ctx():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    torch.cuda.set_device(0)
    return system.Context(0, torch.cuda.current_stream().cuda_stream)


def dev(a, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


def dense_of(A):
    """The dense copy of an AssembledSystem's (or CsrOperator's) matrix"""
    import scipy.sparse as sp
    return sp.csr_matrix((A.values.cpu().numpy(), A.col_ind.cpu().numpy(), A.row_ptr.cpu().numpy()), shape=(A.n, A.n)).toarray()


def value_order(p, nq):
    vo = (nq - 1) // p
    assert system.n_qps1d(p, vo, 0) == nq
    return vo


def elem_dofs(part, e, dpn, field_inds):
    return (part.elem_nodes[e].astype(np.int64)[:, None] * dpn + np.asarray(field_inds)[None, :]).reshape(-1)


# ---------------------------------------------------------------------------------------------------------- 1. goldens
@pytest.mark.parametrize("name", ["quad_p4_diff", "quad_p4_var"])
def test_element_system_vs_golden(ctx, golden, name):
    g = golden(name)
    kid, p, nq, R = int(g["kid"]), int(g["p"]), int(g["nq"]), int(g["R"])
    assert (p, nq, R) == (4, 9, 2)
    mesh = system.DeviceMesh(ctx, SingleQuad(p, g["verts"]), U)
    mf = system.MatrixFreeSystem(mesh, kid, asm_opts=(value_order(p, nq), 0, 0), n_rhs=R)
    if "node_fields" in g:
        mf.set_fields(dev(g["node_fields"].T))
    K, F = mf.element_systems()
    K2, F2 = mf.element_systems()
    torch.cuda.synchronize()
    Nd = (p + 1) ** 2 * U
    assert K.shape == (1, Nd, Nd) and F.shape == (1, R, Nd)
    err = np.abs(K[0].cpu().numpy() - g["K"]).max() / np.abs(g["K"]).max()
    print(f"{name}: max|K - K_golden| / max|K| = {err:.2e}")
    assert err <= 1e-12
    assert torch.equal(K[0], K[0].T)                   # bitwise symmetric
    assert torch.equal(K, K2) and torch.equal(F, F2)   # the same bits on every run
    assert np.array_equal(F[0].cpu().numpy().T, g["F"])  # (no source term: identically zero)
    # either output may be left out
    K3, none = mf.element_systems(want_F=False)
    assert none is None and torch.equal(K3, K)


# ------------------------------------------------------------------------------------------- 2. the oracle, every element
SHAPES = [(D2, p, p + 1, R) for p in range(1, 7) for R in (1, 2)] + [(D2, 4, 9, 1), (D2, 4, 9, 2)] + \
         [(D2V, 2, 3, 1), (D2V, 2, 3, 2), (D2V, 4, 5, 1), (D2V, 4, 9, 1), (D2V, 4, 9, 2)]


@pytest.mark.parametrize("kid,p,nq,R", SHAPES, ids=[f"k{k}-p{p}-nq{nq}-R{R}" for k, p, nq, R in SHAPES])
def test_element_systems_vs_oracle(ctx, kid, p, nq, R):
    part = system.SquarePartition((3, 2), p, perturb=0.15)
    mesh = system.DeviceMesh(ctx, part, U)
    mf = system.MatrixFreeSystem(mesh, kid, asm_opts=(value_order(p, nq), 0, 0), n_rhs=R)
    fields = None
    if kid == D2V:
        fields = np.random.default_rng(p).uniform(0.5, 1.5, (1, part.n_local_nodes))
        mf.set_fields(dev(fields))
    first, count = 1, 4  # not the whole mesh
    K, F = mf.element_systems(first, count)
    torch.cuda.synchronize()
    assert torch.equal(K, K.transpose(1, 2))
    Kh, Fh = K.cpu().numpy(), F.cpu().numpy()
    worst = 0.0
    for i in range(count):
        e = first + i
        nf = None if fields is None else fields[:, part.elem_nodes[e]].T
        K_ref, F_ref = O.assemble_local(ORACLE_ID[kid], p, nq, R, part.elem_verts[e], node_fields=nf)
        err = np.abs(Kh[i] - K_ref).max() / np.abs(K_ref).max()
        worst = max(worst, err)
        assert err <= 1e-12, (e, err)
        assert np.array_equal(Fh[i].T, F_ref)  # zero
    print(f"kernel {kid} p {p} nq {nq} R {R}: worst max|K - K_oracle| / max|K| = {worst:.2e}")


# ------------------------------------------------------------------------------- 3. source term and point dependence
SOURCE_SRC = """
struct QuadAsmSource {
    static constexpr l3k::KernelParams params{.dimension = 2, .n_equations = 4, .n_unknowns = 3};
    template <typename In, typename Out> L3K_HD void operator()(const In& in, Out& out) const {
        const double x = in.point.space.x(), y = in.point.space.y(), t = in.point.time;
        auto& [operators, rhs] = out;
        auto& [A0, Ax, Ay] = operators;
        Ax(0, 1) = -1.; Ay(0, 2) = -1.;
        A0(1, 1) = -(1. + .5 * x * y); Ax(1, 0) = 1.;
        A0(2, 2) = -1.; Ay(2, 0) = 1.;
        Ax(3, 2) = 1.;  Ay(3, 1) = -1.;
        for (int r = 0; r < rhs.cols(); ++r) {
            rhs(0, r) = (r + 1) * (1. + x + 2. * y + t);
            rhs(2, r) = sin(x - y) - r * t;
        }
    }
};"""


def source_kernel(R):
    def kernel(vals, ders, point, normal, time):
        A0, A1, A2, _ = QA.diffusion2d()(vals, ders, point, normal, time)
        x, y = point[0], point[1]
        A0[1, 1] = -(1.0 + 0.5 * x * y)
        f = np.zeros((4, R))
        for r in range(R):
            f[0, r] = (r + 1) * (1.0 + x + 2.0 * y + time)
            f[2, r] = np.sin(x - y) - r * time
        return A0, A1, A2, f
    return kernel


@pytest.fixture(scope="module")
def source_id():
    from l3ster_amd import plugin
    return plugin.compile_kernel("QuadAsmSource", SOURCE_SRC, kernel_id=1341, shapes=[(2, 3, 1), (2, 3, 2), (4, 5, 1), (4, 5, 2)])


@pytest.mark.parametrize("p", [2, 4])
@pytest.mark.parametrize("R", [1, 2])
def test_source_term_vs_restatement(ctx, source_id, p, R):
    part = system.SquarePartition((3, 2), p, perturb=0.15)
    mf = system.MatrixFreeSystem(system.DeviceMesh(ctx, part, U), source_id, n_rhs=R)
    mf.set_time(0.3)
    first, count = 2, 3
    K, F = mf.element_systems(first, count)
    K2, F2 = mf.element_systems(first, count)
    torch.cuda.synchronize()
    assert torch.equal(K, K.transpose(1, 2)) and torch.equal(K, K2) and torch.equal(F, F2)
    for i in range(count):
        K_ref, F_ref = QA.element_system(source_kernel(R), p, p + 1, part.elem_verts[first + i], time=0.3)
        assert np.abs(F_ref).max() > 0
        ek = np.abs(K[i].cpu().numpy() - K_ref).max() / np.abs(K_ref).max()
        ef = np.abs(F[i].cpu().numpy().T - F_ref).max() / np.abs(F_ref).max()
        print(f"source plugin p {p} R {R} element {first + i}: K {ek:.2e}, F {ef:.2e}")
        assert ek <= 1e-12 and ef <= 1e-12


# --------------------------------------------------------------------------------------------------- 4. side systems
@pytest.mark.parametrize("p", [1, 2, 4, 6])
def test_adiabatic_side_systems_vs_oracle(ctx, p):
    """All four sides of every element of a 3 x 2 mesh (each of them is a boundary element)"""
    part = system.SquarePartition((3, 2), p, perturb=0.15)
    assert np.all(part.elem_boundary != 0)
    fe, fs = np.repeat(np.arange(part.n_elems), 4), np.tile(np.arange(4), part.n_elems)
    term = system.BoundaryTerm(system.DeviceMesh(ctx, part, U), ADI, fe, fs)
    K, F = term.side_systems()
    K2, F2 = term.side_systems()
    Ks, Fs = term.side_systems(first=5, count=7)
    torch.cuda.synchronize()
    Nd = (p + 1) ** 2 * U
    assert K.shape == (len(fe), Nd, Nd) and F.shape == (len(fe), 1, Nd)
    assert torch.equal(K, K.transpose(1, 2)) and torch.equal(K, K2) and torch.equal(F, F2)
    assert torch.equal(Ks, K[5:12]) and torch.equal(Fs, F[5:12])
    Kh = K.cpu().numpy()
    worst = 0.0
    for i, (e, s) in enumerate(zip(fe, fs)):
        K_ref, F_ref = O.assemble_local_side(int(s), O.KERNEL_ADIABATIC2D, p, p + 1, 1, part.elem_verts[e])
        err = np.abs(Kh[i] - K_ref).max() / np.abs(K_ref).max()
        worst = max(worst, err)
        assert err <= 1e-12, (e, s, err)
    assert not F.any().item()
    print(f"Adiabatic2D p {p}: worst max|K_s - K_oracle| / max|K_s| = {worst:.2e}")


@pytest.fixture(scope="module")
def wall_id():
    from l3ster_amd import plugin
    return plugin.compile_kernel("QuadAsmWall", QS.PLUGIN_SRC.replace("QuadWallPlugin", "QuadAsmWall"), kernel_id=1342,
                                 shapes=[(2, 3, 2)], kind="boundary")


def wall_kernel(vals, ders, point, normal, time):
    return QS.wall_plugin(vals, ders, point, time, normal)


def test_plugin_side_systems_vs_restatement(ctx, wall_id):
    """A boundary kernel with derivative operators, a field, the point, the time and a source: K_s couples nodes off the side"""
    part = system.SquarePartition((3, 2), 2, perturb=0.15)
    fe, fs = part.boundary_sides()
    fields = np.random.default_rng(3).uniform(0.5, 1.5, (1, part.n_local_nodes))
    term = system.BoundaryTerm(system.DeviceMesh(ctx, part, 4), wall_id, fe, fs, field_inds=[3, 1], n_rhs=2)
    term.set_fields(dev(fields))
    term.set_time(0.4)
    K, F = term.side_systems()
    K2, F2 = term.side_systems()
    torch.cuda.synchronize()
    assert torch.equal(K, K.transpose(1, 2)) and torch.equal(K, K2) and torch.equal(F, F2)
    for i, (e, s) in enumerate(zip(fe, fs)):
        K_ref, F_ref = QA.side_system(wall_kernel, int(s), 2, 3, part.elem_verts[e], fields[:, part.elem_nodes[e]].T, time=0.4)
        assert np.count_nonzero(K_ref) > (3 * 2) ** 2  # derivative operators reach beyond the 3 nodes of the side
        ek = np.abs(K[i].cpu().numpy() - K_ref).max() / np.abs(K_ref).max()
        ef = np.abs(F[i].cpu().numpy().T - F_ref).max() / np.abs(F_ref).max()
        assert ek <= 1e-12 and ef <= 1e-12, (e, s, ek, ef)


@pytest.mark.parametrize("side", range(4))
def test_side_system_is_the_boundary_apply(ctx, wall_id, side):
    """Path check on one element: K_s x_e against BoundaryTerm.apply, F_s against its rhs"""
    part = SingleQuad(2, QUAD)
    dpn, fi = 4, [3, 1]
    term = system.BoundaryTerm(system.DeviceMesh(ctx, part, dpn), wall_id, [0], [side], field_inds=fi, n_rhs=2)
    rng = np.random.default_rng(side)
    term.set_fields(dev(rng.uniform(0.5, 1.5, (1, part.n_local_nodes))))
    term.set_time(0.4)
    K, F = term.side_systems()
    n = part.n_local_nodes * dpn
    x = rng.uniform(-1, 1, (2, n))
    Y = torch.zeros((2, n), dtype=torch.float64, device="cuda")
    term.apply(dev(x), Y)
    dofs = elem_dofs(part, 0, dpn, fi)
    want = np.zeros((2, n))
    want[:, dofs] = (K[0].cpu().numpy() @ x[:, dofs].T).T
    assert rel_err(Y.cpu().numpy(), want) <= 1e-12
    diag = torch.zeros(n, dtype=torch.float64, device="cuda")
    rhs = torch.zeros((2, n), dtype=torch.float64, device="cuda")
    term.diag_rhs(diag, rhs)
    assert rel_err(rhs.cpu().numpy()[:, dofs], F[0].cpu().numpy()) <= 1e-12


# ------------------------------------------------------------------------------ 5. global system = sum of local systems
def host_sum(part, p, fe, fs):
    """Diffusion2D on every element plus Adiabatic2D on the listed sides, summed on the host through elem_nodes"""
    n = part.n_local_nodes * U
    A = np.zeros((n, n))
    for e in range(part.n_elems):
        d = elem_dofs(part, e, U, range(U))
        A[np.ix_(d, d)] += O.assemble_local(O.KERNEL_DIFFUSION2D, p, p + 1, 1, part.elem_verts[e])[0]
    for e, s in zip(fe, fs):
        d = elem_dofs(part, e, U, range(U))
        A[np.ix_(d, d)] += O.assemble_local_side(int(s), O.KERNEL_ADIABATIC2D, p, p + 1, 1, part.elem_verts[e])[0]
    return A


def assemble(asm, mf, bnd, dirichlet_vals=None):
    asm.begin()
    asm.add(mf)
    asm.add(bnd)
    return asm.end(dirichlet_vals)


@pytest.mark.parametrize("p", [2, 3])
def test_global_system_is_the_sum_of_the_local_systems(ctx, p):
    part = system.SquarePartition((5, 4), p, perturb=0.15)
    mesh = system.DeviceMesh(ctx, part, U)  # no Dirichlet mask
    fe, fs = part.boundary_sides([0, 3])
    mf, bnd = system.MatrixFreeSystem(mesh, D2), system.BoundaryTerm(mesh, ADI, fe, fs)
    asm = system.AssembledSystem(mesh)
    assert asm.info.state == "new"
    op = assemble(asm, mf, bnd)
    info = asm.info
    assert info.state == "closed" and info.n_missing == 0 and info.n == part.n_local_nodes * U == op.n
    assert op.values.data_ptr() == asm.values.data_ptr()  # a view, not a copy
    A, want = dense_of(asm), host_sum(part, p, fe, fs)
    scale = np.abs(want).max()
    print(f"p {p}: max|A - sum| / max|A| = {np.abs(A - want).max() / scale:.2e}")
    assert np.abs(A - want).max() <= 1e-12 * scale
    assert not asm.rhs.any().item()
    # again: the scatter's atomics reorder at most four terms per entry
    assemble(asm, mf, bnd)
    assert np.abs(dense_of(asm) - A).max() <= 1e-13 * scale and asm.info.n_missing == 0


# ----------------------------------------------------------------------------------------------------- 6. sub-batches
def test_sub_batches(ctx):
    p = 3
    part = system.SquarePartition((7, 5), p, perturb=0.15)
    mesh = system.DeviceMesh(ctx, part, U)
    fe, fs = part.boundary_sides([1, 2])
    mf, bnd = system.MatrixFreeSystem(mesh, D2), system.BoundaryTerm(mesh, ADI, fe, fs)
    Nd = (p + 1) ** 2 * U
    workspace = 2 * 10 * 8 * Nd * Nd  # two halves of at most ten element matrices
    assert -(-part.n_elems // (workspace // 2 // (8 * Nd * Nd))) >= 3  # at least three sub-batches of element systems
    small, default = system.AssembledSystem(mesh, workspace_bytes=workspace), system.AssembledSystem(mesh)
    assemble(small, mf, bnd)
    assemble(default, mf, bnd)
    A, B = dense_of(small), dense_of(default)
    assert small.info.n_missing == 0 and default.info.n_missing == 0
    assert torch.equal(small.col_ind, default.col_ind) and torch.equal(small.row_ptr, default.row_ptr)
    assert np.abs(B).max() > 0 and np.abs(A - B).max() <= 1e-13 * np.abs(B).max()
    assert np.abs(B - host_sum(part, p, fe, fs)).max() <= 1e-12 * np.abs(B).max()


# ------------------------------------------------------------------------------------------ 7. assembled = matrix-free
@pytest.mark.parametrize("p", [2, 4, 6])
def test_assembled_operator_is_the_matrix_free_one(ctx, p):
    part = system.SquarePartition((4, 3), p, perturb=0.15)
    mask = part.dirichlet_mask(U, sides=(2, 3))
    mesh = system.DeviceMesh(ctx, part, U, mask)
    mf, bnd = system.MatrixFreeSystem(mesh, D2), system.BoundaryTerm(mesh, ADI, *part.boundary_sides([0, 1]))
    mf.attach_boundary(bnd)
    op = assemble(system.AssembledSystem(mesh), mf, bnd)
    free = mask == 0
    x = np.random.default_rng(p).uniform(-1, 1, (1, op.n)) * free
    Ya, Ym = torch.zeros((1, op.n), dtype=torch.float64, device="cuda"), torch.zeros((1, op.n), dtype=torch.float64, device="cuda")
    op.apply(dev(x), Ya)
    mf.apply(dev(x), Ym)
    torch.cuda.synchronize()
    err = rel_err(Ya.cpu().numpy()[0, free], Ym.cpu().numpy()[0, free])
    print(f"p {p}: ||A_csr x - A_mf x|| / ||A_mf x|| on the free rows = {err:.2e}")
    assert err <= 1e-11


# ---------------------------------------------------------------------- 8. the reference's Diffusion2DAssembledTest
def test_diffusion2d_assembled_end_to_end(ctx):
    """tests/Diffusion2D.hpp, Diffusion2DAssembledTest: 4 x 4 quads on [0,1]^2, order 2, Dirichlet T = x on the left and right
    sides (the values of CoordX2D at the nodes), Adiabatic2D on the bottom and top; AssembledSystem -> Jacobi PCG on the CSR
    operator with the reference's solver tolerance 1e-10; the L2 error against T = x, q = (1, 0) over the domain and over the four
    sides stays below the reference's eps = 1e-8 (:116-118)."""
    p = 2
    part = system.SquarePartition(4, p)
    mask = part.dirichlet_mask(U, sides=(2, 3))
    mesh = system.DeviceMesh(ctx, part, U, mask)
    mf, bnd = system.MatrixFreeSystem(mesh, D2), system.BoundaryTerm(mesh, ADI, *part.boundary_sides([0, 1]))
    n = part.n_local_nodes * U
    g = system.values_at_nodes(mesh, system.RESIDUAL_COORDX2D, [0], torch.zeros(n, dtype=torch.float64, device="cuda"),
                               face_elem=part.boundary_sides([2, 3])[0], face_side=part.boundary_sides([2, 3])[1])
    asm = system.AssembledSystem(mesh)
    op = assemble(asm, mf, bnd, g[None, :])
    assert asm.info.n_missing == 0
    minv = op.jacobi_inverse()
    sol = torch.zeros(n, dtype=torch.float64, device="cuda")
    res = solve.pcg(op, asm.rhs[0], sol, minv, tol=1e-10, residual_scaling="rhs", max_iters=20000)
    assert res.converged
    fields = sol.view(-1, U).T.contiguous()
    err = np.linalg.norm(system.norm_l2(mesh, system.RESIDUAL_LINEAR2D_ERROR, fields))
    fe, fs = part.boundary_sides()
    berr = np.linalg.norm(system.norm_l2(mesh, system.RESIDUAL_LINEAR2D_ERROR, fields, face_elem=fe, face_side=fs))
    print(f"assembled PCG: {res.num_iters} iterations, achieved {res.tol:.2e}; L2 error domain {err:.2e}, sides {berr:.2e}")
    assert err < 1e-8 and berr < 1e-8
    # the matrix-free solve of the same problem
    mf.attach_boundary(bnd)
    diag, rhs = mf.diag_rhs(g[None, :])
    sol_mf = torch.zeros_like(rhs[0])
    res_mf = solve.pcg(mf, rhs[0].contiguous(), sol_mf, solve.jacobi_inverse_native(ctx, diag), tol=1e-10, residual_scaling="rhs",
                       max_iters=20000)
    assert res_mf.converged
    diff = (sol - sol_mf).abs().max().item()
    print(f"assembled against matrix-free at the nodes: {diff:.2e}")
    assert diff <= 1e-7


# ------------------------------------------------------------------------------------- 9. hexes through the same object
def test_hexes_through_the_same_object(ctx):
    U3, kpar = 4, [0.7, 1.3]
    part = system.CubePartition(2, 2, perturb=0.15)
    mask = part.dirichlet_mask(U3)
    mesh = system.DeviceMesh(ctx, part, U3, mask)
    mf = system.MatrixFreeSystem(mesh, system.KERNEL_DIFFUSION3D, kpar)
    bnd = system.BoundaryTerm(mesh, system.KERNEL_ADIABATIC3D, *part.boundary_sides([1]))
    n = part.n_local_nodes * U3
    g = dev(np.where(mask != 0, np.sin(np.arange(n) * 0.37), 0.0)[None, :])
    asm = system.AssembledSystem(mesh)
    op = assemble(asm, mf, bnd, g)
    assert asm.info.n_missing == 0 and asm.info.state == "closed"
    # the same system on hand-wired arrays
    graph = mf.sparsity_graph()
    assert torch.equal(graph.row_ptr, asm.row_ptr) and torch.equal(graph.col_ind, asm.col_ind)
    vals = torch.zeros(graph.info.nnz, dtype=torch.float64, device="cuda")
    rhs = torch.zeros((1, n), dtype=torch.float64, device="cuda")
    assert mf.assemble_global(graph.row_ptr, graph.col_ind, vals, rhs) == 0
    assert bnd.assemble_global(graph.row_ptr, graph.col_ind, vals, rhs) == 0
    system.CsrOperator(ctx, graph.row_ptr, graph.col_ind, vals).dirichlet(dev(mask, torch.uint8), g, rhs)
    scale = vals.abs().max().item()
    assert scale > 0 and (asm.values - vals).abs().max().item() <= 1e-12 * scale
    assert (asm.rhs - rhs).abs().max().item() <= 1e-12 * max(rhs.abs().max().item(), scale)
    # element and side systems: the existing launchers, bit for bit
    K, F = mf.element_systems(1, 5)
    K0, F0, _ = mf.local_assemble(1, 5)
    assert torch.equal(K, K0) and torch.equal(F, F0)
    Ks, Fs = bnd.side_systems()
    Ks0, Fs0 = bnd.local_assemble()
    assert torch.equal(Ks, Ks0) and torch.equal(Fs, Fs0)


# ------------------------------------------------------------------------------------------ 10. states and refusals
def test_states_and_refusals(ctx):
    part = system.SquarePartition((3, 2), 2, perturb=0.1)
    mesh = system.DeviceMesh(ctx, part, U, part.dirichlet_mask(U, sides=(2, 3)))
    mf, bnd = system.MatrixFreeSystem(mesh, D2), system.BoundaryTerm(mesh, ADI, *part.boundary_sides([0, 1]))
    asm = system.AssembledSystem(mesh)
    with pytest.raises(system.L3KError, match="not open"):
        asm.add(mf)  # before begin
    with pytest.raises(system.L3KError, match="not open"):
        asm.end()
    op = assemble(asm, mf, bnd)
    A = dense_of(asm)
    with pytest.raises(system.L3KError, match="not open"):
        asm.add(bnd)  # after end
    with pytest.raises(system.L3KError, match="not open"):
        asm.end()  # twice
    # begin after end reopens and zeroes
    asm.begin()
    assert asm.info.state == "open" and not asm.values.any().item() and not asm.rhs.any().item()
    with pytest.raises(system.L3KError, match="range"):
        asm.add(mf, 4, 3)
    with pytest.raises(system.L3KError, match="range"):
        asm.add(bnd, 0, bnd.n_faces + 1)
    with pytest.raises(system.L3KError, match="n_rhs"):
        asm.add(system.MatrixFreeSystem(mesh, D2, n_rhs=2))
    other = system.DeviceMesh(ctx, part, U)
    with pytest.raises(system.L3KError, match="another mesh"):
        asm.add(system.MatrixFreeSystem(other, D2))
    # a 3-D term on a quad system and the reverse
    hexm = system.DeviceMesh(ctx, system.CubePartition(2, 2), 4)
    mf3 = system.MatrixFreeSystem(hexm, system.KERNEL_DIFFUSION3D)
    with pytest.raises(system.L3KError, match="dimension 3 on a system of dimension 2"):
        asm.add(mf3)
    asm3 = system.AssembledSystem(hexm).begin()
    with pytest.raises(system.L3KError, match="dimension 2 on a system of dimension 3"):
        asm3.add(bnd)
    # field_inds that are not a subset of the system's
    wide = system.DeviceMesh(ctx, part, 5)
    narrow = system.AssembledSystem(wide, field_inds=[0, 1, 2]).begin()
    with pytest.raises(system.L3KError, match="not a subset"):
        narrow.add(system.MatrixFreeSystem(wide, D2, field_inds=[0, 1, 4]))
    narrow.add(system.MatrixFreeSystem(wide, D2, field_inds=[2, 0, 1]))  # a subset in any order
    with pytest.raises(system.L3KError, match="field_inds"):
        system.AssembledSystem(wide, field_inds=[2, 1])
    with pytest.raises(system.L3KError, match="n_rhs"):
        system.AssembledSystem(mesh, n_rhs=0)
    # a partitioned mesh
    ghosted = system.DeviceMesh(ctx, system.CubePartition(2, 2, parts=(2, 1, 1), rank=1), 4)  # (rank 1 holds the ghost nodes)
    with pytest.raises(system.L3KError, match="partitioned"):
        system.AssembledSystem(ghosted)
    # the interrupted assembly above left the system open and untouched: it still assembles the same matrix
    asm.add(mf)
    asm.add(bnd)
    asm.end()
    assert np.abs(dense_of(asm) - A).max() <= 1e-13 * np.abs(A).max()
    assert op.values.data_ptr() == asm.values.data_ptr()


def test_a_dropped_system_is_destroyed(ctx):
    """The views and the operator keep the system alive, the system keeps none of them: once they are gone the object is collected
    (and l3k_asm_destroy frees its device arrays)"""
    import gc
    import weakref
    part = system.SquarePartition((3, 2), 2)
    mesh = system.DeviceMesh(ctx, part, U)
    mf, bnd = system.MatrixFreeSystem(mesh, D2), system.BoundaryTerm(mesh, ADI, *part.boundary_sides([0]))
    asm = system.AssembledSystem(mesh)
    op = assemble(asm, mf, bnd)
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


def test_degenerate_quad(ctx):
    """Two vertices of one element swapped: |J| <= 0 there, error -2 from the element systems and from the global sum"""
    part = system.SquarePartition((3, 2), 2, perturb=0.1)
    verts = part.elem_verts.copy()
    verts[4, [0, 1]] = verts[4, [1, 0]]
    part.elem_verts = verts
    mesh = system.DeviceMesh(ctx, part, U)
    mf = system.MatrixFreeSystem(mesh, D2)
    with pytest.raises(system.L3KError, match="error -2: Encountered degenerate element"):
        mf.element_systems()
    K, _ = mf.element_systems(0, 4)  # the sound elements before it
    assert torch.isfinite(K).all().item()
    asm = system.AssembledSystem(mesh).begin()
    with pytest.raises(system.L3KError, match="error -2: Encountered degenerate element"):
        asm.add(mf)
