"""Quadrilateral (2-D) meshes on the device: the matrix-free apply and diag / rhs of Diffusion2D / Diffusion2DVar against the
golden fixtures and the CPU oracle (orc_mf_apply / orc_mf_diag_rhs with dim = 2), the split-phase and multi-rank schedule,
deterministic mode, routes, an end-to-end Jacobi-PCG solve, a 2-D plugin kernel and the refusals of the entry points that
have no quad kernels."""
import threading

import numpy as np
import pytest

import oracle_lib as O
from helpers import rel_err
from l3ster_amd import partition, solve, system

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

U = 3
D2, D2V = system.KERNEL_DIFFUSION2D, system.KERNEL_DIFFUSION2D_VAR


@pytest.fixture(scope="module")
def ctx():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    torch.cuda.set_device(0)
    return system.Context(0, torch.cuda.current_stream().cuda_stream)


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")


class SingleQuad:
    """One quad with identity numbering (duck-types SquarePartition)."""

    def __init__(self, order, verts):
        N = (order + 1) ** 2
        self.dim, self.order = 2, order
        self.n_elems = self.n_interior_elems = 1
        self.n_owned_nodes, self.n_ghost_nodes = N, 0
        self.n_local_nodes = N
        self.elem_nodes = np.arange(N, dtype=np.uint32).reshape(1, N)
        self.elem_verts = np.asarray(verts, dtype=np.float64).reshape(1, 4, 3)


def oracle_mesh2(part, nq, dofs_per_node, field_inds, dirichlet=None, fields=None):
    return O.MeshView(2, part.order, nq, part.elem_nodes, part.elem_verts, part.n_local_nodes, dofs_per_node, field_inds,
                      dirichlet, fields)


def make_mask(part, kind, dpn=U, seed=0):
    if kind == "none":
        return None
    if kind == "boundary":
        return part.dirichlet_mask(dpn)
    return (np.random.default_rng(seed).uniform(size=part.n_local_nodes * dpn) < 0.2).astype(np.uint8)


# ---------------------------------------------------------------------------------------------------------- 1. goldens
@pytest.mark.parametrize("name", ["quad_p4_diff", "quad_p4_var"])
def test_single_quad_vs_golden(ctx, golden, name):
    g = golden(name)
    kid, p, nq, R = int(g["kid"]), int(g["p"]), int(g["nq"]), int(g["R"])
    assert (p, nq, R) == (4, 9, 2)
    vo = (nq - 1) // p
    part = SingleQuad(p, g["verts"])
    mesh = system.DeviceMesh(ctx, part, U)
    mf = system.MatrixFreeSystem(mesh, kid, asm_opts=(vo, 0, 0), n_rhs=R)
    fields = dev(g["node_fields"].T) if "node_fields" in g else None
    if fields is not None:
        mf.set_fields(fields)
    assert "quadApplyKernel<p=4,nq=9" in mf.route(2, R), mf.route(2, R)
    X = dev(g["x"].T)
    Y = torch.full_like(X, 7.0)
    mf.apply(X, Y, 1.0, 0.0)
    torch.cuda.synchronize()
    assert rel_err(Y.cpu().numpy().T, g["y"]) < 1e-12
    Y0 = dev(np.random.default_rng(0).uniform(-1, 1, g["x"].T.shape))
    Y2 = Y0.clone()
    mf.apply(X, Y2, -0.5, 2.0)
    assert rel_err(Y2.cpu().numpy().T, -0.5 * g["y"] + 2.0 * Y0.cpu().numpy().T) < 1e-12
    # one column of the two-column system
    Y1 = torch.zeros_like(X[:1])
    mf.apply(X[:1].contiguous(), Y1)
    torch.cuda.synchronize()
    assert rel_err(Y1.cpu().numpy()[0], g["y"][:, 0]) < 1e-12
    # diag and the lifted rhs with the golden Dirichlet dofs and values
    mask = np.zeros(part.n_local_nodes * U, np.uint8)
    mask[g["dir_inds"]] = 1
    vals = np.zeros((R, part.n_local_nodes * U))
    vals[:, g["dir_inds"]] = g["dir_vals"].T
    mesh_d = system.DeviceMesh(ctx, part, U, mask)
    mf_d = system.MatrixFreeSystem(mesh_d, kid, asm_opts=(vo, 0, 0), n_rhs=R)
    if fields is not None:
        mf_d.set_fields(fields)
    diag, rhs = mf_d.diag_rhs(dev(vals))
    torch.cuda.synchronize()
    free = mask == 0
    assert rel_err(diag.cpu().numpy()[free], g["diag"][free]) < 1e-12
    assert rel_err(rhs.cpu().numpy().T[free], g["rhs_lifted"][free]) < 1e-12
    assert np.all(diag.cpu().numpy()[~free] == 1.0)
    np.testing.assert_array_equal(rhs.cpu().numpy()[:, ~free], vals[:, ~free])


# ------------------------------------------------------------------------------------------------ 2. + 3. mesh parity
MESH_CASES = [(p, ne) for p, ne in [(1, (12, 9)), (2, (9, 7)), (3, (7, 5)), (4, (6, 5)), (5, (4, 5)), (6, (4, 3))]]


@pytest.mark.parametrize("p,ne", MESH_CASES)
@pytest.mark.parametrize("mask_kind", ["none", "boundary", "random"])
@pytest.mark.parametrize("R", [1, 2])
def test_mesh_apply_vs_oracle(ctx, p, ne, mask_kind, R):
    part = system.SquarePartition(ne, p, perturb=0.15)
    mask = make_mask(part, mask_kind, seed=p)
    mesh = system.DeviceMesh(ctx, part, U, mask)
    mf = system.MatrixFreeSystem(mesh, D2, n_rhs=R)
    om = oracle_mesh2(part, p + 1, U, np.arange(U), mask)
    x = part.synthetic_vector(U, ncols=R)
    rng = np.random.default_rng(p + 10 * R)
    for alpha, beta in [(1.0, 0.0), (1.0, 1.0), (rng.uniform(-2, 2), rng.uniform(-2, 2))]:
        y0 = rng.uniform(-1, 1, x.shape)
        y_ref = O.mf_apply(om, D2, x.T, np.asfortranarray(y0.T.copy()), alpha=alpha, beta=beta)
        Y = dev(y0)
        mf.apply(dev(x), Y, alpha, beta)
        torch.cuda.synchronize()
        assert rel_err(Y.cpu().numpy().T, y_ref) < 1e-11, (alpha, beta)
    # diagonal and lifted rhs
    g = rng.uniform(-1, 1, (R, part.n_local_nodes * U))
    diag, rhs = mf.diag_rhs(dev(g))
    d_ref, r_ref = O.mf_diag_rhs(om, D2, R=R, dirichlet_vals=g.T)
    torch.cuda.synchronize()
    assert rel_err(diag.cpu().numpy(), d_ref) < 1e-11
    assert rel_err(rhs.cpu().numpy().T, r_ref) < 1e-11


@pytest.mark.parametrize("p,nq,R", [(2, 3, 1), (2, 3, 2), (4, 5, 1), (4, 9, 2)])
def test_mesh_var_vs_oracle(ctx, p, nq, R):
    part = system.SquarePartition((5, 4), p, perturb=0.1)
    mask = part.dirichlet_mask(U)
    mesh = system.DeviceMesh(ctx, part, U, mask)
    vo = (nq - 1) // p
    mf = system.MatrixFreeSystem(mesh, D2V, asm_opts=(vo, 0, 0), n_rhs=R)
    fields = np.random.default_rng(3).uniform(0.5, 1.5, (1, part.n_local_nodes))
    mf.set_fields(dev(fields))
    om = oracle_mesh2(part, nq, U, np.arange(U), mask, fields)
    x = part.synthetic_vector(U, ncols=R)
    y0 = np.random.default_rng(1).uniform(-1, 1, x.shape)
    y_ref = O.mf_apply(om, D2V, x.T, np.asfortranarray(y0.T.copy()), alpha=1.5, beta=-0.25)
    Y = dev(y0)
    mf.apply(dev(x), Y, 1.5, -0.25)
    g = np.random.default_rng(2).uniform(-1, 1, (R, part.n_local_nodes * U))
    diag, rhs = mf.diag_rhs(dev(g))
    d_ref, r_ref = O.mf_diag_rhs(om, D2V, R=R, dirichlet_vals=g.T)
    torch.cuda.synchronize()
    assert rel_err(Y.cpu().numpy().T, y_ref) < 1e-11
    assert rel_err(diag.cpu().numpy(), d_ref) < 1e-11
    assert rel_err(rhs.cpu().numpy().T, r_ref) < 1e-11


def test_strided_field_inds(ctx):
    """The 3 unknowns on 3 of 4 per-node dofs (dofs_per_node = 4), two columns, padded leading dimension."""
    p, dpn, fi = 3, 4, [2, 0, 3]
    part = system.SquarePartition((6, 4), p, perturb=0.1)
    mask = np.zeros((part.n_local_nodes, dpn), np.uint8)
    mask[part.node_boundary != 0, 2] = 1
    mesh = system.DeviceMesh(ctx, part, dpn, mask.reshape(-1))
    mf = system.MatrixFreeSystem(mesh, D2, field_inds=fi, n_rhs=2)
    assert "non-dense" in mf.route(2, 2), mf.route(2, 2)
    n, pad = part.n_local_nodes * dpn, 37
    rng = np.random.default_rng(4)
    xb, yb = rng.uniform(-1, 1, (2, n + pad)), rng.uniform(-1, 1, (2, n + pad))
    X, Y = dev(xb), dev(yb)
    mf.apply(X[:, :n], Y[:, :n], 2.0, 1.0)
    om = oracle_mesh2(part, p + 1, dpn, fi, mask.reshape(-1))
    y_ref = O.mf_apply(om, D2, xb[:, :n].T, np.asfortranarray(yb[:, :n].T.copy()), alpha=2.0, beta=1.0)
    g = rng.uniform(-1, 1, (2, n))
    diag, rhs = mf.diag_rhs(dev(g))
    d_ref, r_ref = O.mf_diag_rhs(om, D2, R=2, dirichlet_vals=g.T)
    out = Y.cpu().numpy()
    assert rel_err(out[:, :n].T, y_ref) < 1e-11
    np.testing.assert_array_equal(out[:, n:], yb[:, n:])  # the padding is not touched
    assert rel_err(diag.cpu().numpy(), d_ref) < 1e-11
    assert rel_err(rhs.cpu().numpy().T, r_ref) < 1e-11


# --------------------------------------------------------------------------------------------- 4. split phase and ranks
def test_split_phase_which(ctx):
    """which = 0 + 1 and which = 3 + 4 + 1 equal which = 2 on a rank with ghosts: rank 1 of an rcb partition in 2 (the
    lower rank owns the shared nodes)."""
    p = 3
    whole = system.SquarePartition((8, 6), p, perturb=0.1)
    parts = partition.rcb_partition(whole.elem_verts, 2)
    part = partition.PartitionedMesh(whole.elem_nodes, whole.elem_verts, None, parts, 1, 2, p)
    assert part.n_ghost_nodes > 0 and 0 < part.n_interior_elems < part.n_elems
    mask = whole.dirichlet_mask(U).reshape(-1, U)[part.node_grid_id].reshape(-1)
    mesh = system.DeviceMesh(ctx, part, U, mask)
    mf = system.MatrixFreeSystem(mesh, D2)
    rng = np.random.default_rng(5)
    no, ng = part.n_owned_nodes * U, part.n_ghost_nodes * U
    X, XG = dev(rng.uniform(-1, 1, (1, no))), dev(rng.uniform(-1, 1, (1, ng)))
    y0, yg0 = rng.uniform(-1, 1, (1, no)), rng.uniform(-1, 1, (1, ng))
    out = []
    for sequence in ([2], [0, 1], [3, 4, 1]):
        Y, YG = dev(y0), dev(yg0)
        mf.scale(Y, 0.5)
        YG.mul_(0.5)
        for which in sequence:
            mf.apply_elems(which, X, XG, Y, YG, 1.25, 0.5)
        torch.cuda.synchronize()
        out.append((Y.cpu().numpy(), YG.cpu().numpy()))
    for y, yg in out[1:]:
        assert rel_err(y, out[0][0]) < 1e-13 and rel_err(yg, out[0][1]) < 1e-13


def run_ranks(world, body):
    errors = []

    def guarded(rank):
        try:
            torch.cuda.set_device(0)
            with torch.cuda.stream(torch.cuda.Stream()):
                body(rank)
                torch.cuda.synchronize()
        except BaseException as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=guarded, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    if errors:
        raise errors[0]


def test_four_ranks_apply_dist_vs_oracle():
    """Four thread-ranks of an rcb partition of a quad mesh through l3k_mf_apply_dist with the in-process transport, against the
    oracle on the whole mesh."""
    from l3ster_amd.distributed import InprocGroup, NativeDistributedOperator, NativeHalo
    p, world = 3, 4
    whole = system.SquarePartition((9, 7), p, perturb=0.1)
    parts = partition.rcb_partition(whole.elem_verts, world)
    mask_w = whole.dirichlet_mask(U)
    group = InprocGroup(world)
    out = {}

    def xvec(ids, seed):  # a function of the partition-independent node id
        g = np.asarray(ids, np.float64)
        return np.stack([np.sin(0.37 * g + u + seed) for u in range(U)], axis=1).reshape(1, -1)

    def body(rank):
        mesh_h = partition.PartitionedMesh(whole.elem_nodes, whole.elem_verts, None, parts, rank, world, p)
        ids = mesh_h.node_grid_id[:mesh_h.n_local_nodes]
        mask = mask_w.reshape(-1, U)[ids].reshape(-1)
        c = system.Context(0, torch.cuda.current_stream().cuda_stream)
        mesh = system.DeviceMesh(c, mesh_h, U, mask)
        mf = system.MatrixFreeSystem(mesh, D2)
        n_owned = mesh_h.n_owned_nodes * U
        X, Y = dev(xvec(ids, 0)[:, :n_owned]), dev(xvec(ids, 5)[:, :n_owned])
        op = NativeDistributedOperator(mf, NativeHalo(c, mesh_h, U, rank, world, transport=group))
        op.apply(X, Y, 0.5, 2.0)
        torch.cuda.current_stream().synchronize()
        out[rank] = (Y.cpu().numpy(), ids[:mesh_h.n_owned_nodes].copy())

    run_ranks(world, body)
    ids_w = np.arange(whole.n_local_nodes)
    om = oracle_mesh2(whole, p + 1, U, np.arange(U), mask_w)
    y_ref = O.mf_apply(om, D2, xvec(ids_w, 0).T, np.asfortranarray(xvec(ids_w, 5).T.copy()), alpha=0.5, beta=2.0)
    y_ref = y_ref.reshape(-1, U)
    got = np.zeros_like(y_ref)
    seen = np.zeros(whole.n_local_nodes, bool)
    for r in range(world):
        y, ids = out[r]
        got[ids] = y.reshape(-1, U)
        seen[ids] = True
    assert seen.all()
    assert rel_err(got, y_ref) < 1e-11


# ----------------------------------------------------------------------------------------------- 5. deterministic mode
def test_deterministic_mode():
    torch.cuda.set_device(0)
    c = system.Context(0, torch.cuda.current_stream().cuda_stream)
    c.set_deterministic(True)
    p = 4
    part = system.SquarePartition((7, 6), p, perturb=0.1)
    mask = part.dirichlet_mask(U)
    mf = system.MatrixFreeSystem(system.DeviceMesh(c, part, U, mask), D2, n_rhs=2)
    assert "deterministic" in mf.route(), mf.route()
    x = part.synthetic_vector(U, ncols=2)
    outs = []
    for _ in range(2):
        Y = torch.zeros((2, x.shape[1]), dtype=torch.float64, device="cuda")
        mf.apply(dev(x), Y, 1.0, 0.0)
        diag, rhs = mf.diag_rhs(dev(x))
        torch.cuda.synchronize()
        outs.append((Y.cpu().numpy(), diag.cpu().numpy(), rhs.cpu().numpy()))
    for a, b in zip(*outs):
        np.testing.assert_array_equal(a, b)
    om = oracle_mesh2(part, p + 1, U, np.arange(U), mask)
    assert rel_err(outs[0][0].T, O.mf_apply(om, D2, x.T)) < 1e-11
    d_ref, r_ref = O.mf_diag_rhs(om, D2, R=2, dirichlet_vals=x.T)
    assert rel_err(outs[0][1], d_ref) < 1e-11 and rel_err(outs[0][2].T, r_ref) < 1e-11


# ---------------------------------------------------------------------------------------------------------- 6. routes
def test_routes(ctx):
    part = system.SquarePartition(4, 6)
    mf = system.MatrixFreeSystem(system.DeviceMesh(ctx, part, U), D2, n_rhs=2)
    r1, r2 = mf.route(2, 1), mf.route(2, 2)
    assert "quadApplyKernel<p=6,nq=7,U=3,F=0,R=1>" in r1 and "quadApplyKernel<p=6,nq=7,U=3,F=0,R=2>" in r2, (r1, r2)
    assert "not fused" in mf.route(2, 1, with_energy=True) and "not fused" not in r1
    # one quad route: the small-launch threshold of the hex kernels does not apply
    with ctx.tuning(generic_below=1 << 40):
        assert mf.route(2, 1) == r1


# ------------------------------------------------------------------------------------------------------ 7. end to end
@pytest.mark.parametrize("ne,p,perturb", [(16, 4, 0.1), (32, 2, 0.0)])
def test_end_to_end_pcg(ctx, ne, p, perturb):
    """Diffusion2D with T = x on all four sides: device diag / rhs -> Jacobi -> l3k_pcg_solve reproduces T = x, q = (1, 0)."""
    part = system.SquarePartition(ne, p, perturb=perturb)
    mask = part.dirichlet_mask(U)
    xy = part.node_coords()
    g = np.zeros((part.n_local_nodes, U))
    g[:, 0] = xy[:, 0]
    g = g.reshape(1, -1) * mask
    mf = system.MatrixFreeSystem(system.DeviceMesh(ctx, part, U, mask), D2)
    diag, rhs = mf.diag_rhs(dev(g))
    minv = solve.jacobi_inverse_native(ctx, diag)
    sol = torch.zeros_like(rhs[0])
    res = solve.pcg(mf, rhs[0].contiguous(), sol, minv, tol=1e-12, residual_scaling="rhs", max_iters=20000)
    assert res.converged
    s = sol.cpu().numpy().reshape(-1, U)
    assert np.abs(s[:, 0] - xy[:, 0]).max() < 1e-7
    assert np.abs(s[:, 1] - 1.0).max() < 1e-7
    assert np.abs(s[:, 2]).max() < 1e-7


# ---------------------------------------------------------------------------------------------------------- 8. plugin
PLUGIN_SRC = """
struct QuadDiffusionPlugin {
    static constexpr l3k::KernelParams params{.dimension = 2, .n_equations = 4, .n_unknowns = 3};
    template <typename In, typename Out> L3K_HD void operator()(const In&, Out& out) const {
        auto& [operators, rhs] = out;
        auto& [A0, Ax, Ay] = operators;
        Ax(0, 1) = -1.; Ay(0, 2) = -1.;
        A0(1, 1) = -1.; Ax(1, 0) = 1.;
        A0(2, 2) = -1.; Ay(2, 0) = 1.;
        Ax(3, 2) = 1.;  Ay(3, 1) = -1.;
    }
};"""


def test_plugin_2d_kernel(ctx):
    from l3ster_amd import plugin
    kid = plugin.compile_kernel("QuadDiffusionPlugin", PLUGIN_SRC, kernel_id=1201, shapes=[(3, 4, 1)])
    assert system.kernel_info(kid)["dimension"] == 2
    part = system.SquarePartition((6, 5), 3, perturb=0.1)
    mask = part.dirichlet_mask(U)
    mesh = system.DeviceMesh(ctx, part, U, mask)
    mf_p, mf_b = system.MatrixFreeSystem(mesh, kid), system.MatrixFreeSystem(mesh, D2)
    assert "quadApplyKernel<p=3,nq=4" in mf_p.route(), mf_p.route()
    x = dev(part.synthetic_vector(U))
    Yp, Yb = torch.zeros_like(x), torch.zeros_like(x)
    mf_p.apply(x, Yp)
    mf_b.apply(x, Yb)
    torch.cuda.synchronize()
    assert rel_err(Yp.cpu().numpy(), Yb.cpu().numpy()) < 1e-14


# -------------------------------------------------------------------------------------------------------- 9. refusals
def test_refusals_on_quads(ctx):
    part = system.SquarePartition(3, 2)
    mesh = system.DeviceMesh(ctx, part, U, part.dirichlet_mask(U))
    mf = system.MatrixFreeSystem(mesh, D2)
    with pytest.raises(system.L3KError, match="quads"):
        mf.local_assemble(0, 1)
    with pytest.raises(system.L3KError, match="quads"):
        system.BoundaryTerm(mesh, system.KERNEL_ADIABATIC3D, *part.boundary_sides([0]))
    with pytest.raises(system.L3KError, match="quads"):
        system.integrate(mesh, system.RESIDUAL_UNIT3D)
    with pytest.raises(system.L3KError, match="quads"):
        system.values_at_nodes(mesh, system.RESIDUAL_COORDX3D, [0], torch.zeros(part.n_local_nodes * U, dtype=torch.float64, device="cuda"))
    lib = system.capi.load()
    import ctypes as C
    buf = torch.zeros(1 << 16, dtype=torch.float64, device="cuda")
    rc = lib.l3k_local_assemble_tiled(mf._h, 0, 1, C.c_void_p(buf.data_ptr()))
    assert rc < 0 and "quads" in lib.l3k_last_error().decode()
    idx32 = torch.zeros(16, dtype=torch.int32, device="cuda")
    idx64 = torch.zeros(16, dtype=torch.int64, device="cuda")
    rc = lib.l3k_assemble_global(mf._h, 0, 1, C.c_void_p(idx64.data_ptr()), C.c_void_p(idx32.data_ptr()), C.c_void_p(buf.data_ptr()),
                                 C.c_void_p(0), 0, 0, 0, None)
    assert rc < 0 and "quads" in lib.l3k_last_error().decode()


def test_dimension_mismatch(ctx):
    quad = system.DeviceMesh(ctx, system.SquarePartition(2, 2), U)
    hexm = system.DeviceMesh(ctx, system.CubePartition(2, 2), 4)
    with pytest.raises(system.L3KError, match="dimension"):
        system.MatrixFreeSystem(quad, system.KERNEL_DIFFUSION3D)
    with pytest.raises(system.L3KError, match="dimension"):
        system.MatrixFreeSystem(hexm, D2)
