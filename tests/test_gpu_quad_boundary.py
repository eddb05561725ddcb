"""Boundary terms, integrals and values at nodes on quadrilateral (2-D) meshes: known answers on the distorted quad of
tests/MappingTests.cpp, Adiabatic2D against the oracle (orc_bnd_apply / orc_bnd_diag_rhs with dim = 2) standalone and attached,
a 2-D boundary plugin against the numpy restatement of quad_side_ref.py, Linear2DError / CoordX2D against orc_mf_integrate /
orc_values_at_nodes, the reference's 2-D diffusion problem K6 end to end, deterministic mode, four thread-ranks and the
refusals."""
import numpy as np
import pytest

import oracle_lib as O
import quad_side_ref as Q
from helpers import rel_err
from l3ster_amd import partition, solve, system
from test_gpu_quad import SingleQuad, make_mask, oracle_mesh2, run_ranks
from test_oracle_boundary import QUAD

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

U = 3
D2, ADI = system.KERNEL_DIFFUSION2D, system.KERNEL_ADIABATIC2D


@pytest.fixture(scope="module")
def ctx():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    torch.cuda.set_device(0)
    return system.Context(0, torch.cuda.current_stream().cuda_stream)


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")


def zeros(n):
    return torch.zeros(n, dtype=torch.float64, device="cuda")


# A residual plugin with derivatives and the normal: out = (dT/dx, grad T . n, n_x, n_y) on sides, (dT/dx, 0, 0, 0) on elements
FLUX_SRC = """
struct QuadFluxResidual {
    static constexpr l3k::KernelParams params{.dimension = 2, .n_equations = 4, .n_fields = 1};
    template <typename In, typename Out> L3K_HD void operator()(const In& in, Out& out) const {
        out[0] = in.field_ders[0][0];
        if constexpr (requires(const In& i) { i.normal; }) {
            out[1] = in.field_ders[0][0] * in.normal[0] + in.field_ders[1][0] * in.normal[1];
            out[2] = in.normal[0];
            out[3] = in.normal[1];
        }
    }
};"""


@pytest.fixture(scope="module")
def flux_id():
    from l3ster_amd import plugin
    return plugin.compile_kernel("QuadFluxResidual", FLUX_SRC, kernel_id=1311, shapes=[(1, 6), (2, 3)], kind="residual")


@pytest.fixture(scope="module")
def wall_id():
    from l3ster_amd import plugin
    return plugin.compile_kernel("QuadWallPlugin", Q.PLUGIN_SRC, kernel_id=1312, shapes=[(2, 3, 2)], kind="boundary")


# ---------------------------------------------------------------------------------------------------- 1. known answers
def test_quad_lengths_area_normals(ctx, flux_id):
    part = SingleQuad(1, QUAD)
    mesh = system.DeviceMesh(ctx, part, 4)
    opts = (5, 0, 0)  # nq = 6
    for side, length in enumerate([1.0, np.sqrt(5.0), 1.0, np.sqrt(5.0)]):
        got = system.integrate(mesh, system.RESIDUAL_UNIT2D, asm_opts=opts, face_elem=[0], face_side=[side])
        assert got[0] == pytest.approx(length, abs=1e-13)
    assert system.integrate(mesh, system.RESIDUAL_UNIT2D, asm_opts=opts)[0] == pytest.approx(2.0, abs=1e-13)
    zero = torch.zeros((1, part.n_local_nodes), dtype=torch.float64, device="cuda")
    total = np.zeros(2)
    for side, want in enumerate([(0, -1), (-1, 2), (-1, 0), (2, -1)]):
        got = system.integrate(mesh, flux_id, zero, asm_opts=opts, face_elem=[0], face_side=[side])
        np.testing.assert_allclose(got[2:], want, atol=1e-13)
        total += got[2:]
    np.testing.assert_allclose(total, 0.0, atol=1e-13)


@pytest.mark.parametrize("perturb", [0.0, 0.15])
def test_field_derivatives_on_both_forms(ctx, flux_id, perturb):
    """T = x^2 + 3xy is biquadratic under the bilinear map, so exact at p = 2: int dT/dx = 2.5, int_boundary grad T . n = 2;
    at the nodes dT/dx = 2x + 3y.  (The perturbation keeps the boundary of the unit square.)"""
    part = system.SquarePartition((5, 4), 2, perturb=perturb)
    mesh = system.DeviceMesh(ctx, part, 4)
    xy = part.node_coords()
    T = dev((xy[:, 0] ** 2 + 3 * xy[:, 0] * xy[:, 1])[None, :])
    assert system.integrate(mesh, flux_id, T)[0] == pytest.approx(2.5, abs=1e-12)
    fe, fs = part.boundary_sides()
    assert system.integrate(mesh, flux_id, T, face_elem=fe, face_side=fs)[1] == pytest.approx(2.0, abs=1e-12)
    vals = system.values_at_nodes(mesh, flux_id, [0, 1, 2, 3], zeros(part.n_local_nodes * 4), T)
    got = vals.cpu().numpy().reshape(-1, 4)
    assert np.abs(got[:, 0] - (2 * xy[:, 0] + 3 * xy[:, 1])).max() < 1e-11
    assert np.all(got[:, 1:] == 0.0)  # the domain form has no normal


# --------------------------------------------------------------------------------------------------- 2. Adiabatic2D
@pytest.mark.parametrize("p", [1, 2, 4, 6])
@pytest.mark.parametrize("R", [1, 2])
@pytest.mark.parametrize("mask_kind", ["none", "boundary", "random"])
def test_adiabatic_vs_oracle(ctx, p, R, mask_kind):
    part = system.SquarePartition((5, 4), p, perturb=0.15)
    mask = make_mask(part, mask_kind, seed=p)
    mesh = system.DeviceMesh(ctx, part, U, mask)
    fe, fs = part.boundary_sides([0, 1, 3])
    term = system.BoundaryTerm(mesh, ADI, fe, fs, n_rhs=R)
    om = oracle_mesh2(part, p + 1, U, np.arange(U), mask)
    rng = np.random.default_rng(p + 10 * R)
    n = part.n_local_nodes * U
    x, y0 = rng.uniform(-1, 1, (R, n)), rng.uniform(-1, 1, (R, n))
    Y = dev(y0)
    term.apply(dev(x), Y, alpha=1.5)
    want = np.asfortranarray(y0.T.copy())
    O.bnd_apply(om, ADI, fe, fs, np.asfortranarray(x.T), want, alpha=1.5)
    assert rel_err(Y.cpu().numpy().T, want) < 1e-12
    mk = np.zeros(n, np.uint8) if mask is None else mask
    g = np.where(mk[None, :] != 0, rng.uniform(-1, 1, (R, n)), 0.0)
    diag = zeros(n)
    rhs = torch.zeros((R, n), dtype=torch.float64, device="cuda")
    term.diag_rhs(diag, rhs, dirichlet_vals=dev(g))
    wd, wr = np.zeros(n), np.zeros((n, R), order="F")
    O.bnd_diag_rhs(om, ADI, fe, fs, wd, wr, dirichlet_vals=np.asfortranarray(g.T))
    assert rel_err(diag.cpu().numpy(), wd) < 1e-12
    if mask_kind == "none":  # no Dirichlet values to lift and no boundary source
        assert np.all(rhs.cpu().numpy() == 0.0) and np.all(wr == 0.0)
    else:
        assert rel_err(rhs.cpu().numpy().T, wr) < 1e-11


@pytest.mark.parametrize("p,R", [(2, 1), (4, 2), (6, 1)])
def test_attached_adiabatic_in_apply(ctx, p, R):
    part = system.SquarePartition((6, 5), p, perturb=0.1)
    mask = part.dirichlet_mask(U, sides=(2, 3))
    mesh = system.DeviceMesh(ctx, part, U, mask)
    fe, fs = part.boundary_sides([0, 1])
    mf = system.MatrixFreeSystem(mesh, D2, n_rhs=R)
    mf.attach_boundary(system.BoundaryTerm(mesh, ADI, fe, fs, n_rhs=R))
    om = oracle_mesh2(part, p + 1, U, np.arange(U), mask)
    x = part.synthetic_vector(U, seed=3, ncols=R)
    y0 = part.synthetic_vector(U, seed=4, ncols=R)
    Y = dev(y0)
    mf.apply(dev(x), Y, 0.5, -2.0)
    want = O.mf_apply(om, D2, x.T, y=np.asfortranarray(y0.T.copy()), alpha=0.5, beta=-2.0)
    # the boundary rows are added before the Dirichlet rows in the device schedule; both commute
    O.bnd_apply(om, ADI, fe, fs, np.asfortranarray(x.T), want, alpha=0.5)
    assert rel_err(Y.cpu().numpy().T, want) < 1e-12
    g = np.where(mask[None, :] != 0, np.random.default_rng(p).uniform(-1, 1, x.shape), 0.0)
    diag, rhs = mf.diag_rhs(dev(g))
    wd, wr = O.mf_diag_rhs(om, D2, R=R, dirichlet_vals=np.asfortranarray(g.T), finalize=False)
    O.bnd_diag_rhs(om, ADI, fe, fs, wd, wr, dirichlet_vals=np.asfortranarray(g.T))
    wd[mask != 0] = 1.0
    wr[mask != 0] = g.T[mask != 0]
    assert rel_err(diag.cpu().numpy(), wd) < 1e-12
    assert rel_err(rhs.cpu().numpy().T, wr) < 1e-11


# ------------------------------------------------------------------------------------------------ 3. boundary plugin
def _wall_check(ctx, wall_id, part, fe, fs, dpn, fi, seed):
    mesh = system.DeviceMesh(ctx, part, dpn)
    term = system.BoundaryTerm(mesh, wall_id, fe, fs, field_inds=fi, n_rhs=2)
    rng = np.random.default_rng(seed)
    fields = rng.uniform(0.5, 1.5, (1, part.n_local_nodes))
    term.set_fields(dev(fields))
    term.set_time(0.4)
    K, F = Q.mesh_side_system(Q.wall_plugin, 2, 2, part, 3, fe, fs, dpn, fi, fields, time=0.4, R=2)
    assert np.abs(K).max() > 0 and np.abs(F).max() > 0
    n = part.n_local_nodes * dpn
    x, y0 = rng.uniform(-1, 1, (2, n)), rng.uniform(-1, 1, (2, n))
    Y = dev(y0)
    term.apply(dev(x), Y, alpha=-0.75)
    assert rel_err(Y.cpu().numpy(), y0 - 0.75 * (K @ x.T).T) < 1e-12
    diag = zeros(n)
    rhs = torch.zeros((2, n), dtype=torch.float64, device="cuda")
    term.diag_rhs(diag, rhs)
    assert rel_err(diag.cpu().numpy(), np.diag(K)) < 1e-12
    assert rel_err(rhs.cpu().numpy(), F.T) < 1e-11


@pytest.mark.parametrize("side", range(4))
def test_boundary_plugin_on_quad_sides(ctx, wall_id, side):
    _wall_check(ctx, wall_id, SingleQuad(2, QUAD), [0], [side], 4, [3, 1], side)


def test_boundary_plugin_on_mesh(ctx, wall_id):
    part = system.SquarePartition((3, 2), 2, perturb=0.1)
    fe, fs = part.boundary_sides()
    _wall_check(ctx, wall_id, part, fe, fs, 4, [2, 0], 7)


# ------------------------------------------------------------------------------------ 4. integrals, values at nodes
@pytest.mark.parametrize("p", [2, 4])
@pytest.mark.parametrize("square", [False, True])
def test_linear2d_error_integrals_vs_oracle(ctx, p, square):
    part = system.SquarePartition((4, 3), p, perturb=0.1)
    mesh = system.DeviceMesh(ctx, part, U)
    fields = np.random.default_rng(p).uniform(-1, 1, (3, part.n_local_nodes))
    nq = system.n_qps1d(p, 2, 0)
    om = O.MeshView(2, p, nq, part.elem_nodes, part.elem_verts, part.n_local_nodes, U, [0, 1, 2], fields=fields)
    rid = system.RESIDUAL_LINEAR2D_ERROR
    got = system.integrate(mesh, rid, dev(fields), asm_opts=(2, 0, 0), square=square)
    assert rel_err(got, O.mf_integrate(om, rid, nq, square=square)) < 1e-12
    fe, fs = part.boundary_sides([0, 2, 3])
    got = system.integrate(mesh, rid, dev(fields), asm_opts=(2, 0, 0), square=square, face_elem=fe, face_side=fs)
    assert rel_err(got, O.mf_integrate(om, rid, nq, square=square, face_elem=fe, face_side=fs)) < 1e-12
    # the same again: the fixed summation order makes it bitwise reproducible
    again = system.integrate(mesh, rid, dev(fields), asm_opts=(2, 0, 0), square=square, face_elem=fe, face_side=fs)
    np.testing.assert_array_equal(got, again)


@pytest.mark.parametrize("p", [2, 4, 6])
def test_values_at_nodes_vs_oracle(ctx, p):
    part = system.SquarePartition((4, 3), p, perturb=0.1)
    mesh = system.DeviceMesh(ctx, part, U)
    om = O.MeshView(2, p, p + 1, part.elem_nodes, part.elem_verts, part.n_local_nodes, U, [0, 1, 2])
    rid = system.RESIDUAL_COORDX2D
    n = part.n_local_nodes * U
    for fe, fs in [(None, None), part.boundary_sides([1, 2])]:
        init = np.random.default_rng(p).uniform(-1, 1, n)
        got = system.values_at_nodes(mesh, rid, [1], dev(init), face_elem=fe, face_side=fs).cpu().numpy()
        s, c = O.values_at_nodes(om, rid, [1], fe, fs)
        want = np.where(c > 0, s / np.maximum(c, 1), init)
        assert np.abs(got - want).max() < 1e-14
    # Linear2DError reads the fields
    rid = system.RESIDUAL_LINEAR2D_ERROR
    fields = np.random.default_rng(p + 1).uniform(-1, 1, (3, part.n_local_nodes))
    om_f = O.MeshView(2, p, p + 1, part.elem_nodes, part.elem_verts, part.n_local_nodes, U, [0, 1, 2], fields=fields)
    got = system.values_at_nodes(mesh, rid, [0, 1, 2], zeros(n), dev(fields)).cpu().numpy()
    s, c = O.values_at_nodes(om_f, rid, [0, 1, 2])
    assert np.abs(got - s / c).max() < 1e-13


# ------------------------------------------------------------------------------------------------------------ 5. K6
@pytest.mark.parametrize("ne", [4, 32])
@pytest.mark.parametrize("perturb", [0.0, 0.1])
def test_k6_diffusion2d_end_to_end(ctx, ne, perturb):
    """tests/Diffusion2D.hpp on the device: Dirichlet T = x on x = 0 and x = 1 (values_at_nodes of CoordX2D), Adiabatic2D on
    y = 0 and y = 1, diag / rhs, Jacobi-PCG; T = x, q = (1, 0) lies in the discrete space.  ne = 32: 12 675 dofs."""
    p = 2
    part = system.SquarePartition(ne, p, perturb=perturb)
    mask = part.dirichlet_mask(U, sides=(2, 3))
    mesh = system.DeviceMesh(ctx, part, U, mask)
    mf = system.MatrixFreeSystem(mesh, D2)
    mf.attach_boundary(system.BoundaryTerm(mesh, ADI, *part.boundary_sides([0, 1])))
    xy = part.node_coords()
    dfe, dfs = part.boundary_sides([2, 3])
    g = system.values_at_nodes(mesh, system.RESIDUAL_COORDX2D, [0], zeros(part.n_local_nodes * U), face_elem=dfe, face_side=dfs)
    want = np.where(mask.reshape(-1, U) != 0, np.stack([xy[:, 0], np.zeros(len(xy)), np.zeros(len(xy))], axis=1), 0.0)
    assert np.abs(g.cpu().numpy().reshape(-1, U) - want).max() < 1e-14
    diag, rhs = mf.diag_rhs(g[None, :])
    minv = solve.jacobi_inverse_native(ctx, diag)
    sol = torch.zeros_like(rhs[0])
    res = solve.pcg(mf, rhs[0].contiguous(), sol, minv, tol=1e-13, residual_scaling="rhs", max_iters=50000)
    assert res.converged
    s = sol.view(-1, U)
    assert (s[:, 0] - dev(xy[:, 0])).abs().max().item() < 1e-9
    fields = s.T.contiguous()  # SolutionManager layout: SoA [field][node]
    err = system.norm_l2(mesh, system.RESIDUAL_LINEAR2D_ERROR, fields)
    fe, fs = part.boundary_sides()
    berr = system.norm_l2(mesh, system.RESIDUAL_LINEAR2D_ERROR, fields, face_elem=fe, face_side=fs)
    assert np.linalg.norm(err) < 1e-8 and np.linalg.norm(berr) < 1e-8  # tests/Diffusion2D.hpp:117-119
    # oracle parity of the squared norms on the same solution (values are tiny: compare absolutely)
    nq2 = system.n_qps1d(p, 2, 0)
    om = O.MeshView(2, p, p + 1, part.elem_nodes, part.elem_verts, part.n_local_nodes, U, [0, 1, 2], fields=fields.cpu().numpy())
    assert np.allclose(err ** 2, O.mf_integrate(om, O.RESIDUAL_LINEAR2D_ERROR, nq2, square=True), atol=1e-18, rtol=1e-6)
    assert np.allclose(berr ** 2, O.mf_integrate(om, O.RESIDUAL_LINEAR2D_ERROR, nq2, square=True, face_elem=fe, face_side=fs),
                       atol=1e-18, rtol=1e-6)


# ----------------------------------------------------------------------------------------------- 6. deterministic mode
def test_deterministic_mode_with_boundary():
    torch.cuda.set_device(0)
    c = system.Context(0, torch.cuda.current_stream().cuda_stream)
    c.set_deterministic(True)
    p, R = 2, 2
    part = system.SquarePartition((7, 6), p, perturb=0.1)
    mask = part.dirichlet_mask(U, sides=(2, 3))
    mesh = system.DeviceMesh(c, part, U, mask)
    fe, fs = part.boundary_sides()
    mf = system.MatrixFreeSystem(mesh, D2, n_rhs=R)
    mf.attach_boundary(system.BoundaryTerm(mesh, ADI, fe, fs, n_rhs=R))
    x = part.synthetic_vector(U, ncols=R)
    g = np.where(mask[None, :] != 0, x, 0.0)
    outs = []
    for _ in range(2):
        Y = torch.zeros((R, x.shape[1]), dtype=torch.float64, device="cuda")
        mf.apply(dev(x), Y, 1.0, 0.0)
        diag, rhs = mf.diag_rhs(dev(g))
        torch.cuda.synchronize()
        outs.append((Y.cpu().numpy(), diag.cpu().numpy(), rhs.cpu().numpy()))
    for a, b in zip(*outs):
        np.testing.assert_array_equal(a, b)
    om = oracle_mesh2(part, p + 1, U, np.arange(U), mask)
    want = O.mf_apply(om, D2, x.T)
    O.bnd_apply(om, ADI, fe, fs, np.asfortranarray(x.T), want)
    assert rel_err(outs[0][0].T, want) < 1e-11
    wd, wr = O.mf_diag_rhs(om, D2, R=R, dirichlet_vals=np.asfortranarray(g.T), finalize=False)
    O.bnd_diag_rhs(om, ADI, fe, fs, wd, wr, dirichlet_vals=np.asfortranarray(g.T))
    wd[mask != 0] = 1.0
    wr[mask != 0] = g.T[mask != 0]
    assert rel_err(outs[0][1], wd) < 1e-11 and rel_err(outs[0][2].T, wr) < 1e-11


# ------------------------------------------------------------------------------------------------------ 7. four ranks
def test_four_ranks_with_boundary_vs_oracle():
    """Four thread-ranks of an rcb partition: each rank's sides are the whole mesh's sides of its elements (elem_global); the
    attached Adiabatic2D goes through the split-phase schedule of l3k_mf_apply_dist.  Per-rank integrals sum to the whole."""
    from l3ster_amd.distributed import InprocGroup, NativeDistributedOperator, NativeHalo
    p, world = 2, 4
    whole = system.SquarePartition((9, 7), p, perturb=0.1)
    parts = partition.rcb_partition(whole.elem_verts, world)
    mask_w = whole.dirichlet_mask(U, sides=(2, 3))
    fe_w, fs_w = whole.boundary_sides()
    group = InprocGroup(world)
    out = {}

    def xvec(ids, seed):  # a function of the partition-independent node id
        g = np.asarray(ids, np.float64)
        return np.stack([np.sin(0.37 * g + u + seed) for u in range(U)], axis=1).reshape(1, -1)

    def body(rank):
        mesh_h = partition.PartitionedMesh(whole.elem_nodes, whole.elem_verts, None, parts, rank, world, p)
        local = {int(g): i for i, g in enumerate(mesh_h.elem_global)}
        mine = [i for i, e in enumerate(fe_w) if int(e) in local]
        fe, fs = np.array([local[int(fe_w[i])] for i in mine], np.int64), fs_w[mine]
        ids = mesh_h.node_grid_id[:mesh_h.n_local_nodes]
        mask = mask_w.reshape(-1, U)[ids].reshape(-1)
        c = system.Context(0, torch.cuda.current_stream().cuda_stream)
        mesh = system.DeviceMesh(c, mesh_h, U, mask)
        mf = system.MatrixFreeSystem(mesh, D2)
        term = system.BoundaryTerm(mesh, ADI, fe, fs)
        mf.attach_boundary(term)
        n_owned = mesh_h.n_owned_nodes * U
        X, Y = dev(xvec(ids, 0)[:, :n_owned]), dev(xvec(ids, 5)[:, :n_owned])
        op = NativeDistributedOperator(mf, NativeHalo(c, mesh_h, U, rank, world, transport=group))
        op.apply(X, Y, 0.5, 2.0)
        torch.cuda.current_stream().synchronize()
        area = system.integrate(mesh, system.RESIDUAL_UNIT2D)[0]
        length = system.integrate(mesh, system.RESIDUAL_UNIT2D, face_elem=fe, face_side=fs)[0]
        out[rank] = (Y.cpu().numpy(), ids[:mesh_h.n_owned_nodes].copy(), area, length, len(fe))

    run_ranks(world, body)
    assert sum(o[4] for o in out.values()) == len(fe_w)
    ids_w = np.arange(whole.n_local_nodes)
    om = oracle_mesh2(whole, p + 1, U, np.arange(U), mask_w)
    y_ref = O.mf_apply(om, D2, xvec(ids_w, 0).T, np.asfortranarray(xvec(ids_w, 5).T.copy()), alpha=0.5, beta=2.0)
    O.bnd_apply(om, ADI, fe_w, fs_w, np.asfortranarray(xvec(ids_w, 0).T), y_ref, alpha=0.5)
    y_ref = y_ref.reshape(-1, U)
    got = np.zeros_like(y_ref)
    seen = np.zeros(whole.n_local_nodes, bool)
    for r in range(world):
        y, ids = out[r][:2]
        got[ids] = y.reshape(-1, U)
        seen[ids] = True
    assert seen.all()
    assert rel_err(got, y_ref) < 1e-11
    c = system.Context(0, torch.cuda.current_stream().cuda_stream)
    mesh_w = system.DeviceMesh(c, whole, U)
    area_w = system.integrate(mesh_w, system.RESIDUAL_UNIT2D)[0]
    length_w = system.integrate(mesh_w, system.RESIDUAL_UNIT2D, face_elem=fe_w, face_side=fs_w)[0]
    assert sum(o[2] for o in out.values()) == pytest.approx(area_w, rel=1e-13)
    assert sum(o[3] for o in out.values()) == pytest.approx(length_w, rel=1e-13)
    assert area_w == pytest.approx(1.0, rel=1e-13) and length_w == pytest.approx(4.0, rel=1e-13)


# ----------------------------------------------------------------------------------------------------------- 8. errors
def test_errors(ctx):
    quad, cube = system.SquarePartition(2, 2), system.CubePartition(2, 2)
    qmesh, hmesh = system.DeviceMesh(ctx, quad, U), system.DeviceMesh(ctx, cube, 4)
    with pytest.raises(system.L3KError, match="outside the mesh"):
        system.BoundaryTerm(qmesh, ADI, [0], [4])
    with pytest.raises(system.L3KError, match="outside the mesh"):
        system.integrate(qmesh, system.RESIDUAL_UNIT2D, face_elem=[0], face_side=[4])
    with pytest.raises(system.L3KError, match="outside the mesh"):
        system.values_at_nodes(qmesh, system.RESIDUAL_COORDX2D, [0], zeros(quad.n_local_nodes * U), face_elem=[0], face_side=[4])
    with pytest.raises(system.L3KError, match="dimension"):
        system.BoundaryTerm(hmesh, ADI, [0], [0])
    with pytest.raises(system.L3KError, match="dimension"):
        system.integrate(hmesh, system.RESIDUAL_UNIT2D)
    with pytest.raises(system.L3KError, match="dimension"):
        system.values_at_nodes(hmesh, system.RESIDUAL_COORDX2D, [0], zeros(cube.n_local_nodes * 4))
    with pytest.raises(system.L3KError, match="quads"):
        system.BoundaryTerm(qmesh, system.KERNEL_ADIABATIC3D, [0], [0])
    with pytest.raises(system.L3KError, match="quads"):
        system.integrate(qmesh, system.RESIDUAL_UNIT3D)
    with pytest.raises(system.L3KError, match="quads"):
        system.values_at_nodes(qmesh, system.RESIDUAL_COORDX3D, [0], zeros(quad.n_local_nodes * U))
