"""Unstructured meshes on the device: l3k_boundary_match (boundary elements -> (element, side)) against the truth of scrambled
structured meshes and the dictionary restatement of mesh_ref.py, its tie and failure rules, l3k_elevate_order_quads against
geometry, and system.ElevatedMesh end to end: the reference's 2-D diffusion problem (tests/Diffusion2D.hpp) on its own gmsh
square with every boundary condition stated by physical id, its 3-D twin on a scrambled cube, and boundary terms on the two
halves of a partitioned mesh."""
import os

import numpy as np
import pytest

import mesh_ref
from l3ster_amd import capi, gmsh, partition, solve, system

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SQUARE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gmsh_ascii4_square.msh")


@pytest.fixture(scope="module")
def ctx():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    torch.cuda.set_device(0)
    return system.Context(0, torch.cuda.current_stream().cuda_stream)


def zeros(*shape):
    return torch.zeros(shape, dtype=torch.float64, device="cuda")


# ----------------------------------------------------------------------------------------------------------- 1, 2. matching
@pytest.mark.parametrize("make", [lambda: system.CubePartition((3, 2, 2), 1), lambda: system.CubePartition(20, 1),
                                  lambda: system.SquarePartition((5, 3), 1)], ids=["hex3x2x2", "hex20", "quad5x3"])
def test_matching_finds_the_sides_of_a_scrambled_mesh(ctx, make):
    part = make()
    rng = np.random.default_rng(part.n_elems)
    verts, conn, bnd, true_elem, true_side, _ = mesh_ref.scrambled_structured(part, rng)
    n_bnd = {12: 32, 8000: 2400, 15: 16}[part.n_elems]
    assert bnd.shape == (n_bnd, 2 ** (part.dim - 1))
    fe, fs, n_unmatched, n_interior = system.boundary_match(ctx, conn, bnd)
    assert (n_unmatched, n_interior) == (0, 0)
    assert np.array_equal(fe, true_elem) and np.array_equal(fs, true_side)
    de, ds, du, di = mesh_ref.match_by_dictionary(conn, bnd)
    assert np.array_equal(fe, de) and np.array_equal(fs, ds) and (du, di) == (0, 0)
    again = system.boundary_match(ctx, conn, bnd)
    assert np.array_equal(again[0], fe) and np.array_equal(again[1], fs)


# ------------------------------------------------------------------------------------------------ 3. tie and failure rules
@pytest.mark.parametrize("dim", [2, 3])
def test_tie_and_failure_rules(ctx, dim):
    part = system.SquarePartition((3, 2), 1) if dim == 2 else system.CubePartition((3, 2, 2), 1)
    rng = np.random.default_rng(dim)
    verts, conn, bnd, true_elem, true_side, _ = mesh_ref.scrambled_structured(part, rng)
    c = conn.astype(np.int64)
    nsv = 2 ** (dim - 1)
    # an interface inside the mesh: a side two elements have
    sets = {}
    for e in range(c.shape[0]):
        for s, lv in enumerate(mesh_ref.SIDE_VERTS[dim]):
            sets.setdefault(frozenset(c[e, list(lv)].tolist()), []).append((e, s))
    shared = sorted(v for v in sets.values() if len(v) == 2)[-1]  # (the pair whose lower element index is the highest)
    (e_lo, s_lo), (e_hi, s_hi) = shared
    assert e_lo < e_hi
    interior = c[e_hi, list(mesh_ref.SIDE_VERTS[dim][s_hi])]  # written as the higher element has it
    fe, fs, nu, ni = system.boundary_match(ctx, conn, interior[None, :])
    assert (fe.tolist(), fs.tolist(), nu, ni) == ([e_lo], [s_lo], 0, 1)
    # vertices of one element that form no side (a diagonal / a quadruple across two sides)
    no_side = c[0, [0, 3]] if dim == 2 else c[0, [0, 1, 2, 7]]
    fe, fs, nu, ni = system.boundary_match(ctx, conn, no_side[None, :])
    assert (fe.tolist(), fs.tolist(), nu, ni) == ([-1], [255], 1, 0)
    # a repeated vertex, also between good ones: the rest is untouched
    rep = bnd[1].copy()
    rep[-1] = rep[0]
    mixed = np.stack([bnd[0], rep, interior.astype(np.uint32), bnd[2], no_side.astype(np.uint32)])
    fe, fs, nu, ni = system.boundary_match(ctx, conn, mixed)
    assert fe.tolist() == [true_elem[0], -1, e_lo, true_elem[2], -1] and fs.tolist() == [true_side[0], 255, s_lo, true_side[2], 255]
    assert (nu, ni) == (2, 1)
    de, ds, du, di = mesh_ref.match_by_dictionary(conn, mixed)
    assert np.array_equal(fe, de) and np.array_equal(fs, ds) and (du, di) == (2, 1)
    # nothing to match; no elements to match against
    fe, fs, nu, ni = system.boundary_match(ctx, conn, np.zeros((0, nsv), np.uint32))
    assert fe.shape == (0,) and fs.shape == (0,) and (nu, ni) == (0, 0)
    fe, fs, nu, ni = system.boundary_match(ctx, np.zeros((0, 2 ** dim), np.uint32), bnd[:3])
    assert fe.tolist() == [-1] * 3 and fs.tolist() == [255] * 3 and (nu, ni) == (3, 0)


def test_matching_refusals(ctx):
    import ctypes as C
    lib = capi.load()
    conn = np.arange(8, dtype=np.uint32).reshape(1, 8)
    bnd = np.arange(4, dtype=np.uint32).reshape(1, 4)
    fe, fs = np.zeros(1, np.int64), np.zeros(1, np.uint8)
    nu, ni = C.c_int64(), C.c_int64()
    p32, p64, p8 = capi.c_uint32_p, capi.c_int64_p, capi.c_uint8_p
    good = [ctx._h, 3, 1, conn.ctypes.data_as(p32), 1, bnd.ctypes.data_as(p32), fe.ctypes.data_as(p64), fs.ctypes.data_as(p8),
            C.byref(nu), C.byref(ni)]
    assert lib.l3k_boundary_match(*good) == 0 and fe[0] == 0 and fs[0] == 0

    def refused(**change):
        args = list(good)
        for k, v in change.items():
            args[int(k[1:])] = v
        assert lib.l3k_boundary_match(*args) == -1
        assert "l3k_boundary_match" in lib.l3k_last_error().decode()

    refused(a1=1), refused(a1=4)  # dim
    refused(a3=None), refused(a5=None), refused(a6=None), refused(a7=None)  # null arrays with non-zero counts
    refused(a8=None), refused(a9=None), refused(a0=None)
    refused(a2=-1), refused(a4=-1)
    refused(a2=(1 << 32) // 6 + 1)  # n_elems * 2 dim >= 2^32 (refused before anything is read)
    refused(a1=2, a2=1 << 30)
    with pytest.raises(capi.L3KError):
        system.boundary_match(ctx, np.zeros((2, 6), np.uint32), bnd)


# ------------------------------------------------------------------------------------------------------- 4. quad elevation
@pytest.fixture(scope="module")
def scrambled_square():
    part = system.SquarePartition((4, 3), 1, perturb=0.1)
    verts, conn, bnd, true_elem, true_side, on_side = mesh_ref.scrambled_structured(part, np.random.default_rng(43))
    return verts, conn


def sorted_rows(xy):
    return xy[np.lexsort((np.round(xy[:, 1], 9), np.round(xy[:, 0], 9)))]


@pytest.mark.parametrize("p", [1, 2, 4, 6])
def test_quad_elevation(ctx, scrambled_square, p):
    verts, conn = scrambled_square
    en, n_nodes, n_nonint = system.elevate_order_quads(ctx, conn, verts.shape[0], p)
    m, n1 = p - 1, p + 1
    assert en.shape == (12, n1 * n1) and en.dtype == np.uint32
    assert n_nodes == (4 * p + 1) * (3 * p + 1) and n_nonint == n_nodes - 12 * m * m
    ids = en.astype(np.int64)
    assert all(np.unique(row).size == n1 * n1 for row in ids)
    assert np.array_equal(np.unique(ids), np.arange(n_nodes))
    assert np.array_equal(ids[:, [0, p, p * n1, n1 * n1 - 1]], conn.astype(np.int64))  # the vertices keep their ids
    interior = [i + n1 * j for j in range(1, p) for i in range(1, p)]
    if interior:
        assert np.array_equal(ids[:, interior], n_nonint + np.arange(12)[:, None] * (m * m) + np.arange(m * m)[None, :])
    # geometry: the bilinear image of every (element, local node); all elements that hold a node id agree on its location.  Coordinates
    # are O(1), so rounding is a few 1e-16, while an edge walked from the wrong end moves a node by O(h / p)
    g = system.gll_nodes(n1)
    l = np.stack([(1 - g) / 2, (1 + g) / 2], axis=1)
    shape = np.einsum("xi,yj->yxji", l, l).reshape(n1 * n1, 4)
    loc = np.einsum("nv,evs->ens", shape, verts[conn.astype(np.int64)]).reshape(-1, 3)
    lo, hi = np.full((n_nodes, 3), np.inf), np.full((n_nodes, 3), -np.inf)
    np.minimum.at(lo, ids.reshape(-1), loc)
    np.maximum.at(hi, ids.reshape(-1), loc)
    assert np.max(hi - lo) < 1e-13
    want = system.SquarePartition((4, 3), p, perturb=0.1).node_coords()
    assert want.shape == (n_nodes, 3)
    assert np.abs(sorted_rows(0.5 * (lo + hi)) - sorted_rows(want)).max() < 1e-13
    en2, n2, nn2 = system.elevate_order_quads(ctx, conn, verts.shape[0], p)
    assert np.array_equal(en, en2) and (n2, nn2) == (n_nodes, n_nonint)


def test_quad_elevation_argument_checks(ctx, scrambled_square):
    verts, conn = scrambled_square
    en, n_nodes, n_nonint = system.elevate_order_quads(ctx, np.zeros((0, 4), np.uint32), 7, 3)
    assert en.shape == (0, 16) and n_nodes == 7 and n_nonint == 7
    for bad_order in (0, 9):
        with pytest.raises(capi.L3KError, match="l3k_elevate_order_quads"):
            system.elevate_order_quads(ctx, conn, verts.shape[0], bad_order)
    with pytest.raises(capi.L3KError, match="outside"):
        system.elevate_order_quads(ctx, conn, int(conn.max()), 2)  # a vertex id outside [0, n_vertices)


# ----------------------------------------------------------------------------------------------- 5. K6 on a file mesh (quads)
def constant_x_ids(mesh):
    """The boundary ids whose nodes all have one x (found from the node coordinates, not from the file's numbering)."""
    xyz = mesh.node_coords()
    found = []
    for bid in mesh.boundary_ids:
        on = mesh.dirichlet_mask(1, ids=[bid]) != 0
        if np.ptp(xyz[on, 0]) < 1e-9:
            found.append(int(bid))
    return found


def linear_system(ctx, mesh, U, kernel, kernel_params, adiabatic, coordx, dir_ids, wall_ids):
    """T = x on the boundaries dir_ids (values_at_nodes on their sides), the adiabatic boundary kernel on wall_ids, diag / rhs.
    Returns (mf, boundary term, Jacobi inverse, rhs)."""
    mask = mesh.dirichlet_mask(U, ids=dir_ids)
    dm = system.DeviceMesh(ctx, mesh, U, mask)
    mf = system.MatrixFreeSystem(dm, kernel, kernel_params)
    term = system.BoundaryTerm(dm, adiabatic, *mesh.boundary_sides(wall_ids))
    mf.attach_boundary(term)
    dfe, dfs = mesh.boundary_sides(dir_ids)
    g = system.values_at_nodes(dm, coordx, [0], zeros(mesh.n_local_nodes * U), face_elem=dfe, face_side=dfs)
    want = np.zeros((mesh.n_local_nodes, U))
    want[:, 0] = mesh.node_coords()[:, 0]
    want[mask.reshape(-1, U) == 0] = 0.0
    assert np.abs(g.cpu().numpy().reshape(-1, U) - want).max() < 1e-14
    diag, rhs = mf.diag_rhs(g[None, :])
    return mf, term, solve.jacobi_inverse_native(ctx, diag), rhs[0].contiguous()


def solve_linear_problem(ctx, *args):
    """Jacobi-PCG on linear_system(ctx, *args).  Returns the device mesh, the solution as SoA fields and the objects to keep."""
    mf, term, minv, rhs = linear_system(ctx, *args)
    sol = torch.zeros_like(rhs)
    res = solve.pcg(mf, rhs, sol, minv, tol=1e-13, residual_scaling="rhs", max_iters=50000)
    assert res.converged
    return mf.mesh, sol.view(-1, mf.mesh.dofs_per_node).T.contiguous(), (mf, term)


def test_k6_on_the_gmsh_square(ctx):
    m = gmsh.read_mesh(SQUARE)
    mesh = system.ElevatedMesh(ctx, m.verts, m.conn, 2, m.bnd_conn, m.bnd_id, m.elem_domain)
    assert mesh.dim == 2 and mesh.n_owned_nodes == 21 * 21 and mesh.elem_verts.shape == (100, 4, 3)
    assert mesh.boundary_ids.tolist() == [2, 3, 4, 5] and (mesh.n_unmatched, mesh.n_interior) == (0, 0)
    assert np.array_equal(mesh.elements_of([int(m.elem_domain[0])]), np.arange(100))
    fe, fs = mesh.boundary_sides([3])
    de, ds, _, _ = mesh_ref.match_by_dictionary(m.conn, m.bnd_conn[m.bnd_id == 3])
    assert np.array_equal(fe, de) and np.array_equal(fs, ds) and fe.size == 10  # in the order of the file
    with pytest.raises(capi.L3KError):
        mesh.boundary_sides([6])  # getBoundary throws (tests/MeshTests.cpp:40)
    with pytest.raises(capi.L3KError):
        mesh.elements_of([99])
    dir_ids = constant_x_ids(mesh)
    wall_ids = [int(b) for b in mesh.boundary_ids if b not in dir_ids]
    assert len(dir_ids) == 2 and len(wall_ids) == 2
    dm, fields, term = solve_linear_problem(ctx, mesh, 3, system.KERNEL_DIFFUSION2D, None, system.KERNEL_ADIABATIC2D,
                                            system.RESIDUAL_COORDX2D, dir_ids, wall_ids)
    err = system.norm_l2(dm, system.RESIDUAL_LINEAR2D_ERROR, fields)
    print("K6 on the gmsh square: L2 errors", err)
    assert err.shape == (3,) and np.all(err < 1e-8)  # tests/Diffusion2D.hpp:117-119
    for bid in mesh.boundary_ids:
        length = system.integrate(dm, system.RESIDUAL_UNIT2D, face_elem=mesh.boundary_sides([bid])[0],
                                  face_side=mesh.boundary_sides([bid])[1])
        assert abs(length[0] - 1.0) < 1e-12


def test_pmultigrid_takes_the_file_mesh_at_two_orders(ctx):
    """The same file at orders 2 and 1 (same element order: no element map) as the levels of solve.PMultigrid; the preconditioned
    solve reaches the reference's bar for this problem too."""
    m = gmsh.read_mesh(SQUARE)
    levels, keep = [], []
    for p, degree, cond_est in ((2, 3, 20.0), (1, 8, 400.0)):
        mesh = system.ElevatedMesh(ctx, m.verts, m.conn, p, m.bnd_conn, m.bnd_id)
        dir_ids = constant_x_ids(mesh)
        wall_ids = [int(b) for b in mesh.boundary_ids if b not in dir_ids]
        mf, term, minv, rhs = linear_system(ctx, mesh, 3, system.KERNEL_DIFFUSION2D, None, system.KERNEL_ADIABATIC2D,
                                            system.RESIDUAL_COORDX2D, dir_ids, wall_ids)
        levels.append((mf, solve.ChebyshevPreconditioner(mf, minv, degree=degree, cond_est=cond_est)))
        keep.append((term, minv, rhs))
    pm = solve.PMultigrid(levels)
    assert pm.info().order == [2, 1]
    mf, (_, minv, rhs) = levels[0][0], keep[0]
    xj, xm = torch.zeros_like(rhs), torch.zeros_like(rhs)
    rj = solve.pcg(mf, rhs, xj, minv, tol=1e-13, residual_scaling="rhs", max_iters=50000)
    rm = solve.pcg(mf, rhs, xm, precond=pm, tol=1e-13, residual_scaling="rhs", max_iters=50000)
    print(f"gmsh square order 2: iterations Jacobi {rj.num_iters}, p-multigrid {rm.num_iters}")
    assert rj.converged and rm.converged
    err = system.norm_l2(mf.mesh, system.RESIDUAL_LINEAR2D_ERROR, xm.view(-1, 3).T.contiguous())
    assert np.all(err < 1e-8)  # tests/Diffusion2D.hpp:117-119


def test_a_listed_boundary_element_without_a_side_is_an_error(ctx):
    m = gmsh.read_mesh(SQUARE)
    bnd = m.bnd_conn.copy()
    bnd[3] = [int(m.conn[0, 0]), int(m.conn[0, 3])]  # a diagonal of the first quad
    mesh = system.ElevatedMesh(ctx, m.verts, m.conn, 1, bnd, m.bnd_id)
    assert mesh.n_unmatched == 1
    lost_id = int(m.bnd_id[3])
    with pytest.raises(capi.L3KError, match="side of no element"):
        mesh.boundary_sides([lost_id])
    with pytest.raises(capi.L3KError, match="side of no element"):
        mesh.dirichlet_mask(3)
    others = [int(b) for b in mesh.boundary_ids if b != lost_id]
    assert mesh.boundary_sides(others)[0].size == 30  # the other ids are not touched by it
    bare = system.ElevatedMesh(ctx, m.verts, m.conn, 1)  # no boundary elements given
    assert bare.boundary_ids.size == 0 and bare.boundary_sides()[0].size == 0 and not bare.dirichlet_mask(2).any()


# ------------------------------------------------------------------------------------------------ 6, 7. the same for hexes
@pytest.fixture(scope="module")
def scrambled_cube(ctx):
    """CubePartition(3, 1, perturb = 0.1) scrambled, boundary id 10 + s on cube side s, elevated to order 2."""
    part = system.CubePartition(3, 1, perturb=0.1)
    verts, conn, bnd, true_elem, true_side, on_side = mesh_ref.scrambled_structured(part, np.random.default_rng(6))
    mesh = system.ElevatedMesh(ctx, verts, conn, 2, bnd, 10 + on_side)
    assert mesh.dim == 3 and mesh.n_owned_nodes == 7 ** 3 and mesh.boundary_ids.tolist() == [10, 11, 12, 13, 14, 15]
    assert np.array_equal(mesh.face_elem, true_elem) and np.array_equal(mesh.face_side, true_side)
    return mesh


def test_k6_twin_on_a_scrambled_cube(ctx, scrambled_cube):
    mesh = scrambled_cube
    assert constant_x_ids(mesh) == [14, 15]
    dm, fields, term = solve_linear_problem(ctx, mesh, 4, system.KERNEL_DIFFUSION3D, [1.0, 0.0], system.KERNEL_ADIABATIC3D,
                                            system.RESIDUAL_COORDX3D, [14, 15], [10, 11, 12, 13])
    err = system.norm_l2(dm, system.RESIDUAL_LINEAR3D_ERROR, fields)
    print("K6 twin on the scrambled cube: L2 errors", err)
    assert err.shape == (4,) and np.all(err < 1e-8)
    whole = system.CubePartition(3, 2, perturb=0.1)
    wm = system.DeviceMesh(ctx, whole, 4)
    for s in range(6):
        got = system.integrate(dm, system.RESIDUAL_UNIT3D, face_elem=mesh.boundary_sides([10 + s])[0],
                               face_side=mesh.boundary_sides([10 + s])[1])
        want = system.integrate(wm, system.RESIDUAL_UNIT3D, face_elem=whole.boundary_sides([s])[0], face_side=whole.boundary_sides([s])[1])
        assert abs(got[0] - want[0]) < 1e-12 * abs(want[0])


def test_boundary_terms_on_a_partitioned_mesh(ctx, scrambled_cube):
    mesh = scrambled_cube
    U, kp, ids = 4, [2.0, 0.7], [10, 11, 12, 13]
    fe, fs = mesh.boundary_sides(ids)

    def contribution(part, le, ls):
        dm = system.DeviceMesh(ctx, part, U)
        term = system.BoundaryTerm(dm, system.KERNEL_ROBIN3D, le, ls, kernel_params=kp)
        diag, rhs = zeros(part.n_owned_nodes * U), zeros(1, part.n_owned_nodes * U)
        dg, rg = zeros(part.n_ghost_nodes * U), zeros(1, part.n_ghost_nodes * U)
        term.diag_rhs(diag, rhs, diag_ghost=dg if part.n_ghost_nodes else None, rhs_ghost=rg if part.n_ghost_nodes else None)
        torch.cuda.synchronize()
        return (torch.cat([diag, dg]).cpu().numpy().reshape(-1, U), torch.cat([rhs[0], rg[0]]).cpu().numpy().reshape(-1, U))

    d_ref, r_ref = contribution(mesh, fe, fs)
    assert np.linalg.norm(d_ref) > 0 and np.linalg.norm(r_ref) > 0
    elem_part = partition.rcb_partition(mesh.elem_verts, 2)
    d_sum, r_sum = np.zeros_like(d_ref), np.zeros_like(r_ref)
    seen = []
    for rank in range(2):
        part = partition.PartitionedMesh(mesh.elem_nodes, mesh.elem_verts, mesh.n_noninternal, elem_part, rank, 2, 2)
        le, ls = partition.local_sides(part, fe, fs)
        assert 0 < le.size < fe.size
        seen += list(zip(part.elem_global[le].tolist(), ls.tolist()))
        d, r = contribution(part, le, ls)
        np.add.at(d_sum, part.node_grid_id, d)  # node_grid_id: the node's id in the whole mesh, [owned | ghosts]
        np.add.at(r_sum, part.node_grid_id, r)
    assert sorted(seen) == sorted(zip(fe.tolist(), fs.tolist()))
    assert np.linalg.norm(d_sum - d_ref) < 1e-12 * np.linalg.norm(d_ref)
    assert np.linalg.norm(r_sum - r_ref) < 1e-12 * np.linalg.norm(r_ref)
