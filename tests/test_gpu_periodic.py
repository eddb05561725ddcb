"""Periodic boundary conditions on the device: l3k_periodic_match against the all-pairs restatement of periodic_ref.py on
scrambled meshes (straight and curved periodic faces, the tolerance rules, the refusals), and ElevatedMesh.periodic end to end: the
operator identity A_m x = P^T A (P x) between the merged and the unmerged mesh and the oracle on the merged connectivity, several
periodic axes at once, deterministic mode, a mesh one element wide, a partitioned merged mesh, the gmsh square from the file and
the reference's AdvectionPeriodic2D regression test restated.  Boundary ids of the scrambled meshes are 10 + side."""
import ctypes as C
import os

import numpy as np
import pytest

import mesh_ref
import oracle_lib as O
import periodic_ref as R
from helpers import rel_err
from l3ster_amd import capi, gmsh, partition, solve, system

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SQUARE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gmsh_ascii4_square.msh")
D2, D3 = system.KERNEL_DIFFUSION2D, system.KERNEL_DIFFUSION3D
KPAR = {D2: None, D3: [0.7, 1.0]}
UNKNOWNS = {D2: 3, D3: 4}


@pytest.fixture(scope="module")
def ctx():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    torch.cuda.set_device(0)
    return system.Context(0, torch.cuda.current_stream().cuda_stream)


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")


def structured(ne):
    return system.SquarePartition(ne, 1) if len(ne) == 2 else system.CubePartition(ne, 1)


def scrambled(ctx, ne, order, seed=0, move=None):
    """The unit square / cube of ne elements as an unstructured mesh (nothing structured survives), boundary id 10 + side, elevated
    to `order`.  move(verts, bnd_conn, on_side): displaces the order-1 vertices in place before the elevation."""
    part = structured(ne)
    verts, conn, bnd, _, _, on_side = mesh_ref.scrambled_structured(part, np.random.default_rng(seed + 100 * part.n_elems))
    if move is not None:
        move(verts, bnd, on_side)
    return system.ElevatedMesh(ctx, verts, conn, order, bnd, 10 + on_side)


def low_side(dim, axis):
    return 2 * (dim - 1 - axis)


def periodic_definition(dim, axis):
    """(src_ids, dst_ids, translation): the high side of `axis` onto its low side"""
    t = np.zeros(3)
    t[axis] = -1.0
    return [10 + low_side(dim, axis) + 1], [10 + low_side(dim, axis)], t


def match_both(ctx, mesh, definition, tolerance=1e-12):
    """the device match, twice, and the restatement; returns the device result"""
    src_ids, dst_ids, t = definition
    src, dst = mesh.boundary_sides(src_ids), mesh.boundary_sides(dst_ids)
    got = system.periodic_match(ctx, mesh, src, dst, t, tolerance)
    want = R.brute_force_match(mesh, src, dst, t, tolerance)
    assert got[0].dtype == np.uint32 and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert got[2:] == want[2:], (got[2:], want[2:])
    assert np.all(np.diff(got[0].astype(np.int64)) > 0)  # ascending in the source node, one pair per node
    again = system.periodic_match(ctx, mesh, src, dst, t, tolerance)
    assert np.array_equal(again[0], got[0]) and np.array_equal(again[1], got[1]) and again[2:] == got[2:]
    return got


# ------------------------------------------------------------------------------------------------- 1. match against brute force
MATCH_CASES = [((5, 3), p, axis) for p in (1, 2, 4) for axis in (0, 1)] + [((3, 2, 2), p, axis) for p in (1, 3) for axis in (0, 1, 2)] + \
              [((12, 12, 2), 3, 2)]


@pytest.mark.parametrize("ne,p,axis", MATCH_CASES)
def test_match_against_brute_force(ctx, ne, p, axis):
    mesh = scrambled(ctx, ne, p, seed=axis)
    ps, pd, n_unmatched, n_ambiguous, first = match_both(ctx, mesh, periodic_definition(mesh.dim, axis))
    n_face = int(np.prod([n * p + 1 for a, n in enumerate(ne) if a != axis]))
    assert ps.size == n_face and (n_unmatched, n_ambiguous, first) == (0, 0, -1)
    if ne == (12, 12, 2):
        assert n_face == 1369 and mesh.boundary_sides([11])[0].size == 144  # more than one workgroup, nodes listed up to four times
    xyz = mesh.node_coords()
    assert np.abs(xyz[ps, axis] - 1.0).max() < 1e-14 and np.abs(xyz[pd, axis]).max() < 1e-14
    rest = [a for a in range(mesh.dim) if a != axis]
    assert np.abs(xyz[ps][:, rest] - xyz[pd][:, rest]).max() < 1e-14


# -------------------------------------------------------------------------------------------------------- 2. curved periodic faces
def smooth_periodic_displacement(dim, axis, amplitude=0.03):
    """A smooth field with period 1 along `axis` (so both periodic faces move alike and stay images of each other), with all
    components and a dependence on every coordinate: the periodic faces are no longer planes."""

    def move(verts, bnd, on_side):
        x = verts.copy()
        phase = 2.0 * np.pi * x[:, axis]
        others = [a for a in range(dim) if a != axis]
        bend = np.prod([np.cos(1.3 * x[:, a] + 0.2 * (a + 1)) for a in others], axis=0)
        for c in range(dim):
            verts[:, c] += amplitude * np.sin(phase + 0.7 * c + 1.0) * bend * (1.0 + 0.5 * x[:, others[0]])

    return move


def assert_positive_jacobians(mesh):
    corners = [np.array(c, dtype=np.float64) for c in np.ndindex(*(2,) * mesh.dim)]
    points = [2.0 * c - 1.0 for c in corners] + [np.zeros(mesh.dim)]
    for e in range(mesh.n_elems):
        for pt in points:
            assert np.linalg.det(O.jacobi_mat(mesh.dim, mesh.elem_verts[e], pt)) > 0.0, (e, pt)


@pytest.mark.parametrize("ne,p,axis", [((5, 3), 4, 0), ((5, 3), 2, 1), ((3, 2, 2), 3, 0), ((3, 2, 2), 3, 1), ((3, 2, 2), 1, 2),
                                       ((12, 12, 2), 3, 2)])
def test_match_on_curved_periodic_faces(ctx, ne, p, axis):
    mesh = scrambled(ctx, ne, p, seed=7 + axis, move=smooth_periodic_displacement(len(ne), axis))
    assert_positive_jacobians(mesh)
    fe, fs = mesh.boundary_sides([10 + low_side(mesh.dim, axis)])
    _, loc = R.side_node_locations(mesh, fe, fs)
    assert np.ptp(loc[:, axis]) > 1e-3  # the face is not a plane any more
    ps, pd, n_unmatched, n_ambiguous, first = match_both(ctx, mesh, periodic_definition(mesh.dim, axis))
    n_face = int(np.prod([n * p + 1 for a, n in enumerate(ne) if a != axis]))
    assert ps.size == n_face and (n_unmatched, n_ambiguous, first) == (0, 0, -1)


# ---------------------------------------------------------------------------------------------------------------- 3. tolerance rules
def move_one_destination_vertex(dim, axis, by):
    def move(verts, bnd, on_side):
        v = int(bnd[on_side == low_side(dim, axis)][0, 0])
        verts[v, (axis + 1) % dim] += by  # along the face
        verts[v, axis] -= by

    return move


@pytest.mark.parametrize("ne,p,axis", [((5, 3), 3, 0), ((3, 2, 2), 2, 1)])
def test_tolerance_rules(ctx, ne, p, axis):
    dim = len(ne)
    n_face = int(np.prod([n * p + 1 for a, n in enumerate(ne) if a != axis]))
    definition = periodic_definition(dim, axis)
    # moved by 2.3e-13 along two axes, 3.3e-13 in all: a factor 3 inside the tolerance for the vertex, more for every other node
    near = scrambled(ctx, ne, p, seed=3, move=move_one_destination_vertex(dim, axis, 2.3e-13))
    ps, pd, n_unmatched, n_ambiguous, first = match_both(ctx, near, definition)
    assert ps.size == n_face and (n_unmatched, n_ambiguous, first) == (0, 0, -1)
    # 1e-9: the vertex and the nodes of the destination sides around it (bilinear weights >= 0.03 at these orders) are more than a
    # factor 30 outside the tolerance; the restatement says which source nodes lose their partner
    far = scrambled(ctx, ne, p, seed=3, move=move_one_destination_vertex(dim, axis, 1e-9))
    ps, pd, n_unmatched, n_ambiguous, first = match_both(ctx, far, definition)
    assert n_unmatched > 0 and ps.size == n_face - n_unmatched and first >= 0 and n_ambiguous == 0
    # the nodes of the sides around the vertex but those on their far edges: the vertex inside the face, on its rim, at a corner
    assert n_unmatched in ((2 * p - 1, p) if dim == 2 else ((2 * p - 1) ** 2, (2 * p - 1) * p, p * p))
    with pytest.raises(capi.L3KError, match=f"node {first}"):
        far.periodic([definition])
    # a tolerance of 0.6 element edges at order >= 2: the neighbours along the face qualify as well, the nearest wins
    straight = scrambled(ctx, ne, p, seed=3)
    edge = min(1.0 / n for a, n in enumerate(ne) if a != axis)
    ps, pd, n_unmatched, n_ambiguous, first = match_both(ctx, straight, definition, tolerance=0.6 * edge)
    exact = match_both(ctx, straight, definition)
    assert n_ambiguous > 0 and n_unmatched == 0 and np.array_equal(ps, exact[0]) and np.array_equal(pd, exact[1])
    # a tolerance above every distance in the face: every source node sees every destination node (legal, merely slow)
    ps, pd, n_unmatched, n_ambiguous, first = match_both(ctx, straight, definition, tolerance=3.0)
    assert n_ambiguous == n_face and np.array_equal(pd, exact[1])
    # no destination side at all; no source side at all
    src, dst = straight.boundary_sides(definition[0]), straight.boundary_sides(definition[1])
    none = (np.zeros(0, np.int64), np.zeros(0, np.uint8))
    got = system.periodic_match(ctx, straight, src, none, definition[2])
    assert got[0].size == 0 and got[2:] == (n_face, 0, int(exact[0].min()))
    got = system.periodic_match(ctx, straight, none, dst, definition[2])
    assert got[0].size == 0 and got[2:] == (0, 0, -1)
    # a side onto itself with no translation: every node is its own partner, and such pairs are dropped
    got = system.periodic_match(ctx, straight, src, src, np.zeros(3))
    assert got[0].size == 0 and got[2:] == (0, 0, -1)


# --------------------------------------------------------------------------------------------------------------------- 4. refusals
def test_match_refusals(ctx):
    lib = capi.load()
    en = np.arange(8, dtype=np.uint32).reshape(1, 8)
    ev = np.array([[(i, j, k) for k in (0, 1) for j in (0, 1) for i in (0, 1)]], dtype=np.float64)
    se, ss = np.array([0], np.int64), np.array([5], np.uint8)
    de, ds = np.array([0], np.int64), np.array([4], np.uint8)
    t = np.array([-1.0, 0.0, 0.0])
    ps, pd = np.full(4, 99, np.uint32), np.full(4, 99, np.uint32)
    counts = [C.c_int64(-7) for _ in range(4)]
    p32, p64, p8, pdbl = capi.c_uint32_p, capi.c_int64_p, capi.c_uint8_p, capi.c_double_p
    good = [ctx._h, 3, 1, 1, en.ctypes.data_as(p32), ev.ctypes.data_as(pdbl), 1, se.ctypes.data_as(p64), ss.ctypes.data_as(p8),
            1, de.ctypes.data_as(p64), ds.ctypes.data_as(p8), t.ctypes.data_as(pdbl), 1e-12, ps.ctypes.data_as(p32),
            pd.ctypes.data_as(p32)] + [C.byref(c) for c in counts]
    assert lib.l3k_periodic_match(*good) == 0
    assert ps.tolist() == [1, 3, 5, 7] and pd.tolist() == [0, 2, 4, 6] and [c.value for c in counts] == [4, 0, 0, -1]

    def refused(wording="l3k_periodic_match", **change):
        args = list(good)
        for k, v in change.items():
            args[int(k[1:])] = v
        assert lib.l3k_periodic_match(*args) == -1
        message = lib.l3k_last_error().decode()
        assert "l3k_periodic_match" in message and wording in message, message

    refused(a1=1), refused(a1=4)  # dim
    refused(a2=0), refused(a2=9)  # order
    refused(a3=-1), refused(a6=-1), refused(a9=-1)  # negative counts
    refused(a0=None), refused(a4=None), refused(a5=None), refused(a7=None), refused(a8=None), refused(a10=None), refused(a11=None)
    refused(a12=None), refused(a14=None), refused(a15=None), refused(a16=None), refused(a17=None), refused(a18=None), refused(a19=None)
    bad_elem, neg_elem, bad_side = np.array([1], np.int64), np.array([-1], np.int64), np.array([6], np.uint8)
    refused("outside the mesh", a7=bad_elem.ctypes.data_as(p64)), refused("outside the mesh", a10=bad_elem.ctypes.data_as(p64))
    refused("outside the mesh", a7=neg_elem.ctypes.data_as(p64)), refused("outside the mesh", a8=bad_side.ctypes.data_as(p8))
    refused("outside the mesh", a11=bad_side.ctypes.data_as(p8))
    quad_side = np.array([4], np.uint8)  # a hex side that a quad does not have
    refused("outside the mesh", a1=2, a8=quad_side.ctypes.data_as(p8))
    for bad in (np.nan, np.inf, -np.inf):
        tb = np.array([-1.0, bad, 0.0])
        refused(a12=tb.ctypes.data_as(pdbl))
        refused(a13=bad)
    refused(a13=0.0), refused(a13=-1e-12)
    evb = ev.copy()
    evb[0, 3, 1] = np.nan
    refused(a5=evb.ctypes.data_as(pdbl))
    # with dim = 2 the third entries are ignored: the same arrays read as one quad (4 nodes, 4 vertices), z translation not finite
    tz = np.array([-1.0, 0.0, np.nan])
    args = list(good)
    args[1], args[8], args[11], args[12] = 2, np.array([3], np.uint8).ctypes.data_as(p8), np.array([2], np.uint8).ctypes.data_as(p8), \
        tz.ctypes.data_as(pdbl)
    assert lib.l3k_periodic_match(*args) == 0
    assert ps[:2].tolist() == [1, 3] and pd[:2].tolist() == [0, 2] and [c.value for c in counts] == [2, 0, 0, -1]
    with pytest.raises(capi.L3KError, match="l3k_periodic_match"):
        system.periodic_match(ctx, scrambled(ctx, (3, 2), 1), (se, ss), (de, ds), t)  # side 5 on quads


def test_cpp_mirror_matches_and_merges(tmp_path):
    """l3k::periodicMatch and l3k::periodicMerge of include/l3k/operator.hpp on two quads (tests/cpp/periodic_shim.cpp)"""
    import subprocess

    from test_periodic_cpu import build_cpp_shim
    exe = build_cpp_shim(str(tmp_path / "periodic_shim"))
    r = subprocess.run([exe, "match"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr


# ---------------------------------------------------------------------------------------------------------- 5. operator identity
def check_operator_identity(ctx, mesh, pm, kid, dir_ids, seed=0):
    """A_m x = P^T A (P x) on the rows that are not Dirichlet rows, the same for diag and rhs of diag_rhs, and the merged apply,
    diag and rhs against the oracle on the merged connectivity.  The bound is the one the existing apply tests use against the
    oracle for these kernels (tests/test_gpu_quad.py, tests/test_gpu_apply.py): relative l2 error below 1e-11."""
    U, kpar, p = UNKNOWNS[kid], KPAR[kid], mesh.order
    n_m, n_u = pm.n_owned_nodes, mesh.n_owned_nodes
    mask_m = pm.dirichlet_mask(U, ids=dir_ids) if dir_ids else None
    mask_u = mesh.dirichlet_mask(U, ids=dir_ids) if dir_ids else None
    if dir_ids:
        assert mask_m.any() and np.array_equal(mask_u, R.prolong(pm.node_map, mask_m, U))
    free = np.ones(n_m * U, bool) if mask_m is None else mask_m == 0
    mf_u = system.MatrixFreeSystem(system.DeviceMesh(ctx, mesh, U, mask_u), kid, kpar)
    mf_m = system.MatrixFreeSystem(system.DeviceMesh(ctx, pm, U, mask_m), kid, kpar)
    rng = np.random.default_rng(seed)
    x_m = rng.uniform(-1, 1, (1, n_m * U))
    Y_m, Y_u = dev(np.zeros((1, n_m * U))), dev(np.zeros((1, n_u * U)))
    mf_m.apply(dev(x_m), Y_m)
    mf_u.apply(dev(R.prolong(pm.node_map, x_m, U)), Y_u)
    torch.cuda.synchronize()
    y_m = Y_m.cpu().numpy()
    via_p = R.restrict(pm.node_map, Y_u.cpu().numpy(), U, n_m)
    errs = {"identity": rel_err(y_m[:, free], via_p[:, free])}
    om = O.MeshView(mesh.dim, p, system.n_qps1d(p, 1), pm.elem_nodes, pm.elem_verts, n_m, U, np.arange(U), mask_m)
    errs["oracle"] = rel_err(y_m.T, O.mf_apply(om, kid, x_m.T, kparams=kpar))
    g_m = rng.uniform(-1, 1, (1, n_m * U)) * (0 if mask_m is None else mask_m[None, :])
    diag_m, rhs_m = mf_m.diag_rhs(dev(g_m))
    diag_u, rhs_u = mf_u.diag_rhs(dev(R.prolong(pm.node_map, g_m, U)))
    torch.cuda.synchronize()
    diag_m, rhs_m = diag_m.cpu().numpy(), rhs_m.cpu().numpy()
    errs["diag identity"] = rel_err(diag_m[free], R.restrict(pm.node_map, diag_u.cpu().numpy(), U, n_m)[free])
    d_ref, r_ref = O.mf_diag_rhs(om, kid, 1, np.asfortranarray(g_m.T), kparams=kpar)
    errs["diag oracle"] = rel_err(diag_m, d_ref)
    rhs_u = rhs_u.cpu().numpy()
    via_p = R.restrict(pm.node_map, rhs_u, U, n_m)
    if np.linalg.norm(r_ref) > 1e-3 * np.linalg.norm(rhs_u):
        errs["rhs identity"] = rel_err(rhs_m[:, free], via_p[:, free])
        errs["rhs oracle"] = rel_err(rhs_m.T, r_ref)
    elif rhs_u.any():
        # periodic along every axis: the right-hand side of a constant source is the integral of a derivative over a domain without
        # boundary, and the rows of the images cancel to rounding.  The error is then measured against the terms that cancel.
        assert dir_ids is None
        errs["rhs identity (cancelling)"] = np.linalg.norm(rhs_m - via_p) / np.linalg.norm(rhs_u)
        errs["rhs oracle (cancelling)"] = np.linalg.norm(rhs_m.T - r_ref) / np.linalg.norm(rhs_u)
    else:  # (Diffusion2D without Dirichlet values has no right-hand side)
        assert not rhs_m.any() and not r_ref.any()
    print(f"periodic {mesh.dim}-D order {p}, {n_u} -> {n_m} nodes:", {k: f"{v:.1e}" for k, v in errs.items()})
    assert all(v < 1e-11 for v in errs.values()), errs
    assert np.linalg.norm(y_m) > 0 and np.linalg.norm(diag_m[free]) > 0
    return mf_m


def merged(mesh, axes):
    pm = mesh.periodic([periodic_definition(mesh.dim, a) for a in axes])
    pairs = [R.brute_force_match(mesh, mesh.boundary_sides(s), mesh.boundary_sides(d), t)[:2]
             for s, d, t in (periodic_definition(mesh.dim, a) for a in axes)]
    want = R.merge(mesh.elem_nodes, mesh.n_owned_nodes, mesh.n_noninternal, np.concatenate([a for a, _ in pairs]),
                   np.concatenate([b for _, b in pairs]))
    assert np.array_equal(pm.elem_nodes, want[0]) and np.array_equal(pm.node_map, want[1])
    assert (pm.n_owned_nodes, pm.n_noninternal, pm.n_components) == want[2:] and pm.n_global_nodes == pm.n_owned_nodes
    assert pm.n_pairs == sum(a.size for a, _ in pairs) and pm.n_ambiguous == 0
    R.check_numbering(pm.elem_nodes, pm.n_owned_nodes, pm.n_noninternal, mesh.dim, mesh.order, mesh.elem_nodes)
    for name in ("elem_verts", "face_elem", "face_side", "bnd_id", "boundary_ids", "elem_domain"):
        assert getattr(pm, name) is getattr(mesh, name)
    assert pm is not mesh and pm.elem_nodes is not mesh.elem_nodes and mesh.n_owned_nodes > pm.n_owned_nodes
    return pm


@pytest.mark.parametrize("ne,p,kid,route", [((4, 3), 4, D2, "quadApplyKernel<p=4"), ((3, 2, 2), 2, D3, None),
                                            ((2, 2, 2), 6, D3, "sumfactFastKernel<p=6")])
def test_operator_identity(ctx, ne, p, kid, route):
    mesh = scrambled(ctx, ne, p, seed=5, move=smooth_periodic_displacement(len(ne), 0, amplitude=0.02))
    pm = merged(mesh, [0])
    rest = int(np.prod([n * p + 1 for n in ne[1:]]))
    assert pm.n_owned_nodes == ne[0] * p * rest and mesh.n_owned_nodes == (ne[0] * p + 1) * rest
    with ctx.tuning(generic_below=0):  # (eight elements would take the small-launch kernel: run the single-wave one)
        mf = check_operator_identity(ctx, mesh, pm, kid, dir_ids=[10 + low_side(mesh.dim, 1)])
        assert route is None or route in mf.route(), mf.route()


# ------------------------------------------------------------------------------------------- 6. several periodic axes at once
@pytest.mark.parametrize("ne,p,kid", [((4, 3), 3, D2), ((3, 2, 2), 2, D3)])
def test_periodic_along_every_axis(ctx, ne, p, kid):
    mesh = scrambled(ctx, ne, p, seed=11)
    pm = merged(mesh, list(range(mesh.dim)))
    assert pm.n_owned_nodes == int(np.prod([n * p for n in ne]))  # (nx p)(ny p) / (nx p)(ny p)(nz p)
    xyz = mesh.node_coords()
    corners = np.nonzero(((xyz[:, :mesh.dim] < 1e-12) | (xyz[:, :mesh.dim] > 1 - 1e-12)).all(axis=1))[0]
    assert corners.size == 2 ** mesh.dim and np.unique(pm.node_map[corners]).size == 1  # one component of 4 / 8
    assert np.count_nonzero(pm.node_map == pm.node_map[corners[0]]) == 2 ** mesh.dim
    check_operator_identity(ctx, mesh, pm, kid, dir_ids=None)


# ------------------------------------------------------------------------------------------------------- 7. deterministic mode
def test_deterministic_mode_on_a_merged_mesh():
    torch.cuda.set_device(0)
    c = system.Context(0, torch.cuda.current_stream().cuda_stream)
    c.set_deterministic(True)
    mesh = scrambled(c, (3, 2, 2), 2, seed=13)
    pm = merged(mesh, [0])
    U = 4
    mask = pm.dirichlet_mask(U, ids=[12])
    mf = system.MatrixFreeSystem(system.DeviceMesh(c, pm, U, mask), D3, KPAR[D3])
    assert "deterministic" in mf.route(), mf.route()
    x = np.random.default_rng(1).uniform(-1, 1, (1, pm.n_owned_nodes * U))
    outs = []
    for _ in range(2):
        Y = torch.zeros((1, x.shape[1]), dtype=torch.float64, device="cuda")
        mf.apply(dev(x), Y)
        diag, rhs = mf.diag_rhs(dev(x * mask[None, :]))
        torch.cuda.synchronize()
        outs.append((Y.cpu().numpy(), diag.cpu().numpy(), rhs.cpu().numpy()))
    for a, b in zip(*outs):
        np.testing.assert_array_equal(a, b)
    om = O.MeshView(3, 2, 3, pm.elem_nodes, pm.elem_verts, pm.n_owned_nodes, U, np.arange(U), mask)
    assert rel_err(outs[0][0].T, O.mf_apply(om, D3, x.T, kparams=KPAR[D3])) < 1e-11


# ---------------------------------------------------------------------------------------------------------- 8. one element wide
def test_one_element_wide_along_the_periodic_axis(ctx):
    """An element then names a node twice.  Default mode; bitwise reproducibility is not claimed for this shape (include/l3k.h)."""
    mesh = scrambled(ctx, (1, 2, 2), 2, seed=17)
    pm = merged(mesh, [0])
    assert pm.n_owned_nodes == 2 * 5 * 5
    assert all(np.unique(row).size == 27 - 9 for row in pm.elem_nodes)
    check_operator_identity(ctx, mesh, pm, D3, dir_ids=[12])


# -------------------------------------------------------------------------------------------------------------- 9. partitioned
def test_partitioned_merged_mesh(ctx):
    """rcb_partition of the merged mesh in two, cut across the periodic axis.  The lowest part that touches a node owns it, so part 0
    of a two-part mesh has no ghosts at all: the identification shows in the ghosts of part 1 (the nodes of the identified plane
    beside those of the cut) and in what part 0 sends."""
    ne, p, U = (4, 2, 2), 2, 4
    mesh = scrambled(ctx, ne, p, seed=19)
    pm = merged(mesh, [0])
    mf = system.MatrixFreeSystem(system.DeviceMesh(ctx, pm, U), D3, KPAR[D3])
    x = np.random.default_rng(2).uniform(-1, 1, (pm.n_owned_nodes, U))
    Y = dev(np.zeros((1, x.size)))
    mf.apply(dev(x.reshape(1, -1)), Y)
    y_ref = Y.cpu().numpy().reshape(-1, U)
    elem_part = partition.rcb_partition(pm.elem_verts, 2)
    centroid_x = pm.elem_verts[:, :, 0].mean(axis=1)
    assert centroid_x[elem_part == 0].max() < 0.5 < centroid_x[elem_part == 1].min()  # the cut is across x
    n_plane = (ne[1] * p + 1) * (ne[2] * p + 1)
    y_sum = np.zeros_like(y_ref)
    for rank in range(2):
        part = partition.PartitionedMesh(pm.elem_nodes, pm.elem_verts, pm.n_noninternal, elem_part, rank, 2, p)
        plain = partition.PartitionedMesh(mesh.elem_nodes, mesh.elem_verts, mesh.n_noninternal, elem_part, rank, 2, p)
        assert part.n_ghost_nodes == (0, 2 * n_plane)[rank] and plain.n_ghost_nodes == (0, n_plane)[rank]
        assert sum(s.size for s in part.send_nodes) == (2 * n_plane, 0)[rank]
        if rank == 1:  # the ghosts that come from the identification only: images of the plane x = 1, which part 0 never touches
            at_x1 = np.unique(pm.node_map[np.abs(mesh.node_coords()[:, 0] - 1.0) < 1e-12])
            ghosts = part.node_grid_id[part.n_owned_nodes:]
            assert at_x1.size == n_plane and np.all(np.isin(at_x1, ghosts))
        dm = system.DeviceMesh(ctx, part, U)
        op = system.MatrixFreeSystem(dm, D3, KPAR[D3])
        xl = x[part.node_grid_id].reshape(1, -1)
        n_owned = part.n_owned_nodes * U
        X, XG = dev(xl[:, :n_owned]), (dev(xl[:, n_owned:]) if part.n_ghost_nodes else None)
        Yo, YG = dev(np.zeros((1, n_owned))), (dev(np.zeros((1, part.n_ghost_nodes * U))) if part.n_ghost_nodes else None)
        op.scale(Yo, 0.0)
        op.apply_elems(2, X, XG, Yo, YG, 1.0, 0.0)
        torch.cuda.synchronize()
        yl = np.concatenate([Yo.cpu().numpy(), YG.cpu().numpy()], axis=1) if YG is not None else Yo.cpu().numpy()
        np.add.at(y_sum, part.node_grid_id, yl.reshape(-1, U))  # node_grid_id: the node's id in the whole mesh, [owned | ghosts]
    assert np.linalg.norm(y_sum - y_ref) < 1e-12 * np.linalg.norm(y_ref)


# --------------------------------------------------------------------------------------------- 10. the gmsh square from the file
def test_the_gmsh_square_periodic_in_y(ctx):
    m = gmsh.read_mesh(SQUARE)
    mesh = system.ElevatedMesh(ctx, m.verts, m.conn, 2, m.bnd_conn, m.bnd_id, m.elem_domain)
    xyz = mesh.node_coords()
    at_y = {}
    for bid in mesh.boundary_ids:  # the boundaries of constant y, from the coordinates
        on = mesh.dirichlet_mask(1, ids=[bid]) != 0
        if np.ptp(xyz[on, 1]) < 1e-9:
            at_y[float(xyz[on, 1].mean())] = int(bid)
    assert len(at_y) == 2
    (y_lo, bottom), (y_hi, top) = sorted(at_y.items())
    sides = [int(b) for b in mesh.boundary_ids if b not in (bottom, top)]
    definition = ([top], [bottom], [0.0, y_lo - y_hi, 0.0])
    # gmsh wrote the points of opposite edges with different rounding (-0.4000000000002774 ...): the x of partners differ by up to
    # 2.8e-12, so at the reference's default tolerance most top nodes have no partner.  1e-9 is a factor 300 above what the file
    # is off by and seven orders below its node spacing of 0.05.
    assert match_both(ctx, mesh, definition)[2] > 0
    with pytest.raises(capi.L3KError, match="no node at X"):
        mesh.periodic([definition])
    assert match_both(ctx, mesh, definition, tolerance=1e-9)[2:] == (0, 0, -1)
    pm = mesh.periodic([definition], tolerance=1e-9)
    assert mesh.n_owned_nodes == 21 * 21 and pm.n_owned_nodes == 20 * 21 and pm.n_pairs == 21 and pm.n_components == 21
    assert np.array_equal(pm.boundary_sides([top])[0], mesh.boundary_sides([top])[0])
    check_operator_identity(ctx, mesh, pm, D2, dir_ids=sides)


# -------------------------------------------------------------------- 11. the reference's AdvectionPeriodic2D regression test
ADVECTION_SRC = """
struct AdvectionPeriodic2D {
    static constexpr l3k::KernelParams params{.dimension = 2, .n_equations = 1, .n_unknowns = 1, .n_fields = 3};
    static constexpr bool field_derivatives = false;
    template <typename In, typename Out> L3K_HD void operator()(const In& in, Out& out) const {
        constexpr double u = 1., v = 0., dt = .05, bdf_leading = 11. / 6.;
        auto& [operators, rhs] = out;
        auto& [A0, A1, A2] = operators;
        A0(0, 0) = bdf_leading;
        A1(0, 0) = u * dt;
        A2(0, 0) = v * dt;
        rhs[0] = in.field_vals[0] * 3. + in.field_vals[1] * -1.5 + in.field_vals[2] * (1. / 3.);
    }
};"""
ADVECTION_ERROR_SRC = """
struct AdvectionPeriodic2DError {
    static constexpr l3k::KernelParams params{.dimension = 2, .n_equations = 1, .n_fields = 1};
    template <typename In, typename Out> L3K_HD void operator()(const In& in, Out& out) const {
        const double t = in.point.time, x = in.point.space.x();
        double x_dv = x - t * 1.;
        while (x_dv < -.5)
            x_dv += 1.;
        out[0] = in.field_vals[0] - exp(-10. * x_dv * x_dv);
    }
};"""


def analytic(x, t):
    x_dv = x - t * 1.0
    while np.any(x_dv < -0.5):
        x_dv = np.where(x_dv < -0.5, x_dv + 1.0, x_dv)
    return np.exp(-10.0 * x_dv * x_dv)


def test_advection_periodic_2d_restated(ctx):
    """tests/AdvectionPeriodic2D.hpp of the reference (:15-18 the mesh, :30 the periodic definition, :51 dt, :97 the number of steps,
    :124-135 the error and its bar): 4 x 3 elements of [-.5, .5] x [0, .5] at order 4, periodic left -> right with translation
    (1, 0, 0), Dirichlet on top and bottom with the analytic values, BDF3 advection with u = 1, v = 0, dt = .05, history from the
    analytic Gaussian exp(-10 x_dv^2) with the wrap, 20 steps of diag_rhs -> Jacobi-PCG -> update_solution.  After one period the
    pulse has left through the right side and come back; norm_l2(computed - analytic) / (W H) * 100 must be below 5."""
    from l3ster_amd import plugin
    p, dt, W, H = 4, 0.05, 1.0, 0.5
    kid = plugin.compile_kernel("AdvectionPeriodic2D", ADVECTION_SRC, kernel_id=1321, shapes=[(p, system.n_qps1d(p, 1), 1)])
    rid = plugin.compile_kernel("AdvectionPeriodic2DError", ADVECTION_ERROR_SRC, kernel_id=1322,
                                shapes=[(p, system.n_qps1d(p, 2, 0))], kind="residual")
    part = system.SquarePartition((4, 3), 1)
    verts, conn, bnd, _, _, on_side = mesh_ref.scrambled_structured(part, np.random.default_rng(23))
    verts[:, 0] = verts[:, 0] * W - 0.5
    verts[:, 1] = verts[:, 1] * H
    mesh = system.ElevatedMesh(ctx, verts, conn, p, bnd, 10 + on_side)
    bottom, top, left, right = 10, 11, 12, 13
    pm = mesh.periodic([([left], [right], [W, 0.0, 0.0])])
    assert pm.n_owned_nodes == 16 * 13 and pm.n_pairs == 13
    mask = pm.dirichlet_mask(1, ids=[top, bottom])
    on_wall = torch.as_tensor(mask.astype(bool), device="cuda")
    dm = system.DeviceMesh(ctx, pm, 1, mask)
    mf = system.MatrixFreeSystem(dm, kid)
    x = pm.node_coords()[:, 0]  # (an identified node reports one of its images: the analytic solution is the same at both)
    assert np.abs(analytic(np.array([-0.5]), 0.3) - analytic(np.array([0.5]), 0.3)).max() < 1e-15
    fields = dev(np.stack([analytic(x, -i * dt) for i in range(3)]))  # history: u^n, u^{n-1}, u^{n-2}
    mf.set_fields(fields)
    n_steps = round(W / dt)
    assert n_steps == 20
    for step in range(1, n_steps + 1):
        t = step * dt
        g = dev((analytic(x, t) * mask)[None, :])
        mf.set_time(t)
        diag, rhs = mf.diag_rhs(g)
        minv = solve.jacobi_inverse_native(ctx, diag)
        sol = fields[0].clone()
        sol[on_wall] = g[0][on_wall]
        res = solve.pcg(mf, rhs[0].contiguous(), sol, minv, tol=1e-11, residual_scaling="rhs")
        assert res.converged, step
        fields[2].copy_(fields[1])
        fields[1].copy_(fields[0])
        system.update_solution(dm, sol[None, :], [0], fields, [0])
    computed = fields[:1].contiguous()
    error = system.norm_l2(dm, rid, computed, time=n_steps * dt)[0] / (W * H) * 100.0
    pulse = system.norm_l2(dm, rid, torch.zeros_like(computed), time=n_steps * dt)[0] / (W * H) * 100.0
    print(f"AdvectionPeriodic2D restated: normalised L2 error {error:.3f} % (bar 5), the pulse's own norm {pulse:.1f}")
    assert error < 5.0
