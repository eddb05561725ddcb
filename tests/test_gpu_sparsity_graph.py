"""The CSR sparsity graph built on the device (l3k_graph_*, system.SparsityGraph) against the host builders: helpers.csr_graph for
the full graph, system.condensed_graph for the condensed one.  Everything compared is an integer array: every comparison is
exact."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from helpers import PeriodicXPartition, csr_graph
from l3ster_amd import capi, solve, system

pytestmark = pytest.mark.gpu

LAYOUTS = {"4-all": (4, None), "5-13": (5, [1, 3]), "1-0": (1, [0])}
MESHES = {
    "cube-p1": lambda: system.CubePartition((3, 2, 2), 1),
    "cube-p2": lambda: system.CubePartition((3, 2, 2), 2),
    "cube-p4": lambda: system.CubePartition((3, 2, 2), 4),
    "cube-p6": lambda: system.CubePartition((3, 2, 2), 6),
    "ghosts": lambda: system.CubePartition(4, 2, parts=(2, 1, 1), rank=0),
    "quads": lambda: system.SquarePartition((3, 2), 4),
}
_CACHE = {}


def context():
    if "ctx" not in _CACHE:
        torch.cuda.set_device(0)
        _CACHE["ctx"] = system.Context(0, torch.cuda.current_stream().cuda_stream)  # (not in deterministic mode)
    return _CACHE["ctx"]


def part_of(name):
    if ("part", name) not in _CACHE:
        _CACHE["part", name] = MESHES[name]()
    return _CACHE["part", name]


def fields(dpn, fi):
    return np.arange(dpn) if fi is None else np.asarray(fi)


def host_full(name, part, dpn, fi):
    """helpers.csr_graph once per (mesh, layout), never modified"""
    key = ("full", name, dpn, tuple(fields(dpn, fi)))
    if key not in _CACHE:
        _CACHE[key] = csr_graph(part, dpn, fields(dpn, fi))
    return _CACHE[key]


def check_arrays(g, row_ptr, col_ind, n):
    assert g.n == g.info.n == n
    assert g.row_ptr.dtype == torch.int64 and g.col_ind.dtype == torch.int32 and g.row_ptr.is_cuda and g.col_ind.is_cuda
    assert np.array_equal(g.row_ptr.cpu().numpy(), row_ptr)
    assert np.array_equal(g.col_ind.cpu().numpy(), col_ind)
    lens = np.diff(row_ptr)
    assert g.info.nnz == row_ptr[-1] == len(col_ind)
    assert g.info.n_empty_rows == int((lens == 0).sum())
    assert g.info.max_row_len == (int(lens.max()) if len(lens) else 0)


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("mesh", list(MESHES))
def test_full_graph_equals_the_host_graph(mesh, layout):
    dpn, fi = LAYOUTS[layout]
    part = part_of(mesh)
    g = system.SparsityGraph(system.DeviceMesh(context(), part, dpn), fi)
    row_ptr, col_ind, n = host_full(mesh, part, dpn, fi)
    check_arrays(g, row_ptr, col_ind, n)
    assert g.info.max_elems_per_node == int(np.bincount(part.elem_nodes.ravel()).max())
    if mesh.startswith("cube"):
        assert g.info.max_elems_per_node == 8
    assert g.info.n_rows_scratch == 0 and 0 < g.info.lds_key_capacity <= 16384


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("p", [1, 2, 4, 6])
def test_condensed_graph_equals_the_host_graph(p, layout):
    dpn, fi = LAYOUTS[layout]
    name = f"cube-p{p}"
    part = part_of(name)
    U = len(fields(dpn, fi))
    g = system.SparsityGraph(system.DeviceMesh(context(), part, dpn), fi, kind="condensed")
    row_ptr, col_ind = system.condensed_graph(part.elem_nodes, p, dpn, fields(dpn, fi))
    check_arrays(g, row_ptr, col_ind, part.n_local_nodes * dpn)
    n_internal = part.n_elems * (p - 1) ** 3
    assert g.info.n_empty_rows == (n_internal + 0) * U + part.n_local_nodes * (dpn - U)
    if p == 1:  # no internal nodes: the full graph
        full = host_full(name, part, dpn, fi)
        assert np.array_equal(row_ptr, full[0]) and np.array_equal(col_ind, full[1])


def test_identified_nodes_collapse():
    """The connectivity of a mesh periodic in x and one element wide there, with the identification carried out: every element
    lists the nodes of its face x = 0 twice.  (The identified nodes keep their numbers; their rows are empty.)"""
    per = PeriodicXPartition(system.CubePartition((1, 2, 2), 2))
    n_nodes = per.n_local_nodes
    part = types.SimpleNamespace(dim=3, order=2, n_elems=per.n_elems, n_interior_elems=per.n_elems, elem_nodes=per.merged,
                                 elem_verts=per.elem_verts, n_owned_nodes=n_nodes, n_ghost_nodes=0, n_local_nodes=n_nodes)
    assert all(len(np.unique(row)) < len(row) for row in part.elem_nodes)
    for dpn, fi in LAYOUTS.values():
        g = system.SparsityGraph(system.DeviceMesh(context(), part, dpn), fi)
        check_arrays(g, *csr_graph(part, dpn, fields(dpn, fi)))
        assert g.info.n_empty_rows >= per.n_ghost_nodes * dpn


def test_several_rows_per_workgroup():
    """One wave per CU in the tuning: the row launches have CUs / 4 workgroups, which walk the 1053 row nodes of the mesh."""
    ctx, part = context(), part_of("cube-p4")
    assert part.n_local_nodes == 13 * 9 * 9
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert cus // 4 < part.n_local_nodes
    for kind in ("full", "condensed"):
        with ctx.tuning(waves_per_cu=1):
            g = system.SparsityGraph(system.DeviceMesh(ctx, part, 5), [1, 3], kind=kind)
        if kind == "full":
            check_arrays(g, *host_full("cube-p4", part, 5, [1, 3]))
        else:
            check_arrays(g, *system.condensed_graph(part.elem_nodes, 4, 5, [1, 3]), part.n_local_nodes * 5)


def fan(ctx, K, order=4):
    """K hexes around one axis, two layers of vertices: per layer a centre vertex, K spoke vertices and K outer ones; element i
    has the centre, spoke i, outer i and spoke i + 1 (local vertex i + 2j + 4k)."""
    th = 2 * np.pi * np.arange(K) / K
    layer = np.concatenate([[[0.0, 0.0]], np.stack([np.cos(th), np.sin(th)], 1),
                            2 * np.stack([np.cos(th + np.pi / K), np.sin(th + np.pi / K)], 1)])
    nv = 2 * K + 1
    verts = np.concatenate([np.concatenate([layer, np.full((nv, 1), z)], 1) for z in (0.0, 1.0)])
    i = np.arange(K)
    quad = np.stack([np.zeros(K, np.int64), 1 + i, 1 + (i + 1) % K, 1 + K + i], 1)  # (0,0) (1,0) (0,1) (1,1)
    conn = np.concatenate([quad, quad + nv], 1)
    return system.ElevatedHexMesh(ctx, verts, conn, order)


def test_scratch_route():
    ctx = context()
    cap = system.SparsityGraph(system.DeviceMesh(ctx, part_of("cube-p1"), 1)).info.lds_key_capacity
    K = cap // 125 + 1
    assert 3 < K <= 132
    mesh = fan(ctx, K)
    g = system.SparsityGraph(system.DeviceMesh(ctx, mesh, 1))
    print(f"fan of {K} hexes: {g.info}")
    assert g.info.n_rows_scratch >= 5 and g.info.max_elems_per_node == K
    check_arrays(g, *csr_graph(mesh, 1, np.arange(1)))
    gc = system.SparsityGraph(system.DeviceMesh(ctx, mesh, 2), [1], kind="condensed")
    check_arrays(gc, *system.condensed_graph(mesh.elem_nodes, 4, 2, [1]), mesh.n_local_nodes * 2)
    small = fan(ctx, 3)
    g3 = system.SparsityGraph(system.DeviceMesh(ctx, small, 1))
    assert g3.info.n_rows_scratch == 0 and g3.info.max_elems_per_node == 3
    check_arrays(g3, *csr_graph(small, 1, np.arange(1)))


def test_workspace_does_not_grow_with_the_entries():
    """CubePartition(4, 4), one dof per node: in 1-D the 17 nodes couple with 12 * 5 + 3 * 9 + 2 * 5 = 97 partners and the graph is
    the tensor cube of that.  The tables of the design (node -> element table, counters, pointers, scan temporaries) come to
    about 150 KB; a list of node pairs or a copy of col_ind (4 nnz bytes) would not fit nnz bytes."""
    g = system.SparsityGraph(system.DeviceMesh(context(), system.CubePartition(4, 4), 1))
    print(f"nnz {g.info.nnz}, workspace {g.info.workspace_bytes} bytes")
    assert g.info.nnz == 97 ** 3 == 912673 == g.col_ind.numel()
    assert 0 < g.info.workspace_bytes <= g.info.nnz


def test_end_to_end_on_the_device_graph():
    from test_gpu_csr_solve import EPS, TOL, U, case, dense_of, dev, rel, true_residual
    c = case(2, 3)
    ctx, mf, n = c["ctx"], c["mf"], c["n"]
    g = mf.sparsity_graph()
    assert g.n == n and torch.equal(g.row_ptr, c["op"].row_ptr) and torch.equal(g.col_ind, c["op"].col_ind)
    vals = torch.zeros(g.info.nnz, dtype=torch.float64, device="cuda")
    assert mf.assemble_global(g.row_ptr, g.col_ind, vals, None, skip_dirichlet=True) == 0
    csr = system.CsrOperator(ctx, g.row_ptr, g.col_ind, vals)
    assert csr.info().nnz == g.info.nnz and csr.info().n_empty_rows == g.info.n_empty_rows
    x = dev(np.random.default_rng(4).standard_normal(n))
    y_mf, y_csr = torch.empty_like(x), torch.empty_like(x)
    mf.apply(x[None, :], y_mf[None, :])
    csr.apply(x, y_csr)
    free = dev(~c["dmask"], torch.bool)
    err = float((y_mf[free] - y_csr[free]).norm() / y_mf[free].norm())
    print(f"CSR apply on the device graph against the matrix-free apply on the free dofs: {err:.3e}")
    assert err <= 1e-11
    # the condensed system on the device's condensed graph, solved and recovered, against the solve on the full operator
    xa = torch.zeros(n, dtype=torch.float64, device="cuda")
    assert solve.pcg(c["op"], c["b"], xa, c["minv"], tol=TOL, residual_scaling="rhs").converged
    gc = mf.sparsity_graph("condensed")
    vals_c = torch.zeros(gc.info.nnz, dtype=torch.float64, device="cuda")
    rhs = torch.zeros((1, n), dtype=torch.float64, device="cuda")
    assert mf.condense_global(gc.row_ptr, gc.col_ind, vals_c, rhs) == 0
    op = system.CsrOperator(ctx, gc.row_ptr, gc.col_ind, vals_c)
    assert op.info().nnz == gc.info.nnz and op.info().n_empty_rows == gc.info.n_empty_rows == c["part"].n_elems * 8 * U
    op.dirichlet(c["M"], c["G"], rhs)
    minv = op.jacobi_inverse()
    X = torch.zeros((1, n), dtype=torch.float64, device="cuda")
    res = solve.pcg(op, rhs[0], X[0], minv, tol=TOL, residual_scaling="rhs")
    assert res.converged
    live = np.flatnonzero(np.diff(gc.row_ptr.cpu().numpy()) > 0)
    S = dense_of(op)
    true = true_residual(S, rhs[0].cpu().numpy(), X.cpu().numpy()[0], live)
    mf.recover_internal(X)
    torch.cuda.synchronize()
    cond = float(np.linalg.cond(S[np.ix_(live, live)]))
    err, bound = rel(X.cpu().numpy()[0], xa.cpu().numpy()), cond * (true + n * EPS)
    print(f"condensed on the device graph: {res.num_iters} iterations, against the assembled solve {err:.3e}, bound {bound:.3e}")
    assert err <= bound


def test_reproducible_and_refillable():
    ctx, part = context(), part_of("cube-p4")
    mesh = system.DeviceMesh(ctx, part, 5)
    a, b = system.SparsityGraph(mesh, [1, 3]), system.SparsityGraph(mesh, [1, 3])
    assert torch.equal(a.row_ptr, b.row_ptr) and torch.equal(a.col_ind, b.col_ind)
    n, nnz = a.info.n, a.info.nnz
    for _ in range(2):
        rp = torch.full((n + 2,), -7, dtype=torch.int64, device="cuda")
        ci = torch.full((nnz + 1,), -7, dtype=torch.int32, device="cuda")
        a.fill(rp, ci)
        assert torch.equal(rp[:n + 1], a.row_ptr) and torch.equal(ci[:nnz], a.col_ind)
        assert int(rp[n + 1]) == -7 and int(ci[nnz]) == -7  # nothing past the arrays
        assert int(ci[:nnz].min()) >= 0 and int(rp[:n + 1].min()) >= 0  # no sentinel left


def test_refusals():
    ctx, lib = context(), capi.load()
    mesh = system.DeviceMesh(ctx, part_of("cube-p2"), 4)
    quads = system.DeviceMesh(ctx, part_of("quads"), 4)

    def create(m, fi, kind):
        out = C.c_void_p()
        arr = None if fi is None else (C.c_int * len(fi))(*fi)
        rc = lib.l3k_graph_create(m._h, 0 if fi is None else len(fi), arr, kind, C.byref(out))
        return rc, out, lib.l3k_last_error().decode()

    for fi in ([3, 1], [1, 1], [0, 4], [-1, 2]):
        rc, out, msg = create(mesh, fi, 0)
        assert rc == -1 and out.value is None and msg.startswith("l3k_graph_create: field_inds["), (fi, msg)
        with pytest.raises(system.L3KError, match="strictly ascending"):
            system.SparsityGraph(mesh, fi)
    rc, out, msg = create(mesh, None, 2)
    assert rc == -1 and out.value is None and msg.startswith("l3k_graph_create: kind = 2")
    rc, out, msg = create(quads, None, 1)
    assert rc == -1 and out.value is None and "quads" in msg
    with pytest.raises(system.L3KError, match="quads"):
        system.SparsityGraph(quads, kind="condensed")
    g = system.SparsityGraph(mesh)
    assert g.info.nnz > 0
    assert lib.l3k_graph_fill(g._h, None, C.c_void_p(g.col_ind.data_ptr())) == -1
    assert lib.l3k_last_error().decode() == "l3k_graph_fill: null argument"
    assert lib.l3k_graph_fill(g._h, C.c_void_p(g.row_ptr.data_ptr()), None) == -1
    assert lib.l3k_last_error().decode().startswith("l3k_graph_fill: null col_ind")
    # a mesh without elements: every row empty, no col_ind needed
    empty = types.SimpleNamespace(dim=3, order=2, n_elems=0, n_interior_elems=0, elem_nodes=np.zeros((1, 27), np.uint32),
                                  elem_verts=np.zeros((1, 8, 3)), n_owned_nodes=5, n_ghost_nodes=0, n_local_nodes=5)
    g0 = system.SparsityGraph(system.DeviceMesh(ctx, empty, 2))
    assert g0.info.nnz == 0 and g0.info.n == g0.info.n_empty_rows == 10 and not g0.row_ptr.any() and g0.col_ind.numel() == 0
