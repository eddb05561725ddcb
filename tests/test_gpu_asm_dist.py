"""The assembled and the condensed system on partitioned meshes (l3k_asm_create_dist, l3k_csr_dist_*, l3k_csr_dirichlet_dist;
system.AssembledSystem(halo=...), system.DistributedCsrOperator, solve.pcg_distributed on it) with MORE THAN ONE RANK on one GPU:
the ranks are threads of this process, each with its own context and stream, and the exchanges go through the library's in-process
transport, as in tests/test_gpu_pmg_dist.py.  Every rank runs its whole script once per case (assembly, end, applies, diagonal,
a second assembly, the solves) and the tests read what it left; the single-rank twin of every case runs on the device too, and
tests/asm_dist_ref.py restates the matrices on the host (tests/test_asm_dist_cpu.py proves that file).

Meshes: quads SquarePartition((5, 4), 3, perturb=0.1), U = 3, Diffusion2D, cut in 4 by rcb_partition; hexes
CubePartition((4, 2, 2), 2, parts=(2, 1, 1), perturb=0.1), U = 4, Diffusion3D.  Bars: 1e-12 |K|_max entrywise for
matrices, 1e-11 relative L2 for applies, right-hand sides and diagonals, 1e-8 |x| for solutions at the solver tolerance 1e-10."""
import ctypes as C
import threading

import numpy as np
import pytest
import torch

import asm_dist_ref as AD
from l3ster_amd import capi, partition, solve, system
from l3ster_amd.distributed import InprocGroup, NativeHalo

pytestmark = pytest.mark.gpu
D2, D3, ADI2, ADI3 = system.KERNEL_DIFFUSION2D, system.KERNEL_DIFFUSION3D, system.KERNEL_ADIABATIC2D, system.KERNEL_ADIABATIC3D
APPLIES = [(1.0, 0.0, 1), (1.0, 0.0, 3), (1.0, 0.0, 5), (-0.5, 2.0, 1), (-0.5, 2.0, 3), (-0.5, 2.0, 5)]  # (alpha, beta, ncols)
_CASES, _WHOLE, _DIST = {}, {}, {}


def dev(a, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


def host(t):
    return t.detach().cpu().numpy().copy()


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(np.asarray(b)), 1e-300))


class ThreadAllReduce:
    """Sum all-reduce between the rank threads (tests/test_gpu_pmg_dist.py)"""

    def __init__(self, world):
        self.world, self.slots, self.barrier = world, [None] * world, threading.Barrier(world)

    def bind(self, rank):
        def allreduce(view):
            torch.cuda.synchronize()
            self.slots[rank] = view.clone()
            self.barrier.wait(timeout=120)
            total = sum(self.slots[r] for r in range(self.world))
            self.barrier.wait(timeout=120)
            view.copy_(total)
            torch.cuda.synchronize()
        return allreduce


def run_ranks(world, body, red=None):
    """body(rank) in one thread per rank; re-raises the first failure (tests/test_gpu_pmg_dist.py; a failing rank breaks the barrier
    of `red` so that the others do not wait for it)"""
    errors = []

    def guarded(rank):
        try:
            torch.cuda.set_device(0)
            with torch.cuda.stream(torch.cuda.Stream()):
                body(rank)
                torch.cuda.synchronize()
        except BaseException as exc:  # noqa: BLE001
            errors.append((rank, exc))
            if red is not None:
                red.barrier.abort()

    threads = [threading.Thread(target=guarded, args=(r,), daemon=True) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(300)
    assert not errors, errors
    assert not any(t.is_alive() for t in threads), "a rank did not return"


def rank_context():
    return system.Context(0, torch.cuda.current_stream().cuda_stream)


# ------------------------------------------------------------------------------------------------------ cases and scripts
def case(kind):
    if kind not in _CASES:
        q = AD.quad_case() if kind == "quad" else AD.cube_case()
        q.kind = kind
        q.g = AD.prescribed_values(q)  # T = x on the flagged dofs, [1, n]
        n = q.whole.n_local_nodes * q.U
        rng = np.random.default_rng(5)
        q.X = {a: rng.uniform(-1, 1, (a[2], n)) for a in APPLIES}
        q.Y0 = {a: rng.uniform(-1, 1, (a[2], n)) for a in APPLIES}
        _CASES[kind] = q
    return _CASES[kind]


def terms(q, mesh, sides):
    mf = system.MatrixFreeSystem(mesh, D2 if q.dim == 2 else D3, q.kpar)
    fe, fs = sides
    bnd = system.BoundaryTerm(mesh, ADI2 if q.dim == 2 else ADI3, fe, fs) if len(fe) else None
    return mf, bnd


def assemble(asm, mf, bnd):
    asm.begin()
    asm.add(mf)
    if bnd is not None:
        asm.add(bnd)


def csr_host(asm):
    return host(asm.row_ptr), host(asm.col_ind), host(asm.values)


def whole_run(kind, condensed=False):
    """the single-rank twin on the device: the matrix before and after end, rhs, diagonal, applies, the solves"""
    key = (kind, condensed)
    if key in _WHOLE:
        return _WHOLE[key]
    q, w = case(kind), {}
    torch.cuda.set_device(0)
    c = rank_context()
    mesh = system.DeviceMesh(c, q.whole, q.U, q.mask.astype(np.uint8))
    mf, bnd = terms(q, mesh, q.sides)
    asm = system.AssembledSystem(mesh, condensation="element_boundary" if condensed else "none")
    assemble(asm, mf, bnd)
    w["open"] = csr_host(asm)
    op = asm.end(dev(q.g))
    w["closed"], w["rhs"] = csr_host(asm), host(asm.rhs)
    w["diag"], w["minv"] = host(op.diag()), host(op.jacobi_inverse())
    w["apply"] = {}
    for a in ([] if condensed else APPLIES):
        Y = dev(q.Y0[a])
        op.apply(dev(q.X[a]), Y, a[0], a[1])
        w["apply"][a] = host(Y)
    b, minv = asm.rhs[0].contiguous(), op.jacobi_inverse()
    x = torch.zeros_like(b)
    w["jacobi"] = solve.pcg(op, b, x, minv, tol=1e-10, residual_scaling="rhs", max_iters=20000)
    if condensed:
        asm.recover(x)
        w["n_failed"] = asm.cond_info.n_failed
    w["x"] = host(x)
    if not condensed:
        x2 = torch.zeros_like(b)
        w["cheb"] = solve.pcg(op, b, x2, tol=1e-10, residual_scaling="rhs", max_iters=20000,
                              precond=solve.ChebyshevPreconditioner(op, minv, degree=2))
        w["x_cheb"] = host(x2)
    torch.cuda.synchronize()
    _WHOLE[key] = w
    return w


def dist_run(kind, condensed=False):
    """every rank's script, once: what each rank left, by rank"""
    key = (kind, condensed)
    if key in _DIST:
        return _DIST[key]
    q = case(kind)
    group, red, out = InprocGroup(q.world), ThreadAllReduce(q.world), {}

    def body(rank):
        d = out[rank] = {}
        c, part, no = rank_context(), q.parts[rank], q.n_owned(rank)
        mesh = system.DeviceMesh(c, part, q.U, q.local_mask(rank).astype(np.uint8))
        halo = NativeHalo(c, part, q.U, rank, q.world, transport=group)
        mf, bnd = terms(q, mesh, q.part_sides[rank])
        asm = system.AssembledSystem(mesh, condensation="element_boundary" if condensed else None, halo=halo)
        assemble(asm, mf, bnd)
        d["open"] = csr_host(asm)
        d["dist_info_open"] = asm._dist_info().dist
        g = dev(q.scatter(q.g, rank))
        op = asm.end(g)
        assert isinstance(op, system.DistributedCsrOperator) and op.n == no == asm.n_owned and asm.info.state == "closed"
        d["closed"], d["rhs"], d["rhs_ghost"] = csr_host(asm), host(asm.rhs[:, :no]), host(asm.rhs[:, no:])
        i = op.info
        d["counts"] = (i.n_owned, i.n_ghost, i.n_interior_rows, i.n_border_rows, i.n_ghost_rows)
        d["lists"] = tuple(host(t) for t in (i.interior_rows, i.border_rows, i.ghost_rows))
        d["local_n"], d["n_missing"] = op.local.n, asm.info.n_missing
        d["diag"], d["minv"] = host(op.diag()), host(op.jacobi_inverse())
        d["apply"] = {}
        for a in ([] if condensed else APPLIES):
            Y = dev(q.scatter(q.Y0[a], rank)) if a[1] != 0.0 else torch.full((a[2], no), float("nan"), dtype=torch.float64, device="cuda")
            op.apply(dev(q.scatter(q.X[a], rank)), Y, a[0], a[1])
            d["apply"][a] = host(Y)
        # a flagged dof of the whole mesh as a unit vector
        unit = np.zeros((1, q.g.shape[1]))
        unit[0, np.flatnonzero(q.mask)[0]] = 1.0
        d["unit"] = host(op.apply(dev(q.scatter(unit, rank)), torch.empty((1, no), dtype=torch.float64, device="cuda")))
        # the solves
        b, minv = asm.rhs[0, :no].contiguous(), op.jacobi_inverse()
        x = torch.zeros_like(b)
        d["jacobi"] = solve.pcg_distributed(op, c, b, x, minv=minv, tol=1e-10, residual_scaling="rhs", max_iters=20000,
                                            allreduce=red.bind(rank))
        if condensed:
            x = asm.recover(x)
            d["n_failed"] = asm.cond_info.n_failed
        d["x"] = host(x)
        if not condensed:
            x2 = torch.zeros_like(b)
            d["cheb"] = solve.pcg_distributed(op, c, b, x2, minv=minv, tol=1e-10, residual_scaling="rhs", max_iters=20000,
                                              allreduce=red.bind(rank), precond=dict(degree=2))
            d["x_cheb"] = host(x2)
        # the time loop: begin again, the same terms, a second end
        assemble(asm, mf, bnd)
        op2 = asm.end(g)
        d["closed2"], d["rhs2"] = csr_host(asm), host(asm.rhs[:, :no])
        d["same_handles"] = op2._h.value == op._h.value and op2.local._h.value == op.local._h.value

    run_ranks(q.world, body, red)
    _DIST[key] = out
    return out


def dense_sum(q, out, which):
    """sum_r R_r^T A_r R_r of the ranks' downloaded matrices"""
    return AD.sum_of_ranks(q, [AD.dense_of(*out[r][which]) for r in range(q.world)])


KINDS = ["quad", "cube"]


# ------------------------------------------------------------------------------ 1. the local matrices sum to the single-rank one
@pytest.mark.parametrize("kind", KINDS)
def test_local_matrices_sum_to_the_single_rank_matrix(kind):
    q, out, w = case(kind), dist_run(kind), whole_run(kind)
    assert any(m.n_ghost_nodes > 0 for m in q.parts)
    K, K_dev = dense_sum(q, out, "open"), AD.dense_of(*w["open"])
    K_cpu = AD.local_system(q, q.whole, q.sides, np.arange(q.whole.n_elems), with_rhs=False)[0]
    scale = np.abs(K_cpu).max()
    print(f"{kind}: max|sum - K| / |K|_max: device {np.abs(K - K_dev).max() / scale:.2e}, host {np.abs(K - K_cpu).max() / scale:.2e}")
    assert np.abs(K - K_dev).max() <= 1e-12 * scale
    assert np.abs(K - K_cpu).max() <= 1e-12 * scale
    assert all(out[r]["n_missing"] == 0 and out[r]["dist_info_open"] is None for r in range(q.world))


# ---------------------------------------------------------------------------------------------------------- 2. row classes
@pytest.mark.parametrize("kind", KINDS)
def test_row_classes(kind):
    q, out = case(kind), dist_run(kind)
    full = []
    for r in range(q.world):
        row_ptr, col_ind, _ = out[r]["open"]
        no, n = q.n_owned(r), q.parts[r].n_local_nodes * q.U
        want = AD.row_classes(row_ptr, col_ind, no)
        assert out[r]["counts"] == (no, n - no, want[0].size, want[1].size, want[2].size) and out[r]["local_n"] == n
        for got, exp in zip(out[r]["lists"], want):
            assert got.dtype == np.int32 and np.array_equal(got, exp)
        for i in out[r]["lists"][0]:
            assert not (col_ind[row_ptr[i]:row_ptr[i + 1]] >= no).any()  # no interior row holds a ghost column
        full.append(all(x.size > 0 for x in want))
    assert any(full), "no rank has interior, border and ghost rows"


# ---------------------------------------------------------------------------------------------------------------- 3. apply
@pytest.mark.parametrize("kind", KINDS)
def test_apply(kind):
    q, out, w = case(kind), dist_run(kind), whole_run(kind)
    for a in APPLIES:
        got, want = q.gather([out[r]["apply"][a] for r in range(q.world)]), w["apply"][a]
        assert np.isfinite(got).all()  # (beta = 0: y held NaN)
        err = rel(got, want)
        print(f"{kind} alpha {a[0]} beta {a[1]} ncols {a[2]}: {err:.2e}")
        assert err <= 1e-11


# ----------------------------------------------------------------------------------------------------------- 4. world of one
@pytest.mark.parametrize("kind", KINDS)
def test_world_of_one_is_the_csr_operator_bit_for_bit(kind):
    q, w = case(kind), whole_run(kind)
    torch.cuda.set_device(0)
    c = rank_context()
    row_ptr, col_ind, values = (dev(w["closed"][0], torch.int64), dev(w["closed"][1], torch.int32), dev(w["closed"][2]))
    local = system.CsrOperator(c, row_ptr, col_ind, values)
    op = system.DistributedCsrOperator(local, NativeHalo(c, q.whole, q.U, 0, 1, transport=InprocGroup(1)))
    i = op.info
    assert (i.n_owned, i.n_ghost, i.n_border_rows, i.n_ghost_rows) == (local.n, 0, 0, 0) and i.n_interior_rows == local.n
    for a in APPLIES:
        X, Y, Z = dev(q.X[a]), dev(q.Y0[a]), dev(q.Y0[a])
        op.apply(X, Y, a[0], a[1])
        local.apply(X, Z, a[0], a[1])
        assert torch.equal(Y, Z), a
    assert torch.equal(op.jacobi_inverse(0.9, 1e-3), local.jacobi_inverse(0.9, 1e-3)) and torch.equal(op.diag(), local.diag())


# ------------------------------------------------------------------------------------------------------------------ 5. end
@pytest.mark.parametrize("kind", KINDS)
def test_end(kind):
    q, out, w = case(kind), dist_run(kind), whole_run(kind)
    ranks = range(q.world)
    rhs, diag, minv = (q.gather([out[r][k] for r in ranks]) for k in ("rhs", "diag", "minv"))
    print(f"{kind}: rhs {rel(rhs, w['rhs']):.2e}, diag {rel(diag[0], w['diag']):.2e}, minv {rel(minv[0], w['minv']):.2e}")
    assert rel(rhs, w["rhs"]) <= 1e-11 and rel(diag[0], w["diag"]) <= 1e-11 and rel(minv[0], w["minv"]) <= 1e-11
    A, A_w = dense_sum(q, out, "closed"), AD.dense_of(*w["closed"])
    assert np.abs(A - A_w).max() <= 1e-12 * np.abs(A_w).max()
    # a flagged owned row applies as the identity
    unit = np.zeros_like(q.g)
    unit[0, np.flatnonzero(q.mask)[0]] = 1.0
    assert np.array_equal(q.gather([out[r]["unit"] for r in ranks]), unit)
    for r in ranks:
        row_ptr, col_ind, values = out[r]["closed"]
        no, mask = q.n_owned(r), q.local_mask(r)
        assert not out[r]["rhs_ghost"].any()  # exported and set to 0
        for i in np.flatnonzero(mask):
            row = values[row_ptr[i]:row_ptr[i + 1]]
            if i >= no:
                assert not row.any()  # a flagged ghost row is all zero: the owner holds the 1
            else:
                assert np.array_equal(row, (col_ind[row_ptr[i]:row_ptr[i + 1]] == i).astype(np.float64))
        # the second assembly of the time loop reproduces the first (the scatter's atomics reorder a handful of terms per entry)
        scale = np.abs(values).max()
        assert np.abs(out[r]["closed2"][2] - values).max() <= 1e-13 * scale
        assert np.abs(out[r]["rhs2"] - out[r]["rhs"]).max() <= 1e-13 * max(scale, np.abs(out[r]["rhs"]).max())
        assert out[r]["same_handles"]


# ---------------------------------------------------------------------------------------------------------------- 6. solve
@pytest.mark.parametrize("kind", KINDS)
def test_solve(kind):
    q, out, w = case(kind), dist_run(kind), whole_run(kind)
    ranks = range(q.world)
    for name, xk in (("jacobi", "x"), ("cheb", "x_cheb")):
        res = [out[r][name] for r in ranks]
        assert all(s.converged for s in res) and w[name].converged
        assert len({s.num_iters for s in res}) == 1
        x = q.gather([out[r][xk] for r in ranks])[0]
        diff = np.linalg.norm(x - w[xk]) / np.linalg.norm(w[xk])
        print(f"{kind} {name}: {res[0].num_iters} iterations on {q.world} ranks, {w[name].num_iters} on one; |x - x_1| / |x_1| = {diff:.2e}")
        if name == "jacobi":
            assert abs(res[0].num_iters - w[name].num_iters) <= 1  # (the margin tests/test_solve.py gives thread ranks)
        assert diff <= 1e-8


# ------------------------------------------------------------------------------------------ 7. condensed quads on four ranks
def test_condensed_quads_on_four_ranks():
    q, out, w = case("quad"), dist_run("quad", condensed=True), whole_run("quad", condensed=True)
    ranks = range(q.world)
    assert all(out[r]["n_failed"] == 0 for r in ranks) and w["n_failed"] == 0
    assert all(out[r]["jacobi"].converged for r in ranks) and len({out[r]["jacobi"].num_iters for r in ranks}) == 1
    # the rows of element-internal dofs are empty and frozen
    assert any((out[r]["minv"] == 0).any() for r in ranks)
    x = q.gather([out[r]["x"] for r in ranks])[0]
    diff = np.linalg.norm(x - w["x"]) / np.linalg.norm(w["x"])
    print(f"condensed quads: {out[0]['jacobi'].num_iters} iterations on 4 ranks, {w['jacobi'].num_iters} on one; "
          f"all dofs |x - x_1| / |x_1| = {diff:.2e}")
    assert diff <= 1e-8
    assert rel(q.gather([out[r]["rhs"] for r in ranks]), w["rhs"]) <= 1e-11


# ------------------------------------------------------------------------- 8. condensed hexes through the caller's arrays
def test_condensed_hexes_through_the_callers_arrays():
    q = case("cube")
    group, out = InprocGroup(q.world), {}
    rng = np.random.default_rng(9)
    n = q.whole.n_local_nodes * q.U
    X = rng.uniform(-1, 1, (2, n))

    def script(c, part, mask, g_local, n_owned, halo, x_owned):
        """graph -> condense_global -> dirichlet_local -> DistributedCsrOperator -> apply, on one rank"""
        mesh = system.DeviceMesh(c, part, q.U, mask.astype(np.uint8))
        mf = system.MatrixFreeSystem(mesh, D3, q.kpar)
        graph = system.SparsityGraph(mesh, kind="condensed")
        values = torch.zeros(graph.info.nnz, dtype=torch.float64, device="cuda")
        rhs = torch.zeros((1, graph.n), dtype=torch.float64, device="cuda")
        assert mf.condense_global(graph.row_ptr, graph.col_ind, values, rhs) == 0
        local = system.CsrOperator(c, graph.row_ptr, graph.col_ind, values)
        local.dirichlet_local(dev(mask, torch.uint8), dev(g_local), rhs, n_owned)
        op = system.DistributedCsrOperator(local, halo, n_owned)
        Y = torch.full((x_owned.shape[0], n_owned), float("nan"), dtype=torch.float64, device="cuda")
        op.apply(dev(x_owned), Y)
        op.export_add(rhs[:, n_owned:].contiguous(), rhs[:, :n_owned])
        return host(Y), host(rhs[:, :n_owned]), host(op.jacobi_inverse())

    def body(rank):
        c, part = rank_context(), q.parts[rank]
        halo = NativeHalo(c, part, q.U, rank, q.world, transport=group)
        out[rank] = script(c, part, q.local_mask(rank), q.g[:, q.local_dofs(rank)], q.n_owned(rank), halo, q.scatter(X, rank))

    run_ranks(q.world, body)
    torch.cuda.set_device(0)
    c = rank_context()
    Y_w, rhs_w, minv_w = script(c, q.whole, q.mask, q.g, n, NativeHalo(c, q.whole, q.U, 0, 1, transport=InprocGroup(1)), X)
    got = [q.gather([out[r][k] for r in range(q.world)]) for k in range(3)]
    print(f"condensed hexes: apply {rel(got[0], Y_w):.2e}, rhs {rel(got[1], rhs_w):.2e}, minv {rel(got[2], minv_w):.2e}")
    assert np.isfinite(got[0]).all() and rel(got[0], Y_w) <= 1e-11
    assert rel(got[1], rhs_w) <= 1e-11 and rel(got[2][0], minv_w) <= 1e-11
    assert (minv_w == 0).any()  # the element-internal dofs: empty rows, frozen


# -------------------------------------------------------------------------------------------- 9. a rank that owns nothing
def test_a_rank_that_owns_nothing():
    """The unstructured mesh of tests/test_partition_unstructured.py cut in two parts of a world of three (tests/test_gpu_pmg_dist.py):
    rank 1 owns no element and no node; create, assemble, end and apply return on it, the other two match the one-rank result."""
    from test_partition_unstructured import part_vector, small_mesh
    U, world = 4, 3
    en, ev, nn = small_mesh(2, n_keep=120)
    pv = part_vector(ev, 2) * 2
    n_nodes = int(en.max()) + 1
    rng = np.random.default_rng(13)
    x_w, g_w = rng.uniform(-1, 1, (n_nodes, U)), rng.uniform(-1, 1, (n_nodes, U))
    out = {}

    def script(c, part, rank, n_ranks, group):
        ids = part.node_grid_id[:part.n_local_nodes].astype(np.int64)
        mask = np.zeros((len(ids), U), np.uint8)
        mask[ids % 11 == 0, 0] = 1
        mesh = system.DeviceMesh(c, part, U, mask.reshape(-1))
        halo = NativeHalo(c, part, U, rank, n_ranks, transport=group)
        mf = system.MatrixFreeSystem(mesh, D3, [1.0, 0.0])
        asm = system.AssembledSystem(mesh, halo=halo)
        asm.begin()
        asm.add(mf)
        no = part.n_owned_nodes
        op = asm.end(dev(g_w[ids[:no]].reshape(1, -1)))
        Y = torch.full((1, no * U), float("nan"), dtype=torch.float64, device="cuda")
        op.apply(dev(x_w[ids[:no]].reshape(1, -1)), Y)
        minv = op.jacobi_inverse()
        torch.cuda.current_stream().synchronize()
        return ids[:no].copy(), host(Y).reshape(-1, U), host(asm.rhs[:, :no * U]).reshape(-1, U), host(minv).reshape(-1, U), op.info

    groups = [InprocGroup(world)]

    def body(rank):
        out[rank] = script(rank_context(), partition.PartitionedMesh(en, ev, nn, pv, rank, world, 2), rank, world, groups[0])

    run_ranks(world, body)
    assert out[1][0].size == 0 and out[1][1].size == 0 and out[1][4].n_owned == 0 and out[1][4].n_ghost == 0
    torch.cuda.set_device(0)
    whole = partition.PartitionedMesh(en, ev, nn, np.zeros_like(pv), 0, 1, 2)
    ids_w, Y_w, rhs_w, minv_w, _ = script(rank_context(), whole, 0, 1, InprocGroup(1))
    row = np.argsort(ids_w)
    assert np.array_equal(ids_w[row], np.arange(n_nodes))
    got = [np.zeros_like(Y_w) for _ in range(3)]
    for r in (0, 2):
        for k in range(3):
            got[k][row[out[r][0]]] = out[r][1 + k]
    assert sum(len(out[r][0]) for r in (0, 2)) == n_nodes
    print(f"a rank that owns nothing: apply {rel(got[0], Y_w):.2e}, rhs {rel(got[1], rhs_w):.2e}, minv {rel(got[2], minv_w):.2e}")
    assert rel(got[0], Y_w) <= 1e-11 and rel(got[1], rhs_w) <= 1e-11 and rel(got[2], minv_w) <= 1e-11


# ------------------------------------------------------------------------------------------------------------ 10. refusals
def test_refusals():
    lib = capi.load()
    torch.cuda.set_device(0)
    c, c2 = rank_context(), rank_context()
    q = case("cube")
    part = q.parts[1]  # (rank 1 holds the ghost nodes)
    assert part.n_ghost_nodes > 0
    mesh = system.DeviceMesh(c, part, q.U, q.local_mask(1).astype(np.uint8))
    group = InprocGroup(q.world)
    halo = NativeHalo(c, part, q.U, 1, q.world, transport=group)

    def refused(call, name, *more):
        h = C.c_void_p(0xdead)
        rc = call(h)
        msg = lib.l3k_last_error().decode()
        assert rc == -1 and name in msg and h.value == 0xdead, (rc, msg)  # the output is untouched
        for word in more:
            assert word in msg, msg

    create = lambda m, h, cond=0: (lambda out: lib.l3k_asm_create_dist(m._h, h._h if h else None, 0, None, 1, 0, cond, C.byref(out)))
    # without a halo a ghosted mesh is still refused
    with pytest.raises(system.L3KError, match="partitioned"):
        system.AssembledSystem(mesh)
    refused(create(mesh, None), "l3k_asm_create_dist", "null")
    refused(create(mesh, NativeHalo(c, part, q.U + 1, 1, q.world, transport=group)), "l3k_asm_create_dist", "dofs per node")
    refused(create(mesh, NativeHalo(c, q.parts[0], q.U, 0, q.world, transport=group)), "l3k_asm_create_dist", "ghost dofs")
    refused(create(mesh, NativeHalo(c2, part, q.U, 1, q.world, transport=group)), "l3k_asm_create_dist", "different contexts")
    refused(create(mesh, halo, 1), "l3k_asm_create_dist", "hex")  # condensed on hexes
    refused(lambda out: lib.l3k_asm_create_dist(None, halo._h, 0, None, 1, 0, 0, C.byref(out)), "l3k_asm_create_dist", "null")
    assert lib.l3k_asm_create_dist(mesh._h, halo._h, 0, None, 1, 0, 0, None) == -1
    # the distributed operator
    asm = system.AssembledSystem(mesh, halo=halo)
    n, no = asm.n, asm.n_owned
    local = system.CsrOperator(c, asm.row_ptr, asm.col_ind, asm.values)
    refused(lambda out: lib.l3k_csr_dist_create(local._h, halo._h, no - 1, C.byref(out)), "l3k_csr_dist_create", "n_owned")
    refused(lambda out: lib.l3k_csr_dist_create(None, halo._h, no, C.byref(out)), "l3k_csr_dist_create", "null")
    refused(lambda out: lib.l3k_csr_dist_create(local._h, None, no, C.byref(out)), "l3k_csr_dist_create", "null")
    assert lib.l3k_csr_dist_create(local._h, halo._h, no, None) == -1
    local2 = system.CsrOperator(c2, asm.row_ptr, asm.col_ind, asm.values)
    refused(lambda out: lib.l3k_csr_dist_create(local2._h, halo._h, no, C.byref(out)), "l3k_csr_dist_create", "different contexts")
    with pytest.raises(system.L3KError, match="l3k_csr_dirichlet_dist.*n_owned"):
        local.dirichlet_local(dev(q.local_mask(1), torch.uint8), torch.zeros(n, dtype=torch.float64, device="cuda"),
                              torch.zeros(n, dtype=torch.float64, device="cuda"), n + 1)
    assert lib.l3k_csr_dist_apply(None, None, 0, None, 0, 1, 1.0, 0.0) == -1 and lib.l3k_csr_dist_diag(None, None, 1.0, 0.0, None) == -1
    assert lib.l3k_csr_dist_info_get(None, None) == -1
    # the system: the dist info of an open system is NULL; ldg < n_owned leaves it open; end on a system that is not open
    i = capi.AsmDistInfo()
    assert lib.l3k_asm_dist_info_get(asm._h, C.byref(i)) == 0 and i.dist is None and (i.n_owned, i.n_ghost) == (no, n - no)
    assert lib.l3k_asm_dist_info_get(asm._h, None) == -1 and lib.l3k_asm_dist_info_get(None, C.byref(i)) == -1
    with pytest.raises(system.L3KError, match="not open"):
        asm.end()
    asm.begin()
    assert asm._dist_info().dist is None
    g = torch.zeros((1, no), dtype=torch.float64, device="cuda")
    assert lib.l3k_asm_end(asm._h, C.c_void_p(g.data_ptr()), no - 1) == -1
    assert "l3k_asm_end" in lib.l3k_last_error().decode() and "owned" in lib.l3k_last_error().decode()
    assert asm.info.state == "open" and asm._dist_info().dist is None
    # a single-rank system has no dist info
    single = system.AssembledSystem(system.DeviceMesh(c, q.whole, q.U))
    assert lib.l3k_asm_dist_info_get(single._h, C.byref(i)) == -1 and "not partitioned" in lib.l3k_last_error().decode()
    # recover with ldx < n_local on a closed condensed partitioned system (a world of one: nothing to exchange)
    qq = case("quad")
    mesh2 = system.DeviceMesh(c, qq.whole, qq.U, qq.mask.astype(np.uint8))
    halo2 = NativeHalo(c, qq.whole, qq.U, 0, 1, transport=InprocGroup(1))
    cond = system.AssembledSystem(mesh2, condensation="element_boundary", halo=halo2)
    mf2, bnd2 = terms(qq, mesh2, qq.sides)
    assemble(cond, mf2, bnd2)
    x = torch.zeros((1, cond.n), dtype=torch.float64, device="cuda")
    assert lib.l3k_asm_recover(cond._h, C.c_void_p(x.data_ptr()), cond.n) == -1 and "not closed" in lib.l3k_last_error().decode()
    cond.end(dev(qq.g))
    assert lib.l3k_asm_recover(cond._h, C.c_void_p(x.data_ptr()), cond.n - 1) == -1
    assert "l3k_asm_recover" in lib.l3k_last_error().decode() and "leading dimension" in lib.l3k_last_error().decode()
    assert lib.l3k_asm_recover(cond._h, None, cond.n) == -1 and asm.info.state == "open" and cond.info.state == "closed"
