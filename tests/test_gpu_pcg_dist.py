"""The collective solve of a partitioned system inside the library (l3k_halo_allreduce_sum, l3k_csr_dist_apply_energy,
l3k_csr_dist_pcg_solve, l3k_pcg_solve_dist, l3k_csr_dist_cheb_create, l3k_cheb_create_dist; solve.pcg_distributed(native=True))
with MORE THAN ONE RANK on one GPU: the ranks are threads of this process, each with its own context and stream, over the
library's in-process transport, as in tests/test_gpu_asm_dist.py, whose cases, scripts and single-rank twins are reused.  Every rank
runs its whole script once per case and the tests read what it left.

Bars: the all-reduce bit for bit against tests/pcg_dist_ref.py; <x, A x> 1e-11 relative against the host matrices of
tests/asm_dist_ref.py; iteration counts within 1 of the host loop (the reduction orders differ); 1e-8 |x| for solutions at the
solver tolerance 1e-10; lambda_est 1e-10 relative against the host loop's power method."""
import ctypes as C

import numpy as np
import pytest
import torch

import pcg_dist_ref as PD
from l3ster_amd import capi, partition, solve, system
from l3ster_amd.distributed import InprocGroup, NativeDistributedOperator, NativeHalo
from test_gpu_asm_dist import ThreadAllReduce, assemble, case, dev, host, rank_context, rel, run_ranks, terms, whole_run

pytestmark = pytest.mark.gpu
D3 = system.KERNEL_DIFFUSION3D
SOLVE = dict(tol=1e-10, residual_scaling="rhs", max_iters=20000)
DEGREES = (2, 3)
SENTINEL = 7.25
_CSR, _MF, _HOST = {}, {}, {}


def bits(v):
    return np.asarray(v, dtype=np.float64).view(np.uint64).tolist()


def same_on_all_ranks(results):
    """iterations, convergence and the BITS of the achieved tolerance"""
    return len({(s.num_iters, s.converged, bits([s.tol])[0]) for s in results}) == 1 and results[0].tol == results[0].tol


def host_system(kind):
    if kind not in _HOST:
        q = case(kind)
        _HOST[kind] = PD.closed_system(q)
    return _HOST[kind]


# ---------------------------------------------------------------------------------------------------------- 1. all-reduce
def halo_parts(world):
    """one part per rank of a world: the whole cube (no neighbour), the cube's two parts, the square's four"""
    if world == 1:
        q = case("cube")
        return q, [q.whole]
    q = case("cube") if world == 2 else case("quad")
    return q, q.parts


@pytest.mark.parametrize("world,isolated", [(1, False), (2, False), (4, False), (2, True)])
def test_allreduce_is_the_sum_in_rank_order(world, isolated):
    """isolated: both ranks bring the halo of a whole mesh -- no neighbour, nothing to exchange -- and still take part"""
    q, parts = halo_parts(world)
    if isolated:
        parts = [q.whole] * world
    group, out, lib = InprocGroup(world), {}, capi.load()
    steps, chain_count = 200, 3
    start = PD.order_dependent_rows(world, chain_count)

    def body(rank):
        d = out[rank] = {}
        c = rank_context()
        halo = NativeHalo(c, parts[rank], q.U, rank, world, transport=group)
        for count in (1, 3, 8):
            t = dev(PD.order_dependent_rows(world, count)[rank])
            assert halo.allreduce(t) is t
            d[count] = host(t)
        s = dev(start[rank])
        for _ in range(steps):  # (nothing waits for the device in here)
            halo.allreduce(s)
            s.mul_(0.5).add_(float(rank))
        d["chain"] = host(s)
        # refusals leave the values alone and involve no peer
        keep = dev(np.arange(1.0, 10.0))
        for count, ptr in ((0, keep.data_ptr()), (9, keep.data_ptr()), (-1, keep.data_ptr()), (3, None)):
            assert lib.l3k_halo_allreduce_sum(halo._h, C.c_void_p(ptr), count) == -1
            assert "l3k_halo_allreduce_sum" in lib.l3k_last_error().decode()
        assert lib.l3k_halo_allreduce_sum(None, C.c_void_p(keep.data_ptr()), 3) == -1
        with pytest.raises(capi.L3KError):
            halo.allreduce(torch.zeros(9, dtype=torch.float64, device="cuda"))
        d["keep"] = host(keep)

    run_ranks(world, body)
    for count in (1, 3, 8):
        want = PD.sum_in_rank_order(PD.order_dependent_rows(world, count))
        for rank in range(world):
            assert bits(out[rank][count]) == bits(want), (count, rank)
    want = PD.chain(world, chain_count, steps, start)
    for rank in range(world):
        assert bits(out[rank]["chain"]) == bits(want[rank]), rank
        assert np.array_equal(out[rank]["keep"], np.arange(1.0, 10.0))
    assert np.isfinite(want).all() and (world == 1 or not np.array_equal(want[0], start[0]))


# ------------------------------------------------------------------------------------------------- the CSR script of a case
def csr_run(kind, condensed=False):
    """every rank's script on the assembled (or condensed) system of a case, once: what each rank left, by rank"""
    key = (kind, condensed)
    if key in _CSR:
        return _CSR[key]
    q = case(kind)
    group, red, out = InprocGroup(q.world), ThreadAllReduce(q.world), {}
    xw = np.random.default_rng(17).uniform(-1, 1, (1, q.whole.n_local_nodes * q.U))

    def body(rank):
        d = out[rank] = {}
        c, part, no = rank_context(), q.parts[rank], q.n_owned(rank)
        mesh = system.DeviceMesh(c, part, q.U, q.local_mask(rank).astype(np.uint8))
        halo = NativeHalo(c, part, q.U, rank, q.world, transport=group)
        mf, bnd = terms(q, mesh, q.part_sides[rank])
        asm = system.AssembledSystem(mesh, condensation="element_boundary" if condensed else None, halo=halo)
        assemble(asm, mf, bnd)
        op = asm.end(dev(q.scatter(q.g, rank)))
        b, minv = asm.rhs[0, :no].contiguous(), op.jacobi_inverse()
        allreduce = red.bind(rank)
        zeros = lambda: torch.zeros_like(b)
        if not condensed:  # ---- 2. y <- A x with this rank's share of <x, A x>
            X = dev(q.scatter(xw, rank))[0]
            y0 = op.apply(X, torch.full_like(X, float("nan")))
            S = [torch.full((8,), SENTINEL, dtype=torch.float64, device="cuda") for _ in range(3)]
            y1 = op.apply_energy(X, torch.full_like(X, float("nan")), S[0])
            y2 = op.apply_energy(X, torch.full_like(X, float("nan")), S[1])
            y3 = op.apply(X[None, :], torch.full_like(X, float("nan"))[None, :], energy=S[2])[0]
            d["energy"] = dict(y=[host(v) for v in (y0, y1, y2, y3)], s=[host(v) for v in S], fused=op.energy_fused)
        # ---- 3. Jacobi: inside the library, and the host loop with the threads' all-reduce on the same operator
        x = zeros()
        d["native"] = solve.pcg_distributed(op, c, b, x, minv=minv, native=True, **SOLVE)
        d["host"] = solve.pcg_distributed(op, c, b, zeros(), minv=minv, allreduce=allreduce, **SOLVE)
        d["x"] = host(asm.recover(x) if condensed else x)
        d["frozen"] = int((minv == 0).sum().item())
        if not condensed:  # ---- 4. Chebyshev
            d["est_host"] = solve._distributed_lambda_est(op, minv, allreduce)
            for deg in DEGREES:
                ch = solve.DistributedChebyshev(op, minv, degree=deg)
                xc = zeros()
                d["cheb", deg] = dict(info=ch.info, native=solve.pcg_distributed(op, c, b, xc, minv=minv, native=True, precond=ch, **SOLVE),
                                      host=solve.pcg_distributed(op, c, b, zeros(), minv=minv, allreduce=allreduce,
                                                                 precond=dict(degree=deg), **SOLVE),
                                      x=host(xc), given=solve.DistributedChebyshev(op, minv, degree=deg, lambda_max=ch.info.lambda_max).info)
            xd = zeros()  # the options as a dict: the power method inside the library, the object made and dropped by the call
            d["cheb_dict"] = solve.pcg_distributed(op, c, b, xd, native=True, minv=minv, precond=dict(degree=2), **SOLVE)
            d["x_dict"] = host(xd)
        if kind == "cube":  # ---- 7. edges
            e = d["edges"] = {}
            xz = zeros()
            e["zero"] = (solve.pcg_distributed(op, c, zeros(), xz, minv=minv, native=True, **SOLVE), host(xz))
            go = lambda **kw: solve.pcg_distributed(op, c, b, zeros(), minv=minv, native=True, throw_on_fail=False,
                                                    **{**dict(tol=1e-10, residual_scaling="rhs", max_iters=20000), **kw})
            e["three"] = go(max_iters=3)
            e["every5"] = go(check_every=5)
            e["every5_capped"] = go(check_every=5, max_iters=13)
            e["to_the_end"] = go(tol=0.0, max_iters=500)
            again = zeros()
            solve.pcg_distributed(op, c, b, again, minv=minv, native=True, **SOLVE)
            e["again"] = host(again)

    run_ranks(q.world, body, red)
    _CSR[key] = out
    return out


KINDS = ["quad", "cube"]
JACOBI = [("quad", False), ("quad", True), ("cube", False)]


# ------------------------------------------------------------------------------------------- 2. l3k_csr_dist_apply_energy
@pytest.mark.parametrize("kind", KINDS)
def test_apply_energy(kind):
    q, out = case(kind), csr_run(kind)
    ranks = range(q.world)
    total = 0.0
    for r in ranks:
        e = out[r]["energy"]
        y0, y1, y2, y3 = e["y"]
        assert np.isfinite(y0).all() and bits(y1) == bits(y0) and bits(y2) == bits(y0) and bits(y3) == bits(y0), r
        s1, s2, s3 = e["s"]
        keep = [0, 2, 3, 4, 5, 6, 7]
        assert np.array_equal(s1[keep], np.full(7, SENTINEL)) and s1[1] != SENTINEL and bits(s1) == bits(s2) == bits(s3), r
        assert e["fused"]
        total += s1[1]
    A = host_system(kind)[2]
    xw = np.random.default_rng(17).uniform(-1, 1, A.shape[0])
    want = xw @ A @ xw
    print(f"{kind}: sum of the ranks' <x, A x> {total:.15e}, host x^T A x {want:.15e}, relative {abs(total - want) / abs(want):.2e}")
    assert abs(total - want) <= 1e-11 * abs(want)


# -------------------------------------------------------------------------------------------------------- 3. Jacobi, CSR
@pytest.mark.parametrize("kind,condensed", JACOBI)
def test_jacobi_csr(kind, condensed):
    q, out, w = case(kind), csr_run(kind, condensed), whole_run(kind, condensed)
    ranks = range(q.world)
    native, hostloop = [out[r]["native"] for r in ranks], [out[r]["host"] for r in ranks]
    assert all(s.converged for s in native + hostloop) and same_on_all_ranks(native)
    x = q.gather([out[r]["x"] for r in ranks])[0]
    diff = np.linalg.norm(x - w["x"]) / np.linalg.norm(w["x"])
    print(f"{kind}{' condensed' if condensed else ''}: {native[0].num_iters} iterations in the library, {hostloop[0].num_iters} in the "
          f"host loop, {w['jacobi'].num_iters} on one rank; |x - x_1| / |x_1| = {diff:.2e}")
    assert abs(native[0].num_iters - hostloop[0].num_iters) <= 1
    assert diff <= 1e-8
    assert (sum(out[r]["frozen"] for r in ranks) > 0) == condensed


# ------------------------------------------------------------------------------------------------------ 4. Chebyshev, CSR
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("deg", DEGREES)
def test_chebyshev_csr(kind, deg):
    q, out, w = case(kind), csr_run(kind), whole_run(kind)
    check_chebyshev(q, out, w["x"], deg, f"{kind} CSR")
    if deg == 2:
        ranks = range(q.world)
        assert same_on_all_ranks([out[r]["cheb_dict"] for r in ranks])
        assert out[0]["cheb_dict"].num_iters == out[0]["cheb", 2]["native"].num_iters
        assert all(bits(out[r]["x_dict"]) == bits(out[r]["cheb", 2]["x"]) for r in ranks)


def check_chebyshev(q, out, x_one, deg, what):
    ranks = range(q.world)
    runs = [out[r]["cheb", deg] for r in ranks]
    est = [c["info"].lambda_est for c in runs]
    est_host = out[0]["est_host"]
    assert len(set(bits(est))) == 1 and all(c["info"].power_iters == 10 and c["info"].degree == deg for c in runs)
    assert abs(est[0] - est_host) <= 1e-10 * est_host, (est[0], est_host)
    assert all(c["given"].power_iters == 0 and c["given"].lambda_max == c["info"].lambda_max for c in runs)
    native, hostloop = [c["native"] for c in runs], [c["host"] for c in runs]
    assert all(s.converged for s in native + hostloop) and same_on_all_ranks(native)
    x = q.gather([c["x"] for c in runs])[0]
    diff = np.linalg.norm(x - x_one) / np.linalg.norm(x_one)
    print(f"{what} degree {deg}: lambda_est {est[0]:.12f} (host loop {est_host:.12f}); {native[0].num_iters} iterations in the library, "
          f"{hostloop[0].num_iters} in the host loop; |x - x_1| / |x_1| = {diff:.2e}")
    assert abs(native[0].num_iters - hostloop[0].num_iters) <= 1
    assert diff <= 1e-8


# ------------------------------------------------------------------------------------------------------- 5. matrix-free
def mf_whole():
    """the single-rank twin: solve.pcg on the whole cube"""
    if "whole" not in _MF:
        q = case("cube")
        torch.cuda.set_device(0)
        c = rank_context()
        mf = system.MatrixFreeSystem(system.DeviceMesh(c, q.whole, q.U, q.mask.astype(np.uint8)), D3, q.kpar)
        diag, rhs = mf.diag_rhs(dev(q.g))
        minv, b = solve.jacobi_inverse_native(c, diag), rhs[0].contiguous()
        x = torch.zeros_like(b)
        res = solve.pcg(mf, b, x, minv, **SOLVE)
        torch.cuda.synchronize()
        _MF["whole"] = dict(x=host(x), res=res)
    return _MF["whole"]


def mf_run():
    if "dist" in _MF:
        return _MF["dist"]
    q = case("cube")
    group, red, out = InprocGroup(q.world), ThreadAllReduce(q.world), {}

    def body(rank):
        d = out[rank] = {}
        c, part = rank_context(), q.parts[rank]
        mesh = system.DeviceMesh(c, part, q.U, q.local_mask(rank).astype(np.uint8))
        mf = system.MatrixFreeSystem(mesh, D3, q.kpar)
        op = NativeDistributedOperator(mf, NativeHalo(c, part, q.U, rank, q.world, transport=group))
        diag, rhs = op.diag_rhs(dev(q.scatter(q.g, rank)))
        minv, b = solve.jacobi_inverse_native(c, diag), rhs[0].contiguous()
        allreduce = red.bind(rank)
        zeros = lambda: torch.zeros_like(b)
        x = zeros()
        d["native"] = solve.pcg_distributed(op, c, b, x, minv=minv, native=True, **SOLVE)
        d["host"] = solve.pcg_distributed(op, c, b, zeros(), minv=minv, allreduce=allreduce, **SOLVE)
        d["x"] = host(x)
        d["est_host"] = solve._distributed_lambda_est(op, minv, allreduce)
        for deg in DEGREES:
            ch = solve.DistributedChebyshev(op, minv, degree=deg)
            xc = zeros()
            d["cheb", deg] = dict(info=ch.info, native=solve.pcg_distributed(op, c, b, xc, minv=minv, native=True, precond=ch, **SOLVE),
                                  host=solve.pcg_distributed(op, c, b, zeros(), minv=minv, allreduce=allreduce,
                                                             precond=dict(degree=deg), **SOLVE),
                                  x=host(xc), given=solve.DistributedChebyshev(op, minv, degree=deg, lambda_max=ch.info.lambda_max).info)

    run_ranks(q.world, body, red)
    _MF["dist"] = out
    return out


def test_jacobi_matrix_free():
    q, out, w = case("cube"), mf_run(), mf_whole()
    ranks = range(q.world)
    native, hostloop = [out[r]["native"] for r in ranks], [out[r]["host"] for r in ranks]
    assert all(s.converged for s in native + hostloop) and w["res"].converged and same_on_all_ranks(native)
    x = q.gather([out[r]["x"] for r in ranks])[0]
    diff = np.linalg.norm(x - w["x"]) / np.linalg.norm(w["x"])
    print(f"matrix-free cube: {native[0].num_iters} iterations in the library, {hostloop[0].num_iters} in the host loop, "
          f"{w['res'].num_iters} on one rank; |x - x_1| / |x_1| = {diff:.2e}")
    assert abs(native[0].num_iters - hostloop[0].num_iters) <= 1
    assert diff <= 1e-8


@pytest.mark.parametrize("deg", DEGREES)
def test_chebyshev_matrix_free(deg):
    check_chebyshev(case("cube"), mf_run(), mf_whole()["x"], deg, "cube matrix-free")


def test_matrix_free_with_a_rank_that_owns_nothing():
    """The unstructured mesh of tests/test_gpu_dist_cabi.py cut in two parts of a world of three: rank 1 owns no element and no node,
    brings empty vectors, takes part in every reduction and returns the result of the others.  The diagonal and the right-hand side
    are functions of the global node, dealt out from the one-rank system.  The host loop cannot be the yardstick of the iteration
    count here -- its l3k_cg_* pieces refuse the null vectors of the empty rank -- so the solution is held against the one-rank solve
    and the counts are printed; that every rank, the empty one included, reports the same count is asserted."""
    from test_partition_unstructured import part_vector, small_mesh
    U, p, world = 4, 2, 3
    en, ev, nn = small_mesh(p, n_keep=120)
    pv = part_vector(ev, 2) * 2

    def flags(m):
        ids = m.node_grid_id[:m.n_local_nodes].astype(np.int64)
        mask = np.zeros((len(ids), U), np.uint8)
        mask[ids % 11 == 0, 0] = 1
        return ids, mask.reshape(-1)

    torch.cuda.set_device(0)
    c = rank_context()
    whole = partition.PartitionedMesh(en, ev, nn, np.zeros_like(pv), 0, 1, p)
    ids_w, mask_w = flags(whole)
    mf_w = system.MatrixFreeSystem(system.DeviceMesh(c, whole, U, mask_w), D3, [1.0, 0.0])
    diag_w, _ = mf_w.diag_rhs()
    minv_w = solve.jacobi_inverse_native(c, diag_w)
    b_w = dev(np.sin(0.37 * ids_w[:, None] + np.arange(U)[None, :]).reshape(-1))
    x_w = torch.zeros_like(b_w)
    res_w = solve.pcg(mf_w, b_w, x_w, minv_w, **SOLVE)
    torch.cuda.synchronize()
    row = np.full(int(ids_w.max()) + 1, -1, dtype=np.int64)
    row[ids_w] = np.arange(len(ids_w))
    minv_h, b_h, x_h = (host(t).reshape(-1, U) for t in (minv_w, b_w, x_w))
    group, out = InprocGroup(world), {}

    def body(rank):
        part = partition.PartitionedMesh(en, ev, nn, pv, rank, world, p)
        ids, mask = flags(part)
        cr = rank_context()
        mf = system.MatrixFreeSystem(system.DeviceMesh(cr, part, U, mask), D3, [1.0, 0.0])
        op = NativeDistributedOperator(mf, NativeHalo(cr, part, U, rank, world, transport=group))
        owned = row[ids[:part.n_owned_nodes]]
        b, minv = dev(b_h[owned].reshape(-1)), dev(minv_h[owned].reshape(-1))
        x = torch.zeros_like(b)
        res = solve.pcg_distributed(op, cr, b, x, minv=minv, native=True, **SOLVE)
        xc = torch.zeros_like(b)
        res_c = solve.pcg_distributed(op, cr, b, xc, minv=minv, native=True, precond=dict(degree=2), **SOLVE)
        out[rank] = (owned, host(x).reshape(-1, U), res, host(xc).reshape(-1, U), res_c)

    run_ranks(world, body)
    assert out[1][0].size == 0 and sum(out[r][0].size for r in range(world)) == len(ids_w)
    assert same_on_all_ranks([out[r][2] for r in range(world)]) and same_on_all_ranks([out[r][4] for r in range(world)])
    assert out[1][2].converged and out[1][4].converged and res_w.converged
    for k, name in ((1, "Jacobi"), (3, "Chebyshev degree 2")):
        got = np.zeros_like(x_h)
        for r in (0, 2):
            got[out[r][0]] = out[r][k]
        diff = np.linalg.norm(got - x_h) / np.linalg.norm(x_h)
        print(f"a rank that owns nothing, {name}: {out[1][k + 1].num_iters} iterations on three ranks, {res_w.num_iters} (Jacobi) on one; "
              f"|x - x_1| / |x_1| = {diff:.2e}")
        assert diff <= 1e-8
    assert out[1][4].num_iters < out[1][2].num_iters


# ------------------------------------------------------------------------------------------------------- 6. world of one
@pytest.mark.parametrize("kind", KINDS)
def test_world_of_one_is_the_single_rank_solve(kind):
    q, w = case(kind), whole_run(kind)
    torch.cuda.set_device(0)
    c = rank_context()
    row_ptr, col_ind, values = (dev(w["closed"][0], torch.int64), dev(w["closed"][1], torch.int32), dev(w["closed"][2]))
    local = system.CsrOperator(c, row_ptr, col_ind, values)
    op = system.DistributedCsrOperator(local, NativeHalo(c, q.whole, q.U, 0, 1, transport=InprocGroup(1)))
    b, minv = dev(w["rhs"][0]), local.jacobi_inverse()
    x1, x2 = torch.zeros_like(b), torch.zeros_like(b)
    one = solve.pcg(local, b, x1, minv, **SOLVE)
    dist = solve.pcg_distributed(op, c, b, x2, minv=minv, native=True, **SOLVE)
    assert one.converged and dist.converged and dist.num_iters == one.num_iters
    assert rel(host(x2), host(x1)) <= 1e-12
    for deg in DEGREES:
        y1, y2 = torch.zeros_like(b), torch.zeros_like(b)
        ch1, ch2 = solve.ChebyshevPreconditioner(local, minv, degree=deg), solve.DistributedChebyshev(op, minv, degree=deg)
        assert abs(ch1.info.lambda_est - ch2.info.lambda_est) <= 1e-12 * ch1.info.lambda_est
        one = solve.pcg(local, b, y1, precond=ch1, **SOLVE)
        dist = solve.pcg_distributed(op, c, b, y2, minv=minv, native=True, precond=ch2, **SOLVE)
        assert one.converged and dist.converged and dist.num_iters == one.num_iters
        print(f"{kind} degree {deg}: {dist.num_iters} iterations, |x - x_1| / |x_1| = {rel(host(y2), host(y1)):.2e}")
        assert rel(host(y2), host(y1)) <= 1e-12


# ----------------------------------------------------------------------------------------------------------------- 7. edges
def test_edges_are_identical_on_every_rank():
    q, out = case("cube"), csr_run("cube")
    ranks = range(q.world)
    edges = [out[r]["edges"] for r in ranks]
    for name in ("three", "every5", "every5_capped", "to_the_end"):
        assert same_on_all_ranks([e[name] for e in edges]), name
    assert same_on_all_ranks([e["zero"][0] for e in edges])
    zero = edges[0]["zero"][0]
    assert zero.num_iters == 0 and zero.converged and all(not e["zero"][1].any() for e in edges)
    three = edges[0]["three"]
    assert three.num_iters == 3 and not three.converged  # (and the call returned 0: nothing was raised)
    every5, reference = edges[0]["every5"], out[0]["native"]
    assert every5.converged and every5.num_iters % 5 == 0 and reference.num_iters <= every5.num_iters < reference.num_iters + 5
    assert edges[0]["every5_capped"].num_iters == 13 and not edges[0]["every5_capped"].converged
    assert edges[0]["to_the_end"].num_iters == 500 and not edges[0]["to_the_end"].converged
    assert all(bits(edges[r]["again"]) == bits(out[r]["x"]) for r in ranks)


# -------------------------------------------------------------------------------------------------------------- 8. refusals
def test_refusals():
    lib = capi.load()
    torch.cuda.set_device(0)
    c = rank_context()
    q, w = case("cube"), whole_run("cube")
    row_ptr, col_ind, values = (dev(w["closed"][0], torch.int64), dev(w["closed"][1], torch.int32), dev(w["closed"][2]))
    local = system.CsrOperator(c, row_ptr, col_ind, values)
    one = lambda: NativeHalo(c, q.whole, q.U, 0, 1, transport=InprocGroup(1))
    op, other = system.DistributedCsrOperator(local, one()), system.DistributedCsrOperator(local, one())
    b, minv = dev(w["rhs"][0]), local.jacobi_inverse()
    x = torch.full_like(b, 0.5)
    # a preconditioner of another operator
    ch = solve.DistributedChebyshev(other, minv, degree=2)
    with pytest.raises(capi.L3KError, match="l3k_csr_dist_pcg_solve.*another system"):
        solve.pcg_distributed(op, c, b, x, minv=minv, native=True, precond=ch, **SOLVE)
    # ... a minv that is not the preconditioner's, null arguments, the option errors of l3k_cheb_create
    res, out = capi.CgResult(), C.c_void_p(0xdead)
    vp = lambda t: C.c_void_p(t.data_ptr())
    assert lib.l3k_csr_dist_pcg_solve(other._h, vp(b), vp(x), vp(b), ch._h, None, C.byref(res)) == -1
    assert "d_minv" in lib.l3k_last_error().decode()
    assert lib.l3k_csr_dist_pcg_solve(op._h, None, vp(x), vp(minv), None, None, C.byref(res)) == -1
    assert lib.l3k_csr_dist_pcg_solve(op._h, vp(b), vp(x), vp(minv), None, None, None) == -1
    assert lib.l3k_csr_dist_cheb_create(op._h, None, None, C.byref(out)) == -1
    bad = capi.ChebOpts(0, 30.0, 10, 1.1, 0.0)
    assert lib.l3k_csr_dist_cheb_create(op._h, vp(minv), C.byref(bad), C.byref(out)) == -1
    assert "l3k_csr_dist_cheb_create" in lib.l3k_last_error().decode() and out.value == 0xdead
    assert np.array_equal(host(x), np.full(b.numel(), 0.5))
    # a halo that does not fit the mesh, a halo of another context
    part = q.parts[1]
    assert part.n_ghost_nodes > 0 and q.parts[0].n_ghost_nodes != part.n_ghost_nodes
    group = InprocGroup(q.world)
    mf = system.MatrixFreeSystem(system.DeviceMesh(c, part, q.U, q.local_mask(1).astype(np.uint8)), D3, q.kpar)
    n = part.n_owned_nodes * q.U
    bo, xo = torch.ones(n, dtype=torch.float64, device="cuda"), torch.zeros(n, dtype=torch.float64, device="cuda")
    wrong = NativeDistributedOperator(mf, NativeHalo(c, q.parts[0], q.U, 0, q.world, transport=group))
    with pytest.raises(capi.L3KError, match="l3k_pcg_solve_dist.*does not match"):
        solve.pcg_distributed(wrong, c, bo, xo, native=True, **SOLVE)
    with pytest.raises(capi.L3KError, match="l3k_cheb_create_dist.*does not match"):
        solve.DistributedChebyshev(wrong, bo, degree=2)
    elsewhere = NativeDistributedOperator(mf, NativeHalo(rank_context(), part, q.U, 1, q.world, transport=group))
    with pytest.raises(capi.L3KError, match="l3k_pcg_solve_dist.*different contexts"):
        solve.pcg_distributed(elsewhere, c, bo, xo, native=True, **SOLVE)
    assert not xo.any()
    # the Python layer: a reduction of the caller's, the p-multigrid
    with pytest.raises(capi.L3KError, match="native=True.*allreduce must be None"):
        solve.pcg_distributed(op, c, b, x, minv=minv, native=True, allreduce=lambda view: None, **SOLVE)
    with pytest.raises(capi.L3KError, match="host loop"):
        solve.pcg_distributed(op, c, b, x, minv=minv, native=True, precond=object.__new__(solve.DistributedPMultigrid), **SOLVE)
