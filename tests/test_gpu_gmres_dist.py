"""The collective GMRES of a partitioned system (l3k_gmres_create_dist, l3k_csr_dist_gmres_solve, l3k_gmres_solve_dist;
solve.gmres_distributed) with the ranks as threads of this process over the library's in-process transport, as in
tests/test_gpu_pcg_dist.py.  A rank body only computes and stores; every assertion runs afterwards in the main thread.

Bars.  A world of one: the bits of the single-rank solve, in x and in every field of the result.  The non-symmetric chain of
tests/gmres_dist_ref.py over three ranks: converged, the result equal on all ranks on the bits, |x - x*|_inf <= 1e-7 (the bar of
tests/test_gpu_gmres.py::test_nonsymmetric_tridiagonal), the estimate after a step within 1e-10 relative of the restatement's (the
bound stated at the head of that file), the iteration count within 1 of the restatement's where its stopping margins allow
(tests/test_gmres_dist_ref_cpu.py::test_stopping_margins_of_the_chain states which they are).  The partitioned cube and square of
tests/test_gpu_asm_dist.py: 1e-8 |x| against the single-rank solve on the whole mesh at the solver tolerance 1e-10."""
import ctypes as C

import numpy as np
import pytest
import torch

import csr_dist_ref as D
import gmres_dist_ref as GD
import gmres_ref as G
from gmres_ref import LD
from l3ster_amd import capi, solve, system
from l3ster_amd.distributed import InprocGroup, NativeDistributedOperator, NativeHalo
from test_gpu_asm_dist import assemble, case, dev, host, rank_context, run_ranks, terms, whole_run
from test_gpu_pcg_dist import bits

pytestmark = pytest.mark.gpu
D3 = system.KERNEL_DIFFUSION3D
N, C09 = 3000, 0.9
SPLITS = {"three": [1000, 1100, 900], "empty": [1500, 0, 1500]}
SOLVE = dict(tol=1e-10, residual_scaling="rhs")
FIELDS = ("tol", "num_iters", "converged", "restarts", "breakdown", "estimate", "orth_loss")
RESTART = 200  # of the solves on the meshes (GMRES(50) stagnates on the matrix-free square: 39 restarts do not reach 1e-10)
_CHAIN, _REF, _MESH = {}, {}, {}


def fields(r):
    return bits([float(getattr(r, f)) for f in FIELDS])


def whole_halo(c, part=None, U=1):
    return NativeHalo(c, D.ExchangeLists([], [], []) if part is None else part, U, 0, 1, transport=InprocGroup(1))


# ------------------------------------------------------------------------------------------------------- 1. a world of one
# restart lengths 5, 30 and 300: the register, the tile and the chunked pass route (the last one needs more than 255 basis vectors
# in one cycle, so that solve runs 270 steps towards tol = 0)
ROUTES = [(5, dict(SOLVE)), (30, dict(SOLVE)), (300, dict(tol=0.0, residual_scaling="rhs", max_iters=270))]


@pytest.mark.parametrize("precond", ["none", "jacobi", "cheb2"])
@pytest.mark.parametrize("m,kw", ROUTES, ids=["m5", "m30", "m300"])
def test_world_of_one_csr_is_the_single_rank_solve(m, kw, precond):
    from test_gpu_gmres import tri
    torch.cuda.set_device(0)
    T = tri("c09", 1000)
    c = T.op.ctx
    op = system.DistributedCsrOperator(T.op, whole_halo(c))
    b, minv = dev(T(np.cos(0.1 * np.arange(T.n)))), dev(1.0 / T.di)
    ws = solve.GmresWorkspace(c, T.n, m)
    one_kw = dict(minv=minv) if precond == "jacobi" else {} if precond == "none" else dict(precond=solve.ChebyshevPreconditioner(T.op, minv, degree=2))
    dist_kw = dict(minv=minv) if precond == "jacobi" else {} if precond == "none" else dict(precond=solve.DistributedChebyshev(op, minv, degree=2))
    x1, x2 = torch.zeros_like(b), torch.zeros_like(b)
    one = solve.gmres(T.op, b, x1, workspace=ws, throw_on_fail=False, **one_kw, **kw)
    dist = solve.gmres_distributed(op, c, b, x2, workspace=ws, throw_on_fail=False, **dist_kw, **kw)
    print(f"m={m} {precond}: {one!r}")
    assert one.converged if m != 300 else (one.num_iters == 270 or one.breakdown)  # (270 > 255: the chunked route has run)
    assert fields(dist) == fields(one) and torch.equal(x1, x2) and x1.any()


@pytest.mark.parametrize("precond", ["none", "jacobi", "cheb2"])
@pytest.mark.parametrize("m,kw", ROUTES, ids=["m5", "m30", "m300"])
def test_world_of_one_matrix_free_is_the_single_rank_solve(m, kw, precond):
    """on a context in deterministic mode: only there do two matrix-free applies give the same bits, l3k_mf_apply and
    l3k_mf_apply_dist included (the element launches add into y with atomics otherwise)"""
    q = case("cube")
    torch.cuda.set_device(0)
    if "mf1" not in _MESH:
        c = rank_context()
        c.set_deterministic(True)
        mf = system.MatrixFreeSystem(system.DeviceMesh(c, q.whole, q.U, q.mask.astype(np.uint8)), D3, q.kpar)
        diag, rhs = mf.diag_rhs(dev(q.g))
        _MESH["mf1"] = (c, mf, solve.jacobi_inverse_native(c, diag), rhs[0].contiguous())
    c, mf, minv, b = _MESH["mf1"]
    op = NativeDistributedOperator(mf, whole_halo(c, q.whole, q.U))
    ws = solve.GmresWorkspace(c, b.numel(), m)
    if precond == "none":  # (without the mask the Dirichlet rows are solved like the others: A is the identity there)
        one_kw = dist_kw = {}
    elif precond == "jacobi":
        one_kw = dist_kw = dict(minv=minv)
    else:
        one_kw, dist_kw = dict(precond=solve.ChebyshevPreconditioner(mf, minv, degree=2)), dict(precond=solve.DistributedChebyshev(op, minv, degree=2))
    x1, x2 = torch.zeros_like(b), torch.zeros_like(b)
    one = solve.gmres(mf, b, x1, workspace=ws, throw_on_fail=False, **one_kw, **kw)
    dist = solve.gmres_distributed(op, c, b, x2, workspace=ws, throw_on_fail=False, **dist_kw, **kw)
    print(f"m={m} {precond}: {one!r}")
    assert fields(dist) == fields(one) and torch.equal(x1, x2) and x1.any()


# ------------------------------------------------------------------------------------------------- 2. the non-symmetric chain
def history_steps(m, its):
    """the steps of the first cycle: the estimate after every one of them is read back, by one solve with max_iters = k each"""
    return list(range(1, min(m, its) + 1))


def reference(split, m, frozen=False):
    key = (split, m, frozen)
    if key not in _REF:
        k = GD.chain(N, C09, SPLITS[split])
        A = GD.tri_apply(k.lo, k.di, k.up)
        xs = np.cos(0.1 * np.arange(N))
        live, x0, minv = GD.frozen_rows(k) if frozen else (np.ones(N, dtype=bool), np.zeros(N), 1.0 / k.di)
        ref = GD.gmres(A, k.offsets, A(xs), x0, m, prec=lambda v: v * minv.astype(v.dtype), live=live, tol=1e-10, residual_scaling=2, dtype=LD)
        _REF[key] = types_ns(case=k, A=A, xs=xs, b=A(xs), x0=x0, live=live, minv=minv, ref=ref)
    return _REF[key]


def types_ns(**kw):
    import types
    return types.SimpleNamespace(**kw)


def chain_run(split, m, frozen=False):
    """every rank's script on the chain, once per (split, m): what each rank left, by rank"""
    key = (split, m, frozen)
    if key in _CHAIN:
        return _CHAIN[key]
    R = reference(split, m, frozen)
    k, world = R.case, R.case.world
    steps = [] if frozen else history_steps(m, R.ref["iterations"])
    applies = R.ref["iterations"] + R.ref["restarts"] + 2
    group, out = InprocGroup(world), {}

    def body(rank):
        d = out[rank] = {}
        c, kr = rank_context(), k.ranks[rank]
        sl = slice(int(k.offsets[rank]), int(k.offsets[rank + 1]))
        values = kr.values.copy()
        if frozen and rank == 1:
            dead = np.flatnonzero(~R.live[sl])
            for i in dead:
                values[kr.row_ptr[i]:kr.row_ptr[i + 1]] = np.nan
        local = system.CsrOperator(c, dev(kr.row_ptr, torch.int64), dev(kr.col_ind, torch.int32), dev(values))
        op = system.DistributedCsrOperator(local, NativeHalo(c, kr.part, 1, rank, world, transport=group))
        b, minv, x0 = dev(R.b[sl]), dev(R.minv[sl]), dev(R.x0[sl])
        ws = solve.GmresWorkspace(c, kr.n_owned, m, collective=True)
        go = lambda x, **kw: solve.gmres_distributed(op, c, b, x, minv=minv, workspace=ws, throw_on_fail=False, **{**SOLVE, **kw})
        x = x0.clone()
        d["res"] = go(x)
        d["x"] = host(x)
        again = x0.clone()
        d["again"] = (go(again), host(again))
        fresh = x0.clone()  # (a workspace made by the call)
        d["fresh"] = (solve.gmres_distributed(op, c, b, fresh, minv=minv, restart_length=m, throw_on_fail=False, **SOLVE), host(fresh))
        d["history"] = [go(x0.clone(), max_iters=s).estimate for s in steps]
        if not frozen and m == 30:
            xp = torch.zeros_like(b)
            d["pcg"] = solve.pcg_distributed(op, c, b, xp, minv=minv, native=True, throw_on_fail=False, max_iters=applies, **SOLVE)
            d["every5"] = go(x0.clone(), check_every=5)

    run_ranks(world, body)
    _CHAIN[key] = out
    return out


@pytest.mark.parametrize("split", list(SPLITS))
@pytest.mark.parametrize("m", [5, 30, 300])
def test_chain_over_three_ranks(split, m):
    R, out = reference(split, m), chain_run(split, m)
    ref, ranks = R.ref, range(R.case.world)
    res = [out[r]["res"] for r in ranks]
    print(f"{split} m={m}: device {res[0]!r}; restatement {ref['iterations']} / {ref['restarts']} / {ref['achieved_tol']:.3e}")
    assert all(s.converged and not s.breakdown for s in res)
    assert len({tuple(fields(s)) for s in res}) == 1  # iterations, restarts and the bits of achieved_tol, estimate, orth_loss
    x = np.concatenate([out[r]["x"] for r in ranks])
    assert x.size == N and np.abs(x - R.xs).max() <= 1e-7
    assert res[0].orth_loss <= 1e-10
    # the estimates of the first cycle
    steps = history_steps(m, ref["iterations"])
    want = np.array([ref["history"][s - 1] for s in steps])
    for r in ranks:
        got = np.array(out[r]["history"])
        assert bits(got) == bits(out[0]["history"])
        worst = np.max(np.abs(got - want) / want)
        assert worst <= 1e-10, (r, worst)
    print(f"   estimates at steps {steps[0]} .. {steps[-1]}: largest relative distance from the restatement {worst:.2e}")
    # the iteration count: within 1 where both margins are >= 1.5, and -- the chain has none such -- where they are >= 1.02, two
    # hundred million times the distance of the estimates
    below, above = G.stopping_margin(ref["history"], 1e-10)
    print(f"   margins {below:.4f} {above:.4f}")
    assert min(below, above) >= 1.02  # (tests/test_gmres_dist_ref_cpu.py::test_stopping_margins_of_the_chain)
    assert abs(res[0].num_iters - ref["iterations"]) <= 1
    assert (m == 300) == (res[0].restarts == 0)


@pytest.mark.parametrize("split", list(SPLITS))
@pytest.mark.parametrize("m", [5, 30, 300])
def test_two_solves_give_equal_bits(split, m):
    out = chain_run(split, m)
    for r in out:
        first = (fields(out[r]["res"]), bits(out[r]["x"]))
        for name in ("again", "fresh"):
            res, x = out[r][name]
            assert (fields(res), bits(x)) == first, (r, name)


def test_pcg_is_not_the_answer_and_check_every():
    """the collective PCG, given the operator applies the GMRES(30) solve took, is nowhere near the tolerance on this matrix
    (tests/test_gmres_dist_ref_cpu.py states the same of the restatement); check_every = 5 stops at most 4 steps later"""
    out = chain_run("three", 30)
    for r in out:
        p, g, e = out[r]["pcg"], out[r]["res"], out[r]["every5"]
        assert g.converged and not p.converged and not p.tol <= 1e-3, (r, p)
        assert e.converged and g.num_iters <= e.num_iters <= g.num_iters + 4
    assert len({tuple(fields(out[r]["every5"])) for r in out}) == 1
    print(f"PCG after {out[0]['pcg'].num_iters} iterations: {out[0]['pcg'].tol:.3e}; GMRES(30): {out[0]['res']!r}")


def test_frozen_rows_keep_x_and_the_rest_solves():
    """on rank 1 every 101st minv entry is 0 and the matrix holds NaN in those rows; x0 is random: x keeps its bits there"""
    R, out = reference("three", 30, frozen=True), chain_run("three", 30, frozen=True)
    ranks = range(R.case.world)
    res = [out[r]["res"] for r in ranks]
    x = np.concatenate([out[r]["x"] for r in ranks])
    dead = ~R.live
    print(f"frozen rows: {int(dead.sum())} on rank 1; device {res[0]!r}; restatement {R.ref['iterations']} / {R.ref['restarts']}")
    assert dead.sum() == 11 and R.ref["converged"]
    assert all(s.converged for s in res) and len({tuple(fields(s)) for s in res}) == 1
    assert np.isfinite(x).all() and bits(x[dead]) == bits(R.x0[dead])
    assert np.abs(x - R.ref["x"].astype(np.float64))[R.live].max() <= 1e-8
    # (margins 1.25 and 1.012 in the restatement, asserted >= 1.01 in tests/test_gmres_dist_ref_cpu.py: a hundred million times the
    # 1e-10 by which the device's estimates may differ from the restatement's)
    assert min(G.stopping_margin(R.ref["history"], 1e-10)) >= 1.01
    assert abs(res[0].num_iters - R.ref["iterations"]) <= 1


# --------------------------------------------------------------------------- 3. the partitioned cube (2 ranks) and square (4)
def matrix_free(q, mesh, sides):
    """the matrix-free system of test_gpu_asm_dist.terms: the domain kernel, on the square with its boundary term attached (GMRES
    does not reach 1e-10 on the square's domain kernel alone, on one rank or on four, with 8 000 steps of GMRES(200))"""
    mf, bnd = terms(q, mesh, sides)
    if q.dim == 2 and bnd is not None:
        mf.attach_boundary(bnd)
    return mf


def mesh_whole(kind):
    """the single-rank twins: solve.gmres on the closed matrix of the whole mesh, and on its matrix-free system (matrix_free)"""
    if ("whole", kind) not in _MESH:
        q, w = case(kind), whole_run(kind)
        torch.cuda.set_device(0)
        c = rank_context()
        local = system.CsrOperator(c, dev(w["closed"][0], torch.int64), dev(w["closed"][1], torch.int32), dev(w["closed"][2]))
        b, minv = dev(w["rhs"][0]), local.jacobi_inverse()
        mf = matrix_free(q, system.DeviceMesh(c, q.whole, q.U, q.mask.astype(np.uint8)), q.sides)
        diag, rhs = mf.diag_rhs(dev(q.g))
        systems = [("csr", local, b, minv), ("mf", mf, rhs[0].contiguous(), solve.jacobi_inverse_native(c, diag))]
        d = {}
        for name, o, b, minv in systems:  # the same preconditioners as on the ranks
            for pname, kw in (("jacobi", dict(minv=minv)), ("cheb2", dict(precond=solve.ChebyshevPreconditioner(o, minv, degree=2)))):
                x = torch.zeros_like(b)
                d[name, pname] = (solve.gmres(o, b, x, restart_length=RESTART, **kw, **SOLVE), host(x))
        torch.cuda.synchronize()
        _MESH["whole", kind] = d
    return _MESH["whole", kind]


def mesh_run(kind):
    if ("dist", kind) in _MESH:
        return _MESH["dist", kind]
    q = case(kind)
    group, group_mf, out = InprocGroup(q.world), InprocGroup(q.world), {}

    def body(rank):
        d = out[rank] = {}
        c, part, no = rank_context(), q.parts[rank], q.n_owned(rank)
        mesh = system.DeviceMesh(c, part, q.U, q.local_mask(rank).astype(np.uint8))
        mf, bnd = terms(q, mesh, q.part_sides[rank])
        asm = system.AssembledSystem(mesh, condensation=None, halo=NativeHalo(c, part, q.U, rank, q.world, transport=group))
        assemble(asm, mf, bnd)
        op = asm.end(dev(q.scatter(q.g, rank)))
        mfo = NativeDistributedOperator(matrix_free(q, mesh, q.part_sides[rank]), NativeHalo(c, part, q.U, rank, q.world, transport=group_mf))
        diag, rhs = mfo.diag_rhs(dev(q.scatter(q.g, rank)))
        systems = [("csr", op, asm.rhs[0, :no].contiguous(), op.jacobi_inverse()),
                   ("mf", mfo, rhs[0].contiguous(), solve.jacobi_inverse_native(c, diag))]
        for name, o, b, minv in systems:
            for pname, kw in (("jacobi", {}), ("cheb2", dict(precond=dict(degree=2)))):
                x = torch.zeros_like(b)
                d[name, pname] = (solve.gmres_distributed(o, c, b, x, minv=minv, restart_length=RESTART, **kw, **SOLVE), host(x))

    run_ranks(q.world, body)
    _MESH["dist", kind] = out
    return out


@pytest.mark.parametrize("precond", ["jacobi", "cheb2"])
@pytest.mark.parametrize("kind,name", [("cube", "csr"), ("quad", "csr"), ("cube", "mf"), ("quad", "mf")])
def test_partitioned_meshes(kind, name, precond):
    q, out, w = case(kind), mesh_run(kind), mesh_whole(kind)
    ranks = range(q.world)
    res = [out[r][name, precond][0] for r in ranks]
    one, x_one = w[name, precond]
    x = q.gather([out[r][name, precond][1] for r in ranks])[0]
    diff = np.linalg.norm(x - x_one) / np.linalg.norm(x_one)
    print(f"{kind} {name} {precond}: {res[0]!r} on {q.world} ranks; on one rank {one!r}; |x - x_1| / |x_1| = {diff:.2e}")
    assert one.converged and all(s.converged for s in res)
    assert len({(s.num_iters, s.restarts, bits([s.tol])[0]) for s in res}) == 1
    assert diff <= 1e-8


# -------------------------------------------------------------------------------------------------------------- 4. refusals
def test_refusals():
    from test_gpu_gmres import tri
    lib, res = capi.load(), capi.GmresResult()
    torch.cuda.set_device(0)
    T = tri("c09", 1000)
    c, n = T.op.ctx, T.n
    op = system.DistributedCsrOperator(T.op, whole_halo(c))
    b, minv = dev(T(np.cos(0.1 * np.arange(n)))), dev(1.0 / T.di)
    x = torch.full((n + 8,), 0.5, dtype=torch.float64, device="cuda")
    vp = lambda t: C.c_void_p(t.data_ptr())

    def refused(rc, text):
        assert rc == -1 and text in lib.l3k_last_error().decode(), lib.l3k_last_error().decode()

    ws, small = solve.GmresWorkspace(c, n, 30, collective=True), solve.GmresWorkspace(c, n - 1, 30, collective=True)
    call = lib.l3k_csr_dist_gmres_solve
    refused(call(small._h, op._h, vp(b), vp(x), vp(minv), None, None, C.byref(res)),
            "l3k_csr_dist_gmres_solve: the workspace was created for n = 999, the operator has 1000 rows")
    refused(call(ws._h, op._h, vp(b), C.c_void_p(b.data_ptr() + 80), vp(minv), None, None, C.byref(res)), "l3k_csr_dist_gmres_solve: b and x overlap")
    refused(call(ws._h, op._h, None, vp(x), vp(minv), None, None, C.byref(res)), "l3k_csr_dist_gmres_solve: null vector")
    refused(call(None, op._h, vp(b), vp(x), vp(minv), None, None, C.byref(res)), "l3k_csr_dist_gmres_solve: null argument")
    refused(call(ws._h, op._h, vp(b), vp(x), vp(minv), None, None, None), "l3k_csr_dist_gmres_solve: null argument")
    # a single-rank l3k_cheb, one of another partitioned operator, a minv that is not the preconditioner's
    single = solve.ChebyshevPreconditioner(T.op, minv, degree=2)
    refused(call(ws._h, op._h, vp(b), vp(x), None, single._h, None, C.byref(res)), "l3k_csr_dist_gmres_solve: the preconditioner was created for another system")
    other = system.DistributedCsrOperator(T.op, whole_halo(c))
    ch = solve.DistributedChebyshev(other, minv, degree=2)
    refused(call(ws._h, op._h, vp(b), vp(x), None, ch._h, None, C.byref(res)), "l3k_csr_dist_gmres_solve: the preconditioner was created for another system")
    refused(call(ws._h, other._h, vp(b), vp(x), vp(b), ch._h, None, C.byref(res)), "d_minv is not the array")
    with pytest.raises(capi.L3KError, match="DistributedChebyshev or a dict"):
        solve.gmres_distributed(op, c, b, x[:n], precond=single)
    with pytest.raises(capi.L3KError, match="the workspace was created for n = 999"):
        solve.gmres_distributed(op, c, b, x[:n], minv=minv, workspace=small)
    other_ctx = solve.GmresWorkspace(rank_context(), n, 30, collective=True)
    with pytest.raises(capi.L3KError, match="l3k_csr_dist_gmres_solve: the workspace and the system belong to different contexts"):
        solve.gmres_distributed(op, c, b, x[:n], minv=minv, workspace=other_ctx)
    # the creator
    h = C.c_void_p()
    refused(lib.l3k_gmres_create_dist(c._h, -1, 30, 0, C.byref(h)), "l3k_gmres_create_dist: n = -1")
    refused(lib.l3k_gmres_create_dist(c._h, 0, 2047, 0, C.byref(h)), "l3k_gmres_create_dist: restart_length = 2047 above 2046")
    refused(lib.l3k_gmres_create_dist(c._h, n, 30, 0, None), "l3k_gmres_create_dist: null argument")
    empty = solve.GmresWorkspace(c, 0, 30, collective=True)
    assert (empty.info.n, empty.info.restart_length, ws.info.restart_length) == (0, 30, 30)
    assert solve.GmresWorkspace(c, 10, 30, collective=True).restart_length == 30  # (not lowered to the rank's rows)
    assert np.array_equal(host(x), np.full(n + 8, 0.5))
    # a matrix-free system: a halo of another context, a halo that does not fit the mesh; the single-rank entry points still refuse
    # ghost nodes
    q = case("cube")
    part, group = q.parts[1], InprocGroup(q.world)
    mf = system.MatrixFreeSystem(system.DeviceMesh(c, part, q.U, q.local_mask(1).astype(np.uint8)), D3, q.kpar)
    no = part.n_owned_nodes * q.U
    bo, xo = torch.ones(no, dtype=torch.float64, device="cuda"), torch.zeros(no, dtype=torch.float64, device="cuda")
    elsewhere = NativeDistributedOperator(mf, NativeHalo(rank_context(), part, q.U, 1, q.world, transport=group))
    with pytest.raises(capi.L3KError, match="l3k_gmres_solve_dist.*different contexts"):
        solve.gmres_distributed(elsewhere, c, bo, xo, restart_length=5, **SOLVE)
    wrong = NativeDistributedOperator(mf, NativeHalo(c, q.parts[0], q.U, 0, q.world, transport=group))
    with pytest.raises(capi.L3KError, match="l3k_gmres_solve_dist.*does not match"):
        solve.gmres_distributed(wrong, c, bo, xo, restart_length=5, **SOLVE)
    with pytest.raises(capi.L3KError, match="l3k_gmres_solve is the single-rank solver; this mesh has ghost nodes.*l3k_gmres_solve_dist"):
        solve.gmres(mf, bo, xo, restart_length=5)
    assert not xo.any()
