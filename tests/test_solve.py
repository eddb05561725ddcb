"""Jacobi-PCG driven by the matrix-free operator.  CPU: l3ster_amd.solve on top of the oracle's apply (pins solve.py and
the 3-D analogue of the reference's end-to-end diffusion test, tests/Diffusion2D.hpp:17-121: Dirichlet T = x, zero
source, exact solution T = x, q = (1,0,0), error < 1e-8).  GPU: the same through the HIP kernels."""
import numpy as np
import pytest
import torch

import oracle_lib as O
from helpers import oracle_mesh
from l3ster_amd import solve, system


def node_coords(part):
    gll = system.gll_nodes(part.order + 1)
    n = part.order + 1
    xyz = np.zeros((part.n_local_nodes, 3))
    for e in range(part.n_elems):
        for i in range(n ** 3):
            xyz[part.elem_nodes[e, i]] = O.map_to_physical(3, part.elem_verts[e], [gll[i % n], gll[(i // n) % n], gll[i // (n * n)]])
    return xyz


def setup_problem(ne, p):
    U = 4
    part = system.CubePartition(ne, p, perturb=0.1)
    mask = part.dirichlet_mask(U)
    xyz = node_coords(part)
    g = np.zeros((part.n_local_nodes, U))
    g[:, 0] = xyz[:, 0]  # T = x on the boundary (only the masked entries matter)
    g = (g.reshape(-1) * mask)[None, :]
    exact = np.zeros((part.n_local_nodes, U))
    exact[:, 0], exact[:, 1] = xyz[:, 0], 1.0
    return part, mask, g, exact.reshape(-1)


def test_pcg_with_oracle_operator_reproduces_linear_solution():
    p, kpar = 2, [1.0, 0.0]
    part, mask, g, exact = setup_problem(3, p)
    om = oracle_mesh(part, p + 1, 4, np.arange(4), mask)
    diag, rhs = O.mf_diag_rhs(om, 0, 1, np.asfortranarray(g.T), kparams=kpar)
    minv = solve.jacobi_inverse(torch.as_tensor(diag))

    def apply(v, out):
        out.copy_(torch.as_tensor(O.mf_apply(om, 0, v.numpy().reshape(-1, 1), kparams=kpar)[:, 0]))

    x = torch.zeros(len(diag), dtype=torch.float64)
    res = solve.cg(apply, torch.as_tensor(rhs[:, 0].copy()), x, minv, tol=1e-11, residual_scaling="rhs")
    assert res.converged and res.num_iters < 400
    assert np.abs(x.numpy() - exact).max() < 1e-8
    # Jacobi: sign(d)*damping/max(|d|, threshold), solve/NativePreconditioners.hpp:75-96
    d = torch.tensor([2.0, -4.0, 1e-9])
    assert torch.allclose(solve.jacobi_inverse(d, 0.5, 1e-3), torch.tensor([0.25, -0.125, 500.0]))


@pytest.mark.gpu
@pytest.mark.parametrize("kid,ne,p", [(system.KERNEL_DIFFUSION3D, 3, 2), (system.KERNEL_DIFFUSION3D, 2, 4),
                                      (system.KERNEL_ADVDIFF3D, 3, 2)])
def test_gpu_pcg_matches_cpu_restatement(kid, ne, p):
    """Config-5 style solve: iterations to tolerance equal (+-1) to the CPU restatement, same solution; for the pure
    diffusion kernel the exact linear solution is reproduced (< 1e-8)."""
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    ctx = system.Context(0, torch.cuda.current_stream().cuda_stream)
    info = system.kernel_info(kid)
    U, F = info["n_unknowns"], info["n_fields"]
    part, mask, g, exact = setup_problem(ne, p)
    kpar = [1.0, 0.0] if kid == system.KERNEL_DIFFUSION3D else [1.0, 0.3, 0.0]
    fields = None
    if F:  # smooth analytic velocity
        xyz = node_coords(part)
        fields = np.stack([0.2 * np.sin(np.pi * xyz[:, 1]), 0.1 * np.cos(np.pi * xyz[:, 0]), 0.05 * xyz[:, 2]])
    mesh = system.DeviceMesh(ctx, part, U, mask)
    mf = system.MatrixFreeSystem(mesh, kid, kpar)
    if F:
        mf.set_fields(torch.as_tensor(fields, device="cuda"))
    G = torch.as_tensor(g, device="cuda")
    diag, rhs = mf.diag_rhs(G)
    minv = solve.jacobi_inverse(diag)
    x = torch.zeros_like(diag)
    res = solve.cg(lambda v, out: mf.apply(v[None, :], out[None, :]), rhs[0], x, minv, tol=1e-10, residual_scaling="rhs")
    # CPU restatement of the same solve
    om = oracle_mesh(part, p + 1, U, np.arange(U), mask, fields)
    d_ref, r_ref = O.mf_diag_rhs(om, kid, 1, np.asfortranarray(g.T), kparams=kpar)

    def apply_cpu(v, out):
        out.copy_(torch.as_tensor(O.mf_apply(om, kid, v.numpy().reshape(-1, 1), kparams=kpar)[:, 0]))

    x_ref = torch.zeros(len(d_ref), dtype=torch.float64)
    res_ref = solve.cg(apply_cpu, torch.as_tensor(r_ref[:, 0].copy()), x_ref, solve.jacobi_inverse(torch.as_tensor(d_ref)),
                       tol=1e-10, residual_scaling="rhs")
    assert abs(res.num_iters - res_ref.num_iters) <= 1
    assert np.linalg.norm(x.cpu().numpy() - x_ref.numpy()) < 1e-7 * np.linalg.norm(x_ref.numpy())
    if kid == system.KERNEL_DIFFUSION3D:
        assert np.abs(x.cpu().numpy() - exact).max() < 1e-7


@pytest.mark.gpu
def test_native_pcg_matches_torch_pcg():
    """l3k_pcg_solve (fused HIP vector kernels + the matrix-free apply, all behind the C ABI) and the torch-op PCG give
    the same iterates: same iteration count (+-1) and the same solution on a Dirichlet problem with a source term."""
    import torch
    from l3ster_amd import solve, system
    torch.cuda.set_device(0)
    ctx = system.Context(0, torch.cuda.current_stream().cuda_stream)
    p, U = 4, 4
    part = system.CubePartition(5, p, perturb=0.1)
    mesh = system.DeviceMesh(ctx, part, U, part.dirichlet_mask(U))
    mf = system.MatrixFreeSystem(mesh, system.KERNEL_DIFFUSION3D, [1.0, 1.0])
    diag, rhs = mf.diag_rhs(None)
    minv = solve.jacobi_inverse_native(ctx, diag)
    assert torch.equal(minv, solve.jacobi_inverse(diag))
    x1 = torch.zeros_like(diag)
    r1 = solve.cg(lambda v, out: mf.apply(v[None, :], out[None, :]), rhs[0], x1, minv, tol=1e-10, residual_scaling="rhs")
    x2 = torch.zeros_like(diag)
    r2 = solve.pcg(mf, rhs[0], x2, minv, tol=1e-10, residual_scaling="rhs")
    assert r2.converged and abs(r1.num_iters - r2.num_iters) <= 1
    assert (x1 - x2).norm().item() < 1e-8 * x1.norm().item()
    # the partitioned form of the iteration with a trivial (single-rank) operator
    class Op:
        def apply(self, X, Y):
            mf.apply(X, Y)
    x3 = torch.zeros_like(diag)
    r3 = solve.pcg_distributed(Op(), ctx, rhs[0], x3, minv, tol=1e-10, residual_scaling="rhs")
    assert abs(r3.num_iters - r2.num_iters) <= 1 and (x3 - x2).norm().item() < 1e-8 * x2.norm().item()


@pytest.mark.gpu
def test_k1_three_right_hand_sides_through_the_device_solver():
    """K1 at mesh level (tests/LocalAssemblyTests.cpp:3-43: R = D right-hand sides, Dirichlet on unknown 0 at the boundary nodes with
    phi = x_d, the diffusion kernel with zero source -> column d of the solution is T = x_d, q = e_d): value_order 2, three columns
    through l3k_mf_diag_rhs and l3k_pcg_solve_cols (the reference hands its n_rhs-column multivector to Belos Block CG)."""
    import torch
    from l3ster_amd import solve, system
    torch.cuda.set_device(0)
    ctx = system.Context(0, torch.cuda.current_stream().cuda_stream)
    p, U, R = 3, 4, 3
    part = system.CubePartition(3, p, perturb=0.15)
    mask = part.dirichlet_mask(U)
    mf = system.MatrixFreeSystem(system.DeviceMesh(ctx, part, U, mask), system.KERNEL_DIFFUSION3D, [1.0, 0.0], asm_opts=(2, 0, 0), n_rhs=R)
    xyz = part.node_coords()
    g = np.zeros((R, part.n_local_nodes, U))
    for d in range(R):
        g[d, :, 0] = xyz[:, d]
    g = g.reshape(R, -1) * mask[None, :]
    diag, rhs = mf.diag_rhs(torch.as_tensor(g, device="cuda"))
    minv = solve.jacobi_inverse_native(ctx, diag)
    x = torch.zeros_like(rhs)
    results = solve.pcg(mf, rhs, x, minv, tol=1e-12, residual_scaling="rhs")
    assert len(results) == R and all(r.converged for r in results)
    sol = x.cpu().numpy().reshape(R, -1, U)
    for d in range(R):
        want = np.zeros((part.n_local_nodes, U))
        want[:, 0] = xyz[:, d]
        want[:, 1 + d] = 1.0
        assert np.abs(sol[d] - want).max() < 1e-6, d  # the reference's bar (rel 1e-6)
        assert np.abs(sol[d] - want).max() < 1e-8, d
    # one column through the single-column entry point gives the same bits as that column of the multivector solve
    x0 = torch.zeros_like(rhs[0])
    solve.pcg(mf, rhs[0].contiguous(), x0, minv, tol=1e-12, residual_scaling="rhs")
    assert (x0 - x[0]).abs().max().item() < 1e-10


@pytest.mark.gpu
def test_pcg_on_a_subset_of_the_node_dofs():
    """A system whose kernel acts on 4 of 6 dofs per node (field_inds): the device PCG runs its applies on the strided-dof variant of
    the one-wave kernel (which does not fuse <p, A p>: the dot product runs as a pass of its own), the dofs of other kernels are
    frozen rows (zero preconditioner entries) -- and the solution on the kernel's dofs is the one of the same problem on a dense
    dof map."""
    import numpy as np
    import torch
    from l3ster_amd import solve, system
    torch.cuda.set_device(0)
    ctx = system.Context(0, torch.cuda.current_stream().cuda_stream)
    ctx.set_tuning(generic_below=0)
    p, U, dpn, fi = 4, 4, 6, [4, 0, 5, 2]
    part = system.CubePartition(4, p, perturb=0.1)
    mask_u = part.dirichlet_mask(U, unknowns=[0]).reshape(-1, U)
    g_u = np.zeros((part.n_local_nodes, U))
    g_u[:, 0] = part.node_coords()[:, 0] * mask_u[:, 0]  # T = x on the boundary
    sols = {}
    for name in ("dense", "subset"):
        d, f = (U, list(range(U))) if name == "dense" else (dpn, fi)
        mask = np.zeros((part.n_local_nodes, d), np.uint8)
        mask[:, f] = mask_u
        g = np.zeros((part.n_local_nodes, d))
        g[:, f] = g_u
        mf = system.MatrixFreeSystem(system.DeviceMesh(ctx, part, d, mask.reshape(-1)), system.KERNEL_DIFFUSION3D, [1.0, 0.0],
                                     field_inds=None if name == "dense" else f)
        if name == "subset":
            assert "strided-dofs" in mf.route(2, 1, True) and " energy" not in mf.route(2, 1, True), mf.route(2, 1, True)
        diag, rhs = mf.diag_rhs(torch.as_tensor(g.reshape(1, -1), device="cuda"))
        minv = torch.where(diag != 0, 1.0 / diag, torch.zeros_like(diag))
        x = torch.zeros_like(rhs[0])
        r = solve.pcg(mf, rhs[0].contiguous(), x, minv, tol=1e-12, residual_scaling="rhs", max_iters=5000)
        assert r.converged
        sols[name] = x.cpu().numpy().reshape(-1, d)[:, f]
        if name == "subset":  # the other kernels' dofs: untouched
            others = np.setdiff1d(np.arange(d), f)
            assert np.all(x.cpu().numpy().reshape(-1, d)[:, others] == 0.0)
    assert np.abs(sols["subset"] - sols["dense"]).max() < 1e-9 * np.abs(sols["dense"]).max()
    assert np.abs(sols["dense"][:, 0] - part.node_coords()[:, 0]).max() < 1e-8  # (T = x, the reference's K1 / K6 solution)


@pytest.mark.gpu
def test_pcg_with_zero_preconditioner_entries():
    """the iteration keeps z = M^-1 r, and r = z / minv was 0 / 0 = NaN on rows where the caller's preconditioner is
    zero (the common way to freeze constrained dofs; l3k_jacobi_inverse with damping 0).  Such rows are frozen now: x keeps its
    initial value there and the other rows solve the system restricted to them, A_ff x_f = b_f - A_fc x_c -- checked against the
    torch-op restatement (solve.cg, which keeps r itself) on that restricted system written out explicitly -- and the single-rank
    and the partitioned entry points agree."""
    import torch
    from l3ster_amd import solve, system
    torch.cuda.set_device(0)
    ctx = system.Context(0, torch.cuda.current_stream().cuda_stream)
    p, U = 3, 4
    part = system.CubePartition(4, p, perturb=0.1)
    mf = system.MatrixFreeSystem(system.DeviceMesh(ctx, part, U, part.dirichlet_mask(U)), system.KERNEL_DIFFUSION3D, [1.0, 1.0])
    diag, rhs = mf.diag_rhs(None)
    minv = solve.jacobi_inverse_native(ctx, diag)
    frozen = torch.zeros_like(minv, dtype=torch.bool)
    frozen[torch.randperm(minv.numel(), generator=torch.Generator().manual_seed(3))[:200].cuda()] = True
    minv[frozen] = 0.0
    x0 = torch.as_tensor(part.synthetic_vector(U)[0, :minv.numel()], device="cuda") * 0.1
    # the restricted system, explicitly: identity on the frozen rows, their columns moved to the right-hand side
    def apply_restricted(v, out):
        vf = v.clone()
        vf[frozen] = 0.0
        mf.apply(vf[None, :], out[None, :])
        out[frozen] = v[frozen]
    xc = torch.zeros_like(x0)
    xc[frozen] = x0[frozen]
    b_r = torch.empty_like(x0)
    mf.apply(xc[None, :], b_r[None, :])
    b_r = rhs[0] - b_r
    b_r[frozen] = x0[frozen]
    minv_r = minv.clone()
    minv_r[frozen] = 1.0
    x1 = x0.clone()
    r1 = solve.cg(apply_restricted, b_r, x1, minv_r, tol=1e-12, residual_scaling="rhs", max_iters=3000)
    assert r1.converged
    x2 = x0.clone()
    r2 = solve.pcg(mf, rhs[0], x2, minv, tol=1e-11, residual_scaling="rhs", throw_on_fail=False, max_iters=3000)
    assert bool(torch.isfinite(x2).all()) and r2.tol == r2.tol  # no NaN
    assert torch.equal(x2[frozen], x0[frozen])  # frozen rows keep the initial guess
    assert r2.converged  # (its residual norm leaves the frozen rows out)
    assert (x1 - x2).norm().item() < 1e-7 * x1.norm().item()

    class Op:
        def apply(self, X, Y):
            mf.apply(X, Y)
    x3 = x0.clone()
    r3 = solve.pcg_distributed(Op(), ctx, rhs[0], x3, minv, tol=1e-11, residual_scaling="rhs", throw_on_fail=False, max_iters=3000)
    assert abs(r3.num_iters - r2.num_iters) <= 1 and (x3 - x2).norm().item() < 1e-9 * x2.norm().item()
    # damping 0: every row frozen -- nothing moves, nothing is NaN
    zero = solve.jacobi_inverse_native(ctx, diag, damping=0.0)
    assert float(zero.abs().max()) == 0.0
    x4 = x0.clone()
    r4 = solve.pcg(mf, rhs[0], x4, zero, tol=1e-11, residual_scaling="rhs", throw_on_fail=False, max_iters=10)
    assert torch.equal(x4, x0) and r4.tol == r4.tol


@pytest.mark.gpu
@pytest.mark.parametrize("p,ne,fast", [(6, 4, True), (4, 5, True), (2, 6, True), (6, 3, False)])
def test_apply_energy_equals_dot_product(p, ne, fast):
    """l3k_mf_apply_energy: y = A x and <x, A x> from the quadrature stage of the element kernel (fast = single-wave route)
    or from the fallback dot product (small mesh on the generic route): both equal the explicit dot product."""
    import torch
    from l3ster_amd import system
    U = 4
    ctx = system.Context(0, torch.cuda.current_stream().cuda_stream)
    ctx.set_tuning(generic_below=0 if fast else 1000000)
    part = system.CubePartition(ne, p, perturb=0.1)
    mask = part.dirichlet_mask(U)
    mf = system.MatrixFreeSystem(system.DeviceMesh(ctx, part, U, mask), system.KERNEL_DIFFUSION3D, [0.7, 1.0])
    X = torch.as_tensor(part.synthetic_vector(U), device="cuda")  # non-zero on the Dirichlet rows too
    Y = torch.full_like(X, 3.0)
    S = torch.full((8,), 7.0, dtype=torch.float64, device="cuda")
    assert ("sumfactFastKernel" in mf.route(with_energy=True) and " energy" in mf.route(with_energy=True)) == fast
    mf.apply_energy(X, Y, S)
    Yr = torch.zeros_like(X)
    mf.apply(X, Yr)
    torch.cuda.synchronize()
    want = float((X * Yr).sum())
    assert float((Y - Yr).abs().max()) <= 1e-12 * float(Yr.abs().max())
    assert abs(float(S[1]) - want) <= 1e-12 * abs(want)
    assert float(S[0]) == 7.0 and float(S[2]) == 7.0  # only slot 1 is written


@pytest.mark.gpu
def test_config5_partitioned_pcg_advdiff_order4():
    """BASELINE.json configs[4] as stated, at a size the oracle solves in seconds: advection-diffusion kernel (U = 4,
    E = 7, velocity = 3 interpolated fields), order 4, element partition over 8 ranks (2 x 2 x 2; threads
    sharing the GPU, queues in place of RCCL), Jacobi-PCG driven by the partitioned matrix-free apply with all-reduced
    scalars, rel. tol 1e-6 -- against the same PCG on the CPU with the oracle's operator on the whole mesh:
    iterations to tolerance +-1; both solves are then continued to 1e-11 and the solutions agree to 1e-7 (relative L2)."""
    import queue
    import threading
    from l3ster_amd.distributed import DistributedOperator, HaloPlan
    from test_gpu_apply import ThreadTransport
    from test_gpu_boundary import ThreadAllReduce
    assert torch.cuda.is_available()
    kid, p, U, ne, parts = system.KERNEL_ADVDIFF3D, 4, 4, (4, 4, 4), (2, 2, 2)
    kpar, tol = [1.0, 0.3, 1.0], 1e-6
    world = int(np.prod(parts))

    def velocity(xyz):  # smooth analytic velocity field at the nodes
        return np.stack([0.2 * np.sin(np.pi * xyz[:, 1]), 0.1 * np.cos(np.pi * xyz[:, 0]), 0.05 * xyz[:, 2]])

    def dirichlet_values(part, mask):  # c = x + y on the boundary
        xyz = part.node_coords()
        g = np.zeros((part.n_local_nodes, U))
        g[:, 0] = xyz[:, 0] + xyz[:, 1]
        return g.reshape(-1) * mask

    boxes = {(a, b): queue.Queue() for a in range(world) for b in range(world)}
    red = ThreadAllReduce(world)
    out, errors = {}, []

    def run(rank):
        try:
            torch.cuda.set_device(0)
            part = system.CubePartition(ne, p, parts, rank, perturb=0.1)
            mask = part.dirichlet_mask(U)
            c = system.Context(0, torch.cuda.current_stream().cuda_stream)
            mf = system.MatrixFreeSystem(system.DeviceMesh(c, part, U, mask), kid, kpar)
            mf.set_fields(torch.as_tensor(velocity(part.node_coords()), device="cuda"))
            op = DistributedOperator(mf, HaloPlan(part, U, "cuda"), transport=ThreadTransport(rank, boxes))
            n_owned = part.n_owned_nodes * U
            g = torch.as_tensor(dirichlet_values(part, mask)[:n_owned], device="cuda")
            diag, rhs = op.diag_rhs(g[None, :])
            x = torch.zeros(n_owned, dtype=torch.float64, device="cuda")
            minv = solve.jacobi_inverse_native(c, diag)
            res = solve.pcg_distributed(op, c, rhs[0], x, minv, tol=tol, residual_scaling="rhs", max_iters=20000, allreduce=red.bind(rank))
            # the iterates of two runs that both meet 1e-6 differ by about that much: the solutions are compared after
            # continuing to 1e-11
            solve.pcg_distributed(op, c, rhs[0], x, minv, tol=1e-11, residual_scaling="rhs", max_iters=20000, allreduce=red.bind(rank))
            torch.cuda.synchronize()
            out[rank] = (res.num_iters, x.cpu().numpy(), part.node_grid_id[:part.n_owned_nodes].copy())
        except Exception as exc:  # pragma: no cover
            errors.append((rank, repr(exc)))
            try:
                red.barrier.abort()
            except Exception:
                pass

    threads = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(600)
    assert not errors, errors
    # the same solve on the CPU: oracle operator on the whole mesh, torch-op PCG
    whole = system.CubePartition(ne, p, perturb=0.1)
    mask = whole.dirichlet_mask(U)
    om = oracle_mesh(whole, p + 1, U, np.arange(U), mask, velocity(whole.node_coords()))
    g = dirichlet_values(whole, mask)
    d_ref, r_ref = O.mf_diag_rhs(om, kid, 1, np.asfortranarray(g[:, None]), kparams=kpar, nthreads=4)

    def apply_cpu(v, o):
        o.copy_(torch.as_tensor(O.mf_apply(om, kid, v.numpy().reshape(-1, 1), kparams=kpar, nthreads=4)[:, 0]))

    x_ref = torch.zeros(len(d_ref), dtype=torch.float64)
    minv_ref = solve.jacobi_inverse(torch.as_tensor(d_ref))
    res_ref = solve.cg(apply_cpu, torch.as_tensor(r_ref[:, 0].copy()), x_ref, minv_ref, tol=tol, residual_scaling="rhs", max_iters=20000)
    solve.cg(apply_cpu, torch.as_tensor(r_ref[:, 0].copy()), x_ref, minv_ref, tol=1e-11, residual_scaling="rhs", max_iters=20000)
    iters = {v[0] for v in out.values()}
    assert len(iters) == 1, iters
    assert abs(iters.pop() - res_ref.num_iters) <= 1, (out[0][0], res_ref.num_iters)
    row_of = {int(gid): i for i, gid in enumerate(whole.node_grid_id)}
    xr = x_ref.numpy().reshape(-1, U)
    num = den = 0.0
    for r in range(world):
        _, x, gid = out[r]
        rows = np.array([row_of[int(k)] for k in gid])
        num += np.sum((x.reshape(-1, U) - xr[rows]) ** 2)
        den += np.sum(xr[rows] ** 2)
    assert np.sqrt(num / den) < 1e-7


# ------------------------------------------------------------------------------------------------ the driver l3k_pcg_solve
_SMALL = {}


def _small_problem(deterministic=False):
    """A 2^3 order-2 perturbed cube, Diffusion3D with a source, Dirichlet mask (500 dofs), with its operator as a dense matrix:
    column j is mf.apply on the unit vector e_j.  Cached per module; `deterministic`: on a context in deterministic mode."""
    if deterministic in _SMALL:
        return _SMALL[deterministic]
    torch.cuda.set_device(0)
    ctx = system.Context(0, torch.cuda.current_stream().cuda_stream)
    if deterministic:
        ctx.set_deterministic(True)
    p, U = 2, 4
    part = system.CubePartition(2, p, perturb=0.1)
    mesh = system.DeviceMesh(ctx, part, U, part.dirichlet_mask(U))
    mf = system.MatrixFreeSystem(mesh, system.KERNEL_DIFFUSION3D, [1.0, 1.0])
    diag, rhs = mf.diag_rhs(None)
    n = diag.numel()
    assert n == 5 ** 3 * U
    E, Y = torch.zeros(n, dtype=torch.float64, device="cuda"), torch.empty(n, dtype=torch.float64, device="cuda")
    A = np.empty((n, n))
    for j in range(n):
        E.zero_()
        E[j] = 1.0
        mf.apply(E[None, :], Y[None, :])
        A[:, j] = Y.cpu().numpy()
    assert np.abs(A - A.T).max() <= 1e-12 * np.abs(A).max()
    A = 0.5 * (A + A.T)
    minv = solve.jacobi_inverse_native(ctx, diag)
    x0 = torch.as_tensor(0.1 * np.random.default_rng(7).standard_normal(n), device="cuda")
    P = dict(ctx=ctx, mesh=mesh, mf=mf, A=A, b=rhs[0].contiguous(), minv=minv, x0=x0, n=n)
    _SMALL[deterministic] = P
    return P


def _float64_cost(P):
    """What float64 alone costs on this matrix: the distance between cg_ref.pcg_ref in longdouble and the same recurrence in
    float64 numpy (both on the CPU, neither is the code under test), largest value over the first six steps.  Distances:
    ||x_64 - x_ld|| / ||x_ld|| and |res_64 - res_ld| / ||b - A x0|| -- rounding errors of a residual are absolute (eps |A| |x|),
    so they are measured against the residual the iteration starts from, not against the one it has reached."""
    import cg_ref as R
    if "cost" not in P:
        A, b, x0, minv = P["A"], P["b"].cpu().numpy(), P["x0"].cpu().numpy(), P["minv"].cpu().numpy()
        r0 = float(R.pcg_ref(A, b, x0, minv, 0)[1])
        worst = 0.0
        for k in range(1, 7):
            x_ld, res_ld, _, _ = R.pcg_ref(A, b, x0, minv, k)
            x_64, res_64, _, _ = R.pcg_ref(A, b, x0, minv, k, dtype=np.float64)
            dx = float(np.linalg.norm((x_64.astype(R.LD) - x_ld).astype(np.float64)) / np.linalg.norm(x_ld.astype(np.float64)))
            worst = max(worst, dx, abs(float(res_64) - float(res_ld)) / r0)
        P["cost"], P["r0"] = worst, r0
        print(f"float64 against longdouble over the first six steps: {worst:.3e}; bound 10x = {10 * worst:.3e}")
    return P["cost"]


def _true_residual(P, x, minv=None):
    import cg_ref as R
    r = P["b"].cpu().numpy().astype(R.LD) - P["A"].astype(R.LD) @ x.cpu().numpy().astype(R.LD)
    return float(np.sqrt(np.sum(r * r)))


@pytest.mark.gpu
def test_first_pcg_steps_match_the_longdouble_recurrence():
    """k = 1..6 iterations of l3k_pcg_solve from a non-zero start against k steps of Hestenes-Stiefel PCG in longdouble on the
    dense operator: x, and achieved_tol against the true ||b - A x||.  A beta that is slightly off or a dot product that drops
    entries shows here at once; in a converged solve it would not."""
    import cg_ref as R
    P = _small_problem()
    # measured on this matrix: float64 against longdouble 1.232e-15 (largest of the six steps, both distances); the bound is
    # 10x the value measured in this run, 1.232e-14 (the matrix comes from applies that scatter with atomics, so the last
    # digits may move).  The factor 10 covers the different summation order on the device, which stayed below 1.5e-15 in x
    # and 3e-17 in the residual.
    bound = 10 * _float64_cost(P)
    assert 1e-16 < bound < 1e-12
    A, b, x0, minv = P["A"], P["b"].cpu().numpy(), P["x0"].cpu().numpy(), P["minv"].cpu().numpy()
    for k in range(1, 7):
        x_ld, res_ld, steps, _ = R.pcg_ref(A, b, x0, minv, k)
        assert len(steps) == k
        x = P["x0"].clone()
        res = solve.pcg(P["mf"], P["b"], x, P["minv"], tol=0.0, max_iters=k, residual_scaling="none", throw_on_fail=False)
        assert res.num_iters == k and not res.converged
        dx = float(np.linalg.norm((x.cpu().numpy().astype(R.LD) - x_ld).astype(np.float64)) / np.linalg.norm(x_ld.astype(np.float64)))
        dres = abs(res.tol - float(res_ld)) / P["r0"]
        dtrue = abs(res.tol - _true_residual(P, x)) / P["r0"]
        print(f"k={k}: x {dx:.3e} achieved_tol against pcg_ref {dres:.3e} against ||b - A x|| {dtrue:.3e} (bound {bound:.3e})")
        assert dx <= bound and dres <= bound and dtrue <= bound


@pytest.mark.gpu
def test_pcg_residual_scaling_modes():
    """residual_scaling "none" / "initial" / "rhs": achieved_tol is the true residual over 1, ||b - A x0||, ||b||, and the larger
    the scale the fewer iterations reach one tolerance."""
    P = _small_problem()
    bound = 10 * _float64_cost(P)
    bnorm = float(np.linalg.norm(P["b"].cpu().numpy()))
    scales = {"none": 1.0, "initial": P["r0"], "rhs": bnorm}
    its = {}
    for mode, scale in scales.items():
        x = P["x0"].clone()
        res = solve.pcg(P["mf"], P["b"], x, P["minv"], tol=1e-3, residual_scaling=mode)
        assert res.converged and res.tol <= 1e-3
        true = _true_residual(P, x)
        print(f"{mode}: scale {scale:.6e} iterations {res.num_iters} achieved {res.tol:.6e} true/scale {true / scale:.6e}")
        assert abs(res.tol * scale - true) <= bound * P["r0"]
        its[mode] = res.num_iters
    order = sorted(scales, key=lambda m: scales[m])
    assert len({round(scales[m], 6) for m in order}) == 3  # three different scales, or the test says nothing
    assert its[order[0]] >= its[order[1]] >= its[order[2]] and its[order[0]] > its[order[2]]


@pytest.mark.gpu
def test_pcg_check_every_on_the_single_rank_driver():
    """check_every = 7: the driver looks at the residual every 7th iteration only, so it stops at a multiple of 7 (or at
    max_iters), with the iterate the every-iteration driver has at that count -- bit for bit on a context in deterministic mode
    (no atomics in the apply, <p, A p> from the fixed-order dot product)."""
    P = _small_problem(deterministic=True)
    x1 = P["x0"].clone()
    r1 = solve.pcg(P["mf"], P["b"], x1, P["minv"], tol=1e-8, residual_scaling="rhs")
    x7 = P["x0"].clone()
    r7 = solve.pcg(P["mf"], P["b"], x7, P["minv"], tol=1e-8, residual_scaling="rhs", check_every=7)
    assert r7.converged and r7.num_iters % 7 == 0 and r1.num_iters <= r7.num_iters < r1.num_iters + 7
    xs = P["x0"].clone()
    rs = solve.pcg(P["mf"], P["b"], xs, P["minv"], tol=0.0, residual_scaling="rhs", max_iters=r7.num_iters, throw_on_fail=False)
    assert rs.num_iters == r7.num_iters and torch.equal(xs, x7) and rs.tol == r7.tol
    # max_iters that is no multiple of 7: the last iteration is checked as well
    xm = P["x0"].clone()
    rm = solve.pcg(P["mf"], P["b"], xm, P["minv"], tol=0.0, residual_scaling="rhs", max_iters=10, check_every=7, throw_on_fail=False)
    xe = P["x0"].clone()
    re = solve.pcg(P["mf"], P["b"], xe, P["minv"], tol=0.0, residual_scaling="rhs", max_iters=10, throw_on_fail=False)
    assert rm.num_iters == 10 and torch.equal(xm, xe) and rm.tol == re.tol


@pytest.mark.gpu
def test_pcg_max_iters_reached():
    P = _small_problem()
    x = P["x0"].clone()
    res = solve.pcg(P["mf"], P["b"], x, P["minv"], tol=1e-10, residual_scaling="rhs", max_iters=3, throw_on_fail=False)
    assert res.converged is False and res.num_iters == 3 and res.tol > 1e-10
    bnorm = float(np.linalg.norm(P["b"].cpu().numpy()))
    assert abs(res.tol * bnorm - _true_residual(P, x)) <= 10 * _float64_cost(P) * P["r0"]
    with pytest.raises(RuntimeError, match="failed to converge"):
        solve.pcg(P["mf"], P["b"], P["x0"].clone(), P["minv"], tol=1e-10, residual_scaling="rhs", max_iters=3)


@pytest.mark.gpu
def test_pcg_null_opts_are_the_documented_defaults():
    """opts == NULL through the raw C call behaves as {1e-6, 10000, 0, 1} (bit for bit on a deterministic context); d_minv ==
    NULL is the preconditioner of ones."""
    import ctypes as C
    from l3ster_amd import capi
    P = _small_problem(deterministic=True)
    vp = lambda t: C.c_void_p(t.data_ptr())
    xn, res = P["x0"].clone(), capi.CgResult()
    capi.check(capi.load().l3k_pcg_solve(P["mf"]._h, vp(P["b"]), vp(xn), vp(P["minv"]), None, C.byref(res)))
    xd = P["x0"].clone()
    rd = solve.pcg(P["mf"], P["b"], xd, P["minv"], tol=1e-6, max_iters=10000, residual_scaling="none", check_every=1)
    assert res.converged == 1 and res.iterations == rd.num_iters and res.achieved_tol == rd.tol and torch.equal(xn, xd)
    assert res.achieved_tol <= 1e-6 and res.iterations > 3
    # a tolerance ten times tighter takes more iterations: the 1e-6 above is the one that stopped the NULL run
    rt = solve.pcg(P["mf"], P["b"], P["x0"].clone(), P["minv"], tol=1e-7, residual_scaling="none")
    assert rt.num_iters > rd.num_iters
    x_none, x_ones = P["x0"].clone(), P["x0"].clone()
    r_none = solve.pcg(P["mf"], P["b"], x_none, None, tol=1e-6)
    r_ones = solve.pcg(P["mf"], P["b"], x_ones, torch.ones_like(P["minv"]), tol=1e-6)
    assert r_none.num_iters == r_ones.num_iters and r_none.tol == r_ones.tol and torch.equal(x_none, x_ones)


@pytest.mark.gpu
def test_pcg_start_vector_that_solves_the_system():
    P = _small_problem()
    x = P["x0"].clone()
    assert solve.pcg(P["mf"], P["b"], x, P["minv"], tol=1e-12, residual_scaling="rhs").converged
    before = x.clone()
    res = solve.pcg(P["mf"], P["b"], x, P["minv"], tol=1e-10, residual_scaling="rhs")
    assert res.converged and res.num_iters == 0 and torch.equal(x, before) and res.tol <= 1e-10
    # b = 0 from x0 = 0 under "rhs" scaling: 0 / max(0, 1e-300), not 0 / 0
    zero, x = torch.zeros_like(P["b"]), torch.zeros_like(P["b"])
    res = solve.pcg(P["mf"], zero, x, P["minv"], tol=1e-6, residual_scaling="rhs")
    assert res.converged and res.num_iters == 0 and res.tol == 0.0 and float(x.abs().max()) == 0.0


@pytest.mark.gpu
def test_native_pcg_past_the_grid_caps():
    """One solve whose vectors are longer than one grid of the vector kernels (1024 blocks of 256 threads = 262 144 entries):
    cube 12^3, order 4, U = 4.  l3k_pcg_solve and the partitioned form against the torch-op PCG (independent of the HIP vector
    kernels), and the true residual recomputed with one apply."""
    torch.cuda.set_device(0)
    ctx = system.Context(0, torch.cuda.current_stream().cuda_stream)
    p, U, tol = 4, 4, 1e-10
    part = system.CubePartition(12, p, perturb=0.1)
    mesh = system.DeviceMesh(ctx, part, U, part.dirichlet_mask(U))
    mf = system.MatrixFreeSystem(mesh, system.KERNEL_DIFFUSION3D, [1.0, 1.0])
    diag, rhs = mf.diag_rhs(None)
    n = diag.numel()
    assert n == 49 ** 3 * 4 == 470596 and n > 256 * 1024
    minv = solve.jacobi_inverse_native(ctx, diag)
    assert torch.equal(minv, solve.jacobi_inverse(diag))
    b = rhs[0]
    x1 = torch.zeros_like(diag)
    r1 = solve.cg(lambda v, out: mf.apply(v[None, :], out[None, :]), b, x1, minv, tol=tol, residual_scaling="rhs")
    x2 = torch.zeros_like(diag)
    r2 = solve.pcg(mf, b, x2, minv, tol=tol, residual_scaling="rhs")
    assert r2.converged and abs(r1.num_iters - r2.num_iters) <= 1
    assert (x1 - x2).norm().item() < 1e-8 * x1.norm().item()

    class Op:
        def apply(self, X, Y):
            mf.apply(X, Y)
    x3 = torch.zeros_like(diag)
    r3 = solve.pcg_distributed(Op(), ctx, b, x3, minv, tol=tol, residual_scaling="rhs")
    assert abs(r3.num_iters - r2.num_iters) <= 1 and (x3 - x2).norm().item() < 1e-8 * x2.norm().item()
    ax = torch.empty_like(diag)
    for x in (x2, x3):
        mf.apply(x[None, :], ax[None, :])
        true = ((b - ax).norm() / b.norm()).item()
        print(f"n={n}: iterations {r1.num_iters} / {r2.num_iters} / {r3.num_iters}, true residual {true:.3e}")
        assert true <= 2 * tol


@pytest.mark.gpu
def test_apply_energy_with_a_boundary_term_takes_the_dot_product():
    """With a boundary term attached the element kernel does not accumulate <x, A x> (the term's share would be missing):
    l3k_mf_apply_energy is the apply followed by l3k_cg_dot_pap, and writes slot 1 alone."""
    U, p = 4, 4
    ctx = system.Context(0, torch.cuda.current_stream().cuda_stream)
    ctx.set_tuning(generic_below=0)
    part = system.CubePartition(5, p, perturb=0.1)
    mesh = system.DeviceMesh(ctx, part, U, part.dirichlet_mask(U, sides=(4, 5)))
    mf = system.MatrixFreeSystem(mesh, system.KERNEL_DIFFUSION3D, [0.7, 1.0])
    assert " energy" in mf.route(with_energy=True)
    mf.attach_boundary(system.BoundaryTerm(mesh, system.KERNEL_ROBIN3D, *part.boundary_sides([1]), kernel_params=[2.0, 0.7]))
    assert "sumfactFastKernel" in mf.route(with_energy=True) and " energy" not in mf.route(with_energy=True), mf.route(with_energy=True)
    X = torch.as_tensor(part.synthetic_vector(U), device="cuda")
    Y = torch.full_like(X, 3.0)
    S = torch.as_tensor(np.arange(8) + 7.5, device="cuda")
    mf.apply_energy(X, Y, S)
    Yr = torch.zeros_like(X)
    mf.apply(X, Yr)
    Y0 = torch.zeros_like(X)  # the boundary term is in: the operator without it gives another product
    torch.cuda.synchronize()
    want = float((X * Yr).sum())
    assert float((Y - Yr).abs().max()) <= 1e-12 * float(Yr.abs().max())
    assert abs(float(S[1]) - want) <= 1e-12 * abs(want)
    h = S.cpu().numpy()
    assert np.array_equal(np.delete(h, 1), np.delete(np.arange(8) + 7.5, 1))  # slots 0 and 2 (and 3..7) untouched
    plain = system.MatrixFreeSystem(mesh, system.KERNEL_DIFFUSION3D, [0.7, 1.0])
    plain.apply(X, Y0)
    assert abs(float((X * Y0).sum()) - want) > 1e-6 * abs(want)
