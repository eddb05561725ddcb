"""The matrix-free Chebyshev-Jacobi preconditioner on the device (l3k_cheb_*, l3k_pcg_solve_cheb and the exported pieces) against
solve.chebyshev_reference / solve.cg driven by the oracle's dense operator on the CPU, and against torch ops on the same device
vectors where a single kernel is checked."""
import ctypes as C

import numpy as np
import pytest
import torch

import oracle_lib as O
from helpers import oracle_mesh
from l3ster_amd import capi, solve, system
from test_solve import node_coords, setup_problem

pytestmark = pytest.mark.gpu
COND = 30.0
D3, AD3 = system.KERNEL_DIFFUSION3D, system.KERNEL_ADVDIFF3D
SHAPES = [(D3, 3, 2), (D3, 2, 4), (AD3, 3, 2)]
_CASES = {}


def vp(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def rel(a, b):
    return float((a - b).norm() / b.norm())


def case(kid, ne, p, deterministic=False):
    """One problem of test_solve.py::test_gpu_pcg_matches_cpu_restatement (perturbed cube, Dirichlet mask, T = x on the boundary;
    AdvDiff3D with the analytic velocity field) on the device and on the CPU: there the oracle's operator as a dense matrix
    (mf_apply on the identity), its diagonal / rhs and the largest eigenvalue of D^-1 A.  Computed once per module."""
    key = (kid, ne, p, deterministic)
    if key in _CASES:
        return _CASES[key]
    torch.cuda.set_device(0)
    ctx = system.Context(0, torch.cuda.current_stream().cuda_stream)
    if deterministic:
        ctx.set_deterministic(True)
    info = system.kernel_info(kid)
    U, F = info["n_unknowns"], info["n_fields"]
    part, mask, g, exact = setup_problem(ne, p)
    kpar = [1.0, 0.0] if kid == D3 else [1.0, 0.3, 0.0]
    fields = None
    if F:
        xyz = node_coords(part)
        fields = np.stack([0.2 * np.sin(np.pi * xyz[:, 1]), 0.1 * np.cos(np.pi * xyz[:, 0]), 0.05 * xyz[:, 2]])
    mf = system.MatrixFreeSystem(system.DeviceMesh(ctx, part, U, mask), kid, kpar)
    if F:
        mf.set_fields(torch.as_tensor(fields, device="cuda"))
    diag, rhs = mf.diag_rhs(torch.as_tensor(g, device="cuda"))
    minv = solve.jacobi_inverse_native(ctx, diag)
    om = oracle_mesh(part, p + 1, U, np.arange(U), mask, fields)
    d_ref, r_ref = O.mf_diag_rhs(om, kid, 1, np.asfortranarray(g.T), kparams=kpar)
    n = len(d_ref)
    A = np.ascontiguousarray(O.mf_apply(om, kid, np.eye(n), kparams=kpar, nthreads=4))
    assert np.abs(A - A.T).max() <= 1e-11 * np.abs(A).max()
    At = torch.as_tensor(A)
    minv_ref = solve.jacobi_inverse(torch.as_tensor(d_ref))
    sq = np.sqrt(minv_ref.numpy())
    lam = np.linalg.eigvalsh(sq[:, None] * (0.5 * (A + A.T)) * sq[None, :])
    assert lam[0] > 0
    c = dict(ctx=ctx, mf=mf, minv=minv, b=rhs[0].contiguous(), n=n, exact=exact, A=A, kid=kid,
             apply_cpu=lambda v, out: out.copy_(At @ v), minv_ref=minv_ref, b_ref=torch.as_tensor(r_ref[:, 0].copy()),
             lmax=float(lam[-1]))
    _CASES[key] = c
    return c


# ------------------------------------------------------------------------------------------------ 1. the application
@pytest.mark.parametrize("kid,ne,p", SHAPES)
def test_cheb_apply_matches_the_cpu_restatement(kid, ne, p):
    """l3k_cheb_apply against chebyshev_reference over the oracle's dense matrix, lambda_max passed in, degrees 1, 2, 3, 5:
    relative L2 <= 1e-11, the mesh-level bar of the apply (the polynomial's coefficients are O(1))."""
    c = case(kid, ne, p)
    r_cpu = torch.as_tensor(np.random.default_rng(5).standard_normal(c["n"]))
    r, z = r_cpu.cuda(), torch.full((c["n"],), 7.0, dtype=torch.float64, device="cuda")
    for degree in (1, 2, 3, 5):
        cheb = solve.ChebyshevPreconditioner(c["mf"], c["minv"], degree=degree, cond_est=COND, lambda_max=c["lmax"])
        info = cheb.info
        assert (info.degree, info.applies_per_call, info.power_iters) == (degree, degree - 1, 0)
        assert info.lambda_max == c["lmax"] == info.lambda_est and info.lambda_min == c["lmax"] / COND
        cheb.apply(r, z)
        want = solve.chebyshev_reference(c["apply_cpu"], c["minv_ref"], r_cpu, c["lmax"], COND, degree)
        err = rel(z.cpu(), want)
        print(f"kernel {kid} ne {ne} p {p} degree {degree}: device against the CPU restatement {err:.3e}")
        assert err <= 1e-11
        cheb.close()
        cheb.close()  # (idempotent)


# ------------------------------------------------------------------------------------------------ 2. the power method
def test_power_iteration_matches_numpy_and_is_reproducible():
    """lambda_est against the numpy power method from the documented start vector on the oracle's dense D^-1 A (same number of
    steps, 1e-10 relative); two creations bitwise equal -- on a context in deterministic mode, where the apply itself is
    reproducible (its atomics are not); lambda_max = boost_factor * lambda_est; a given lambda_max runs no power iteration."""
    c = case(D3, 3, 2, deterministic=True)
    n, steps = c["n"], 7
    h = np.arange(n, dtype=np.uint32)
    h ^= h >> np.uint32(16)
    h *= np.uint32(0x7FEB352D)
    h ^= h >> np.uint32(15)
    h *= np.uint32(0x846CA68B)
    h ^= h >> np.uint32(16)
    d = c["minv_ref"].numpy()
    y = np.where(d != 0, h.astype(np.float64) * 2.0 ** -31 - 1.0, 0.0)
    lam = None
    for _ in range(steps):
        x = y * (1.0 / np.sqrt(y @ y))
        y = d * (c["A"] @ x)
        lam = x @ y
    a = solve.ChebyshevPreconditioner(c["mf"], c["minv"], degree=2, cond_est=COND, max_power_iters=steps, boost_factor=1.25)
    b = solve.ChebyshevPreconditioner(c["mf"], c["minv"], degree=2, cond_est=COND, max_power_iters=steps, boost_factor=1.25)
    ia, ib = a.info, b.info
    print(f"lambda_est device {ia.lambda_est!r} numpy {lam!r} exact lambda_max {c['lmax']!r}")
    assert abs(ia.lambda_est - lam) <= 1e-10 * lam
    assert ia.lambda_est == ib.lambda_est and ia.lambda_max == ib.lambda_max
    assert ia.lambda_max == 1.25 * ia.lambda_est and ia.lambda_min == ia.lambda_max / COND and ia.power_iters == steps
    assert abs(ia.lambda_est - c["lmax"]) < 0.5 * c["lmax"]  # (an estimate of the right size; <x, D^-1 A x> is no bound)
    given = solve.ChebyshevPreconditioner(c["mf"], c["minv"], degree=2, lambda_max=2.5)
    assert given.info.power_iters == 0 and given.info.lambda_max == 2.5


# ------------------------------------------------------------------------------------------------ 3. the solve
@pytest.mark.parametrize("kid,ne,p", SHAPES)
def test_pcg_cheb_matches_the_cpu_restatement(kid, ne, p):
    """solve.pcg(precond=cheb) against solve.cg with chebyshev_reference over the oracle's operator: same lambda_max, degree 3,
    tol 1e-10, scaling "rhs": iterations +-1, solutions to 1e-7 (the bars of test_gpu_pcg_matches_cpu_restatement), Diffusion3D
    reproduces the exact linear solution; the device's outer count is below the CPU Jacobi count if the CPU Chebyshev count is."""
    c = case(kid, ne, p)
    cheb = solve.ChebyshevPreconditioner(c["mf"], c["minv"], degree=3, cond_est=COND, lambda_max=c["lmax"])
    x = torch.zeros_like(c["b"])
    res = solve.pcg(c["mf"], c["b"], x, precond=cheb, tol=1e-10, residual_scaling="rhs")
    x_ref = torch.zeros(c["n"], dtype=torch.float64)
    res_ref = solve.cg(c["apply_cpu"], c["b_ref"], x_ref, tol=1e-10, residual_scaling="rhs",
                       precond=lambda r: solve.chebyshev_reference(c["apply_cpu"], c["minv_ref"], r, c["lmax"], COND, 3))
    x_jac = torch.zeros(c["n"], dtype=torch.float64)
    res_jac = solve.cg(c["apply_cpu"], c["b_ref"], x_jac, c["minv_ref"], tol=1e-10, residual_scaling="rhs")
    print(f"kernel {kid} ne {ne} p {p}: outer iterations device {res.num_iters}, CPU Chebyshev {res_ref.num_iters}, "
          f"CPU Jacobi {res_jac.num_iters}; solutions {rel(x.cpu(), x_ref):.3e}")
    assert res.converged and abs(res.num_iters - res_ref.num_iters) <= 1
    assert rel(x.cpu(), x_ref) < 1e-7
    if kid == D3:
        assert np.abs(x.cpu().numpy() - c["exact"]).max() < 1e-7
    if res_ref.num_iters < res_jac.num_iters:
        assert res.num_iters < res_jac.num_iters
    # a multivector: its columns one after the other
    B = torch.stack([c["b"], 2.0 * c["b"]])
    X = torch.zeros_like(B)
    out = solve.pcg(c["mf"], B, X, precond=cheb, tol=1e-10, residual_scaling="rhs")
    assert len(out) == 2 and all(r.converged for r in out)
    assert rel(X[0], x) < 1e-9 and rel(X[1], 2.0 * x) < 1e-9


# ------------------------------------------------------------------------------------------------ 4. the partitioned form
class _Op:
    def __init__(self, mf):
        self.mf = mf

    def apply(self, X, Y):
        self.mf.apply(X, Y)


def test_pcg_distributed_with_the_pieces_matches_the_driver():
    c = case(D3, 2, 4)
    cheb = solve.ChebyshevPreconditioner(c["mf"], c["minv"], degree=3, cond_est=COND, lambda_max=c["lmax"])
    x = torch.zeros_like(c["b"])
    res = solve.pcg(c["mf"], c["b"], x, precond=cheb, tol=1e-10, residual_scaling="rhs")
    for precond in (dict(degree=3, cond_est=COND, lambda_max=c["lmax"]), cheb):
        xd = torch.zeros_like(c["b"])
        rd = solve.pcg_distributed(_Op(c["mf"]), c["ctx"], c["b"], xd, c["minv"], tol=1e-10, residual_scaling="rhs", precond=precond)
        assert rd.converged and abs(rd.num_iters - res.num_iters) <= 1 and rel(xd, x) < 1e-8
    # its own power method (torch ops, the reduction hook sees <x, y> and <y, y>) against the library's: same start, same steps
    seen = []
    own = solve.ChebyshevPreconditioner(c["mf"], c["minv"], degree=3, cond_est=COND, max_power_iters=6)
    xo = torch.zeros_like(c["b"])
    ro = solve.pcg(c["mf"], c["b"], xo, precond=own, tol=1e-10, residual_scaling="rhs")
    xp = torch.zeros_like(c["b"])
    rp = solve.pcg_distributed(_Op(c["mf"]), c["ctx"], c["b"], xp, c["minv"], tol=1e-10, residual_scaling="rhs",
                               precond=dict(degree=3, cond_est=COND, max_power_iters=6), allreduce=lambda v: seen.append(v.numel()))
    assert abs(rp.num_iters - ro.num_iters) <= 1 and rel(xp, xo) < 1e-8
    assert seen[:8] == [1] + [2] * 6 + [1]  # <y, y> of the start, six steps, then <r, r>
    with pytest.raises(capi.L3KError, match="needs minv"):
        solve.pcg_distributed(_Op(c["mf"]), c["ctx"], c["b"], xp, None, precond=dict(degree=2))


# ------------------------------------------------------------------------------------------------ 5. past one grid
def test_pieces_past_one_grid():
    """n = 41^3 * 4 = 275 684 owned dofs: more than one grid of the vector kernels (1024 x 256 = 262 144) and no multiple of 256.
    Each exported piece once and one l3k_cheb_apply at degree 2 against torch ops on the same device vectors: bitwise where the
    arithmetic is products only (no contraction can change them), 1e-14 relative where a sum may be fused into an FMA;
    reductions 1e-12 relative.  Deterministic context: the apply inside l3k_cheb_apply is then the same bits as the one the
    restatement takes."""
    torch.cuda.set_device(0)
    ctx = system.Context(0, torch.cuda.current_stream().cuda_stream)
    ctx.set_deterministic(True)
    p, U = 4, 4
    part = system.CubePartition(10, p, perturb=0.1)
    mf = system.MatrixFreeSystem(system.DeviceMesh(ctx, part, U, part.dirichlet_mask(U)), D3, [1.0, 1.0])
    diag, _ = mf.diag_rhs(None)
    n = diag.numel()
    assert n == 275684 and n > 1024 * 256 and n % 256 != 0
    lib = capi.load()
    minv = solve.jacobi_inverse_native(ctx, diag)
    minv[torch.arange(5, n, 1001, device="cuda")] = 0.0  # some frozen rows, the last block's tail among them
    minv[n - 1] = 0.0
    live = minv != 0
    gen = torch.Generator(device="cuda").manual_seed(9)
    rnd = lambda: torch.randn(n, dtype=torch.float64, device="cuda", generator=gen)
    r, az, w0, z0, x0, p0, ap = rnd(), rnd(), rnd(), rnd(), rnd(), rnd(), rnd()
    zero = torch.zeros_like(r)
    s = torch.full((8,), 3.5, dtype=torch.float64, device="cuda")
    untouched = lambda *slots: all(float(s[k]) == 3.5 for k in range(8) if k not in slots)
    # l3k_cheb_first
    w, z = torch.full_like(r, 9.0), torch.full_like(r, 9.0)
    capi.check(lib.l3k_cheb_first(ctx._h, vp(r), vp(minv), 0.37, vp(w), vp(z), n, vp(s)))
    want = torch.where(live, 0.37 * (minv * r), zero)
    assert torch.equal(w, want) and torch.equal(z, want)
    assert abs(float(s[2]) - float(torch.dot(r, want))) <= 1e-12 * abs(float(torch.dot(r, want))) and untouched(2)
    s[2] = 3.5
    w.fill_(9.0)
    capi.check(lib.l3k_cheb_first(ctx._h, vp(r), vp(minv), 0.37, vp(w), vp(z), n, None))
    assert torch.equal(w, want) and untouched()
    # l3k_cheb_step
    a, b = 0.21, 1.7
    w, z = w0.clone(), z0.clone()
    capi.check(lib.l3k_cheb_step(ctx._h, vp(r), vp(az), vp(minv), a, b, vp(w), vp(z), n, vp(s)))
    w_want = torch.where(live, a * w0 + b * (minv * (r - az)), zero)
    z_want = torch.where(live, z0 + w_want, zero)
    assert rel(w, w_want) <= 1e-14 and rel(z, z_want) <= 1e-14
    assert torch.equal(w[~live], zero[~live]) and torch.equal(z[~live], zero[~live])
    assert abs(float(s[2]) - float(torch.dot(r, z_want))) <= 1e-12 * abs(float(torch.dot(r, z_want))) and untouched(2)
    w2, z2 = w0.clone(), z0.clone()
    s[2] = 3.5
    capi.check(lib.l3k_cheb_step(ctx._h, vp(r), vp(az), vp(minv), a, b, vp(w2), vp(z2), n, None))
    assert torch.equal(w2, w) and torch.equal(z2, z) and untouched()
    # l3k_cg_update_rx
    s[0], s[1] = 0.8, 2.9
    alpha = 0.8 / 2.9
    rr = r.clone()
    rr[~live] = 0.0  # (as the iteration keeps it)
    x, r1 = x0.clone(), rr.clone()
    capi.check(lib.l3k_cg_update_rx(ctx._h, vp(x), vp(r1), vp(p0), vp(ap), vp(minv), n, vp(s)))
    x_want, r_want = torch.where(live, x0 + alpha * p0, x0), torch.where(live, rr - alpha * ap, zero)
    assert rel(x, x_want) <= 1e-14 and rel(r1, r_want) <= 1e-14
    assert torch.equal(x[~live], x0[~live]) and torch.equal(r1[~live], zero[~live])
    assert abs(float(s[3]) - float(torch.dot(r_want, r_want))) <= 1e-12 * float(torch.dot(r_want, r_want))
    assert float(s[0]) == 0.8 and float(s[1]) == 2.9 and untouched(0, 1, 3)
    # l3k_cg_update_p
    s[2] = 1.3
    pp = p0.clone()
    capi.check(lib.l3k_cg_update_p(ctx._h, vp(pp), vp(z0), n, vp(s)))
    assert rel(pp, z0 + (1.3 / 0.8) * p0) <= 1e-14
    assert float(s[0]) == 1.3 and float(s[2]) == 1.3 and float(s[1]) == 2.9
    # one application at degree 2
    cheb = solve.ChebyshevPreconditioner(mf, minv, degree=2, cond_est=COND, lambda_max=2.0)
    c0, steps = solve.chebyshev_coefficients(2.0, 2.0 / COND, 2)
    zc = torch.full_like(r, 9.0)
    cheb.apply(r, zc)
    w_t = torch.where(live, c0 * (minv * r), zero)
    az_t = torch.empty_like(r)
    mf.apply(w_t[None, :], az_t[None, :])
    z_t = torch.where(live, w_t + (steps[0][0] * w_t + steps[0][1] * (minv * (r - az_t))), zero)
    print(f"n={n}: l3k_cheb_apply at degree 2 against torch ops {rel(zc, z_t):.3e}")
    assert rel(zc, z_t) <= 1e-14 and torch.equal(zc[~live], zero[~live])


# ------------------------------------------------------------------------------------------------ 6. frozen rows
def test_frozen_rows_stay_zero_and_keep_x():
    c = case(D3, 3, 2)
    n, mf, ctx = c["n"], c["mf"], c["ctx"]
    minv = c["minv"].clone()
    frozen = torch.zeros(n, dtype=torch.bool, device="cuda")
    frozen[torch.randperm(n, generator=torch.Generator().manual_seed(3))[:200].cuda()] = True
    minv[frozen] = 0.0
    first = int(torch.nonzero(frozen)[0])
    gen = torch.Generator(device="cuda").manual_seed(4)
    r, az, w, z = (torch.randn(n, dtype=torch.float64, device="cuda", generator=gen) for _ in range(4))
    az[first] = float("nan")  # a non-finite A z on a frozen row must not reach w or z
    capi.check(capi.load().l3k_cheb_step(ctx._h, vp(r), vp(az), vp(minv), 0.3, 1.1, vp(w), vp(z), n, None))
    assert bool(torch.isfinite(w).all()) and bool(torch.isfinite(z).all())
    assert float(w[frozen].abs().max()) == 0.0 and float(z[frozen].abs().max()) == 0.0 and float(w[~frozen].abs().min()) > 0.0
    s = torch.zeros(8, dtype=torch.float64, device="cuda")
    capi.check(capi.load().l3k_cheb_step(ctx._h, vp(r), vp(az), vp(minv), 0.3, 1.1, vp(w), vp(z), n, vp(s)))
    assert bool(torch.isfinite(s).all())  # ... nor <r, z>
    # the whole application, and a solve from a non-zero start
    cheb = solve.ChebyshevPreconditioner(mf, minv, degree=3, cond_est=COND, lambda_max=c["lmax"])
    cheb.apply(r, z)
    assert bool(torch.isfinite(z).all()) and float(z[frozen].abs().max()) == 0.0
    tol = 1e-9
    x0 = 0.1 * torch.randn(n, dtype=torch.float64, device="cuda", generator=gen)
    x = x0.clone()
    res = solve.pcg(mf, c["b"], x, precond=cheb, tol=tol, residual_scaling="rhs", max_iters=2000)
    assert res.converged and torch.equal(x[frozen], x0[frozen]) and not torch.equal(x[~frozen], x0[~frozen])
    ax = torch.empty_like(x)
    mf.apply(x[None, :], ax[None, :])
    true = float((c["b"] - ax)[~frozen].norm() / c["b"].norm())
    print(f"frozen rows: {res.num_iters} iterations, achieved {res.tol:.3e}, true residual on the live rows {true:.3e}")
    assert true <= tol
    # the power method leaves them out as well: an estimate, not NaN
    own = solve.ChebyshevPreconditioner(mf, minv, degree=2, max_power_iters=5)
    assert 0.0 < own.info.lambda_est < 2.0 * c["lmax"]


# ------------------------------------------------------------------------------------------------ 7. options and errors
def test_check_every_and_max_iters():
    c = case(D3, 3, 2, deterministic=True)
    mf, b = c["mf"], c["b"]
    cheb = solve.ChebyshevPreconditioner(mf, c["minv"], degree=2, cond_est=COND, lambda_max=c["lmax"])
    x1, x4 = torch.zeros_like(b), torch.zeros_like(b)
    r1 = solve.pcg(mf, b, x1, precond=cheb, tol=1e-8, residual_scaling="rhs")
    r4 = solve.pcg(mf, b, x4, precond=cheb, tol=1e-8, residual_scaling="rhs", check_every=4)
    assert r4.converged and r4.num_iters % 4 == 0 and r1.num_iters <= r4.num_iters < r1.num_iters + 4
    xs = torch.zeros_like(b)
    rs = solve.pcg(mf, b, xs, precond=cheb, tol=0.0, residual_scaling="rhs", max_iters=r4.num_iters, throw_on_fail=False)
    assert rs.num_iters == r4.num_iters and torch.equal(xs, x4) and rs.tol == r4.tol
    # max_iters that is no multiple of 4: the last iteration is checked as well
    xm, xe = torch.zeros_like(b), torch.zeros_like(b)
    rm = solve.pcg(mf, b, xm, precond=cheb, tol=0.0, residual_scaling="rhs", max_iters=6, check_every=4, throw_on_fail=False)
    re = solve.pcg(mf, b, xe, precond=cheb, tol=0.0, residual_scaling="rhs", max_iters=6, throw_on_fail=False)
    assert rm.num_iters == 6 and torch.equal(xm, xe) and rm.tol == re.tol
    x = torch.zeros_like(b)
    res = solve.pcg(mf, b, x, precond=cheb, tol=1e-10, residual_scaling="rhs", max_iters=3, throw_on_fail=False)
    assert res.converged is False and res.num_iters == 3 and res.tol > 1e-10
    ax = torch.empty_like(x)
    mf.apply(x[None, :], ax[None, :])
    assert abs(res.tol - float((b - ax).norm() / b.norm())) <= 1e-12  # achieved_tol is the residual of the x returned
    with pytest.raises(RuntimeError, match="failed to converge"):
        solve.pcg(mf, b, torch.zeros_like(b), precond=cheb, tol=1e-10, residual_scaling="rhs", max_iters=3)
    # a start vector that solves the system: no iteration, x untouched
    before = x1.clone()
    r0 = solve.pcg(mf, b, x1, precond=cheb, tol=1e-7, residual_scaling="rhs")
    assert r0.converged and r0.num_iters == 0 and torch.equal(x1, before)
    with pytest.raises(capi.L3KError, match="not both"):
        solve.pcg(mf, b, x1, c["minv"], precond=cheb)
    # r and z, b and x that share memory would give a silently wrong result: refused, nothing written
    v = x1.clone()
    with pytest.raises(capi.L3KError, match="do not overlap"):
        cheb.apply(v, v)
    two = torch.zeros(b.numel() + 2, dtype=torch.float64, device="cuda")
    with pytest.raises(capi.L3KError, match="do not overlap"):
        cheb.apply(two[:-2], two[2:])
    with pytest.raises(capi.L3KError, match="share memory"):
        solve.pcg(mf, v, v, precond=cheb)
    assert torch.equal(v, x1) and not two.any()


def test_error_paths():
    c = case(D3, 3, 2)
    mf, minv = c["mf"], c["minv"]
    for kw, msg in ((dict(degree=0), "degree < 1"), (dict(cond_est=1.0), "cond_est <= 1"), (dict(cond_est=float("nan")), "cond_est <= 1"),
                    (dict(boost_factor=0.99), "boost_factor < 1"), (dict(max_power_iters=0), "max_power_iters < 1"),
                    (dict(lambda_max=float("inf")), "lambda_max is not finite")):
        with pytest.raises(capi.L3KError, match="libl3k error -1: l3k_cheb_create: " + msg):
            solve.ChebyshevPreconditioner(mf, minv, **kw)
    # an operator or diagonal that is unusable: the estimate is negative
    with pytest.raises(capi.L3KError, match="libl3k error -1: l3k_cheb_create: the power method .* finite and positive"):
        solve.ChebyshevPreconditioner(mf, -minv, degree=2)
    lib, out = capi.load(), C.c_void_p()
    for args in ((None, vp(minv), None, C.byref(out)), (mf._h, None, None, C.byref(out)), (mf._h, vp(minv), None, None)):
        assert lib.l3k_cheb_create(*args) == -1 and lib.l3k_last_error().decode() == "l3k_cheb_create: null argument"
    # opts == NULL: the documented defaults
    assert lib.l3k_cheb_create(mf._h, vp(minv), None, C.byref(out)) == 0
    info = capi.ChebInfo()
    assert lib.l3k_cheb_info_get(out, C.byref(info)) == 0
    assert (info.degree, info.power_iters, info.applies_per_call) == (1, 10, 0) and info.lambda_max == 1.1 * info.lambda_est
    assert info.lambda_min == info.lambda_max / 30.0
    res, z = capi.CgResult(), torch.zeros_like(minv)
    assert lib.l3k_cheb_apply(out, None, vp(z)) == -1 and lib.l3k_last_error().decode() == "l3k_cheb_apply: null argument"
    assert lib.l3k_cheb_apply(out, vp(z), vp(z)) == -1 and lib.l3k_last_error().decode() == "l3k_cheb_apply: r and z overlap"
    assert lib.l3k_cheb_apply(out, vp(z[:-1]), vp(z[1:])) == -1 and lib.l3k_last_error().decode() == "l3k_cheb_apply: r and z overlap"
    assert lib.l3k_pcg_solve_cheb(mf._h, vp(c["b"]), vp(z), None, None, C.byref(res)) == -1
    assert lib.l3k_last_error().decode() == "l3k_pcg_solve_cheb: null argument"
    other = case(D3, 2, 4)
    assert lib.l3k_pcg_solve_cheb(other["mf"]._h, vp(other["b"]), vp(torch.zeros_like(other["b"])), out, None, C.byref(res)) == -1
    assert "another system" in lib.l3k_last_error().decode()
    assert lib.l3k_cheb_destroy(out) == 0
    # a mesh with ghost nodes: the single-rank object refuses it and says where to go
    part = system.CubePartition(4, 2, (2, 1, 1), 1, perturb=0.1)
    assert part.n_ghost_nodes > 0
    gmf = system.MatrixFreeSystem(system.DeviceMesh(c["ctx"], part, 4, part.dirichlet_mask(4)), D3, [1.0, 0.0])
    ones = torch.ones(part.n_owned_nodes * 4, dtype=torch.float64, device="cuda")
    with pytest.raises(capi.L3KError, match="libl3k error -1: l3k_cheb_create serves single-rank systems.*pcg_distributed"):
        solve.ChebyshevPreconditioner(gmf, ones, degree=2, lambda_max=2.0)


# ------------------------------------------------------------------------------------------------ 8. quads
def test_cheb_apply_on_a_quad_mesh():
    """The preconditioner sits above l3k_mf_apply and does not care about the element type: SquarePartition(3, 2) with
    KERNEL_DIFFUSION2D, degree 3, against the torch restatement driven by the device apply itself.  Bound 1e-13 relative L2: the
    two sides share every input and differ in the summation order of the applies' atomics and in FMA contraction, a few ulp per
    entry through coefficients of O(1)."""
    torch.cuda.set_device(0)
    ctx = system.Context(0, torch.cuda.current_stream().cuda_stream)
    U = system.kernel_info(system.KERNEL_DIFFUSION2D)["n_unknowns"]
    part = system.SquarePartition(3, 2, perturb=0.1)
    mf = system.MatrixFreeSystem(system.DeviceMesh(ctx, part, U, part.dirichlet_mask(U)), system.KERNEL_DIFFUSION2D)
    diag, _ = mf.diag_rhs(None)
    n = diag.numel()
    assert n == 49 * U
    minv = solve.jacobi_inverse_native(ctx, diag)
    cheb = solve.ChebyshevPreconditioner(mf, minv, degree=3, cond_est=COND)
    info = cheb.info
    assert info.power_iters == 10 and 0.0 < info.lambda_est < info.lambda_max
    r = torch.as_tensor(np.random.default_rng(8).standard_normal(n), device="cuda")
    z = torch.empty_like(r)
    cheb.apply(r, z)
    want = solve.chebyshev_reference(lambda v, out: mf.apply(v[None, :], out[None, :]), minv, r, info.lambda_max, COND, 3)
    print(f"quads: device against the torch restatement {rel(z, want):.3e}")
    assert rel(z, want) <= 1e-13 and float(z.norm()) > 0.0
