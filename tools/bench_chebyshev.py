"""Jacobi-PCG against PCG with the matrix-free Chebyshev-Jacobi preconditioner (l3k_pcg_solve_cheb), one GPU, same process:
time to tolerance, outer iterations and total operator applies per leg.
    python tools/bench_chebyshev.py [--ne5 64] [--ne6 32] [--tol 1e-6] [--repeats 3] [--degrees 2 3 4 6]
Problems: BASELINE.json config 5 (advection-diffusion, order 4, as tools/bench_config5.py states it) and Diffusion3D at order 6
with a source term.  Legs: Jacobi (l3k_pcg_solve) and degree d in --degrees.  Every leg is run once untimed (code objects, the
context's workspaces), then --repeats times alternating with the other legs of its problem; the time reported is the median of
a host clock around the solve, which ends in a stream synchronise.  The power method of l3k_cheb_create is timed apart
(create_s) and its applies are counted (power_applies): a solve that reuses the preconditioner does not pay them again.
One JSON line per leg on stdout and in profiles/chebyshev.jsonl (--out)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from l3ster_amd import solve, system  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--ne5", type=int, default=64, help="elements per edge of the config-5 problem (order 4)")
ap.add_argument("--ne6", type=int, default=32, help="elements per edge of the Diffusion3D problem (order 6)")
ap.add_argument("--tol", type=float, default=1e-6)
ap.add_argument("--check-every", type=int, default=10)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--degrees", type=int, nargs="*", default=[2, 3, 4, 6])
ap.add_argument("--cond-est", type=float, default=30.0)
ap.add_argument("--max-iters", type=int, default=20000)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chebyshev.jsonl"))
a = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_chebyshev.py measures on the GPU: no device found")
torch.cuda.set_device(0)
ctx = system.Context(0, torch.cuda.current_stream().cuda_stream)
U = 4


def config5(ne):
    p, kid = 4, system.KERNEL_ADVDIFF3D
    part = system.CubePartition(ne, p, perturb=0.1)
    mf = system.MatrixFreeSystem(system.DeviceMesh(ctx, part, U, part.dirichlet_mask(U)), kid, [1.0, 0.5, 1.0])  # k, sigma, s
    N = p * ne + 1
    gid = torch.as_tensor(part.node_grid_id, device="cuda")
    gx, gy, gz = (gid % N).double() / (N - 1), ((gid // N) % N).double() / (N - 1), (gid // (N * N)).double() / (N - 1)
    mf.set_fields(torch.stack([0.5 * torch.sin(np.pi * gy), 0.25 * torch.cos(np.pi * gx), 0.1 * gz]).contiguous())
    return f"config 5: advection-diffusion 3D (F=3 fields), hex {ne}^3, order {p}", mf


def diffusion6(ne):
    p = 6
    part = system.CubePartition(ne, p, perturb=0.1)
    mf = system.MatrixFreeSystem(system.DeviceMesh(ctx, part, U, part.dirichlet_mask(U)), system.KERNEL_DIFFUSION3D, [1.0, 1.0])
    return f"Diffusion3D with a source, hex {ne}^3, order {p}", mf


def timed_solve(mf, b, minv, precond):
    x = torch.zeros_like(b)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = solve.pcg(mf, b, x, None if precond is not None else minv, tol=a.tol, residual_scaling="rhs", max_iters=a.max_iters,
                    check_every=a.check_every, throw_on_fail=False, precond=precond)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, res, x


lines = []
for name, mf in (config5(a.ne5), diffusion6(a.ne6)):
    diag, rhs = mf.diag_rhs(None)  # homogeneous Dirichlet values
    minv = solve.jacobi_inverse_native(ctx, diag)
    b = rhs[0].contiguous()
    legs = {"jacobi": (None, 0.0)}
    for d in a.degrees:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        c = solve.ChebyshevPreconditioner(mf, minv, degree=d, cond_est=a.cond_est)  # (synchronises: it reads the estimate back)
        legs[f"chebyshev degree {d}"] = (c, time.perf_counter() - t0)
    for leg, (c, _) in legs.items():  # warm-up: every leg once, untimed
        timed_solve(mf, b, minv, c)
    times, last = {leg: [] for leg in legs}, {}
    for _ in range(a.repeats):  # alternating: a drift of the machine touches every leg alike
        for leg, (c, _) in legs.items():
            dt, res, x = timed_solve(mf, b, minv, c)
            times[leg].append(dt)
            last[leg] = (res, x)
    ax = torch.empty_like(b)
    t_jac = statistics.median(times["jacobi"])
    for leg, (c, create_s) in legs.items():
        res, x = last[leg]
        mf.apply(x[None, :], ax[None, :])
        info = c.info if c is not None else None
        per_iter = 1 + (info.applies_per_call if c is not None else 0)
        # one apply for the initial residual; the preconditioner runs before the first and between the iterations, not after the last
        applies = 1 + res.num_iters * per_iter if res.num_iters else 1
        t = statistics.median(times[leg])
        lines.append({"problem": name, "dofs": b.numel(), "leg": leg, "tol": a.tol, "check_every": a.check_every,
                      "converged": res.converged, "achieved_tol": res.tol, "true_residual_over_rhs": float((b - ax).norm() / b.norm()),
                      "outer_iterations": res.num_iters, "applies": applies, "solve_s_median": t, "solve_s_min": min(times[leg]),
                      "solve_s_max": max(times[leg]), "repeats": a.repeats, "speedup_over_jacobi": t_jac / t,
                      **({"lambda_max": info.lambda_max, "lambda_est": info.lambda_est, "cond_est": a.cond_est, "create_s": create_s,
                          "power_applies": info.power_iters} if c is not None else {})})
        print(json.dumps(lines[-1]), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    for line in lines:
        f.write(json.dumps(line) + "\n")
