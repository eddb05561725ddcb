"""Jacobi-PCG and Chebyshev-PCG against PCG with the p-multigrid preconditioner (l3k_pcg_solve_pmg), one GPU, same process: time to
tolerance, outer iterations and fine-level applies per leg, and where the time of one V-cycle goes.
    python tools/bench_pmg.py [--ne5 64] [--ne6 32] [--tol 1e-6] [--repeats 3] [--cycle-reps 10]
Problems, at the sizes of tools/bench_chebyshev.py: BASELINE.json config 5 (advection-diffusion, order 4, levels 4 -> 2 -> 1) and
Diffusion3D at order 6 with a source term (levels 6 -> 3 -> 1).  Config 5's velocity field is evaluated at node_coords() on every
level (tools/bench_chebyshev.py evaluates it at the uniform grid index of the node: nearly, not exactly, the same fine problem, so
compare the legs of this tool with each other, not with that tool's).  The levels are CubePartition's of one perturbed mesh at the
level's order, paired by system.match_elements.  Legs: Jacobi (l3k_pcg_solve), Chebyshev degree --cheb-degree (l3k_pcg_solve_cheb)
and p-multigrid with Chebyshev smoothers (--smooth-degree / --smooth-cond-est on every level but the last, --coarse-degree /
--coarse-cond-est on the last; every lambda_max from the power method of l3k_cheb_create).  Every leg is run once untimed, then
--repeats times alternating with the other legs of its problem; the time reported is the median of a host clock around the solve,
which ends in a stream synchronise.  Building the hierarchy (meshes, diagonals, power methods, ownership tables) is timed apart
(create_s): a solve that reuses the preconditioner does not pay it again.

Shares of a cycle.  The pieces of one V-cycle that have an entry point of their own -- the smoother of each level (l3k_cheb_apply),
the operator apply behind each `d = r - A z` (l3k_mf_apply), the restriction and the prolongation of each pair -- are timed one by
one between two HIP events (--cycle-reps calls each, after one untimed call) and multiplied by how often a cycle runs them; the
whole cycle (l3k_pmg_apply) is timed the same way.  `rest` is a difference, not a measurement: the cycle minus the sum of the pieces.
It stands for the `d = r - A z` and `z += e` vector kernels, but every piece timed alone also carries the host's cost of one call
through Python and ctypes, which the cycle pays once, so on small problems `rest` can come out negative; read it only at sizes where
a piece takes far longer than a launch.  One JSON line per leg on stdout and in profiles/pmg.jsonl (--out)."""
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
ap.add_argument("--check-every", type=int, default=10, help="of the Jacobi and Chebyshev legs")
ap.add_argument("--check-every-pmg", type=int, default=1, help="of the p-multigrid leg: a cycle costs several applies, a check 32 bytes")
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--cycle-reps", type=int, default=10)
ap.add_argument("--cheb-degree", type=int, default=3)
ap.add_argument("--cond-est", type=float, default=30.0, help="of the Chebyshev leg")
ap.add_argument("--smooth-degree", type=int, default=3)
ap.add_argument("--smooth-cond-est", type=float, default=20.0)
ap.add_argument("--coarse-degree", type=int, default=8)
ap.add_argument("--coarse-cond-est", type=float, default=400.0)
ap.add_argument("--max-iters", type=int, default=20000)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pmg.jsonl"))
a = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_pmg.py measures on the GPU: no device found")
torch.cuda.set_device(0)
ctx = system.Context(0, torch.cuda.current_stream().cuda_stream)
U = 4


def config5_level(ne, p):
    part = system.CubePartition(ne, p, perturb=0.1)
    mf = system.MatrixFreeSystem(system.DeviceMesh(ctx, part, U, part.dirichlet_mask(U)), system.KERNEL_ADVDIFF3D, [1.0, 0.5, 1.0])
    # the velocity field at the nodes' physical coordinates: every level samples ONE coefficient function, so the coarse operators
    # are rediscretisations of the fine one (a grid index in its place would shift with the GLL spacing of the order)
    gx, gy, gz = torch.as_tensor(part.node_coords(), device="cuda").T
    mf.set_fields(torch.stack([0.5 * torch.sin(np.pi * gy), 0.25 * torch.cos(np.pi * gx), 0.1 * gz]).contiguous())
    return part, mf


def diffusion_level(ne, p):
    part = system.CubePartition(ne, p, perturb=0.1)
    return part, system.MatrixFreeSystem(system.DeviceMesh(ctx, part, U, part.dirichlet_mask(U)), system.KERNEL_DIFFUSION3D, [1.0, 1.0])


def hierarchy(make_level, ne, orders):
    """[(part, mf, minv, rhs)] per level, finest first, and the p-multigrid on them"""
    out, levels = [], []
    for i, p in enumerate(orders):
        part, mf = make_level(ne, p)
        diag, rhs = mf.diag_rhs(None)  # homogeneous Dirichlet values
        minv = solve.jacobi_inverse_native(ctx, diag)
        last = i + 1 == len(orders)
        cheb = solve.ChebyshevPreconditioner(mf, minv, degree=a.coarse_degree if last else a.smooth_degree,
                                             cond_est=a.coarse_cond_est if last else a.smooth_cond_est)
        levels.append((mf, cheb, system.match_elements(out[-1][0], part) if i else None))
        out.append((part, mf, minv, rhs[0].contiguous()))
    return out, solve.PMultigrid(levels)


def timed_solve(mf, b, minv, precond):
    x = torch.zeros_like(b)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = solve.pcg(mf, b, x, None if precond is not None else minv, tol=a.tol, residual_scaling="rhs", max_iters=a.max_iters,
                    check_every=a.check_every_pmg if isinstance(precond, solve.PMultigrid) else a.check_every, throw_on_fail=False,
                    precond=precond)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, res, x


def event_ms(call):
    """milliseconds of one `call` between two HIP events, the mean of --cycle-reps calls after one untimed call"""
    call()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(a.cycle_reps):
        call()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / a.cycle_reps


def cycle_shares(data, pm):
    """{piece: ms per cycle} and the whole cycle's ms"""
    n_levels = len(data)
    vec = [[torch.randn(minv.numel(), dtype=torch.float64, device="cuda") * (minv != 0) for _ in range(2)] for _, _, minv, _ in data]
    pieces = {}
    for l, (_, mf, _, _) in enumerate(data):
        r, z = vec[l]
        last = l + 1 == n_levels
        cheb = pm.levels[l][1]
        pieces[f"smoother_level{l}"] = (1 if last else 2) * event_ms(lambda: cheb.apply(r, z))
        if not last:
            pieces[f"residual_apply_level{l}"] = 2 * event_ms(lambda: mf.apply(r[None, :], z[None, :]))
            pieces[f"restrict_{l}_to_{l + 1}"] = event_ms(lambda: pm.restrict(l + 1, r, vec[l + 1][0]))
            pieces[f"prolong_{l + 1}_to_{l}"] = event_ms(lambda: pm.prolong(l + 1, vec[l + 1][0], z, add=True))
    r, z = vec[0]
    total = event_ms(lambda: pm.apply(r, z))
    pieces["rest"] = total - sum(pieces.values())
    return pieces, total


lines = []
for name, make_level, ne, orders in (("config 5: advection-diffusion 3D (F=3 fields)", config5_level, a.ne5, (4, 2, 1)),
                                     ("Diffusion3D with a source", diffusion_level, a.ne6, (6, 3, 1))):
    name = f"{name}, hex {ne}^3, order {orders[0]}"
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    data, pm = hierarchy(make_level, ne, orders)
    torch.cuda.synchronize()
    pmg_create_s = time.perf_counter() - t0
    _, mf, minv, b = data[0]
    t0 = time.perf_counter()
    cheb = solve.ChebyshevPreconditioner(mf, minv, degree=a.cheb_degree, cond_est=a.cond_est)  # (synchronises: it reads the estimate back)
    legs = {"jacobi": (None, 0.0), f"chebyshev degree {a.cheb_degree}": (cheb, time.perf_counter() - t0),
            "p-multigrid " + " -> ".join(map(str, orders)): (pm, pmg_create_s)}
    for leg, (c, _) in legs.items():  # warm-up: every leg once, untimed
        timed_solve(mf, b, minv, c)
    times, last = {leg: [] for leg in legs}, {}
    for _ in range(a.repeats):  # alternating: a drift of the machine touches every leg alike
        for leg, (c, _) in legs.items():
            dt, res, x = timed_solve(mf, b, minv, c)
            times[leg].append(dt)
            last[leg] = (res, x)
    pieces, cycle_ms = cycle_shares(data, pm)
    info = pm.info()
    ax = torch.empty_like(b)
    t_jac = statistics.median(times["jacobi"])
    for leg, (c, create_s) in legs.items():
        res, x = last[leg]
        mf.apply(x[None, :], ax[None, :])
        is_pmg = c is pm
        # fine-level applies: one for the initial residual, one per iteration, and the preconditioner's, which runs before the first
        # and between the iterations, not after the last
        per_iter = 1 + (0 if c is None else info.applies_per_cycle[0] if is_pmg else c.info.applies_per_call)
        t = statistics.median(times[leg])
        line = {"problem": name, "dofs": b.numel(), "leg": leg, "tol": a.tol,
                "check_every": a.check_every_pmg if is_pmg else a.check_every, "converged": res.converged, "achieved_tol": res.tol,
                "true_residual_over_rhs": float((b - ax).norm() / b.norm()), "outer_iterations": res.num_iters,
                "fine_applies": 1 + res.num_iters * per_iter if res.num_iters else 1, "solve_s_median": t, "solve_s_min": min(times[leg]),
                "solve_s_max": max(times[leg]), "repeats": a.repeats, "speedup_over_jacobi": t_jac / t}
        if c is not None:
            line["create_s"] = create_s
        if is_pmg:
            line.update({"orders": info.order, "level_dofs": info.n_dofs, "applies_per_cycle": info.applies_per_cycle,
                         "lambda_max": [lv[1].info.lambda_max for lv in pm.levels],
                         "smoothers": {"degree": a.smooth_degree, "cond_est": a.smooth_cond_est, "coarse_degree": a.coarse_degree,
                                       "coarse_cond_est": a.coarse_cond_est},
                         "cycle_ms": cycle_ms, "cycle_reps": a.cycle_reps, "cycle_ms_by_piece": pieces,
                         "cycle_share_by_piece": {k: v / cycle_ms for k, v in pieces.items()}})
        elif c is not None:
            line.update({"lambda_max": c.info.lambda_max, "cond_est": a.cond_est})
        lines.append(line)
        print(json.dumps(line), flush=True)
    del pm, cheb, legs, last, data  # (the next problem's vectors take their place)
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    for line in lines:
        f.write(json.dumps(line) + "\n")
