"""The triangular preconditioners (l3k_tri_*: SGS and ILU(0)) on matrices from the library's own assembly: an assembled quad system
(Diffusion2D, U = 3) and an assembled hex system (Diffusion3D, U = 4), both made with system.AssembledSystem, Dirichlet conditions
applied.

    python tools/bench_tri.py [--out profiles/tri.jsonl] [--cases quad:48:3,hex:10:2] [--reps 7]

One process.  Per system, one JSON line with
  (a) the levels, the launches of the default plan and the widest level, for both kinds;
  (b) the time of one l3k_tri_factor per kind;
  (c) the time of one l3k_tri_apply per kind next to one l3k_csr_apply, the legs run alternately --reps times after a warm-up,
      the median per leg;
  (d) PCG to 1e-10 |b| with Jacobi, Chebyshev(3)-Jacobi, SGS and ILU(0): iterations and seconds (median of 3 after a warm-up; the
      set-up -- power method, factor -- is not in the seconds).  Jacobi and Chebyshev run the library's existing entry points in
      this same process;
  (e) a sweep of fuse_rows: seconds of one apply (median) and of one factor (timed once after a warm-up) per value, ILU(0) and SGS.
The default of fuse_rows (256 / lanes_per_row, csrc/api_tri.hip) is to be judged from (e)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FUSE_SWEEP = (1, 4, 16, 64, 256, 1024, 1_000_000)


def alternate(legs, reps, inner=3):
    """legs: {name: fn}.  Every leg once as warm-up, then reps rounds of all legs in turn; {name: median seconds}"""
    import torch
    for fn in legs.values():
        fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in legs}
    for _ in range(reps):
        for k, fn in legs.items():
            t0 = time.perf_counter()
            for _ in range(inner):
                fn()
            torch.cuda.synchronize()
            ts[k].append((time.perf_counter() - t0) / inner)
    return {k: float(np.median(v)) for k, v in ts.items()}


def quad_system(ctx, ne, p):
    import torch
    from l3ster_amd import system
    U = 3
    part = system.SquarePartition(ne, p)
    mesh = system.DeviceMesh(ctx, part, U, part.dirichlet_mask(U, sides=(2, 3)))
    mf = system.MatrixFreeSystem(mesh, system.KERNEL_DIFFUSION2D)
    bnd = system.BoundaryTerm(mesh, system.KERNEL_ADIABATIC2D, *part.boundary_sides([0, 1]))
    n = part.n_local_nodes * U
    g = system.values_at_nodes(mesh, system.RESIDUAL_COORDX2D, [0], torch.zeros(n, dtype=torch.float64, device="cuda"),
                               face_elem=part.boundary_sides([2, 3])[0], face_side=part.boundary_sides([2, 3])[1])
    asm = system.AssembledSystem(mesh)
    return asm, asm.begin().add(mf).add(bnd).end(g[None, :]), "Diffusion2D"


def hex_system(ctx, ne, p):
    import torch
    from l3ster_amd import system
    U = 4
    part = system.CubePartition(ne, p, perturb=0.1)
    mask = part.dirichlet_mask(U)
    mesh = system.DeviceMesh(ctx, part, U, mask)
    mf = system.MatrixFreeSystem(mesh, system.KERNEL_DIFFUSION3D, [1.0, 0.0])
    n = part.n_local_nodes * U
    g = torch.as_tensor(np.where(np.asarray(mask).ravel()[:n] != 0, np.sin(0.37 * np.arange(n)), 0.0)[None, :], device="cuda")
    asm = system.AssembledSystem(mesh)
    return asm, asm.begin().add(mf).end(g), "Diffusion3D"


def run_case(ctx, kind, ne, p, reps):
    import torch
    from l3ster_amd import solve
    asm, op, kernel = (quad_system if kind == "quad" else hex_system)(ctx, ne, p)
    n, info = asm.n, op.info()
    b = asm.rhs[0].contiguous()
    r = torch.as_tensor(np.random.default_rng(0).standard_normal(n), device="cuda")
    z, y = torch.empty_like(r), torch.empty_like(r)
    rec = dict(kernel=kernel, mesh=f"{ne}^{2 if kind == 'quad' else 3}", order=p, n=n, nnz=info.nnz, mean_row_len=info.mean_row_len,
               max_row_len=info.max_row_len, lanes_per_row=info.lanes_per_row)
    pre, legs = {}, {"csr_apply": lambda: op.apply(r, y)}
    for k in ("sgs", "ilu0"):
        t0 = time.perf_counter()
        pre[k] = solve.TriangularPreconditioner(op, k)
        rec[f"{k}_create_seconds"] = time.perf_counter() - t0
        i = pre[k].info
        rec[f"{k}_plan"] = dict(n_levels_lower=i.n_levels_lower, n_levels_upper=i.n_levels_upper, max_level_rows=i.max_level_rows,
                                n_launches_lower=i.n_launches_lower, n_launches_upper=i.n_launches_upper, bytes=i.bytes)
        pre[k].factor()
        legs[f"{k}_factor"] = pre[k].factor
        legs[f"{k}_apply"] = lambda T=pre[k]: T.apply(r, z)
    rec["seconds"] = alternate(legs, reps)
    # PCG to 1e-10 |b|
    minv = op.jacobi_inverse()
    cheb = solve.ChebyshevPreconditioner(op, minv, degree=3)
    solves = dict(jacobi=dict(minv=minv), chebyshev3=dict(precond=cheb), sgs=dict(precond=pre["sgs"]), ilu0=dict(precond=pre["ilu0"]))
    rec["pcg"] = {}
    for name, kw in solves.items():
        ts = []
        for rep in range(4):
            x = torch.zeros(n, dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = solve.pcg(op, b, x, tol=1e-10, residual_scaling="rhs", max_iters=100_000, check_every=10, throw_on_fail=False, **kw)
            torch.cuda.synchronize()
            if rep:
                ts.append(time.perf_counter() - t0)
        rec["pcg"][name] = dict(iterations=res.num_iters, converged=res.converged, achieved_tol=res.tol, seconds=float(np.median(ts)))
    # the sweep of fuse_rows
    rec["fuse_rows_sweep"] = {}
    for k in ("sgs", "ilu0"):
        sweep = {}
        for fuse in FUSE_SWEEP:
            T = solve.TriangularPreconditioner(op, k, fuse_rows=fuse).factor()  # (the warm-up of the factorisation)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            T.factor()  # timed once: a factorisation fused into one workgroup takes seconds (factor synchronises itself)
            t_factor = time.perf_counter() - t0
            t = alternate({"apply": lambda T=T: T.apply(r, z)}, max(3, reps // 2))
            sweep[str(fuse)] = dict(n_launches_lower=T.info.n_launches_lower, n_launches_upper=T.info.n_launches_upper,
                                    apply_seconds=t["apply"], factor_seconds=t_factor)
            T.close()
        rec["fuse_rows_sweep"][k] = sweep
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--cases", default="quad:48:3,hex:10:2")
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    import torch
    from l3ster_amd import system
    assert torch.cuda.is_available(), "bench_tri.py measures on the GPU; there is no fallback"
    torch.cuda.set_device(0)
    ctx = system.Context(0, torch.cuda.current_stream().cuda_stream)
    out = open(a.out, "a") if a.out else None
    for case in a.cases.split(","):
        kind, ne, p = case.split(":")
        line = json.dumps(run_case(ctx, kind, int(ne), int(p), a.reps))
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()


if __name__ == "__main__":
    main()
