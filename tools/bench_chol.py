"""The band Cholesky solver (solve.CholeskySolver) against Jacobi-PCG on the assembled Diffusion2D system, full and condensed.

    python tools/bench_chol.py [--out profiles/chol.jsonl] [--ne 16,32,64] [--order 4] [--reps 3] [--tol 1e-10] [--kernel-stats FILE]

One process, Diffusion2D (U = 3) on ne x ne quads (SquarePartition), Adiabatic2D on the sides y = 0 and y = 1, Dirichlet T = x on the
sides x = 0 and x = 1.  Per size two JSON lines, AssembledSystem(condensation="element_boundary") and the full system: the host time
of the symbolic phase (creation), the median over --reps of factor and of solve (host-timed around synchronised calls; one untimed
round first), the sizes of the factor (block, block columns, largest H, bytes, flops and the share of the trailing updates), the
backward error ||b - A x|| / ||b|| through the operator's apply, and Jacobi-PCG to --tol (residual scaled by the rhs) on the same
system.  factor_flops_per_s counts every flop of the factorisation over the whole factor time -- a LOWER bound of what the
matrix-core kernel achieves, since the diagonal and panel launches are in the time.  The kernel's own rate needs a kernel trace:
run this tool for ONE size under `rocprofv3 --kernel-trace --stats`, then again with --kernel-stats <the kernel stats csv>: the
last line then divides the update flops of all factorisations of the run by the total time of cholUpdateKernel and sets it
against the FP64 matrix peak."""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
U = 3
FP64_MFMA_PEAK = 78.6e12  # AMD's figure for the MI355X, FLOP/s


def timed(f):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = f()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def one_system(mesh, part, g, condensation, reps, tol, max_iters, max_bytes):
    import torch
    from l3ster_amd import solve, system
    asm = system.AssembledSystem(mesh, condensation=condensation).begin()
    asm.add(system.MatrixFreeSystem(mesh, system.KERNEL_DIFFUSION2D))
    asm.add(system.BoundaryTerm(mesh, system.KERNEL_ADIABATIC2D, *part.boundary_sides([0, 1])))
    op = asm.end(g)
    b = asm.rhs[0]
    line = dict(what="chol", condensation=condensation, order=part.order, n_elems=part.n_elems, n=asm.n, nnz=asm.nnz, reps=reps)
    t_sym, chol = timed(lambda: solve.CholeskySolver(op, max_bytes=max_bytes))
    info = chol.info
    line.update(symbolic_seconds=t_sym, n_active=info.n_active, block=info.block, n_blocks=info.n_blocks, max_height=info.max_height,
                factor_bytes=info.factor_bytes, factor_flops=info.factor_flops, update_flops=info.update_flops)
    x = torch.zeros(asm.n, dtype=torch.float64, device="cuda")
    tf, ts = [], []
    for _ in range(reps + 1):
        tf.append(timed(chol.factor)[0])
        ts.append(timed(lambda: chol.solve(b, x))[0])
    y = torch.zeros_like(x)
    op.apply(x, y)
    line.update(factor_seconds=float(np.median(tf[1:])), solve_seconds=float(np.median(ts[1:])), n_factorisations=reps + 1,
                residual=(b - y).norm().item() / b.norm().item())
    line["factor_flops_per_s"] = info.factor_flops / line["factor_seconds"]
    line["fraction_of_fp64_matrix_peak"] = line["factor_flops_per_s"] / FP64_MFMA_PEAK
    if condensation != "none":
        asm.recover(x)
    fields = x.view(-1, U).T.contiguous()
    line["l2_error"] = float(np.linalg.norm(system.norm_l2(mesh, system.RESIDUAL_LINEAR2D_ERROR, fields)))
    chol.close()
    xp = torch.zeros(asm.n, dtype=torch.float64, device="cuda")
    t_pcg, res = timed(lambda: solve.pcg(op, b, xp, op.jacobi_inverse(), tol=tol, residual_scaling="rhs", max_iters=max_iters,
                                         throw_on_fail=False))
    line.update(pcg_tol=tol, pcg_iterations=res.num_iters, pcg_converged=bool(res.converged), pcg_achieved=res.tol, pcg_seconds=t_pcg)
    return line


def update_kernel_seconds(path):
    with open(path, newline="") as f:
        return sum(int(row["TotalDurationNs"]) for row in csv.DictReader(f) if "cholUpdateKernel" in row["Name"]) * 1e-9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chol.jsonl"))
    ap.add_argument("--ne", default="16,32,64")
    ap.add_argument("--order", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--tol", type=float, default=1e-10)
    ap.add_argument("--max-iters", type=int, default=100000)
    ap.add_argument("--max-bytes", type=int, default=0)
    ap.add_argument("--kernel-stats", default=None, help="kernel stats csv of a rocprofv3 --kernel-trace --stats run of this tool with the same arguments")
    ap.add_argument("--append", action="store_true")
    a = ap.parse_args()
    import torch
    from l3ster_amd import system
    torch.cuda.set_device(0)
    ctx = system.Context(0, torch.cuda.current_stream().cuda_stream)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    update_flops = 0.0
    with open(a.out, "a" if a.append else "w") as f:
        def emit(line):
            line.update(device=torch.cuda.get_device_name(0))
            f.write(json.dumps(line) + "\n")
            f.flush()
            print(json.dumps(line), flush=True)

        for ne in (int(s) for s in a.ne.split(",")):
            part = system.SquarePartition(ne, a.order)
            mesh = system.DeviceMesh(ctx, part, U, part.dirichlet_mask(U, sides=(2, 3)))
            n = part.n_local_nodes * U
            fe, fs = part.boundary_sides([2, 3])
            g = system.values_at_nodes(mesh, system.RESIDUAL_COORDX2D, [0], torch.zeros(n, dtype=torch.float64, device="cuda"),
                                       face_elem=fe, face_side=fs)[None, :]
            for condensation in ("element_boundary", "none"):
                line = one_system(mesh, part, g, condensation, a.reps, a.tol, a.max_iters, a.max_bytes)
                line.update(ne=ne)
                update_flops += line["update_flops"] * line["n_factorisations"]
                emit(line)
        if a.kernel_stats:
            t = update_kernel_seconds(a.kernel_stats)
            emit(dict(what="chol_update_kernel", ne=a.ne, order=a.order, update_flops_executed=update_flops, kernel_seconds=t,
                      flops_per_s=update_flops / t if t > 0 else None,
                      fraction_of_fp64_matrix_peak=update_flops / t / FP64_MFMA_PEAK if t > 0 else None))


if __name__ == "__main__":
    main()
