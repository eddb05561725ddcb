"""Static condensation on quads inside the assembled system against the full assembled system on the same mesh.

    python tools/bench_quad_condense.py [--out profiles/quad_condense.jsonl] [--ne 256] [--orders 4,6] [--reps 5] [--tol 1e-10]

One process, Diffusion2D (U = 3) on an ne x ne quad mesh, Adiabatic2D on the sides y = 0 and y = 1, Dirichlet T = x on the sides
x = 0 and x = 1.  Per order two JSON lines, one for AssembledSystem(condensation="element_boundary") and one for the full
AssembledSystem: after one untimed round the median of --reps rounds of begin + adds + end, split into its phases (begin, the
domain add, the boundary add, end -- on the condensed system the adds end in the split kernel and end starts with the elimination
kernel), the nnz, the Jacobi-PCG iterations and time to --tol (residual scaled by the rhs), and on the condensed system the median
time of recover.  The phases are host-timed around synchronised calls; the per-kernel shares come from a kernel trace of this tool
(profiles/README.md)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
U = 3


def timed(f):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = f()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def one_system(ctx, mesh, part, mf, bnd, g, condensation, reps, tol, max_iters):
    import torch
    from l3ster_amd import solve, system
    t_create, asm = timed(lambda: system.AssembledSystem(mesh, condensation=condensation))
    phases = {k: [] for k in ("begin", "add_domain", "add_boundary", "end", "total")}
    op = None
    for rep in range(reps + 1):  # (the first round is not timed: workspace allocation, operator creation)
        tb, _ = timed(asm.begin)
        td, _ = timed(lambda: asm.add(mf))
        ts, _ = timed(lambda: asm.add(bnd))
        te, op = timed(lambda: asm.end(g))
        if rep:
            for k, v in zip(phases, (tb, td, ts, te, tb + td + ts + te)):
                phases[k].append(v)
    x = torch.zeros(asm.n, dtype=torch.float64, device="cuda")
    minv = op.jacobi_inverse()
    t_pcg, res = timed(lambda: solve.pcg(op, asm.rhs[0], x, minv, tol=tol, residual_scaling="rhs", max_iters=max_iters,
                                         throw_on_fail=False))
    line = dict(what="quad_condense", condensation=condensation, order=part.order, n_elems=part.n_elems, n=asm.n, nnz=asm.nnz,
                n_missing=asm.info.n_missing, create_seconds=t_create, reps=reps, tol=tol, pcg_iterations=res.num_iters,
                pcg_converged=bool(res.converged), pcg_achieved=res.tol, pcg_seconds=t_pcg)
    line.update({k + "_seconds": float(np.median(v)) for k, v in phases.items()})
    if condensation != "none":
        ci = asm.cond_info
        line.update(store_bytes=ci.store_bytes, n_failed=ci.n_failed)
        ts = []
        for _ in range(reps + 1):
            ts.append(timed(lambda: asm.recover(x))[0])
        line["recover_seconds"] = float(np.median(ts[1:]))
    fields = x.view(-1, U).T.contiguous()
    line["l2_error"] = float(np.linalg.norm(system.norm_l2(mesh, system.RESIDUAL_LINEAR2D_ERROR, fields)))
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "quad_condense.jsonl"))
    ap.add_argument("--ne", type=int, default=256)
    ap.add_argument("--orders", default="4,6")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--tol", type=float, default=1e-10)
    ap.add_argument("--max-iters", type=int, default=100000)
    ap.add_argument("--append", action="store_true")
    a = ap.parse_args()
    import torch
    from l3ster_amd import system
    torch.cuda.set_device(0)
    ctx = system.Context(0, torch.cuda.current_stream().cuda_stream)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a" if a.append else "w") as f:
        for p in (int(s) for s in a.orders.split(",")):
            part = system.SquarePartition(a.ne, p)
            mesh = system.DeviceMesh(ctx, part, U, part.dirichlet_mask(U, sides=(2, 3)))
            mf = system.MatrixFreeSystem(mesh, system.KERNEL_DIFFUSION2D)
            bnd = system.BoundaryTerm(mesh, system.KERNEL_ADIABATIC2D, *part.boundary_sides([0, 1]))
            n = part.n_local_nodes * U
            fe, fs = part.boundary_sides([2, 3])
            g = system.values_at_nodes(mesh, system.RESIDUAL_COORDX2D, [0], torch.zeros(n, dtype=torch.float64, device="cuda"),
                                       face_elem=fe, face_side=fs)[None, :]
            for condensation in ("element_boundary", "none"):
                line = one_system(ctx, mesh, part, mf, bnd, g, condensation, a.reps, a.tol, a.max_iters)
                line.update(ne=a.ne, device=torch.cuda.get_device_name(0))
                f.write(json.dumps(line) + "\n")
                f.flush()
                print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
