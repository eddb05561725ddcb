#!/usr/bin/env python
"""bench_quad.py -- throughput of the quad (2-D) matrix-free Diffusion2D apply on one MI355X.

    python tools/bench_quad.py [--orders 2 4 6] [--dofs 2e8] [--reps 20] [--out profiles/quad_apply.jsonl] [--boundary]

Per order: a square mesh of about --dofs dofs (2048^2 elements at p = 4 = 201 M dofs), perturbed vertices, T Dirichlet on the
four sides, x ~ U(-1, 1).  Warm-up until two consecutive element-kernel times agree to 1 %, then the median of --reps timed
element launches (l3k_mf_apply_elems, which = 2) and of --reps whole applies (scale + element kernel + Dirichlet rows).
Whole-vector parity against the CPU oracle (orc_mf_apply) runs on a 64^2-element mesh of the same order.  One JSON line per
order goes to stdout and to --out.  --boundary attaches the Adiabatic2D boundary term on the sides y = 0 and y = 1 (so the applies
include the side kernel) and also times the side kernel alone (l3k_bnd_apply over all its sides); default --out then
profiles/quad_boundary.jsonl.

Bytes/dof model (algorithmic minimum of one apply, every array streamed once): x read 8 B + y written 8 B per dof, the element
connectivity 4 (p+1)^2 B and the 4 vertices 96 B per element over p^2 U dofs per element, the Dirichlet mask 1 B per dof.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from l3ster_amd import system  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec
U = 3


def bytes_per_dof(p):
    return 16.0 + 1.0 + (4.0 * (p + 1) ** 2 + 96.0) / (p * p * U)


def timed(fn, reps):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = []
    for _ in range(reps):
        start.record()
        fn()
        end.record()
        end.synchronize()
        out.append(start.elapsed_time(end))
    return out


def parity(ctx, p):
    import oracle_lib as O
    from helpers import rel_err
    part = system.SquarePartition(64, p, perturb=0.1)
    mask = part.dirichlet_mask(U)
    mf = system.MatrixFreeSystem(system.DeviceMesh(ctx, part, U, mask), system.KERNEL_DIFFUSION2D)
    x = part.synthetic_vector(U)
    Y = torch.zeros((1, x.shape[1]), dtype=torch.float64, device="cuda")
    mf.apply(torch.as_tensor(x, device="cuda"), Y)
    torch.cuda.synchronize()
    om = O.MeshView(2, p, p + 1, part.elem_nodes, part.elem_verts, part.n_local_nodes, U, np.arange(U), mask)
    return rel_err(Y.cpu().numpy().T, O.mf_apply(om, O.KERNEL_DIFFUSION2D, x.T, nthreads=16))


def run(ctx, p, target_dofs, reps, boundary=False):
    ne = max(1, int(round((target_dofs / U) ** 0.5 / p)))
    part = system.SquarePartition(ne, p, perturb=0.1)
    n_dofs = part.n_owned_nodes * U
    mesh = system.DeviceMesh(ctx, part, U, part.dirichlet_mask(U))
    mf = system.MatrixFreeSystem(mesh, system.KERNEL_DIFFUSION2D)
    term = None
    if boundary:
        term = system.BoundaryTerm(mesh, system.KERNEL_ADIABATIC2D, *part.boundary_sides([0, 1]))
        mf.attach_boundary(term)
    X = torch.rand((1, n_dofs), dtype=torch.float64, device="cuda") * 2 - 1
    Y = torch.zeros_like(X)
    elems = lambda: mf.apply_elems(2, X, None, Y, None, 1.0, 1.0)  # noqa: E731 (beta = 1: the rows need no scaling pass)
    whole = lambda: mf.apply(X, Y, 1.0, 0.0)  # noqa: E731
    prev, n_warm = None, 0
    while n_warm < 200:
        t = statistics.median(timed(elems, 3))
        n_warm += 3
        if prev is not None and abs(t - prev) <= 0.01 * prev:
            break
        prev = t
    t_elem = statistics.median(timed(elems, reps))
    timed(whole, 3)
    t_whole = statistics.median(timed(whole, reps))
    bpd = bytes_per_dof(p)
    extra = {}
    if term is not None:
        sides = lambda: term.apply(X, Y, 1.0)  # noqa: E731
        timed(sides, 3)
        t_side = statistics.median(timed(sides, reps))
        extra = dict(boundary="adiabatic2d on sides 0, 1", n_sides=term.n_faces, side_kernel_ms=t_side,
                     side_share_of_apply=t_side / t_whole)
    return dict(kernel="diffusion2d", order=p, ne=[ne, ne], n_elems=part.n_elems, dofs=n_dofs, reps=reps, warmup_applies=n_warm,
                element_kernel_ms=t_elem, whole_apply_ms=t_whole, dofs_per_s=n_dofs / (t_whole * 1e-3),
                element_dofs_per_s=n_dofs / (t_elem * 1e-3), bytes_per_dof_model=bpd,
                hbm_fraction=n_dofs * bpd / (t_whole * 1e-3) / (HBM_PEAK_GBS * 1e9), route=mf.route(),
                parity_rel_err_64x64=parity(ctx, p), **extra)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--orders", type=int, nargs="+", default=[2, 4, 6])
    ap.add_argument("--dofs", type=float, default=2.0e8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--boundary", action="store_true", help="attach Adiabatic2D on sides 0 and 1 and time the side kernel")
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "quad_boundary.jsonl" if a.boundary else "quad_apply.jsonl")
    torch.cuda.set_device(0)
    ctx = system.Context(0, torch.cuda.current_stream().cuda_stream)
    lines = []
    for p in a.orders:
        rec = run(ctx, p, a.dofs, a.reps, a.boundary)
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
