"""Boundary equation kernels in the assembled path: what the side systems add to l3k_assemble_global.  Diffusion3D (U = 4) on a
cube with Robin3D on all six faces, orders 2 and 4, at sizes where the domain assembly takes tens of milliseconds.

    python tools/bench_bnd_assembly.py [--out profiles/bnd_assembly.jsonl] [--cases 2:48,4:20] [--reps 5]

One process.  Per mesh one JSON line with the legs
  off        : MatrixFreeSystem.assemble_global with l3k_mf_assemble_boundary off -- the parent's domain-only assembly, the yardstick;
  on         : the same call with the switch on (domain route, then the side route over the attached term);
  standalone : BoundaryTerm.assemble_global over all sides into zeroed values.
After a warm-up of every leg the legs run alternately --reps times; the median per leg.  Reported: side matrices per second of the
standalone leg, the on / off time ratio next to the sides / elements ratio.  No pass mark: the numbers are written down."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
U = 4


def run_case(ctx, p, ne, reps):
    import torch
    from l3ster_amd import system
    part = system.CubePartition(ne, p)
    mask = part.dirichlet_mask(U, unknowns=(0,), sides=(4, 5))
    mesh = system.DeviceMesh(ctx, part, U, mask)
    mf = system.MatrixFreeSystem(mesh, system.KERNEL_DIFFUSION3D, [0.7, 1.3])
    fe, fs = part.boundary_sides()
    term = system.BoundaryTerm(mesh, system.KERNEL_ROBIN3D, fe, fs, kernel_params=[2.0, 1.0])
    mf.attach_boundary(term)
    g = mf.sparsity_graph()
    vals = torch.zeros(g.col_ind.numel(), dtype=torch.float64, device="cuda")
    rhs = torch.zeros((1, g.n), dtype=torch.float64, device="cuda")

    def leg(on, standalone=False):
        vals.zero_()
        rhs.zero_()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if standalone:
            missing = term.assemble_global(g.row_ptr, g.col_ind, vals, rhs)
        else:
            mf.assemble_boundary(on)
            missing = mf.assemble_global(g.row_ptr, g.col_ind, vals, rhs)
        torch.cuda.synchronize()
        assert missing == 0
        return time.perf_counter() - t0

    legs = {"off": lambda: leg(False), "on": lambda: leg(True), "standalone": lambda: leg(False, True)}
    for fn in legs.values():
        fn()
    ts = {k: [] for k in legs}
    for _ in range(reps):
        for k, fn in legs.items():
            ts[k].append(fn())
    sec = {k: float(np.median(v)) for k, v in ts.items()}
    return dict(kernel="Diffusion3D + Robin3D on six faces", order=p, mesh=f"{ne}^3", n_elems=part.n_elems, n_sides=len(fe), n=g.n,
                nnz=g.info.nnz, seconds=sec, side_matrices_per_s=len(fe) / sec["standalone"], elem_matrices_per_s=part.n_elems / sec["off"],
                on_over_off=sec["on"] / sec["off"], sides_over_elems=len(fe) / part.n_elems)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--cases", default="2:48,4:20")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch
    from l3ster_amd import system
    assert torch.cuda.is_available(), "bench_bnd_assembly.py measures on the GPU; there is no fallback"
    torch.cuda.set_device(0)
    ctx = system.Context(0, torch.cuda.current_stream().cuda_stream)
    out = open(a.out, "a") if a.out else None
    for case in a.cases.split(","):
        p, ne = case.split(":")
        line = json.dumps(run_case(ctx, int(p), int(ne), a.reps))
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()


if __name__ == "__main__":
    main()
