"""What a sum of matrix-free terms (system.MultiTermSystem, l3k_mfs_*) costs next to a single MatrixFreeSystem: inside a sum no term
writes the rows of its element-internal nodes (every row is accumulated), and the scale pass covers every row.

    python tools/bench_multiterm.py [--out profiles/multiterm.jsonl] [--cases 4:64,6:48] [--reps 9]

One process, the method of tools/bench_csr.py: every leg once as a warm-up, then --reps rounds of all legs in turn, 50 applies per
timing, wall clock around work that ends in a synchronise, the median per leg.  Per case (order:elements per direction) of
Diffusion3D (U = 4) on a perturbed cube, y <- A x (alpha = 1, beta = 0), one JSON line with the legs
  (a) single      l3k_mf_apply of the one term on the whole mesh: fused stores of the exclusive rows, scale of the shared rows only;
  (b) sum_of_one  l3k_mfs_apply of the sum that holds that single term;
  (c) sum_of_two  l3k_mfs_apply of two terms of the same kernel on the two halves of the elements (two subset meshes);
and the ratios (b) / (a) -- the price of the unfused exclusive rows plus the full scale pass -- and (c) / (a), and the relative L2
difference of (b) and (c) from (a) on the timed vectors."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
U = 4


def alternate(legs, reps, inner=50):
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
    return {k: float(np.median(v)) for k, v in ts.items()}, {k: [float(min(v)), float(max(v))] for k, v in ts.items()}


def run_case(ctx, p, ne, reps):
    import torch
    from l3ster_amd import partition, system
    part = system.CubePartition(ne, p, perturb=0.1)
    mask = part.dirichlet_mask(U)
    rows = system.DeviceMesh(ctx, part, U, mask)
    kpar = [1.0, 1.0]
    single = system.MatrixFreeSystem(rows, system.KERNEL_DIFFUSION3D, kpar)
    one = system.MultiTermSystem(rows).add(system.MatrixFreeSystem(rows, system.KERNEL_DIFFUSION3D, kpar)).finalize()
    k = part.n_elems // 2
    halves = [system.MatrixFreeSystem(system.DeviceMesh(ctx, partition.element_subset(part, e), U, mask), system.KERNEL_DIFFUSION3D, kpar)
              for e in (np.arange(0, k), np.arange(k, part.n_elems))]
    two = system.MultiTermSystem(rows).add(halves[0]).add(halves[1]).finalize()
    n = rows.n_owned_dofs
    X = torch.as_tensor(part.synthetic_vector(U)[:, :n].copy(), device="cuda")
    Y = {name: torch.empty_like(X) for name in ("single", "sum_of_one", "sum_of_two")}
    legs = {"single": lambda: single.apply(X, Y["single"], 1.0, 0.0), "sum_of_one": lambda: one.apply(X, Y["sum_of_one"], 1.0, 0.0),
            "sum_of_two": lambda: two.apply(X, Y["sum_of_two"], 1.0, 0.0)}
    t, spread = alternate(legs, reps)
    torch.cuda.synchronize()
    ref = Y["single"].norm()
    return dict(kernel="Diffusion3D", order=p, mesh=f"{ne}^3", n_elems=part.n_elems, n_dofs=n, route_single=single.route(),
                apply_seconds=t, min_max_seconds=spread, dofs_per_second={name: n / v for name, v in t.items()},
                sum_of_one_over_single=t["sum_of_one"] / t["single"], sum_of_two_over_single=t["sum_of_two"] / t["single"],
                rel_diff_from_single={name: float((Y[name] - Y["single"]).norm() / ref) for name in ("sum_of_one", "sum_of_two")},
                active_rows=[one.info.n_active_rows, two.info.n_active_rows], reps=reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--cases", default="4:64,6:48")
    ap.add_argument("--reps", type=int, default=9)
    a = ap.parse_args()
    import torch
    from l3ster_amd import system
    assert torch.cuda.is_available(), "bench_multiterm.py measures on the GPU; there is no fallback"
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
