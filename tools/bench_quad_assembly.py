"""The assembled path on quads: element systems per second with K_e stored, and the whole begin -> add -> end of an AssembledSystem.

    python tools/bench_quad_assembly.py [--out profiles/quad_assembly.jsonl] [--ne 256] [--orders 2,4,6] [--system-order 4] [--reps 5]

One process, Diffusion2D (U = 3) on an ne x ne perturbed quad mesh.  One JSON line per order with
  (a) l3k_asm_element_systems into a preallocated buffer, K_e only, in batches of at most 2 GiB: after one warm-up pass over the
      mesh the median of --reps passes; element systems per second and the share of the HBM write roofline that the stores reach,
      8 Nd^2 bytes per element over the time against the 8 TB/s of the specification (what that share says: DESIGN.md 4.18);
and one line for --system-order with
  (b) AssembledSystem: the construction (sparsity graph and arrays), then begin -> add(domain) -> add(boundary, two sides) -> end
      with the Dirichlet mask on the other two sides, the median of --reps rounds, and the n, nnz of the system.
There is no earlier route to compare with."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
U = 3
HBM_PEAK = 8.0e12  # bytes/s, MI355X HBM3E specification


def element_systems(ctx, ne, p, reps):
    import torch
    from l3ster_amd import capi, system
    part = system.SquarePartition(ne, p, perturb=0.1)
    mf = system.MatrixFreeSystem(system.DeviceMesh(ctx, part, U), system.KERNEL_DIFFUSION2D)
    Nd = (p + 1) ** 2 * U
    batch = max(1, min(part.n_elems, (2 << 30) // (8 * Nd * Nd)))
    K = torch.empty((batch, Nd, Nd), dtype=torch.float64, device="cuda")
    lib = capi.load()

    def one_pass():
        for first in range(0, part.n_elems, batch):
            capi.check(lib.l3k_asm_element_systems(mf._h, first, min(batch, part.n_elems - first), K.data_ptr(), None))
        torch.cuda.synchronize()

    one_pass()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        one_pass()
        ts.append(time.perf_counter() - t0)
    t = float(np.median(ts))
    return dict(what="element_systems", order=p, ne=ne, n_elems=part.n_elems, Nd=Nd, batch=batch, seconds=t,
                systems_per_s=part.n_elems / t, store_bytes_per_elem=8 * Nd * Nd,
                hbm_write_roofline_share=part.n_elems * 8 * Nd * Nd / t / HBM_PEAK, reps=reps)


def whole_system(ctx, ne, p, reps):
    import torch
    from l3ster_amd import system
    part = system.SquarePartition(ne, p, perturb=0.1)
    mesh = system.DeviceMesh(ctx, part, U, part.dirichlet_mask(U, sides=(2, 3)))
    mf = system.MatrixFreeSystem(mesh, system.KERNEL_DIFFUSION2D)
    bnd = system.BoundaryTerm(mesh, system.KERNEL_ADIABATIC2D, *part.boundary_sides([0, 1]))
    t0 = time.perf_counter()
    asm = system.AssembledSystem(mesh)
    torch.cuda.synchronize()
    t_create = time.perf_counter() - t0

    def one_round():
        asm.begin()
        asm.add(mf)
        asm.add(bnd)
        asm.end()
        torch.cuda.synchronize()

    one_round()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        one_round()
        ts.append(time.perf_counter() - t0)
    info = asm.info
    return dict(what="begin_add_end", order=p, ne=ne, n_elems=part.n_elems, n=info.n, nnz=info.nnz, n_missing=info.n_missing,
                create_seconds=t_create, seconds=float(np.median(ts)), systems_per_s=part.n_elems / float(np.median(ts)), reps=reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "quad_assembly.jsonl"))
    ap.add_argument("--ne", type=int, default=256)
    ap.add_argument("--orders", default="2,4,6")
    ap.add_argument("--system-order", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch
    from l3ster_amd import system
    torch.cuda.set_device(0)
    ctx = system.Context(0, torch.cuda.current_stream().cuda_stream)
    lines = [element_systems(ctx, a.ne, int(p), a.reps) for p in a.orders.split(",")]
    lines.append(whole_system(ctx, a.ne, a.system_order, a.reps))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for line in lines:
            line["device"] = torch.cuda.get_device_name(0)
            f.write(json.dumps(line) + "\n")
            print(json.dumps(line))


if __name__ == "__main__":
    main()
