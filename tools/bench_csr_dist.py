"""The distributed CSR operator (l3k_csr_dist_apply) on the matrices of tools/bench_csr.py -- Diffusion3D (U = 4) at order 2 and order
4 on the full graph and at order 4 on the condensed graph -- and on a Diffusion2D quad matrix (U = 3, order 4) from
system.AssembledSystem, each far larger than the L2 and the 256 MiB Infinity Cache.

    python tools/bench_csr_dist.py [--out profiles/csr_dist.jsonl] [--cases 2:full:32,4:full:12,4:condensed:12,quad:4:160]
                                   [--ranks 2,4] [--rank-case 2:32] [--reps 7]

One process, one GPU.  A record, not a gate.  Per line of JSON:
  (a) "world_of_one": l3k_csr_dist_apply in a world of one rank (a halo without neighbours: two launches over the halves of the
      interior list, no exchange) against l3k_csr_apply on the SAME arrays: after a warm-up of both legs they run alternately --reps
      times, five applies per timing behind one synchronise, the median per leg, their ratio, and whether the two results are equal
      bit for bit.  Effective bandwidth counts 12 B per stored entry + row_ptr + x + y, as bench_csr.py does; the distributed
      operator reads 4 B per row of row list on top.
  (b) "thread_ranks": R ranks as threads of this process on ONE GPU (the in-process transport; the tests' arrangement), each with
      its block of CubePartition(ne, p, parts=(R, 1, 1)): per rank the three row counts, the median wall time of an apply
      between barriers, and the device time of its three groups of launches (first half of the interior rows; border and ghost
      rows; second half) from l3k_halo_timing_*, with their shares.  The ranks share one device, so this shows the schedule and the
      size of the border work, NOT a multi-GPU speed: that is not measured here."""
import argparse
import ctypes as C
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
U = 4


def world_of_one(ctx, name, row_ptr, col_ind, values, part, dofs_per_node, reps, extra):
    import torch
    from bench_csr import alternate
    from l3ster_amd import system
    from l3ster_amd.distributed import InprocGroup, NativeHalo
    local = system.CsrOperator(ctx, row_ptr, col_ind, values)
    op = system.DistributedCsrOperator(local, NativeHalo(ctx, part, dofs_per_node, 0, 1, transport=InprocGroup(1)))
    info, n = local.info(), local.n
    x = torch.as_tensor(np.random.default_rng(0).standard_normal(n), device="cuda")
    y, z = torch.empty_like(x), torch.empty_like(x)
    op.apply(x, y)
    local.apply(x, z)
    equal = bool(torch.equal(y, z))
    t = alternate({"csr_apply": lambda: local.apply(x, z), "csr_dist_apply": lambda: op.apply(x, y)}, reps)
    bytes_moved = 12 * info.nnz + 8 * (n + 1) + 16 * n
    return dict(kind="world_of_one", matrix=name, n=n, nnz=info.nnz, mean_row_len=info.mean_row_len, lanes=info.lanes_per_row,
                matrix_gib=12 * info.nnz / 2 ** 30, bytes_counted=bytes_moved, row_list_bytes=4 * n, apply_seconds=t,
                apply_gb_per_s={k: bytes_moved / v / 1e9 for k, v in t.items()},
                dist_over_csr=t["csr_dist_apply"] / t["csr_apply"], bitwise_equal=equal, **extra)


def hex_case(ctx, p, graph, ne, reps):
    import torch
    from l3ster_amd import system
    part = system.CubePartition(ne, p, perturb=0.1)
    mf = system.MatrixFreeSystem(system.DeviceMesh(ctx, part, U, part.dirichlet_mask(U)), system.KERNEL_DIFFUSION3D, [1.0, 0.0])
    g = mf.sparsity_graph(graph)  # (the graph bench_csr.py builds on the host, from the device)
    RP, CI = g.row_ptr, g.col_ind
    vals = torch.zeros(g.info.nnz, dtype=torch.float64, device="cuda")
    rhs = torch.zeros((1, part.n_local_nodes * U), dtype=torch.float64, device="cuda")
    assert (mf.condense_global if graph == "condensed" else mf.assemble_global)(RP, CI, vals, rhs) == 0
    return world_of_one(ctx, f"Diffusion3D p{p} {graph} {ne}^3", RP, CI, vals, part, U, reps, dict(order=p, graph=graph))


def quad_case(ctx, p, ne, reps):
    from l3ster_amd import system
    part = system.SquarePartition(ne, p, perturb=0.1)
    mesh = system.DeviceMesh(ctx, part, 3, part.dirichlet_mask(3, sides=(2, 3)))
    asm = system.AssembledSystem(mesh)
    asm.begin().add(system.MatrixFreeSystem(mesh, system.KERNEL_DIFFUSION2D))
    asm.end()
    return world_of_one(ctx, f"Diffusion2D p{p} full {ne}^2", asm.row_ptr, asm.col_ind, asm.values, part, 3, reps, dict(order=p, graph="full"))


def thread_ranks(world, p, ne, reps):
    import torch
    from l3ster_amd import capi, system
    from l3ster_amd.distributed import InprocGroup, NativeHalo
    group, barrier, out, errors = InprocGroup(world), threading.Barrier(world), {}, []
    lib = capi.load()

    def body(rank):
        torch.cuda.set_device(0)
        with torch.cuda.stream(torch.cuda.Stream()):
            ctx = system.Context(0, torch.cuda.current_stream().cuda_stream)
            part = system.CubePartition(ne, p, (world, 1, 1), rank, perturb=0.1)
            mesh = system.DeviceMesh(ctx, part, U, part.dirichlet_mask(U))
            mf = system.MatrixFreeSystem(mesh, system.KERNEL_DIFFUSION3D, [1.0, 0.0])
            g = mf.sparsity_graph()
            vals = torch.zeros(g.info.nnz, dtype=torch.float64, device="cuda")
            rhs = torch.zeros((1, g.n), dtype=torch.float64, device="cuda")
            assert mf.assemble_global(g.row_ptr, g.col_ind, vals, rhs) == 0
            halo = NativeHalo(ctx, part, U, rank, world, transport=group)
            op = system.DistributedCsrOperator(system.CsrOperator(ctx, g.row_ptr, g.col_ind, vals), halo)
            x = torch.as_tensor(part.synthetic_vector(U)[:, :op.n], device="cuda")
            y = torch.empty_like(x)
            for _ in range(3):
                op.apply(x, y)
            torch.cuda.synchronize()
            wall = []
            for _ in range(reps):
                barrier.wait(timeout=300)
                t0 = time.perf_counter()
                for _ in range(5):
                    op.apply(x, y)
                torch.cuda.synchronize()
                wall.append((time.perf_counter() - t0) / 5)
            capi.check(lib.l3k_halo_timing_begin(halo._h, reps))
            barrier.wait(timeout=300)
            for _ in range(reps):
                op.apply(x, y)
            ms = np.zeros((reps, 3))
            for k in range(reps):
                buf = (C.c_double * 3)()
                capi.check(lib.l3k_halo_timing_get(halo._h, k, buf))
                ms[k] = list(buf)
            torch.cuda.synchronize()
            i, med = op.info, np.median(ms, axis=0)
            out[rank] = dict(n_owned=i.n_owned, n_ghost=i.n_ghost, interior_rows=i.n_interior_rows, border_rows=i.n_border_rows,
                             ghost_rows=i.n_ghost_rows, nnz=op.local.info().nnz, apply_wall_seconds=float(np.median(wall)),
                             launch_ms=dict(interior_first_half=med[0], border_and_ghost=med[1], interior_second_half=med[2]),
                             launch_share=[float(v / med.sum()) for v in med])

    def guarded(rank):
        try:
            body(rank)
        except BaseException as exc:  # noqa: BLE001
            errors.append((rank, exc))
            barrier.abort()

    threads = [threading.Thread(target=guarded, args=(r,), daemon=True) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(900)
    assert not errors, errors
    return dict(kind="thread_ranks", matrix=f"Diffusion3D p{p} full {ne}^3", ranks=world, one_gpu=True,
                note="thread ranks share one GPU: the schedule and the shares of the launches, not a multi-GPU speed",
                per_rank=[out[r] for r in range(world)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--cases", default="2:full:32,4:full:12,4:condensed:12,quad:4:160")
    ap.add_argument("--ranks", default="2,4")
    ap.add_argument("--rank-case", default="2:32")
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    import torch
    from l3ster_amd import system
    assert torch.cuda.is_available(), "bench_csr_dist.py measures on the GPU; there is no fallback"
    torch.cuda.set_device(0)
    ctx = system.Context(0, torch.cuda.current_stream().cuda_stream)
    out = open(a.out, "a") if a.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    for case in [c for c in a.cases.split(",") if c]:
        f = case.split(":")
        emit(quad_case(ctx, int(f[1]), int(f[2]), a.reps) if f[0] == "quad" else hex_case(ctx, int(f[0]), f[1], int(f[2]), a.reps))
    p, ne = (int(v) for v in a.rank_case.split(":"))
    for world in [int(r) for r in a.ranks.split(",") if r]:
        emit(thread_ranks(world, p, ne, a.reps))


if __name__ == "__main__":
    main()
