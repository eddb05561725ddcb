"""The collective PCG inside the library (l3k_pcg_solve_dist, l3k_csr_dist_pcg_solve: solve.pcg_distributed(native=True)) against the
host loop of solve.pcg_distributed as it stood before that entry point existed: the l3k_cg_* pieces driven from Python, <p, A p> of
the CSR operator as a pass of its own, the all-reduce outside the library.

    python tools/bench_pcg_dist.py [--out profiles/pcg_dist.jsonl] [--mf 4:16] [--csr 2:24] [--ranks 1,2] [--iters 200] [--reps 5]

One process, one GPU.  A record, not a gate: no threshold is set in advance.  Cases: Diffusion3D (U = 4) matrix-free
at order 4 and as a distributed CSR operator (system.AssembledSystem(halo=...)) at order 2, each in a world of one and with 2 ranks
as THREADS of this process on one GPU through the in-process transport.  Both legs run a fixed number of Jacobi iterations (tol = 0,
max_iters = --iters, one convergence check at the end) from x = 0 on the same right-hand side; after a warm-up of both legs they run
alternately --reps times and the medians are kept.  Per line of JSON: ms per iteration of either leg and their ratio
(library / host).  The thread ranks share one device and meet on the host inside every reduction, so their figures show the cost of
the loop's plumbing, NOT a multi-GPU speed; multi-GPU speed and the latency of the all-reduce over RCCL are not measured here."""
import argparse
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
U = 4


class BarrierAllReduce:
    """the host loop's sum all-reduce between thread ranks: device synchronisation, a barrier, the sum in rank order"""

    def __init__(self, world):
        self.world, self.slots, self.barrier = world, [None] * world, threading.Barrier(world)

    def bind(self, rank):
        import torch

        def allreduce(view):
            if self.world == 1:
                return
            torch.cuda.synchronize()
            self.slots[rank] = view.clone()
            self.barrier.wait(timeout=300)
            total = sum(self.slots[r] for r in range(self.world))
            self.barrier.wait(timeout=300)
            view.copy_(total)
        return allreduce


class WithoutEnergy:
    """an operator as the host loop saw it before apply(..., energy=) existed: <p, A p> is l3k_cg_dot_pap's pass"""

    def __init__(self, op):
        self.op = op

    def apply(self, X, Y, alpha=1.0, beta=0.0):
        return self.op.apply(X, Y, alpha, beta)


def one_rank(kind, p, ne, world, rank, group, red, barrier, iters, reps):
    import torch
    from l3ster_amd import solve, system
    from l3ster_amd.distributed import NativeDistributedOperator, NativeHalo
    ctx = system.Context(0, torch.cuda.current_stream().cuda_stream)
    part = system.CubePartition((ne, ne, ne), p, (world, 1, 1), rank, perturb=0.1)
    mesh = system.DeviceMesh(ctx, part, U, part.dirichlet_mask(U))
    mf = system.MatrixFreeSystem(mesh, system.KERNEL_DIFFUSION3D, [1.0, 0.0])
    halo = NativeHalo(ctx, part, U, rank, world, transport=group)
    if kind == "mf":
        op = NativeDistributedOperator(mf, halo)
        minv = solve.jacobi_inverse_native(ctx, op.diag_rhs()[0])
        host_op = op  # (it never had an energy= keyword)
    else:
        asm = system.AssembledSystem(mesh, halo=halo)
        asm.begin()
        asm.add(mf)
        op = asm.end()
        minv, host_op = op.jacobi_inverse(), WithoutEnergy(op)
    n = part.n_owned_nodes * U
    b = torch.as_tensor(part.synthetic_vector(U)[0, :n].copy(), device="cuda") * (minv != 0)
    run = dict(tol=0.0, max_iters=iters, check_every=iters, throw_on_fail=False)
    legs = {"library": lambda x: solve.pcg_distributed(op, ctx, b, x, minv=minv, native=True, **run),
            "host": lambda x: solve.pcg_distributed(host_op, ctx, b, x, minv=minv, allreduce=red.bind(rank), **run)}
    times, done = {k: [] for k in legs}, {}
    for rep in range(-1, reps):  # (rep -1: the warm-up of both legs)
        for name, leg in legs.items():
            x = torch.zeros_like(b)
            torch.cuda.synchronize()
            barrier.wait(timeout=300)
            t0 = time.perf_counter()
            res = leg(x)
            torch.cuda.synchronize()
            if rep >= 0:
                times[name].append(time.perf_counter() - t0)
            done[name] = res.num_iters
    return dict(n_owned=n, iterations=done, ms_per_iteration={k: 1e3 * float(np.median(v)) / max(done[k], 1) for k, v in times.items()})


def case(kind, p, ne, world, iters, reps):
    import torch
    from l3ster_amd.distributed import InprocGroup
    group, red, barrier, out, errors = InprocGroup(world), BarrierAllReduce(world), threading.Barrier(world), {}, []

    def guarded(rank):
        try:
            torch.cuda.set_device(0)
            with torch.cuda.stream(torch.cuda.Stream()):
                out[rank] = one_rank(kind, p, ne, world, rank, group, red, barrier, iters, reps)
        except BaseException as exc:  # noqa: BLE001
            errors.append((rank, exc))
            barrier.abort()
            red.barrier.abort()

    threads = [threading.Thread(target=guarded, args=(r,), daemon=True) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(1200)
    assert not errors, errors
    ms = {k: max(out[r]["ms_per_iteration"][k] for r in range(world)) for k in ("library", "host")}  # (the slowest rank)
    return dict(kind="pcg_dist", operator={"mf": "matrix-free", "csr": "distributed CSR"}[kind], order=p, elements=f"{ne}^3", ranks=world,
                one_gpu=True, iterations=iters, ms_per_iteration=ms, library_over_host=ms["library"] / ms["host"],
                per_rank=[out[r] for r in range(world)],
                note="thread ranks share one GPU: the loop's plumbing, not a multi-GPU speed; RCCL latency not measured")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--mf", default="4:16", help="order:elements per edge of the matrix-free case")
    ap.add_argument("--csr", default="2:24", help="order:elements per edge of the distributed CSR case")
    ap.add_argument("--ranks", default="1,2")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_pcg_dist.py measures on the GPU; there is no fallback"
    out = open(a.out, "a") if a.out else None
    for world in [int(r) for r in a.ranks.split(",") if r]:
        for kind, spec in (("mf", a.mf), ("csr", a.csr)):
            p, ne = (int(v) for v in spec.split(":"))
            line = json.dumps(case(kind, p, ne, world, a.iters, a.reps))
            print(line, flush=True)
            if out:
                out.write(line + "\n")
                out.flush()


if __name__ == "__main__":
    main()
