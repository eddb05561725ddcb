"""The collective GMRES inside the library (l3k_csr_dist_gmres_solve: solve.gmres_distributed) on one mesh cut for worlds of 1, 2 and 4
ranks, against the single-rank solve.gmres on the whole system in the same process.

    python tools/bench_gmres_dist.py [--out profiles/gmres_dist.jsonl] [--case 2:16] [--ranks 1,2,4] [--k 1,8,30,60] [--steps 120] [--reps 5]

One process, one GPU.  A record, not a gate: no threshold is set in advance.  The system is Diffusion3D (U = 4) as a
distributed CSR operator (system.AssembledSystem(halo=...)) on a cube of order p, the ranks are THREADS of this process on one GPU
through the in-process transport.  For every restart length k a solve runs whole cycles of k steps towards tol = 0 (about --steps
steps, the host reads once per cycle) with the Jacobi preconditioner; ms per step is the wall time over the steps and contains the
cycle heads.  A step has three all-reduces of up to k + 1 doubles; ms per all-reduce is measured apart, on a chain of 200
NativeHalo.allreduce_n of k + 1 doubles with nothing waiting on the device in between.  Medians of --reps runs behind a warm-up, the
slowest rank.  The thread ranks share one device and meet on the host inside every reduction, so the figures show the cost of the
loop's plumbing, NOT a multi-GPU speed; multi-GPU speed and the latency of the reductions over RCCL are not measured here."""
import argparse
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
U, CHAIN = 4, 200


def timed(fn, reps, barrier=None):
    import torch
    out = []
    for rep in range(-1, reps):  # (rep -1: the warm-up)
        torch.cuda.synchronize()
        if barrier is not None:
            barrier.wait(timeout=300)
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if rep >= 0:
            out.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(out))


def build(p, ne, world, rank, group):
    import torch
    from l3ster_amd import system
    from l3ster_amd.distributed import NativeHalo
    ctx = system.Context(0, torch.cuda.current_stream().cuda_stream)
    part = system.CubePartition((ne, ne, ne), p, (world, 1, 1), rank, perturb=0.1)
    mesh = system.DeviceMesh(ctx, part, U, part.dirichlet_mask(U))
    mf = system.MatrixFreeSystem(mesh, system.KERNEL_DIFFUSION3D, [1.0, 0.0])
    halo = NativeHalo(ctx, part, U, rank, world, transport=group) if group is not None else None
    asm = system.AssembledSystem(mesh, halo=halo) if halo is not None else system.AssembledSystem(mesh)
    asm.begin()
    asm.add(mf)
    op = asm.end()
    minv = op.jacobi_inverse()
    n = part.n_owned_nodes * U
    b = torch.as_tensor(part.synthetic_vector(U)[0, :n].copy(), device="cuda") * (minv != 0)
    return ctx, op, halo, minv, b, (asm, mesh, mf)


def run_kw(k, steps):
    cycles = max(1, steps // k)
    return dict(tol=0.0, max_iters=k * cycles, check_every=k * cycles, max_restarts=cycles, throw_on_fail=False), k * cycles


def one_rank(p, ne, world, rank, group, barrier, ks, steps, reps):
    import torch
    from l3ster_amd import solve
    ctx, op, halo, minv, b, keep = build(p, ne, world, rank, group)
    out = dict(n_owned=b.numel(), ms_per_step={}, ms_per_allreduce={}, iterations={})
    halo.reduce_reserve(max(ks) + 1)
    for k in ks:
        kw, total = run_kw(k, steps)
        ws = solve.GmresWorkspace(ctx, b.numel(), k, collective=True)
        done = {}

        def leg():
            done["res"] = solve.gmres_distributed(op, ctx, b, torch.zeros_like(b), minv=minv, workspace=ws, **kw)
        out["ms_per_step"][k] = timed(leg, reps, barrier) / max(done["res"].num_iters, 1)
        out["iterations"][k] = done["res"].num_iters
        vals = torch.ones(k + 1, dtype=torch.float64, device="cuda")

        def chain():
            for _ in range(CHAIN):
                halo.allreduce_n(vals)
                vals.mul_(1.0 / world)
        out["ms_per_allreduce"][k] = timed(chain, reps, barrier) / CHAIN
    return out


def single_rank(p, ne, ks, steps, reps):
    import torch
    from l3ster_amd import solve
    ctx, op, _, minv, b, keep = build(p, ne, 1, 0, None)
    out = dict(n=b.numel(), ms_per_step={})
    for k in ks:
        kw, total = run_kw(k, steps)
        ws = solve.GmresWorkspace(ctx, b.numel(), k)
        done = {}

        def leg():
            done["res"] = solve.gmres(op, b, torch.zeros_like(b), minv, workspace=ws, **kw)
        out["ms_per_step"][k] = timed(leg, reps) / max(done["res"].num_iters, 1)
    return out


def case(p, ne, world, ks, steps, reps, single):
    import torch
    from l3ster_amd.distributed import InprocGroup
    group, barrier, out, errors = InprocGroup(world), threading.Barrier(world), {}, []

    def guarded(rank):
        try:
            torch.cuda.set_device(0)
            with torch.cuda.stream(torch.cuda.Stream()):
                out[rank] = one_rank(p, ne, world, rank, group, barrier, ks, steps, reps)
        except BaseException as exc:  # noqa: BLE001
            errors.append((rank, exc))
            barrier.abort()

    threads = [threading.Thread(target=guarded, args=(r,), daemon=True) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(1200)
    assert not errors, errors
    slowest = lambda key: {str(k): max(out[r][key][k] for r in range(world)) for k in ks}
    step = slowest("ms_per_step")
    return dict(kind="gmres_dist", operator="distributed CSR", order=p, elements=f"{ne}^3", n=single["n"], ranks=world, one_gpu=True,
                restart_lengths=ks, steps=out[0]["iterations"], ms_per_step=step, ms_per_allreduce=slowest("ms_per_allreduce"),
                single_rank_ms_per_step={str(k): single["ms_per_step"][k] for k in ks},
                over_single_rank={str(k): step[str(k)] / single["ms_per_step"][k] for k in ks}, per_rank=[out[r] for r in range(world)],
                note="thread ranks share one GPU: the loop's plumbing, not a multi-GPU speed; RCCL latency not measured")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--case", default="2:16", help="order:elements per edge of the cube")
    ap.add_argument("--ranks", default="1,2,4")
    ap.add_argument("--k", default="1,8,30,60")
    ap.add_argument("--steps", type=int, default=120)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_gmres_dist.py measures on the GPU; there is no fallback"
    p, ne = (int(v) for v in a.case.split(":"))
    ks = [int(k) for k in a.k.split(",") if k]
    torch.cuda.set_device(0)
    single = single_rank(p, ne, ks, a.steps, a.reps)
    out = open(a.out, "a") if a.out else None
    for world in [int(r) for r in a.ranks.split(",") if r]:
        line = json.dumps(case(p, ne, world, ks, a.steps, a.reps, single))
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()


if __name__ == "__main__":
    main()
