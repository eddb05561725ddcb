"""The device builder of the CSR sparsity graph (l3k_graph_create + l3k_graph_fill, system.SparsityGraph) on Diffusion3D meshes
(U = 4): the full graph at orders 2, 4 and 6 and the condensed one at orders 4 and 6, at the mesh sizes of tools/bench_csr.py.

    python tools/bench_graph.py [--out profiles/graph.jsonl] [--cases 2:full:32,4:full:12,6:full:6,4:condensed:12,6:condensed:6] [--reps 5]

One process.  Per graph one JSON line with the legs
  device : system.SparsityGraph -- create, the readback and the fill into fresh torch tensors;
  torch  : tools/bench_assembled_pipeline.py:csr_graph_device, torch.unique over chunks of node pairs (full graphs only: it has
           no condensed form) -- the yardstick at the same size; no threshold on time is fixed in advance;
  host   : system.condensed_graph, np.unique on the host plus the upload (condensed graphs only).
After a warm-up of every leg the legs run alternately --reps times; the median per leg.  Then each leg runs once more from an
emptied torch cache: free device memory (hipMemGetInfo) before it and at its end, with its results -- and the torch cache, which
keeps the leg's peak reservation -- still alive; the difference is the leg's footprint at its low-water mark.  The device leg's
arrays are compared with the yardstick's (they must be equal)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
U = 4


def run_case(ctx, p, kind, ne, reps):
    import torch
    from bench_assembled_pipeline import csr_graph_device
    from l3ster_amd import system
    part = system.CubePartition(ne, p)
    mesh = system.DeviceMesh(ctx, part, U)
    out = {}

    def device():
        g = system.SparsityGraph(mesh, None, kind)
        out["device"] = (g.row_ptr, g.col_ind)
        out["info"] = g.info
        return g

    def torch_route():
        out["torch"] = csr_graph_device(part, U)
        return out["torch"]

    def host():
        rp, ci = system.condensed_graph(part.elem_nodes, p, U, np.arange(U))
        out["host"] = (torch.as_tensor(rp, device="cuda"), torch.as_tensor(ci, device="cuda"))
        return out["host"]

    legs = {"device": device}
    legs.update({"torch": torch_route} if kind == "full" else {"host": host})
    for fn in legs.values():
        fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in legs}
    for _ in range(reps):
        for k, fn in legs.items():
            out.pop(k, None)
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts[k].append(time.perf_counter() - t0)
    yardstick = "torch" if kind == "full" else "host"
    same = bool(torch.equal(out["device"][0], out[yardstick][0]) and torch.equal(out["device"][1], out[yardstick][1]))
    info = out["info"]
    mem = {}
    for k, fn in legs.items():
        out.clear()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        free0 = torch.cuda.mem_get_info()[0]
        keep = fn()
        torch.cuda.synchronize()
        free1 = torch.cuda.mem_get_info()[0]
        mem[k] = dict(free_before=free0, free_low_water=free1, footprint_bytes=free0 - free1)
        del keep
    return dict(kernel="Diffusion3D", order=p, graph=kind, mesh=f"{ne}^3", n=info.n, nnz=info.nnz, col_ind_bytes=4 * info.nnz,
                workspace_bytes=info.workspace_bytes, n_rows_scratch=info.n_rows_scratch, max_elems_per_node=info.max_elems_per_node,
                seconds={k: float(np.median(v)) for k, v in ts.items()}, memory=mem, equal_to_yardstick=same, yardstick=yardstick)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--cases", default="2:full:32,4:full:12,6:full:6,4:condensed:12,6:condensed:6")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch
    from l3ster_amd import system
    assert torch.cuda.is_available(), "bench_graph.py measures on the GPU; there is no fallback"
    torch.cuda.set_device(0)
    ctx = system.Context(0, torch.cuda.current_stream().cuda_stream)
    out = open(a.out, "a") if a.out else None
    for case in a.cases.split(","):
        p, kind, ne = case.split(":")
        line = json.dumps(run_case(ctx, int(p), kind, int(ne), a.reps))
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()


if __name__ == "__main__":
    main()
