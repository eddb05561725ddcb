"""Times l3k_periodic_match on the two opposite faces of a structured cube, one GPU:
    python tools/bench_periodic_match.py [--ne 128] [--order 6] [--repeats 5]
Mesh: the two layers of elements of the ne^3 order-p cube that touch x = 0 and x = 1 (the call reads the elements of the listed sides
only, so the 2 ne^2 elements of the layers stand for the cube), node ids those of the whole cube's grid, the elements in a random
order.  Source: the ne^2 sides on x = 1; destination: those on x = 0; translation (-1, 0, 0); tolerance 1e-12: (ne p + 1)^2 node pairs.
The call is made once untimed, then --repeats times; the figure is the median of a host clock around the call, which takes host
arrays, gathers the sides, copies them to the device and ends in a stream synchronise after the copy back (the call a user makes:
transfers included).  Every answer is checked against the grid.  One JSON line on stdout and in profiles/periodic_match.jsonl
(--out)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from l3ster_amd import system  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--ne", type=int, default=128, help="elements per edge of the cube")
ap.add_argument("--order", type=int, default=6)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "periodic_match.jsonl"))
a = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_periodic_match.py measures on the GPU: no device found")
torch.cuda.set_device(0)
ctx = system.Context(0, torch.cuda.current_stream().cuda_stream)

ne, p = a.ne, a.order
n1, NX = p + 1, ne * p + 1
rng = np.random.default_rng(2025)
ex, ey, ez = np.meshgrid([0, ne - 1], np.arange(ne), np.arange(ne), indexing="ij")
ex, ey, ez = (v.reshape(-1) for v in (ex, ey, ez))
order = rng.permutation(ex.size)
ex, ey, ez = ex[order], ey[order], ez[order]
k, j, i = (v.reshape(-1) for v in np.meshgrid(np.arange(n1), np.arange(n1), np.arange(n1), indexing="ij"))  # local node i + n (j + n k)
grid_id = (ex[:, None] * p + i[None, :]) + NX * ((ey[:, None] * p + j[None, :]) + NX * (ez[:, None] * p + k[None, :]))
assert grid_id.max() < 2 ** 32


class Layers:
    dim, order = 3, p
    elem_nodes = grid_id.astype(np.uint32)
    elem_verts = np.stack([np.stack([(ex + (v & 1)) / ne, (ey + ((v >> 1) & 1)) / ne, (ez + ((v >> 2) & 1)) / ne], axis=1) for v in range(8)],
                          axis=1)


src = (np.nonzero(ex == ne - 1)[0].astype(np.int64), np.full(ne * ne, 5, np.uint8))
dst = (np.nonzero(ex == 0)[0].astype(np.int64), np.full(ne * ne, 4, np.uint8))
call = lambda: system.periodic_match(ctx, Layers, src, dst, [-1.0, 0.0, 0.0])  # noqa: E731
ps, pd, n_unmatched, n_ambiguous, first = call()
ts = []
for _ in range(a.repeats):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ps, pd, n_unmatched, n_ambiguous, first = call()
    ts.append(time.perf_counter() - t0)
    assert ps.size == NX * NX and (n_unmatched, n_ambiguous, first) == (0, 0, -1)
    assert np.all(ps % NX == NX - 1) and np.array_equal(pd.astype(np.int64), ps.astype(np.int64) - (NX - 1))
med = statistics.median(ts)
line = {"leg": "l3k_periodic_match", "mesh": f"two faces of hex {ne}^3, order {p}", "n_src_sides": int(src[0].size),
        "n_dst_sides": int(dst[0].size), "n_side_nodes_listed": int(2 * ne * ne * n1 * n1), "n_pairs": int(ps.size),
        "tolerance": 1e-12, "call_s_median": med, "call_s_min": min(ts), "call_s_max": max(ts), "repeats": a.repeats,
        "pairs_per_s": ps.size / med}
print(json.dumps(line), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write(json.dumps(line) + "\n")
