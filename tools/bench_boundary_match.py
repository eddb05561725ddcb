"""Times l3k_boundary_match and l3k_elevate_order_quads on generated meshes, one GPU:
    python tools/bench_boundary_match.py [--hex 32 128] [--quad 1024] [--dict-hex 32] [--order 4] [--repeats 5]
Meshes: the structured cube (ne^3 hexes, all 6 ne^2 boundary quads listed) and square (ne^2 quads, 4 ne lines) with the elements in
a random order, the vertex ids renumbered at random and every boundary element written from a random start in a random direction,
so that neither the sort nor the searches see a structured input.  Every call is made once untimed, then --repeats times; the
figure is the median of a host clock around the call, which takes host arrays, copies them to the device, and ends in a stream
synchronise after the copy back (the call a user makes: transfers included).  The answers of the timed calls are checked against
the generator's truth.  dict_s is the time of the host restatement of tests/mesh_ref.py (a Python dictionary over vertex sets) on
the --dict-hex cube: what the matching would cost outside the library.  One JSON line per leg on stdout and in
profiles/boundary_match.jsonl (--out)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import mesh_ref  # noqa: E402
from l3ster_amd import system  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--hex", type=int, nargs="*", default=[32, 128], help="elements per edge of the cubes")
ap.add_argument("--quad", type=int, nargs="*", default=[1024], help="elements per edge of the squares")
ap.add_argument("--dict-hex", type=int, default=32, help="cube of the dictionary restatement (0: skip)")
ap.add_argument("--order", type=int, default=4, help="of the quad elevation")
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "boundary_match.jsonl"))
a = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_boundary_match.py measures on the GPU: no device found")
torch.cuda.set_device(0)
ctx = system.Context(0, torch.cuda.current_stream().cuda_stream)


def generated(dim, ne, rng):
    """(conn, bnd_conn, true_elem, true_side) of the shuffled structured mesh"""
    nv1 = ne + 1
    grid = np.arange(nv1 ** dim, dtype=np.int64).reshape((nv1,) * dim)  # [k][j][i]
    corner = lambda off: grid[tuple(slice(o, o + ne) for o in off)].reshape(-1)  # noqa: E731  (offsets in (k, j, i) order)
    offs = [tuple((v >> (dim - 1 - ax)) & 1 for ax in range(dim)) for v in range(2 ** dim)]  # local vertex v = i + 2j + 4k
    conn = np.stack([corner(o) for o in offs], axis=1)
    elem = np.arange(ne ** dim, dtype=np.int64).reshape((ne,) * dim)
    bnd, be, bs = [], [], []
    for s, lv in enumerate(mesh_ref.SIDE_VERTS[dim]):
        axis, at = s // 2, (0 if s % 2 == 0 else ne - 1)  # side pairs: the last axis first
        e = np.take(elem, at, axis=axis).reshape(-1)
        bnd.append(conn[e][:, list(lv)]), be.append(e), bs.append(np.full(e.size, s, dtype=np.uint8))
    bnd, be, bs = np.concatenate(bnd), np.concatenate(be), np.concatenate(bs)
    # the same start and direction for a whole quarter of the boundary elements would be a structure too: one draw per element
    nsv = bnd.shape[1]
    flip, roll = rng.integers(0, 2, bnd.shape[0]), rng.integers(0, nsv, bnd.shape[0])
    idx = (np.where(flip[:, None] == 1, -np.arange(nsv)[None, :], np.arange(nsv)[None, :]) + roll[:, None]) % nsv
    bnd = np.take_along_axis(bnd, idx, axis=1)
    relabel, order = rng.permutation(nv1 ** dim), rng.permutation(conn.shape[0])
    new_index = np.empty_like(order)
    new_index[order] = np.arange(order.size)
    return relabel[conn[order]].astype(np.uint32), relabel[bnd].astype(np.uint32), new_index[be], bs


def timed(call):
    call()
    ts = []
    for _ in range(a.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = call()
        ts.append(time.perf_counter() - t0)
    return out, statistics.median(ts), min(ts), max(ts)


lines = []
rng = np.random.default_rng(2024)
for dim, sizes in ((3, a.hex), (2, a.quad)):
    for ne in sizes:
        conn, bnd, true_elem, true_side = generated(dim, ne, rng)
        (fe, fs, nu, ni), med, lo, hi = timed(lambda: system.boundary_match(ctx, conn, bnd))
        assert np.array_equal(fe, true_elem) and np.array_equal(fs, true_side) and (nu, ni) == (0, 0)
        line = {"leg": "l3k_boundary_match", "mesh": f"{'hex' if dim == 3 else 'quad'} {ne}^{dim}", "n_elems": int(conn.shape[0]),
                "n_sides_sorted": int(conn.shape[0]) * 2 * dim, "n_bnd": int(bnd.shape[0]), "call_s_median": med, "call_s_min": lo,
                "call_s_max": hi, "repeats": a.repeats, "boundary_elements_per_s": bnd.shape[0] / med, "sides_per_s": conn.shape[0] * 2 * dim / med}
        if dim == 3 and ne == a.dict_hex:
            t0 = time.perf_counter()
            de, ds, _, _ = mesh_ref.match_by_dictionary(conn, bnd)
            line["dict_s"] = time.perf_counter() - t0
            line["dict_over_call"] = line["dict_s"] / med
            assert np.array_equal(de, fe) and np.array_equal(ds, fs)
        lines.append(line)
        print(json.dumps(line), flush=True)
        if dim == 2:
            n_vertices = (ne + 1) ** 2
            (en, n_nodes, n_nonint), med, lo, hi = timed(lambda: system.elevate_order_quads(ctx, conn, n_vertices, a.order))
            assert n_nodes == (ne * a.order + 1) ** 2
            line = {"leg": "l3k_elevate_order_quads", "mesh": f"quad {ne}^2", "order": a.order, "n_elems": int(conn.shape[0]),
                    "n_nodes": int(n_nodes), "call_s_median": med, "call_s_min": lo, "call_s_max": hi, "repeats": a.repeats,
                    "nodes_per_s": n_nodes / med}
            lines.append(line)
            print(json.dumps(line), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    for line in lines:
        f.write(json.dumps(line) + "\n")
