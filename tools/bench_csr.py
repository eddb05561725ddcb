"""The device CSR operator on matrices from the library's own assembly: Diffusion3D (U = 4) at order 2 and order 4 on the full
graph and at order 4 on the condensed graph, each far larger than the L2 and the 256 MiB Infinity Cache.

    python tools/bench_csr.py [--out profiles/csr.jsonl] [--cases 2:full:32,4:full:12,4:condensed:12] [--reps 7]

One process.  Per matrix, one JSON line with
  (a) l3k_csr_apply for forced lanes_per_row 4, 16, 64 and the automatic choice: after a warm-up of every leg the legs run
      alternately --reps times, the median per leg; effective bandwidth = (12 B per stored entry + row_ptr + x + y) / time;
  (b) the same product by torch's CSR mat-vec on the same col_ind / values arrays (row_ptr as int32, which torch wants to match
      col_ind), timed as another leg of the same alternation: the yardstick -- there is no earlier version to compare with;
  (c) condensed matrices only: l3k_csr_pcg_solve on the condensed system (Dirichlet conditions applied, Jacobi) against the
      matrix-free solve.pcg on the same mesh, kernel, boundary values, tolerance and residual scaling; seconds and iterations of
      both, the condensation, the recovery, and the difference of the two solutions.
The cut points of the automatic lanes_per_row (chooseLanes in csrc/api_csr.hip) are to be set from (a)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
U = 4


def dof_graph(elem_nodes, local_nodes):
    """CSR graph over the dofs that couples the listed local nodes of every element (all U unknowns of a node pair)"""
    en = np.asarray(elem_nodes).astype(np.int64)[:, local_nodes]
    n_nodes = int(np.asarray(elem_nodes).max()) + 1
    key = np.unique((en[:, :, None] * n_nodes + en[:, None, :]).ravel())
    ra, cb = key // n_nodes, key % n_nodes
    deg = np.bincount(ra, minlength=n_nodes).astype(np.int64)
    node_ptr = np.concatenate([[0], np.cumsum(deg)])
    row_len = np.repeat(deg * U, U)
    row_ptr = np.concatenate([[0], np.cumsum(row_len)]).astype(np.int64)
    col_ind = np.empty(int(row_ptr[-1]), dtype=np.int32)
    cols = (cb[:, None] * U + np.arange(U)).astype(np.int32)  # per node pair: the U columns, ascending
    for a in range(n_nodes):  # (node a's U rows are copies of one segment)
        seg = cols[node_ptr[a]:node_ptr[a + 1]].ravel()
        for u in range(U):
            r = a * U + u
            col_ind[row_ptr[r]:row_ptr[r + 1]] = seg
    return row_ptr, col_ind


def alternate(legs, reps):
    """legs: {name: fn}.  Every leg once as warm-up, then reps rounds of all legs in turn; {name: median seconds}"""
    import torch
    for fn in legs.values():
        fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in legs}
    for _ in range(reps):
        for k, fn in legs.items():
            t0 = time.perf_counter()
            for _ in range(5):
                fn()
            torch.cuda.synchronize()
            ts[k].append((time.perf_counter() - t0) / 5)
    return {k: float(np.median(v)) for k, v in ts.items()}


def run_case(ctx, p, graph, ne, reps):
    import torch
    from l3ster_amd import solve, system
    part = system.CubePartition(ne, p, perturb=0.1)
    mask = part.dirichlet_mask(U)
    mf = system.MatrixFreeSystem(system.DeviceMesh(ctx, part, U, mask), system.KERNEL_DIFFUSION3D, [1.0, 0.0], asm_opts=(1, 0, 0))
    n = part.n_local_nodes * U
    primary, _ = system.element_node_split(p)
    rp, ci = dof_graph(part.elem_nodes, primary if graph == "condensed" else np.arange((p + 1) ** 3))
    RP, CI = torch.as_tensor(rp, device="cuda"), torch.as_tensor(ci, device="cuda")
    vals = torch.zeros(len(ci), dtype=torch.float64, device="cuda")
    rhs = torch.zeros((1, n), dtype=torch.float64, device="cuda")
    t0 = time.perf_counter()
    missing = (mf.condense_global if graph == "condensed" else mf.assemble_global)(RP, CI, vals, rhs)
    torch.cuda.synchronize()
    t_fill = time.perf_counter() - t0
    assert missing == 0
    ops = {L: system.CsrOperator(ctx, RP, CI, vals, L) for L in (4, 16, 64, 0)}
    info = ops[0].info()
    x = torch.as_tensor(np.random.default_rng(0).standard_normal(n), device="cuda")
    y = torch.empty_like(x)
    legs = {f"lanes_{L or 'auto'}": (lambda op=op: op.apply(x, y)) for L, op in ops.items()}
    yardstick = None
    try:
        At = torch.sparse_csr_tensor(RP.to(torch.int32), CI, vals, size=(n, n))
        yt = torch.mv(At, x)
        ops[0].apply(x, y)
        yardstick = float((yt - y).norm() / y.norm())
        legs["torch_csr_mv"] = lambda: torch.mv(At, x)
    except Exception as e:  # (a torch build without the sparse back end: recorded, not hidden)
        yardstick = f"unavailable: {e}"
    t = alternate(legs, reps)
    bytes_moved = 12 * info.nnz + 8 * (n + 1) + 16 * n
    rec = dict(kernel="Diffusion3D", order=p, graph=graph, mesh=f"{ne}^3", n=n, nnz=info.nnz, empty_rows=info.n_empty_rows,
               max_row_len=info.max_row_len, mean_row_len=info.mean_row_len, automatic_lanes=info.lanes_per_row,
               matrix_gib=12 * info.nnz / 2 ** 30, fill_seconds=t_fill, bytes_counted=bytes_moved,
               apply_seconds=t, apply_gb_per_s={k: bytes_moved / v / 1e9 for k, v in t.items()},
               torch_csr_mv_rel_diff=yardstick)
    if graph == "condensed":
        dmask = torch.as_tensor(np.asarray(mask).astype(np.uint8).ravel()[:n], device="cuda")
        g = torch.as_tensor(np.where(np.asarray(mask).ravel()[:n] != 0, np.sin(0.37 * np.arange(n)), 0.0)[None, :], device="cuda")
        op = ops[0]
        op.dirichlet(dmask, g, rhs)
        minv = op.jacobi_inverse()
        diag, rhs_mf = mf.diag_rhs(g)
        minv_mf = solve.jacobi_inverse_native(ctx, diag)
        out = {}

        def csr_leg():
            X = torch.zeros((1, n), dtype=torch.float64, device="cuda")
            out["csr"] = solve.pcg(op, rhs[0], X[0], minv, tol=1e-8, residual_scaling="rhs", check_every=10)
            t1 = time.perf_counter()
            mf.recover_internal(X)
            torch.cuda.synchronize()
            out["recover_s"], out["x_csr"] = time.perf_counter() - t1, X[0]

        def mf_leg():
            xm = torch.zeros(n, dtype=torch.float64, device="cuda")
            out["mf"] = solve.pcg(mf, rhs_mf[0].contiguous(), xm, minv_mf, tol=1e-8, residual_scaling="rhs", check_every=10)
            out["x_mf"] = xm

        ts = {"csr": [], "mf": []}
        csr_leg(), mf_leg()
        for _ in range(3):
            for k, leg in (("csr", csr_leg), ("mf", mf_leg)):
                t1 = time.perf_counter()
                leg()
                torch.cuda.synchronize()
                ts[k].append(time.perf_counter() - t1)
        rec["pcg"] = dict(tol=1e-8, residual_scaling="rhs", condense_seconds=t_fill, recover_seconds=out["recover_s"],
                          csr_seconds_with_recovery=float(np.median(ts["csr"])), csr_iterations=out["csr"].num_iters,
                          matrix_free_seconds=float(np.median(ts["mf"])), matrix_free_iterations=out["mf"].num_iters,
                          solutions_rel_diff=float((out["x_csr"] - out["x_mf"]).norm() / out["x_mf"].norm()))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--cases", default="2:full:32,4:full:12,4:condensed:12")
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    import torch
    from l3ster_amd import system
    assert torch.cuda.is_available(), "bench_csr.py measures on the GPU; there is no fallback"
    torch.cuda.set_device(0)
    ctx = system.Context(0, torch.cuda.current_stream().cuda_stream)
    out = open(a.out, "a") if a.out else None
    for case in a.cases.split(","):
        p, graph, ne = case.split(":")
        line = json.dumps(run_case(ctx, int(p), graph, int(ne), a.reps))
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()


if __name__ == "__main__":
    main()
