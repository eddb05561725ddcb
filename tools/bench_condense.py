"""Rate of static condensation on the assembled path: l3k_condense_global (element systems formed, the internal dofs eliminated
by the kernels of device/condense.hpp, S_e / g_e summed into a condensed CSR graph) for Diffusion3D at orders 2, 4 and 6.

    python tools/bench_condense.py [--out profiles/condense.jsonl] [--cases 2:16,4:8,6:4,6:6] [--reps 3]

Per case, one JSON line: elements/s of the whole call; the flops per element of the elimination with W^T W formed as a
triangle (FLOPS below) and the executed fraction of the 78.6 TFLOP/s FP64 peak; the time split between assembly (l3k_local_assemble
of the same elements), condensation (l3k_condense_local minus the assembly: the elimination and the S_e / g_e stores) and scatter
(l3k_condense_global minus l3k_condense_local); and the seconds per element of a host LAPACK Schur complement (numpy Cholesky +
triangular solves) on a sample of the same element matrices.  Times are medians of --reps runs after one warm-up run."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK = 78.6e12  # FP64 (vector and matrix) peak of the MI355X, FLOP/s


def flops_per_element(Nid, Nbd, R):
    """Cholesky of K_ii (Nid^3 / 3), W = L^-1 K_ib (Nbd Nid^2), the triangle of W^T W (Nbd^2 Nid), and the R right-hand sides:
    h = L^-1 F_i (R Nid^2) and W^T h (2 R Nbd Nid)."""
    return Nid ** 3 / 3 + Nbd * Nid ** 2 + Nbd ** 2 * Nid + R * (Nid ** 2 + 2 * Nbd * Nid)


def timed(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def host_schur(K, F, b, i):
    import scipy.linalg as sl
    t0 = time.perf_counter()
    L = np.linalg.cholesky(K[np.ix_(i, i)])
    W = sl.solve_triangular(L, np.concatenate([K[np.ix_(i, b)], F[i]], axis=1), lower=True)
    S = K[np.ix_(b, b)] - W[:, :len(b)].T @ W[:, :len(b)]
    g = F[b] - W[:, :len(b)].T @ W[:, len(b):]
    return time.perf_counter() - t0, S, g


def run_case(ctx, p, ne, reps):
    import torch
    from l3ster_amd import system
    U, R = 4, 1
    part = system.CubePartition(ne, p, perturb=0.1)
    mesh = system.DeviceMesh(ctx, part, U, part.dirichlet_mask(U))
    mf = system.MatrixFreeSystem(mesh, system.KERNEL_DIFFUSION3D, [1.0, 1.0], asm_opts=(1, 0, 0), n_rhs=R)
    primary, internal = system.element_node_split(p)
    Nid, Nbd, E = len(internal) * U, len(primary) * U, part.n_elems
    rp, ci = system.condensed_graph(part.elem_nodes, p, U, np.arange(U))
    RP, CI = torch.as_tensor(rp, device="cuda"), torch.as_tensor(ci, device="cuda")
    vals = torch.zeros(len(ci), dtype=torch.float64, device="cuda")
    rhs = torch.zeros((R, part.n_local_nodes * U), dtype=torch.float64, device="cuda")
    Nd = (p + 1) ** 3 * U
    # (assembly and condense_local on chunks that fit beside the outputs: 4 GiB of K_e per call)
    chunk = max(1, min(E, (4 << 30) // (8 * Nd * Nd)))
    Kbuf = torch.empty((chunk, Nd, Nd), dtype=torch.float64, device="cuda")
    Sbuf = torch.empty((chunk, Nbd, Nbd), dtype=torch.float64, device="cuda")
    Gbuf = torch.empty((chunk, R, Nbd), dtype=torch.float64, device="cuda")
    lib = system.capi.load()

    def each_chunk(f):
        for first in range(0, E, chunk):
            f(first, min(chunk, E - first))

    def asm():
        each_chunk(lambda f, n: mf.local_assemble_into(Kbuf, f, n))

    def cond_local():
        import ctypes as C
        each_chunk(lambda f, n: system.check(lib.l3k_condense_local(mf._h, f, n, C.c_void_p(Sbuf.data_ptr()), C.c_void_p(Gbuf.data_ptr()))))

    def cond_global():
        vals.zero_()
        rhs.zero_()
        mf.condense_global(RP, CI, vals, rhs)

    t_glob = timed(cond_global, reps)
    t_asm = timed(asm, reps)
    t_loc = timed(cond_local, reps)
    fl = flops_per_element(Nid, Nbd, R)
    # host LAPACK on a sample of the same element systems
    K, Fe, _ = mf.local_assemble(0, min(4, E))
    K, Fe = K.cpu().numpy(), Fe.cpu().numpy()
    b = (primary[:, None] * U + np.arange(U)).ravel()
    i = (internal[:, None] * U + np.arange(U)).ravel()
    host = [host_schur(K[e], Fe[e].T, b, i)[0] for e in range(len(K))]
    host_s = float(np.median(host))
    return dict(kernel="Diffusion3D", order=p, mesh=f"{ne}^3", elements=E, unknowns=U, n_rhs=R, internal_dofs=Nid, primary_dofs=Nbd,
                graph_nnz=int(len(ci)), seconds=t_glob, elements_per_s=E / t_glob, flops_per_element=fl,
                flops_formula="Nid^3/3 + Nbd*Nid^2 + Nbd^2*Nid + R*(Nid^2 + 2*Nbd*Nid)", tflops=fl * E / t_glob / 1e12,
                fraction_of_fp64_peak=fl * E / t_glob / PEAK,
                split_s=dict(assembly=t_asm, condensation=max(t_loc - t_asm, 0.0), scatter=max(t_glob - t_loc, 0.0)),
                condensation_only_fraction_of_peak=fl * E / max(t_loc - t_asm, 1e-12) / PEAK,
                host_lapack_s_per_element=host_s, host_lapack_elements_per_s=1.0 / host_s,
                speedup_vs_host_one_core=(E / t_glob) * host_s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--cases", default="2:16,4:8,6:4,6:6")
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    import torch
    from l3ster_amd import system
    torch.cuda.set_device(0)
    ctx = system.Context(0, torch.cuda.current_stream().cuda_stream)
    out = open(a.out, "a") if a.out else None
    for case in a.cases.split(","):
        p, ne = (int(v) for v in case.split(":"))
        r = run_case(ctx, p, ne, a.reps)
        line = json.dumps(r)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()


if __name__ == "__main__":
    main()
