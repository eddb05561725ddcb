"""Restarted GMRES on the device (l3k_gmres_*), one GPU: where the time of an Arnoldi step goes, what the orthogonalisation passes
reach of the HBM rate, and the time to 1e-10 next to the PCG on the same system.
    python tools/bench_gmres.py
Problems: Diffusion3D with a source, U = 4, hexes 64^3 at order 1 and 16^3 at order 4, Jacobi.  Per problem:
  passes   for k in --ks: the three orthogonalisation passes on k basis vectors through the exported pieces (l3k_gmres_multi_dot,
           l3k_gmres_project twice), the apply and the normalisation-sized copy, each as the median of --repeats timings between two
           events on the stream after one untimed call; bytes per pass as counted from device/gmres.hpp (the header of that file):
           registers (k < 8) and the LDS row tile (8 <= k < 256): multiDot k + 1 vectors, projectRedot k + 2; the chunked sweeps (the
           route of every k >= 8 when L3K_GMRES_TILE=0 is in the environment: the leg the tile is measured against; 16, 32 or 64
           there set the tile's LDS budget in KB): multiDot
           k + ceil((k + 1) / 8), projectRedot 2 k + 2 + ceil((k + 1) / 8); rate = bytes / time
  step     next_4_steps_mean_ms: (t(k + 4 steps) - t(k steps)) / 4 of solves cut off at max_iters within one cycle, on the host
           clock: the mean of the four steps that orthogonalise against k + 1 .. k + 4 vectors, apply and Jacobi included (the two
           solves share their allocation, first residual and combine up to 4 columns of the latter)
  solve    time to 1e-10 |b| of solve.gmres (restart_length 30 and 250) and of solve.pcg, median of --solve-repeats, after a warm-up
           (--no-solves leaves them out)
One JSON line per record on stdout and in profiles/gmres.jsonl (--out)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from l3ster_amd import capi, solve, system  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--problems", type=int, nargs="*", default=[64, 1, 16, 4], help="pairs: elements per edge, order")
ap.add_argument("--ks", type=int, nargs="*", default=[1, 4, 7, 8, 16, 30, 60])
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--solve-repeats", type=int, default=3)
ap.add_argument("--no-solves", action="store_true")
ap.add_argument("--tol", type=float, default=1e-10)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gmres.jsonl"))
a = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_gmres.py measures on the GPU: no device found")
torch.cuda.set_device(0)
ctx = system.Context(0, torch.cuda.current_stream().cuda_stream)
lib, U = capi.load(), 4
TILE_KB = int(os.environ.get("L3K_GMRES_TILE", "64"))
TILE = TILE_KB > 0


def vp(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def event_time(fn):
    """median milliseconds of fn() on the stream, one untimed call first"""
    fn()
    out = []
    for _ in range(a.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return statistics.median(out)


def host_time(fn, repeats=None):
    fn()
    out = []
    for _ in range(repeats or a.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return statistics.median(out), r


lines = []


def emit(rec):
    lines.append(rec)
    print(json.dumps(rec), flush=True)


for ne, p in zip(a.problems[::2], a.problems[1::2]):
    part = system.CubePartition(ne, p, perturb=0.1)
    mf = system.MatrixFreeSystem(system.DeviceMesh(ctx, part, U, part.dirichlet_mask(U)), system.KERNEL_DIFFUSION3D, [1.0, 1.0])
    diag, rhs = mf.diag_rhs(None)
    minv = solve.jacobi_inverse_native(ctx, diag)
    b = rhs[0].contiguous()
    n = b.numel()
    name = f"Diffusion3D with a source, hex {ne}^3, order {p}"
    ld = (n + 3) // 4 * 4
    kmax = max(a.ks)
    V = torch.randn((kmax, ld), dtype=torch.float64, device="cuda") / n ** 0.5
    w, z = torch.randn(n, dtype=torch.float64, device="cuda"), torch.empty(n, dtype=torch.float64, device="cuda")
    h1, h2, t3 = (torch.zeros(kmax + 1, dtype=torch.float64, device="cuda") for _ in range(3))
    t_apply = event_time(lambda: mf.apply(w[None, :], z[None, :]))
    t_copy = event_time(lambda: z.copy_(w))  # (one read, one write: the size of the normalisation)
    for k in a.ks:
        chunks = -(-(k + 1) // 8)
        fits = k * 17 + 528 <= TILE_KB * 128  # (a tile of 16 rows, the lowest)
        route = "registers" if k < 8 else "lds tile" if TILE and k < 256 and fits else "chunked sweeps"
        vec_dot, vec_proj = (k + chunks, 2 * k + 2 + chunks) if route == "chunked sweeps" else (k + 1, k + 2)
        t_dot = event_time(lambda: capi.check(lib.l3k_gmres_multi_dot(ctx._h, vp(V), ld, k, vp(w), vp(minv), n, vp(h1))))
        t_p1 = event_time(lambda: capi.check(lib.l3k_gmres_project(ctx._h, vp(V), ld, k, vp(w), vp(minv), n, vp(h1), vp(h2))))
        t_p2 = event_time(lambda: capi.check(lib.l3k_gmres_project(ctx._h, vp(V), ld, k, vp(w), vp(minv), n, vp(h2), vp(t3))))
        ws = solve.GmresWorkspace(ctx, n, k + 4)

        def cut(steps):
            x = torch.zeros_like(b)
            return solve.gmres(mf, b, x, minv, tol=0.0, max_iters=steps, check_every=10 ** 6, max_restarts=0, workspace=ws,
                               throw_on_fail=False)

        (t_lo, _), (t_hi, _) = host_time(lambda: cut(k)), host_time(lambda: cut(k + 4))
        ws.close()
        step_ms = (t_hi - t_lo) / 4 * 1e3
        gb = lambda vecs: vecs * n * 8 / 1e9
        emit({"record": "step", "problem": name, "dofs": n, "k": k, "apply_ms": t_apply, "multi_dot_ms": t_dot, "project_1_ms": t_p1,
              "project_2_ms": t_p2, "copy_ms": t_copy, "next_4_steps_mean_ms": step_ms, "route": route, "tile_lds_kb": TILE_KB if route == "lds tile" else None,
              "multi_dot_vectors": vec_dot, "project_vectors": vec_proj, "multi_dot_TBps": gb(vec_dot) / t_dot, "project_1_TBps": gb(vec_proj) / t_p1,
              "project_2_TBps": gb(vec_proj) / t_p2, "design_vectors_per_step": 3 * k + 7,
              "read_vectors_per_step": vec_dot + 2 * vec_proj + 2, "repeats": a.repeats})
    for leg, fn in () if a.no_solves else (("gmres(30)", lambda x: solve.gmres(mf, b, x, minv, tol=a.tol, residual_scaling="rhs", restart_length=30, max_restarts=10 ** 3,
                                                         max_iters=30000, check_every=5, throw_on_fail=False)),
                    ("gmres(250)", lambda x: solve.gmres(mf, b, x, minv, tol=a.tol, residual_scaling="rhs", restart_length=250, max_restarts=10 ** 3,
                                                          max_iters=30000, check_every=5, throw_on_fail=False)),
                    ("pcg", lambda x: solve.pcg(mf, b, x, minv, tol=a.tol, residual_scaling="rhs", max_iters=30000, check_every=5,
                                                throw_on_fail=False))):
        t, res = host_time(lambda: fn(torch.zeros_like(b)), a.solve_repeats)
        emit({"record": "solve", "problem": name, "dofs": n, "leg": leg, "tol": a.tol, "solve_s_median": t, "iterations": res.num_iters,
              "restarts": getattr(res, "restarts", None), "converged": res.converged, "achieved_tol": res.tol, "repeats": a.solve_repeats})
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    for line in lines:
        f.write(json.dumps(line) + "\n")
