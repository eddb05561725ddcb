"""The collective PCG of a partitioned system restated in numpy over the host matrices of tests/asm_dist_ref.py: the all-reduce that
adds the ranks' values in ascending rank order (l3k_halo_allreduce_sum), the partitioned apply in the sub-assembled form (import,
local matrix, export-add), and the Jacobi iteration of l3k_pcg_solve with every dot product taken rank by rank over the owned rows
and summed in rank order.  tests/test_pcg_dist_cpu.py proves this file on the CPU against tests/cg_ref.py on the whole matrix; it is
the reference of tests/test_gpu_pcg_dist.py.  Everything is float64 and dense; the meshes are small."""
import numpy as np

import asm_dist_ref as AD


def sum_in_rank_order(rows):
    """rows [world][count] -> ((rows[0] + rows[1]) + ...) + rows[world - 1], entry by entry: what every rank holds after
    l3k_halo_allreduce_sum"""
    rows = np.asarray(rows, dtype=np.float64)
    acc = rows[0].copy()
    for r in range(1, rows.shape[0]):
        acc = acc + rows[r]
    return acc


def order_dependent_rows(world, count):
    """[world][count] values whose sum depends on the order of the additions: 1e16, 1, -1e16, 3 dealt over the ranks, shifted by the
    column, with a small distinct term so that no two columns agree"""
    base = [1e16, 1.0, -1e16, 3.0]
    return np.array([[base[(r + c) % 4] * (1.0 + 0.125 * c) + 0.5 * r for c in range(count)] for r in range(world)], dtype=np.float64)


def chain(world, count, steps, start):
    """s_r <- 0.5 * allreduce(s)_r + r, `steps` times from start [world][count]: what rank r holds at the end, [world][count]"""
    s = np.asarray(start, dtype=np.float64).copy()
    for _ in range(steps):
        total = sum_in_rank_order(s)
        s = np.array([0.5 * total + float(r) for r in range(world)])
    return s


# ------------------------------------------------------------------------------------------------ the partitioned system
def closed_system(q):
    """The ranks' local matrices after the Dirichlet step with the owner rule, and the owned right-hand sides after the export-add:
    (mats [r] dense over the local dofs, b [r] over the owned rows, A the whole matrix = sum_r R_r^T A_r R_r, b_whole)"""
    g = AD.prescribed_values(q)
    mats, vecs = [], []
    for r in range(q.world):
        A, rhs, _ = AD.local_system(q, q.parts[r], q.part_sides[r], q.elem_of[r])
        A, rhs = AD.dirichlet_owner_rule(A, rhs, q.local_mask(r), g[:, q.local_dofs(r)], q.n_owned(r))
        mats.append(A)
        vecs.append(rhs)
    b_whole = AD.export_add(q, vecs)[0]
    return mats, [q.scatter(b_whole, r)[0] for r in range(q.world)], AD.sum_of_ranks(q, mats), b_whole


def dist_apply(q, mats, x):
    """y_r = the owned rows of A x from the ranks' owned x_r: import (every rank reads its ghost values from their owners), the local
    matrix, export-add (the ghost rows of the local products are added into their owners' rows)"""
    whole = q.gather([v[None, :] for v in x])[0]
    y = AD.export_add(q, [(mats[r] @ whole[q.local_dofs(r)])[None, :] for r in range(q.world)])
    return [q.scatter(y, r)[0] for r in range(q.world)]


def dist_dot(u, v):
    """<u, v>: every rank's share over its owned rows, the shares added in rank order"""
    return float(sum_in_rank_order([[np.dot(a, b)] for a, b in zip(u, v)])[0])


def dist_diag(q, mats):
    """the diagonal of the whole matrix on every rank's owned rows"""
    d = AD.export_add(q, [np.diag(M)[None, :] for M in mats])
    return [q.scatter(d, r)[0] for r in range(q.world)]


def pcg(q, mats, b, x0, minv, tol, max_iters, residual_scaling="rhs"):
    """Jacobi-PCG on the partitioned system, the loop of l3k_pcg_solve (rows with minv == 0 frozen and out of <r, r>); b, x0, minv:
    per-rank arrays over the owned rows.  Returns (x per rank, iterations, scaled residual)."""
    ranks = range(q.world)
    x = [np.array(v, dtype=np.float64) for v in x0]
    live = [m != 0 for m in minv]
    ax = dist_apply(q, mats, x)
    r = [np.where(live[k], b[k] - ax[k], 0.0) for k in ranks]
    z = [minv[k] * r[k] for k in ranks]
    p = [v.copy() for v in z]
    rz, rr = dist_dot(r, z), dist_dot(r, r)
    scale = {"none": 1.0, "initial": np.sqrt(rr) if rr > 0 else 1.0, "rhs": max(np.sqrt(dist_dot(b, b)), 1e-300)}[residual_scaling]
    res, it = np.sqrt(rr) / scale, 0
    while res > tol and it < max_iters:
        ap = dist_apply(q, mats, p)
        alpha = rz / dist_dot(p, ap)
        x = [np.where(live[k], x[k] + alpha * p[k], x[k]) for k in ranks]
        r = [np.where(live[k], r[k] - alpha * ap[k], 0.0) for k in ranks]
        z = [minv[k] * r[k] for k in ranks]
        rz_new, rr = dist_dot(r, z), dist_dot(r, r)
        p = [z[k] + (rz_new / rz) * p[k] for k in ranks]
        rz = rz_new
        it += 1
        res = np.sqrt(rr) / scale
    return x, it, res
