"""A small numpy restatement (float64, dense, nothing sum-factorised) of assembleLocalSystem on a quad and on one of its sides
(algsys/AssembleLocalSystem.hpp:77-216) for an equation kernel given as a Python function:

    K = sum_q w_q jac_q B_q^T B_q,   F = sum_q w_q jac_q B_q^T f_q,
    B_q[:, a U + u] = A0[:, u] phi_a(q) + A1[:, u] dphi_a/dx(q) + A2[:, u] dphi_a/dy(q),   node a = ix + (p+1) iy.

The element basis at the points comes from the oracle's tables (O.ref_basis_at_qps, O.side_basis_at_qps), the geometry from
O.jacobi_mat (J[d][s] = dx_s / dxi_d), O.map_to_physical and O.boundary_geometry.  A kernel is

    kernel(vals [F], ders [2][F], point [3], normal [2] or None, time) -> (A0 [E][U], A1 [E][U], A2 [E][U], rhs [E][R])

`normal` is None for a domain kernel.  tests/test_quad_asm_ref_cpu.py proves this file against O.assemble_local and
O.assemble_local_side for the built-in kernels; the GPU tests then use it for plugin kernels with a source term, which the
oracle does not have."""
import numpy as np

import oracle_lib as O


def _assemble(kernel, side, p, nq, verts, node_fields, time):
    verts = np.ascontiguousarray(verts, dtype=np.float64).reshape(4, 3)
    if side is None:
        vals, ders, w, pts = O.ref_basis_at_qps(2, p, nq)
    else:
        vals, ders, w, pts = O.side_basis_at_qps(2, p, nq, side)
    N = vals.shape[1]
    nf = np.zeros((N, 0)) if node_fields is None else np.asarray(node_fields, dtype=np.float64).reshape(N, -1)
    K = F = None
    for q in range(len(w)):
        J = O.jacobi_mat(2, verts, pts[q])
        phys = np.linalg.solve(J, ders[q])  # d/dxi_d = sum_s J[d][s] d/dx_s
        if side is None:
            normal, jac = None, np.linalg.det(J)
        else:
            normal, jac = O.boundary_geometry(2, verts, pts[q], side)
        point = O.map_to_physical(2, verts, pts[q])
        A0, A1, A2, f = (np.asarray(m, dtype=np.float64) for m in kernel(vals[q] @ nf, phys @ nf, point, normal, time))
        B = (np.einsum("eu,a->eau", A0, vals[q]) + np.einsum("eu,a->eau", A1, phys[0]) + np.einsum("eu,a->eau", A2, phys[1]))
        B = B.reshape(A0.shape[0], -1)
        if K is None:
            K, F = np.zeros((B.shape[1], B.shape[1])), np.zeros((B.shape[1], f.shape[1]))
        K += w[q] * jac * (B.T @ B)
        F += w[q] * jac * (B.T @ f)
    return K, F


def element_system(kernel, p, nq, verts, node_fields=None, time=0.0):
    """(K [Nd][Nd], F [Nd][R]) of one quad: verts [4][3] (vertex i + 2j), node_fields [N][F] or None."""
    return _assemble(kernel, None, p, nq, verts, node_fields, time)


def side_system(kernel, side, p, nq, verts, node_fields=None, time=0.0):
    """... of the whole element from the nq points of one side (0 y-, 1 y+, 2 x-, 3 x+)."""
    return _assemble(kernel, side, p, nq, verts, node_fields, time)


# ---- the built-in 2-D kernels restated (l3ster_amd/csrc/user_kernels.hpp), R right-hand sides that are all zero
def diffusion2d(R=1):
    def kernel(vals, ders, point, normal, time):
        A0, A1, A2 = np.zeros((4, 3)), np.zeros((4, 3)), np.zeros((4, 3))
        A1[0, 1] = A2[0, 2] = -1.0
        A0[1, 1], A1[1, 0] = -1.0, 1.0
        A0[2, 2], A2[2, 0] = -1.0, 1.0
        A1[3, 2], A2[3, 1] = 1.0, -1.0
        return A0, A1, A2, np.zeros((4, R))
    return kernel


def diffusion2d_var(R=1):
    base = diffusion2d(R)

    def kernel(vals, ders, point, normal, time):
        A0, A1, A2, f = base(vals, ders, point, normal, time)
        A0[0, 1], A0[0, 2] = -ders[0][0], -ders[1][0]
        A1[0, 1] = A2[0, 2] = -vals[0]
        return A0, A1, A2, f
    return kernel


def adiabatic2d(R=1):
    def kernel(vals, ders, point, normal, time):
        A0 = np.zeros((1, 3))
        A0[0, 1], A0[0, 2] = normal[0], normal[1]
        return A0, np.zeros((1, 3)), np.zeros((1, 3)), np.zeros((1, R))
    return kernel
