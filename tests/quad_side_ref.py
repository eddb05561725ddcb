"""A short numpy restatement of one quad side's boundary operator, built from the oracle's side basis and geometry
(side_basis_at_qps, jacobi_mat, boundary_geometry, map_to_physical): K = sum_q w_q |J_t| B_q^T B_q and F = sum_q w_q |J_t| B_q^T f_q
with B_q[e, b*U + u] = A0[e, u] phi_b + A1[e, u] dphi_b/dx + A2[e, u] dphi_b/dy.  Kernels are numpy callables
kernel(field_vals [F], field_ders [2][F], point [3], time, normal [2]) -> (A0, A1, A2 [E][U], rhs [E][R]).  Used by the CPU test
against the oracle's Adiabatic2D and by the GPU tests for a boundary plugin kernel the oracle does not know."""
import numpy as np

import oracle_lib as O


def side_system(kernel, U, E, p, nq, side, verts, node_fields=None, time=0.0, R=1):
    """(K [N*U][N*U], F [N*U][R]) of one side of one quad; node_fields [N][F] (None: no fields)."""
    vals, ders, w, pts = O.side_basis_at_qps(2, p, nq, side)
    N = (p + 1) ** 2
    K, F = np.zeros((N * U, N * U)), np.zeros((N * U, R))
    for q in range(len(w)):
        J = O.jacobi_mat(2, verts, pts[q])  # J[d][s] = dx_s / dxi_d
        nrm, jac = O.boundary_geometry(2, verts, pts[q], side)
        xyz = O.map_to_physical(2, verts, pts[q])
        dphys = np.linalg.solve(J, ders[q])  # [2][N]: dphi_b / dx_s
        fv = np.zeros(0) if node_fields is None else vals[q] @ node_fields
        fd = np.zeros((2, 0)) if node_fields is None else dphys @ node_fields
        A0, A1, A2, rhs = kernel(fv, fd, xyz, time, nrm)
        B = np.zeros((E, N * U))
        for u in range(U):
            B[:, u::U] = np.outer(A0[:, u], vals[q]) + np.outer(A1[:, u], dphys[0]) + np.outer(A2[:, u], dphys[1])
        K += w[q] * jac * B.T @ B
        F += w[q] * jac * B.T @ np.asarray(rhs).reshape(E, R)
    return K, F


def adiabatic2d(fv, fd, xyz, t, n):
    """The oracle's boundary kernel 5 (U = 3, E = 1): q . n = 0."""
    A0, A1, A2 = np.zeros((1, 3)), np.zeros((1, 3)), np.zeros((1, 3))
    A0[0, 1], A0[0, 2] = n[0], n[1]
    return A0, A1, A2, np.zeros((1, 1))


# A boundary kernel with every ingredient (U = 2, E = 2, F = 1, R = 2): non-zero A0, A1 and A2 and rhs, reading the normal, the
# point, the time and the field's value and derivatives.  PLUGIN_SRC is the same functor for the device.
def wall_plugin(fv, fd, xyz, t, n):
    x, y = xyz[0], xyz[1]
    h = 1.0 + 0.5 * np.sin(x - 2.0 * y + t)
    A0, A1, A2 = np.zeros((2, 2)), np.zeros((2, 2)), np.zeros((2, 2))
    A0[0, 0] = h * fv[0]
    A0[0, 1] = n[0]
    A0[1, 1] = 1.0 + x * y
    A1[0, 0] = n[0]
    A2[0, 0] = n[1]
    A1[1, 1] = 0.3 * n[1]
    A2[1, 0] = 0.2 + fd[0][0]
    A1[1, 0] = 0.1 * fd[1][0]
    rhs = np.array([[h, 2.0 * h], [t + x, t - y]])
    return A0, A1, A2, rhs


PLUGIN_SRC = """
struct QuadWallPlugin {
    static constexpr l3k::KernelParams params{.dimension = 2, .n_equations = 2, .n_unknowns = 2, .n_fields = 1, .n_rhs = 2};
    template <typename In, typename Out> L3K_HD void operator()(const In& in, Out& out) const {
        const double x = in.point.space.x(), y = in.point.space.y(), t = in.point.time;
        const double h = 1. + .5 * sin(x - 2. * y + t);
        auto& [operators, rhs] = out;
        auto& [A0, A1, A2] = operators;
        A0(0, 0) = h * in.field_vals[0];
        A0(0, 1) = in.normal[0];
        A0(1, 1) = 1. + x * y;
        A1(0, 0) = in.normal[0];
        A2(0, 0) = in.normal[1];
        A1(1, 1) = .3 * in.normal[1];
        A2(1, 0) = .2 + in.field_ders[0][0];
        A1(1, 0) = .1 * in.field_ders[1][0];
        rhs(0, 0) = h;
        rhs(0, 1) = 2. * h;
        rhs(1, 0) = t + x;
        rhs(1, 1) = t - y;
    }
};"""


def mesh_side_system(kernel, U, E, part, nq, face_elem, face_side, dofs_per_node, field_inds, node_fields=None, time=0.0, R=1):
    """The side systems of a mesh assembled into (K, F) over its local dofs (node * dofs_per_node + field_inds[u])."""
    p = part.order
    n_dofs = part.n_local_nodes * dofs_per_node
    K, F = np.zeros((n_dofs, n_dofs)), np.zeros((n_dofs, R))
    for e, s in zip(face_elem, face_side):
        nodes = part.elem_nodes[e].astype(np.int64)
        nf = None if node_fields is None else node_fields[:, nodes].T
        Ke, Fe = side_system(kernel, U, E, p, nq, int(s), part.elem_verts[e], nf, time, R)
        dofs = (nodes[:, None] * dofs_per_node + np.asarray(field_inds)[None, :U]).reshape(-1)
        K[np.ix_(dofs, dofs)] += Ke
        F[dofs] += Fe
    return K, F
