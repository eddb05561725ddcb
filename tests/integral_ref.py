"""A plain numpy restatement (float64; no oracle, no torch, no device library) of the hex post-processing operations:
integrals of residual kernels over elements / element sides (post/Integral.hpp, post/NormL2.hpp) and the residual kernel
evaluated at the nodes (algsys/ComputeValuesAtNodes.hpp).  Dense like the reference: the full element basis at every point,
B[q][node] and dB[q][3][node], built once per (p, points); nothing is sum-factorised.

Conventions (mesh/ElementTraits.hpp): node ix + n*iy + n^2*iz on the GLL grid, vertex i + 2j + 4k, sides 0 z-, 1 z+, 2 y-,
3 y+, 4 x-, 5 x+.  J[d][s] = dx_s / dxi_d.  A residual is a numpy callable
    residual(vals [..., F], ders [..., 3, F], point [..., 3], normal [..., 3] or None, time) -> [..., E]
`normal` is None where the device hands the kernel an input without a normal (domain integrals)."""
import functools

import numpy as np
from numpy.polynomial import legendre as L

# side -> (normal axis, tangential axes (ascending), sign of the outward normal against t1 x t2, reference coordinate of the side)
# z-: x^ x y^ = z^ points inwards -> -1;  y-: x^ x z^ = -y^ outwards -> +1;  x-: y^ x z^ = x^ inwards -> -1; the upper sides opposite
SIDES = {0: (2, (0, 1), -1.0, -1.0), 1: (2, (0, 1), 1.0, 1.0), 2: (1, (0, 2), 1.0, -1.0), 3: (1, (0, 2), -1.0, 1.0),
         4: (0, (1, 2), -1.0, -1.0), 5: (0, (1, 2), 1.0, 1.0)}


@functools.lru_cache(maxsize=None)
def gll_nodes(n):
    """The n Gauss-Lobatto-Legendre points: -1, the roots of P'_{n-1}, 1."""
    c = np.zeros(n)
    c[-1] = 1.0
    d1, d2 = L.legder(c), L.legder(c, 2)
    x = np.sort(L.legroots(d1).real) if n > 2 else np.zeros(0)
    for _ in range(2):  # Newton polish of the companion-matrix roots
        x = x - L.legval(x, d1) / L.legval(x, d2)
    return np.concatenate([[-1.0], x, [1.0]])


@functools.lru_cache(maxsize=None)
def gauss_rule(nq):
    return L.leggauss(nq)


def lagrange_1d(nodes, x):
    """(V [len(x)][n], D [len(x)][n]): the Lagrange polynomials on `nodes` and their derivatives at the points x."""
    nodes, x = np.asarray(nodes, float), np.asarray(x, float)
    n = len(nodes)
    V, D = np.ones((len(x), n)), np.zeros((len(x), n))
    for j in range(n):
        others = [m for m in range(n) if m != j]
        for m in others:
            V[:, j] *= (x - nodes[m]) / (nodes[j] - nodes[m])
        for k in others:
            term = np.full(len(x), 1.0 / (nodes[j] - nodes[k]))
            for m in others:
                if m != k:
                    term *= (x - nodes[m]) / (nodes[j] - nodes[m])
            D[:, j] += term
    return V, D


def tensor_tables(p, pts):
    """B [Q][N], dB [Q][3][N] of the order-p GLL Lagrange basis at the tensor grid pts[0] x pts[1] x pts[2] (x fastest in q)."""
    g = gll_nodes(p + 1)
    V, D = zip(*(lagrange_1d(g, a) for a in pts))
    Q, N = len(pts[0]) * len(pts[1]) * len(pts[2]), (p + 1) ** 3
    B = np.einsum("ax,by,cz->cbazyx", V[0], V[1], V[2]).reshape(Q, N)
    dB = np.stack([np.einsum("ax,by,cz->cbazyx", D[0], V[1], V[2]).reshape(Q, N),
                   np.einsum("ax,by,cz->cbazyx", V[0], D[1], V[2]).reshape(Q, N),
                   np.einsum("ax,by,cz->cbazyx", V[0], V[1], D[2]).reshape(Q, N)], axis=1)
    return B, dB


@functools.lru_cache(maxsize=None)
def point_tables(p, kind, nq, side):
    """Everything that depends on (p, point set, side or domain) only: the points are the tensor Gauss rule (kind 'gauss') or the
    GLL nodes themselves (kind 'nodes'), on the element (side None) or on one of its sides.  Returns a dict with the basis tables
    B, dB, the tables of the trilinear map S [Q][8], dS [Q][3][8], the weights w [Q] and node [Q]: the element node under each
    point (kind 'nodes' only)."""
    if kind == "gauss":
        x1, w1 = gauss_rule(nq)
    else:
        x1, w1 = gll_nodes(p + 1), np.ones(p + 1)
    pts, wts = [x1] * 3, [w1] * 3
    if side is not None:
        axis, _, _, end = SIDES[side]
        pts[axis], wts[axis] = np.array([end]), np.ones(1)
    B, dB = tensor_tables(p, pts)
    S, dS = tensor_tables(1, pts)  # the order-1 basis on the nodes -1, 1 is the trilinear map, vertex i + 2j + 4k
    w = np.einsum("a,b,c->cba", *wts).reshape(-1)
    node = None
    if kind == "nodes":  # the element node under each point: the side's end on its normal axis
        n = p + 1
        idx = [np.arange(n)] * 3
        if side is not None:
            idx[axis] = np.array([p if end > 0 else 0])
        node = (idx[0][None, None, :] + n * idx[1][None, :, None] + n * n * idx[2][:, None, None]).reshape(-1)
    return dict(B=B, dB=dB, S=S, dS=dS, w=w, node=node)


def evaluate(tab, side, elem_nodes, elem_verts, fields, residual, time):
    """The residual at every point of `tab` in every listed element: (values [e][Q][E], measure [e][Q]) with measure = |det J|
    on elements and |dx/dxi_t1 x dx/dxi_t2| on sides (the weights are not in it)."""
    verts = np.asarray(elem_verts, float).reshape(-1, 8, 3)
    en = np.asarray(elem_nodes).astype(np.int64)
    local = np.zeros((0,) + en.shape) if fields is None else np.asarray(fields, float)[:, en]  # [F][e][N]
    point = np.einsum("qv,evs->eqs", tab["S"], verts)
    J = np.einsum("qdv,evs->eqds", tab["dS"], verts)
    vals = np.tensordot(tab["B"], local, axes=([1], [2])).transpose(2, 0, 1)  # [q][f][e] -> [e][q][f]
    ders_ref = np.tensordot(tab["dB"], local, axes=([2], [2])).transpose(3, 0, 1, 2)  # [q][d][f][e] -> [e][q][d][f]
    # d/dxi_d = sum_s J[d][s] d/dx_s: the physical derivatives solve J g = g_ref
    ders = np.linalg.solve(J, ders_ref) if local.shape[0] else ders_ref
    if side is None:
        measure, normal = np.abs(np.linalg.det(J)), None
    else:
        _, (t1, t2), sign, _ = SIDES[side]
        cr = np.cross(J[:, :, t1, :], J[:, :, t2, :])
        measure = np.linalg.norm(cr, axis=-1)
        normal = sign * cr / measure[..., None]
    return np.asarray(residual(vals, ders, point, normal, time), float), measure, normal


def _by_side(face_elem, face_side):
    fe, fs = np.asarray(face_elem, np.int64).reshape(-1), np.asarray(face_side, np.int64).reshape(-1)
    assert fe.shape == fs.shape
    return [(int(s), fe[fs == s]) for s in np.unique(fs)]


def integrate(elem_nodes, elem_verts, fields, p, nq, residual, square, face_elem=None, face_side=None, time=0.0):
    """Integral of the residual (of its square: `square`) over all elements, or over the listed sides (a side listed twice
    counts twice).  fields [F][n_nodes] or None.  Returns [E]."""
    en, ev = np.asarray(elem_nodes), np.asarray(elem_verts, float).reshape(-1, 8, 3)
    groups = [(None, np.arange(en.shape[0]))] if face_elem is None else _by_side(face_elem, face_side)
    total = 0.0
    for side, elems in groups:
        tab = point_tables(p, "gauss", nq, side)
        r, measure, _ = evaluate(tab, side, en[elems], ev[elems], fields, residual, time)
        total = total + np.einsum("q,eq,eqi->i", tab["w"], measure, r * r if square else r)
    return np.atleast_1d(total)


def values_at_nodes(elem_nodes, elem_verts, fields, p, residual, dof_inds, dofs_per_node, n_nodes, face_elem=None,
                    face_side=None, time=0.0):
    """The residual at the nodes of all elements, or of the listed sides, through the GLL differentiation matrix: equation i is
    added to dof `node * dofs_per_node + dof_inds[i]`, with one count per visit.  The domain form hands the kernel a zero normal
    (valuesAtNodesKernel builds a boundary input either way).  Returns (sum, count), each [n_nodes * dofs_per_node]."""
    en, ev = np.asarray(elem_nodes), np.asarray(elem_verts, float).reshape(-1, 8, 3)
    groups = [(None, np.arange(en.shape[0]))] if face_elem is None else _by_side(face_elem, face_side)
    s, c = np.zeros(n_nodes * dofs_per_node), np.zeros(n_nodes * dofs_per_node)
    di = np.asarray(dof_inds, np.int64)
    for side, elems in groups:
        tab = point_tables(p, "nodes", 0, side)
        if side is None:
            kernel = lambda v, d, x, n, t: residual(v, d, x, np.zeros_like(x), t)
        else:
            kernel = residual
        r, _, _ = evaluate(tab, side, en[elems], ev[elems], fields, kernel, time)
        dofs = en[elems].astype(np.int64)[:, tab["node"], None] * dofs_per_node + di[None, None, :]
        np.add.at(s, dofs.reshape(-1), r.reshape(-1))
        np.add.at(c, dofs.reshape(-1), 1.0)
    return s, c


def node_coords(elem_nodes, elem_verts, p, n_nodes):
    """Physical location of every node (the trilinear map at the GLL positions), [n_nodes][3]."""
    tab = point_tables(p, "nodes", 0, None)
    xyz = np.einsum("qv,evs->eqs", tab["S"], np.asarray(elem_verts, float).reshape(-1, 8, 3))
    out = np.zeros((n_nodes, 3))
    out[np.asarray(elem_nodes).astype(np.int64)[:, tab["node"]].reshape(-1)] = xyz.reshape(-1, 3)
    return out


# ---------------------------------------------------------------------------------------------------------- residual kernels
def diffusion3d_error(k, s):
    """Diffusion3DError (benchmarks/Diffusion3D.hpp:81-103): fields (T, qx, qy, qz)."""
    def residual(vals, ders, point, normal, time):
        return np.stack([k * (ders[..., 0, 1] + ders[..., 1, 2] + ders[..., 2, 3]) + s, ders[..., 0, 0] - vals[..., 1],
                         ders[..., 1, 0] - vals[..., 2], ders[..., 2, 0] - vals[..., 3]], axis=-1)
    return residual


def linear3d_error(vals, ders, point, normal, time):
    return np.stack([vals[..., 0] - point[..., 0], vals[..., 1] - 1.0, vals[..., 2], vals[..., 3]], axis=-1)


def unit3d(vals, ders, point, normal, time):
    return np.ones(point.shape[:-1] + (1,))


def coordx3d(vals, ders, point, normal, time):
    return point[..., :1].copy()


def probe3d(vals, ders, point, normal, time):
    """The probe plugin of test_gpu_hex_integrals.py (2 fields, 8 equations): every input of a residual kernel on its own."""
    out = np.zeros(point.shape[:-1] + (8,))
    out[..., 0:3] = ders[..., :, 0]
    out[..., 3] = vals[..., 1] * (1.0 + time)
    out[..., 4] = point @ np.array([1.0, 2.0, 4.0])
    if normal is not None:
        out[..., 5] = np.einsum("...s,...s->...", ders[..., :, 0], normal)
        out[..., 6] = normal @ np.array([1.0, 2.0, 4.0])
        out[..., 7] = ders[..., 2, 1] * normal[..., 1]
    return out


PROBE_SRC = """
struct HexProbeResidual {
    static constexpr l3k::KernelParams params{.dimension = 3, .n_equations = 8, .n_fields = 2};
    template <typename In, typename Out> L3K_HD void operator()(const In& in, Out& out) const {
        out[0] = in.field_ders[0][0];
        out[1] = in.field_ders[1][0];
        out[2] = in.field_ders[2][0];
        out[3] = in.field_vals[1] * (1. + in.point.time);
        out[4] = in.point.space.x() + 2. * in.point.space.y() + 4. * in.point.space.z();
        if constexpr (requires(const In& i) { i.normal; }) {
            out[5] = in.field_ders[0][0] * in.normal[0] + in.field_ders[1][0] * in.normal[1] + in.field_ders[2][0] * in.normal[2];
            out[6] = in.normal[0] + 2. * in.normal[1] + 4. * in.normal[2];
            out[7] = in.field_ders[2][1] * in.normal[1];
        }
    }
};"""


def poly_fields(xyz):
    """T = x^2 + 3xy - 2yz + z^2 and q = grad T at the points xyz [n][3], as the fields (T, qx, qy, qz) [4][n]; div q = 4."""
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    return np.stack([x * x + 3 * x * y - 2 * y * z + z * z, 2 * x + 3 * y, 3 * x - 2 * z, -2 * y + 2 * z])


def rel_max(a, b):
    """Error of the vector a against b, relative to b's largest component."""
    a, b = np.asarray(a, float), np.asarray(b, float)
    return np.abs(a - b).max() / np.abs(b).max()
