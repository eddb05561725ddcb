"""Host-side mirror of the reference's interface for the hot path, on top of the C ABI (include/l3k.h).

Mirrors (names, argument meaning, error behaviour) for this path only:
  * tables            -- math::getLobattoRuleAbsc, quad::getReferenceQuadrature, SumFactorization tables
  * CubePartition     -- generateAndDistributeMesh for structured cubes (comm/DistributeMesh.hpp:284-299)
  * SquarePartition   -- makeSquareMesh + convertMeshToOrder on one part (quads, mesh/primitives/SquareMesh.hpp)
  * ElevatedMesh      -- readMesh + convertMeshToOrder for unstructured quads / hexes, boundaries by physical id (getBoundary)
  * MatrixFreeSystem  -- algsys::MatrixFreeSystem: assembleProblem -> Operator.apply(X, Y, alpha, beta)
                         (algsys/MatrixFreeSystem.hpp:24-89,1020-1140)
  * MultiTermSystem   -- ... as the sum of several assembleProblem calls: kernels by domain and by dof set (:24-89, 789-802)
Vectors are torch tensors of shape (ncols, n_owned_dofs), i.e. column-major [row][col] multivectors with owned rows
only -- the host-view layout of the Tpetra multivectors of the reference.  torch is plumbing here (device memory,
streams); all compute goes through libl3k.so.
"""
import contextlib
import ctypes as C

import numpy as np

from . import capi
from .capi import L3KError, check

KERNEL_DIFFUSION3D = 0
KERNEL_DIFFUSION3D_VAR = 1
KERNEL_DIFFUSION2D = 2  # quads: E = 4, U = 3 (T, qx, qy)
KERNEL_DIFFUSION2D_VAR = 3  # quads, diffusivity as an external field (F = 1)
KERNEL_ADVDIFF3D = 4
KERNEL_MASS3D = 8  # A0 = I: known answers for w * detJ
KERNEL_DIFFUSION3D_POINT = 10  # operators and rhs read point.space.{x,y,z} and point.time
KERNEL_ADVECTION3D = 11  # scalar BDF3 advection, U = E = 1, F = 3, velocity from the point
KERNEL_DIVCURL3D = 12  # div-curl system, U = 3, E = 4
KERNEL_ADIABATIC2D = 5  # boundary equation kernel on quads: U = 3 (T, qx, qy), q . n = 0
KERNEL_ADIABATIC3D = 6  # boundary equation kernels
KERNEL_ROBIN3D = 7
KERNEL_NORMALFLUX3D = 9  # boundary kernel with derivative operators (A1..A3)
KERNEL_ROBINPOINT3D = 14  # boundary kernel whose coefficients read point.space and point.time
RESIDUAL_DIFFUSION3D_ERROR = 0
RESIDUAL_LINEAR3D_ERROR = 2
RESIDUAL_UNIT3D = 4
RESIDUAL_COORDX3D = 6
RESIDUAL_LINEAR2D_ERROR = 1  # quads: fields (T, qx, qy), error against T = x, q = (1, 0)
RESIDUAL_UNIT2D = 3  # quads: integrand 1
RESIDUAL_COORDX2D = 5  # quads: out[0] = x (Dirichlet values)


# ------------------------------------------------------------------------------------------------------- tables
def gll_nodes(n):
    x = np.zeros(n)
    check(capi.load().l3k_gll_nodes(n, x.ctypes.data_as(capi.c_double_p)))
    return x


def gl_rule(nq):
    x, w = np.zeros(nq), np.zeros(nq)
    check(capi.load().l3k_gl_rule(nq, x.ctypes.data_as(capi.c_double_p), w.ctypes.data_as(capi.c_double_p)))
    return x, w


def n_qps1d(p, value_order=1, derivative_order=0):
    return capi.load().l3k_n_qps1d(p, value_order, derivative_order)


def basis_1d(p, nq):
    I, D = np.zeros((p + 1, nq)), np.zeros((p + 1, nq))
    check(capi.load().l3k_basis_1d(p, nq, I.ctypes.data_as(capi.c_double_p), D.ctypes.data_as(capi.c_double_p)))
    return I, D


def colloc_deriv(nq):
    Cm = np.zeros((nq, nq))
    check(capi.load().l3k_colloc_deriv(nq, Cm.ctypes.data_as(capi.c_double_p)))
    return Cm


def interp_1d(p_from, p_to):
    """[p_to + 1][p_from + 1]: the order-p_from GLL Lagrange basis at the GLL nodes of order p_to (l3k_interp_1d), the 1-D factor
    of the transfer between two orders of one element."""
    T = np.zeros((p_to + 1, p_from + 1))
    check(capi.load().l3k_interp_1d(int(p_from), int(p_to), T.ctypes.data_as(capi.c_double_p)))
    return T


def match_elements(fine_part, coarse_part):
    """elem_map[e_fine] = e_coarse (int64) for two partitions of ONE mesh at two orders, paired by their elem_verts rows (bitwise),
    or None when the pairing is the identity: what l3k_pmg_level.d_elem_map takes.  CubePartition traverses its elements in bricks
    whose edge depends on the order, so CubePartition(ne, p, perturb=...) at two orders lists the same elements in different
    sequences once the mesh is larger than a brick; the perturbation itself depends on the mesh spacing only, not on the order,
    so the vertices agree bit for bit.  Raises L3KError if some element has no partner (two different meshes); levels can then
    be built from one order-1 connectivity with elevate_order / ElevatedHexMesh instead, which keeps the element order."""
    vf = np.ascontiguousarray(fine_part.elem_verts, dtype=np.float64)
    vc = np.ascontiguousarray(coarse_part.elem_verts, dtype=np.float64)
    if vf.shape != vc.shape:
        raise L3KError(f"match_elements: the partitions hold {vf.shape[0]} and {vc.shape[0]} elements of {vf.shape[1:]} / {vc.shape[1:]} vertices")
    where = {}
    for e in range(vc.shape[0]):
        if where.setdefault(vc[e].tobytes(), e) != e:
            raise L3KError(f"match_elements: coarse elements {where[vc[e].tobytes()]} and {e} have the same vertices")
    out = np.empty(vf.shape[0], dtype=np.int64)
    for e in range(vf.shape[0]):
        ec = where.get(vf[e].tobytes())
        if ec is None:
            raise L3KError(f"match_elements: fine element {e} has no coarse element with the same vertices")
        out[e] = ec
    return None if np.array_equal(out, np.arange(out.size)) else out


def kernel_info(kernel_id):
    kp, name, nbytes = capi.KParams(), C.c_char_p(), C.c_size_t()
    check(capi.load().l3k_kernel_info(kernel_id, C.byref(kp), C.byref(name), C.byref(nbytes)))
    return dict(dimension=kp.dimension, n_equations=kp.n_equations, n_unknowns=kp.n_unknowns, n_fields=kp.n_fields,
                name=name.value.decode(), param_bytes=nbytes.value)


def residual_info(residual_id):
    kp, name, nbytes = capi.KParams(), C.c_char_p(), C.c_size_t()
    check(capi.load().l3k_residual_info(residual_id, C.byref(kp), C.byref(name), C.byref(nbytes)))
    return dict(dimension=kp.dimension, n_equations=kp.n_equations, n_fields=kp.n_fields, name=name.value.decode(),
                param_bytes=nbytes.value)


def instances():
    lib = capi.load()
    out = []
    for i in range(lib.l3k_instance_count()):
        v = [C.c_int() for _ in range(4)]
        check(lib.l3k_instance_info(i, *[C.byref(x) for x in v]))
        out.append(tuple(x.value for x in v))
    return out


def last_fast_launch():
    """The variant of the single-wave element kernel this thread launched last, as a set of names (l3k_last_fast_launch)."""
    v = C.c_uint(0)
    check(capi.load().l3k_last_fast_launch(C.byref(v)))
    names = ["launched", "split-ghost", "affine", "energy", "multi-column", "strided-dofs", "dynamic", "rhs"]
    return {n for i, n in enumerate(names) if v.value >> i & 1}


# ------------------------------------------------------------------------------------------------------- mesh
class CubePartition:
    """One rank's block of a structured order-p hex mesh of [0,1]^3 (host arrays, reference numbering conventions).
    perturb: every vertex moves by perturb * h_min * sin(2 pi x) sin(2 pi y) sin(2 pi z) along (1, 1, 1); the cube's boundary stays, and so
    does every vertex with a coordinate of 1/2: a mesh with no more than two elements in some direction is not distorted at all."""

    def __init__(self, ne, order, parts=(1, 1, 1), rank=0, perturb=0.0):
        lib = capi.load()
        ne = (ne,) * 3 if np.isscalar(ne) else tuple(ne)
        self.ne, self.order, self.parts, self.rank = ne, order, tuple(parts), rank
        h = C.c_void_p()
        check(lib.l3k_cube_partition_create((C.c_int * 3)(*ne), order, (C.c_int * 3)(*parts), rank, perturb,
                                            C.byref(h)))
        try:
            v = capi.HostMeshView()
            check(lib.l3k_hostmesh_view_get(h, C.byref(v)))
            N = (order + 1) ** 3
            as_np = lambda ptr, shape: np.ctypeslib.as_array(ptr, shape=shape).copy() if np.prod(shape) else \
                np.zeros(shape, dtype=np.ctypeslib.as_ctypes_type(ptr._type_))
            self.dim = 3
            self.n_elems, self.n_interior_elems = v.n_elems, v.n_interior_elems
            self.n_owned_nodes, self.n_ghost_nodes = v.n_owned_nodes, v.n_ghost_nodes
            self.global_node_base, self.n_global_nodes = v.global_node_base, v.n_global_nodes
            self.elem_nodes = as_np(v.elem_nodes, (v.n_elems, N))
            self.elem_verts = as_np(v.elem_verts, (v.n_elems, 8, 3))
            nl = v.n_owned_nodes + v.n_ghost_nodes
            self.node_grid_id = as_np(v.node_grid_id, (nl,))
            self.node_boundary = as_np(v.node_boundary, (nl,))
            self.elem_boundary = as_np(v.elem_boundary, (v.n_elems,))
            self.ghost_global_id = as_np(v.ghost_global_id, (v.n_ghost_nodes,))
            nn = v.n_nbrs
            self.nbr_rank = [v.nbr_rank[i] for i in range(nn)]
            so = [v.send_offsets[i] for i in range(nn + 1)]
            go = [v.ghost_offsets[i] for i in range(nn + 1)]
            send = as_np(v.send_nodes, (so[-1],)) if so[-1] else np.zeros(0, np.int32)
            self.send_nodes = [send[so[i]:so[i + 1]] for i in range(nn)]
            self.ghost_ranges = [(go[i], go[i + 1]) for i in range(nn)]
        finally:
            lib.l3k_hostmesh_destroy(h)

    @property
    def n_local_nodes(self):
        return self.n_owned_nodes + self.n_ghost_nodes

    def dirichlet_mask(self, dofs_per_node, unknowns=(0,), sides=range(6)):
        """Byte mask over local dofs: the listed unknowns on the listed cube sides (BCDefinition::defineDirichlet,
        benchmarks/Diffusion3D.hpp:39-41)."""
        side_bits = 0
        for s in sides:
            side_bits |= 1 << s
        on = (self.node_boundary & side_bits) != 0
        mask = np.zeros((self.n_local_nodes, dofs_per_node), dtype=np.uint8)
        for u in unknowns:
            mask[on, u] = 1
        return mask.reshape(-1)

    def boundary_sides(self, sides=range(6)):
        """(element index, side) of this rank's element sides on the listed cube sides: the BoundaryViews of
        makeCubeMesh (mesh/primitives/CubeMesh.hpp:66-138).  Returns (int64[n], uint8[n])."""
        fe, fs = [], []
        for s in sides:
            e = np.nonzero(self.elem_boundary & (1 << s))[0]
            fe.append(e.astype(np.int64))
            fs.append(np.full(e.size, s, dtype=np.uint8))
        if not fe:
            return np.zeros(0, np.int64), np.zeros(0, np.uint8)
        return np.concatenate(fe), np.concatenate(fs)

    def node_coords(self):
        """Physical location of every local node (mesh/NodePhysicalLocation.hpp: tri-linear map -- bilinear on quads -- of
        the element vertices at the GLL reference positions).  Returns float64 [n_local_nodes, 3]."""
        g = gll_nodes(self.order + 1)
        l = np.stack([(1 - g) / 2, (1 + g) / 2], axis=1)  # [n][2] linear shape functions at the GLL points
        n = self.order + 1
        if self.elem_verts.shape[1] == 4:  # quads: shape[(ix,iy) lexicographic, v = i + 2j]
            shape = np.einsum("xi,yj->yxji", l, l).reshape(n ** 2, 4)
        else:  # shape[(ix,iy,iz) lexicographic, v = i + 2j + 4k]
            shape = np.einsum("xi,yj,zk->zyxkji", l, l, l).reshape(n ** 3, 8)
        coords = np.zeros((self.n_local_nodes, 3))
        for e0 in range(0, self.n_elems, 65536):
            ev = self.elem_verts[e0:e0 + 65536]
            coords[self.elem_nodes[e0:e0 + 65536].reshape(-1)] = np.einsum("nv,evs->ens", shape, ev).reshape(-1, 3)
        return coords

    def synthetic_vector(self, dofs_per_node, seed=42, ncols=1):
        """x ~ U(-1,1) as a function of (partition-independent grid node id, dof, column): every partition of the same
        mesh sees the same global vector.  Counter-based splitmix64.  Shape (ncols, n_local_dofs)."""
        key = (self.node_grid_id.astype(np.uint64)[:, None] * np.uint64(dofs_per_node) +
               np.arange(dofs_per_node, dtype=np.uint64)[None, :]).reshape(-1)
        out = np.empty((ncols, key.size))
        for c in range(ncols):
            with np.errstate(over="ignore"):
                z = key + np.uint64(seed) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(c) * np.uint64(0xD1B54A32D192ED03)
                z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
                z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
                z = z ^ (z >> np.uint64(31))
            out[c] = (z >> np.uint64(11)).astype(np.float64) * (2.0 / (1 << 53)) - 1.0
        return out


class SquarePartition:
    """A single-part structured order-p quad mesh of [0,1]^2 (host arrays; l3k_square_mesh_create): the attributes of
    CubePartition with dim = 2, elem_verts [n_elems][4][3] (z = 0), node_grid_id = gx + NX*gy and the quad side order
    0 y=0, 1 y=1, 2 x=0, 3 x=1 (mesh/ElementTraits.hpp:84-95).  Multi-part quad meshes: partition.rcb_partition +
    partition.PartitionedMesh on its arrays."""

    def __init__(self, ne, order, perturb=0.0):
        lib = capi.load()
        ne = (ne,) * 2 if np.isscalar(ne) else tuple(ne)
        self.ne, self.order, self.parts, self.rank = ne, order, (1, 1), 0
        h = C.c_void_p()
        check(lib.l3k_square_mesh_create((C.c_int * 2)(*ne), order, perturb, C.byref(h)))
        try:
            v = capi.HostMeshView()
            check(lib.l3k_hostmesh_view_get(h, C.byref(v)))
            N = (order + 1) ** 2
            as_np = lambda ptr, shape: np.ctypeslib.as_array(ptr, shape=shape).copy()
            self.dim = v.dim
            self.n_elems, self.n_interior_elems = v.n_elems, v.n_interior_elems
            self.n_owned_nodes, self.n_ghost_nodes = v.n_owned_nodes, v.n_ghost_nodes
            self.global_node_base, self.n_global_nodes = v.global_node_base, v.n_global_nodes
            self.elem_nodes = as_np(v.elem_nodes, (v.n_elems, N))
            self.elem_verts = as_np(v.elem_verts, (v.n_elems, 4, 3))
            self.node_grid_id = as_np(v.node_grid_id, (v.n_owned_nodes,))
            self.node_boundary = as_np(v.node_boundary, (v.n_owned_nodes,))
            self.elem_boundary = as_np(v.elem_boundary, (v.n_elems,))
            self.ghost_global_id = np.zeros(0, np.int64)
            self.nbr_rank, self.send_nodes, self.ghost_ranges = [], [], []
        finally:
            lib.l3k_hostmesh_destroy(h)

    n_local_nodes = CubePartition.n_local_nodes
    node_coords = CubePartition.node_coords
    synthetic_vector = CubePartition.synthetic_vector

    def dirichlet_mask(self, dofs_per_node, unknowns=(0,), sides=range(4)):
        """Byte mask over local dofs: the listed unknowns on the listed square sides."""
        return CubePartition.dirichlet_mask(self, dofs_per_node, unknowns, sides)

    def boundary_sides(self, sides=range(4)):
        """(element index, side) of the element sides on the listed square sides.  Returns (int64[n], uint8[n])."""
        return CubePartition.boundary_sides(self, sides)


def synthetic_vector_torch(node_grid_id, dofs_per_node, device, seed=42, ncols=1):
    """Same function as CubePartition.synthetic_vector, evaluated with torch on `device` (int64 two's-complement
    arithmetic == uint64 arithmetic modulo 2^64; logical shifts emulated by masking)."""
    import torch

    def s64(v):  # python int -> signed 64-bit representative
        v &= (1 << 64) - 1
        return v - (1 << 64) if v >= (1 << 63) else v

    def lsr(z, k):
        return (z >> k) & ((1 << (64 - k)) - 1)

    ids = torch.as_tensor(node_grid_id, dtype=torch.int64, device=device)
    key = (ids[:, None] * dofs_per_node + torch.arange(dofs_per_node, dtype=torch.int64, device=device)[None, :]).reshape(-1)
    out = torch.empty((ncols, key.numel()), dtype=torch.float64, device=device)
    for c in range(ncols):
        z = key + s64(seed * 0x9E3779B97F4A7C15 + c * 0xD1B54A32D192ED03)
        z = (z ^ lsr(z, 30)) * s64(0xBF58476D1CE4E5B9)
        z = (z ^ lsr(z, 27)) * s64(0x94D049BB133111EB)
        z = z ^ lsr(z, 31)
        out[c] = lsr(z, 11).to(torch.float64) * (2.0 / (1 << 53)) - 1.0
    return out


# ------------------------------------------------------------------------------------------------------- device
class Context:
    def __init__(self, device=0, stream=None):
        self._h = C.c_void_p()
        check(capi.load().l3k_ctx_create(device, C.c_void_p(stream or 0), C.byref(self._h)))
        self.device = device

    def set_stream(self, stream):
        check(capi.load().l3k_ctx_set_stream(self._h, C.c_void_p(stream or 0)))

    def set_deterministic(self, on=True):
        """Bitwise-reproducible element launches (colour by colour) for the meshes created from now on."""
        check(capi.load().l3k_ctx_set_deterministic(self._h, int(bool(on))))

    def set_reference_z0(self, on=True):
        """Applies pass Point{x, y, 0.} to domain kernels as the reference's hex sum-factorisation path does
        (algsys/SumFactorization.hpp:732); default off: the true point (l3k_ctx_set_reference_z0 in include/l3k.h)."""
        check(capi.load().l3k_ctx_set_reference_z0(self._h, int(bool(on))))

    def get_tuning(self):
        """The context's launch-route settings as a dict (l3k_tuning in include/l3k.h)."""
        t = capi.Tuning()
        check(capi.load().l3k_ctx_get_tuning(self._h, C.byref(t)))
        return {name: getattr(t, name) for name, _ in capi.Tuning._fields_}

    def set_tuning(self, **fields):
        t = capi.Tuning()
        check(capi.load().l3k_ctx_get_tuning(self._h, C.byref(t)))
        for name, value in fields.items():
            if name not in dict(capi.Tuning._fields_):
                raise L3KError(f"l3k_tuning has no field {name!r}")
            setattr(t, name, int(value))
        check(capi.load().l3k_ctx_set_tuning(self._h, C.byref(t)))

    @contextlib.contextmanager
    def tuning(self, **fields):
        """with ctx.tuning(generic_below=0): ...  -- the settings inside the block, the previous ones afterwards."""
        before = self.get_tuning()
        self.set_tuning(**fields)
        try:
            yield self
        finally:
            self.set_tuning(**before)

    def synchronize(self):
        check(capi.load().l3k_ctx_synchronize(self._h))

    def __del__(self):
        if getattr(self, "_h", None) and capi is not None:  # (module globals may be gone at interpreter shutdown)
            capi.load().l3k_ctx_destroy(self._h)
            self._h = None


def elevate_order(ctx, conn, n_vertices, order):
    """Order elevation of an order-1 hex mesh on the device (l3k_elevate_order; mesh::convertMeshToOrder +
    LocalMeshView's numbering): conn [n_elems][8] vertex ids (local vertex i + 2j + 4k) -> (elem_nodes
    [n_elems][(order+1)^3] uint32, n_nodes, n_noninternal)."""
    lib = capi.load()
    c = np.ascontiguousarray(conn, dtype=np.uint32).reshape(-1, 8)
    out = np.empty((c.shape[0], (order + 1) ** 3), dtype=np.uint32)
    nn, nni = C.c_int64(), C.c_int64()
    capi.check(lib.l3k_elevate_order(ctx._h, c.shape[0], c.ctypes.data_as(capi.c_uint32_p), int(n_vertices), int(order),
                                     out.ctypes.data_as(capi.c_uint32_p), C.byref(nn), C.byref(nni)))
    return out, nn.value, nni.value


class ElevatedHexMesh:
    """A single-rank order-p hex mesh made from an unstructured order-1 one on the device: the mesh object DeviceMesh
    and the operators take (same attributes as CubePartition; no ghosts, no neighbours)."""

    def __init__(self, ctx, verts, conn, order):
        verts = np.ascontiguousarray(verts, dtype=np.float64).reshape(-1, 3)
        conn = np.ascontiguousarray(conn, dtype=np.uint32).reshape(-1, 8)
        self.dim, self.order, self.rank, self.parts = 3, order, 0, (1, 1, 1)
        self.elem_nodes, n_nodes, self.n_noninternal = elevate_order(ctx, conn, verts.shape[0], order)
        self.elem_verts = verts[conn.astype(np.int64)]  # [n_elems][8][3]
        self.n_elems = self.n_interior_elems = conn.shape[0]
        self.n_owned_nodes, self.n_ghost_nodes = n_nodes, 0
        self.global_node_base, self.n_global_nodes = 0, n_nodes
        self.nbr_rank, self.send_nodes, self.ghost_ranges = [], [], []

    n_local_nodes = CubePartition.n_local_nodes
    node_coords = CubePartition.node_coords


def elevate_order_quads(ctx, conn, n_vertices, order):
    """The quad twin of elevate_order (l3k_elevate_order_quads): conn [n_elems][4] vertex ids (local vertex i + 2j) ->
    (elem_nodes [n_elems][(order+1)^2] uint32, n_nodes, n_noninternal)."""
    lib = capi.load()
    c = np.ascontiguousarray(conn, dtype=np.uint32).reshape(-1, 4)
    out = np.empty((c.shape[0], (order + 1) ** 2), dtype=np.uint32)
    nn, nni = C.c_int64(), C.c_int64()
    capi.check(lib.l3k_elevate_order_quads(ctx._h, c.shape[0], c.ctypes.data_as(capi.c_uint32_p), int(n_vertices), int(order),
                                           out.ctypes.data_as(capi.c_uint32_p), C.byref(nn), C.byref(nni)))
    return out, nn.value, nni.value


def boundary_match(ctx, conn, bnd_conn):
    """The element and side of every boundary element (l3k_boundary_match): conn [n_elems][2^dim] and bnd_conn
    [n_bnd][2^(dim-1)] vertex ids, dim from conn's width.  Returns (face_elem int64 [n_bnd], face_side uint8 [n_bnd], n_unmatched,
    n_interior); an unmatched boundary element has face_elem -1 and face_side 255."""
    conn = np.asarray(conn)
    if conn.ndim != 2 or conn.shape[1] not in (4, 8):
        raise L3KError("conn must be [n_elems][4] (quads) or [n_elems][8] (hexes)")
    dim = 2 if conn.shape[1] == 4 else 3
    c = np.ascontiguousarray(conn, dtype=np.uint32)
    b = np.ascontiguousarray(bnd_conn, dtype=np.uint32).reshape(-1, 2 ** (dim - 1))
    fe = np.empty(b.shape[0], dtype=np.int64)
    fs = np.empty(b.shape[0], dtype=np.uint8)
    nu, ni = C.c_int64(), C.c_int64()
    capi.check(capi.load().l3k_boundary_match(ctx._h, dim, c.shape[0], c.ctypes.data_as(capi.c_uint32_p), b.shape[0],
                                              b.ctypes.data_as(capi.c_uint32_p), fe.ctypes.data_as(capi.c_int64_p),
                                              fs.ctypes.data_as(capi.c_uint8_p), C.byref(nu), C.byref(ni)))
    return fe, fs, nu.value, ni.value


def side_nodes(dim, order):
    """[2 dim][(order+1)^(dim-1)] element-local node indices of every side of an order-p quad (i + n j) or hex (i + n (j + n k)),
    sides numbered as for BoundaryTerm: the last axis first, low side before high side."""
    n = order + 1
    idx = np.arange(n ** dim).reshape((n,) * dim)  # [k][j][i] / [j][i]
    return np.stack([np.take(idx, at, axis=axis).reshape(-1) for axis in range(dim) for at in (0, order)])


def periodic_match(ctx, mesh, src, dst, translation, tolerance=1e-12):
    """The destination node every source node is the image of (l3k_periodic_match; bcs/PeriodicBC.hpp): mesh supplies dim, order,
    elem_nodes and elem_verts; src and dst are (face_elem, face_side) lists of element sides; source node s matches destination
    node d iff |x_s + translation - x_d| < tolerance, the nearest wins, ties to the lowest id.  Returns (pair_src uint32 [n],
    pair_dst uint32 [n], n_unmatched, n_ambiguous, first_unmatched), pairs ascending in the source node.  L3KError for what the
    call refuses (include/l3k.h), a box of the destination vertices or a tolerance from which no grid can be made among it."""
    en = np.ascontiguousarray(mesh.elem_nodes, dtype=np.uint32)
    ev = np.ascontiguousarray(mesh.elem_verts, dtype=np.float64)
    se, ss = _sides(*src)
    de, ds = _sides(*dst)
    t = np.zeros(3)
    tr = np.asarray(translation, dtype=np.float64).reshape(-1)
    if tr.size not in (mesh.dim, 3):
        raise L3KError("the translation has one entry per dimension")
    t[:tr.size] = tr
    cap = se.size * (mesh.order + 1) ** (mesh.dim - 1)
    ps, pd = np.empty(cap, dtype=np.uint32), np.empty(cap, dtype=np.uint32)
    n_pairs, n_unmatched, n_ambiguous, first = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
    check(capi.load().l3k_periodic_match(
        ctx._h, mesh.dim, mesh.order, en.shape[0], en.ctypes.data_as(capi.c_uint32_p), ev.ctypes.data_as(capi.c_double_p),
        se.size, se.ctypes.data_as(capi.c_int64_p), ss.ctypes.data_as(capi.c_uint8_p), de.size, de.ctypes.data_as(capi.c_int64_p),
        ds.ctypes.data_as(capi.c_uint8_p), t.ctypes.data_as(capi.c_double_p), float(tolerance), ps.ctypes.data_as(capi.c_uint32_p),
        pd.ctypes.data_as(capi.c_uint32_p), C.byref(n_pairs), C.byref(n_unmatched), C.byref(n_ambiguous), C.byref(first)))
    return ps[:n_pairs.value].copy(), pd[:n_pairs.value].copy(), n_unmatched.value, n_ambiguous.value, first.value


def periodic_merge(elem_nodes, n_nodes, n_noninternal, pair_a, pair_b):
    """The node pairs carried out on a connectivity (l3k_periodic_merge, host only): every connected component of the pair graph
    becomes its lowest node, ids stay compact and the [non-internal | internal] numbering survives.  The pairs may come from several
    periodic_match calls on the UNMERGED mesh.  Returns (new elem_nodes uint32, node_map uint32 [n_nodes] old -> new, n_nodes,
    n_noninternal, n_components); elem_nodes itself is not touched."""
    en = np.array(elem_nodes, dtype=np.uint32, order="C")
    a = np.ascontiguousarray(pair_a, dtype=np.uint32).reshape(-1)
    b = np.ascontiguousarray(pair_b, dtype=np.uint32).reshape(-1)
    if a.size != b.size:
        raise L3KError("pair_a and pair_b must have the same length")
    node_map = np.empty(int(n_nodes), dtype=np.uint32)
    nn, nni, nc = C.c_int64(), C.c_int64(), C.c_int64()
    check(capi.load().l3k_periodic_merge(int(n_nodes), int(n_noninternal), a.size, a.ctypes.data_as(capi.c_uint32_p),
                                         b.ctypes.data_as(capi.c_uint32_p), en.size, en.ctypes.data_as(capi.c_uint32_p),
                                         node_map.ctypes.data_as(capi.c_uint32_p), C.byref(nn), C.byref(nni), C.byref(nc)))
    return en, node_map, nn.value, nni.value, nc.value


class ElevatedMesh:
    """A single-rank order-p quad or hex mesh made from an unstructured order-1 one on the device, with its boundary by
    physical id: what mesh::readMesh + convertMeshToOrder give the reference (gmsh.read_mesh supplies the arguments).  The
    attributes of ElevatedHexMesh (DeviceMesh, MatrixFreeSystem, partition.PartitionedMesh and solve.PMultigrid take it as they take
    that class; quads keep elem_verts [n][4][3]), plus boundary_ids (sorted unique), elem_domain, and the (element, side) of every
    boundary element from l3k_boundary_match."""

    def __init__(self, ctx, verts, conn, order, bnd_conn=None, bnd_id=None, elem_domain=None):
        verts = np.ascontiguousarray(verts, dtype=np.float64).reshape(-1, 3)
        conn = np.asarray(conn)
        if conn.ndim != 2 or conn.shape[1] not in (4, 8):
            raise L3KError("conn must be [n_elems][4] (quads) or [n_elems][8] (hexes)")
        conn = np.ascontiguousarray(conn, dtype=np.uint32)
        self.dim = 2 if conn.shape[1] == 4 else 3
        self.ctx, self.order, self.rank, self.parts = ctx, order, 0, (1,) * self.dim
        elevate = elevate_order_quads if self.dim == 2 else elevate_order
        self.elem_nodes, n_nodes, self.n_noninternal = elevate(ctx, conn, verts.shape[0], order)
        self.elem_verts = verts[conn.astype(np.int64)]  # [n_elems][2^dim][3]
        self.n_elems = self.n_interior_elems = conn.shape[0]
        self.n_owned_nodes, self.n_ghost_nodes = n_nodes, 0
        self.global_node_base, self.n_global_nodes = 0, n_nodes
        self.nbr_rank, self.send_nodes, self.ghost_ranges = [], [], []
        self.elem_domain = np.zeros(conn.shape[0], np.int32) if elem_domain is None else np.asarray(elem_domain, dtype=np.int32)
        if self.elem_domain.shape != (conn.shape[0],):
            raise L3KError("elem_domain must hold one id per element")
        n_side_verts = 2 ** (self.dim - 1)
        bnd_conn = np.zeros((0, n_side_verts), np.uint32) if bnd_conn is None else np.asarray(bnd_conn).reshape(-1, n_side_verts)
        self.bnd_id = np.zeros(0, np.int32) if bnd_id is None else np.asarray(bnd_id, dtype=np.int32).reshape(-1)
        if self.bnd_id.size != bnd_conn.shape[0]:
            raise L3KError("bnd_id must hold one id per boundary element")
        self.boundary_ids = np.unique(self.bnd_id)
        self.face_elem, self.face_side, self.n_unmatched, self.n_interior = boundary_match(ctx, conn, bnd_conn)

    n_local_nodes = CubePartition.n_local_nodes
    node_coords = CubePartition.node_coords

    def _select(self, ids):
        ids = np.atleast_1d(np.asarray(self.boundary_ids if ids is None else ids, dtype=np.int64))
        missing = np.setdiff1d(ids, self.boundary_ids)
        if missing.size:
            raise L3KError(f"the mesh has no boundary with id {missing.tolist()}")  # getBoundary throws (tests/MeshTests.cpp:40)
        sel = np.nonzero(np.isin(self.bnd_id, ids))[0]
        lost = sel[self.face_elem[sel] < 0]
        if lost.size:
            raise L3KError(f"{lost.size} boundary elements (the first: number {int(lost[0])} of the file, id "
                           f"{int(self.bnd_id[lost[0]])}) are the side of no element")
        return sel

    def boundary_sides(self, ids=None):
        """(element index, side) of the boundary elements with the listed physical ids (default: all), in the order of the
        file: MeshPartition::getBoundary(id).  Returns (int64[m], uint8[m]); L3KError for an id the mesh does not have and for a
        listed boundary element that is the side of no element."""
        sel = self._select(ids)
        return self.face_elem[sel].copy(), self.face_side[sel].copy()

    def dirichlet_mask(self, dofs_per_node, unknowns=(0,), ids=None):
        """Byte mask over local dofs: the listed unknowns at the nodes of the sides with the listed boundary ids (default: all)
        (BCDefinition::defineDirichlet)."""
        fe, fs = self.boundary_sides(ids)
        nodes = self.elem_nodes[fe[:, None], side_nodes(self.dim, self.order)[fs]].reshape(-1)
        mask = np.zeros((self.n_local_nodes, dofs_per_node), dtype=np.uint8)
        for u in unknowns:
            mask[nodes, u] = 1
        return mask.reshape(-1)

    def periodic(self, definitions, tolerance=1e-12):
        """BCDefinition::definePeriodic (bcs/BCDefinition.hpp:92-104) for every (src_ids, dst_ids, translation) of `definitions`, by
        boundary id: a new mesh in which every node of the source boundaries is the node of the destination boundaries it is the
        image of.  All definitions are matched on this (unmerged) mesh and merged at once, so the corners of a mesh periodic along
        several axes become one node.  Raises L3KError naming the definition and the lowest unmatched node when a source node has
        no partner ("each node at X belonging to source must have a corresponding node at X + translation"), and with the message
        of l3k_periodic_match for a tolerance or a destination boundary it refuses (include/l3k.h).
        The new mesh is taken by everything that takes this one (DeviceMesh, MatrixFreeSystem, BoundaryTerm,
        partition.PartitionedMesh, solve.PMultigrid, SparsityGraph); it has the same elem_verts, face_elem / face_side, bnd_id,
        boundary_ids and elem_domain, new elem_nodes, n_owned_nodes, n_global_nodes and n_noninternal, and carries node_map (old
        -> new), n_pairs and n_ambiguous.  dirichlet_mask and boundary_sides work on it as here.  node_coords() of an identified
        node returns the location of one of its images."""
        import copy
        pa, pb, n_ambiguous = [], [], 0
        for k, (src_ids, dst_ids, translation) in enumerate(definitions):
            s, d, n_unmatched, amb, first = periodic_match(self.ctx, self, self.boundary_sides(src_ids), self.boundary_sides(dst_ids),
                                                           translation, tolerance)
            if n_unmatched:
                raise L3KError(f"periodic definition {k} ({list(np.atleast_1d(src_ids))} -> {list(np.atleast_1d(dst_ids))}): "
                               f"{n_unmatched} source nodes have no node at X + translation, the first: node {first}")
            pa.append(s), pb.append(d)
            n_ambiguous += amb
        pa = np.concatenate(pa) if pa else np.zeros(0, np.uint32)
        pb = np.concatenate(pb) if pb else np.zeros(0, np.uint32)
        new = copy.copy(self)
        new.elem_nodes, new.node_map, n_nodes, new.n_noninternal, new.n_components = periodic_merge(
            self.elem_nodes, self.n_owned_nodes, self.n_noninternal, pa, pb)
        new.n_owned_nodes = new.n_global_nodes = n_nodes
        new.n_pairs, new.n_ambiguous = int(pa.size), n_ambiguous
        return new

    def elements_of(self, domain_ids):
        """Indices of the elements with the listed domain (physical) ids, ascending; L3KError for an id no element has."""
        ids = np.atleast_1d(np.asarray(domain_ids, dtype=np.int64))
        missing = np.setdiff1d(ids, self.elem_domain)
        if missing.size:
            raise L3KError(f"the mesh has no domain with id {missing.tolist()}")
        return np.nonzero(np.isin(self.elem_domain, ids))[0]

    def subset(self, domain_ids):
        """The elements with the listed domain ids as a part over the nodes of this mesh (partition.element_subset): what
        DeviceMesh takes for a term of a MultiTermSystem that lives on those domains only."""
        from . import partition
        return partition.element_subset(self, self.elements_of(domain_ids))


class DeviceMesh:
    def __init__(self, ctx, part, dofs_per_node, dirichlet=None):
        self.ctx, self.part, self.dofs_per_node = ctx, part, dofs_per_node
        d = capi.MeshDesc()
        d.dim, d.order = part.dim, part.order
        d.n_elems, d.n_interior_elems = part.n_elems, part.n_interior_elems
        en = np.ascontiguousarray(part.elem_nodes, dtype=np.uint32)
        ev = np.ascontiguousarray(part.elem_verts, dtype=np.float64)
        d.elem_nodes = en.ctypes.data_as(capi.c_uint32_p)
        d.elem_verts = ev.ctypes.data_as(capi.c_double_p)
        d.n_owned_nodes, d.n_ghost_nodes = part.n_owned_nodes, part.n_ghost_nodes
        d.dofs_per_node = dofs_per_node
        if dirichlet is not None:
            dm = np.ascontiguousarray(dirichlet, dtype=np.uint8)
            if dm.size != part.n_local_nodes * dofs_per_node:
                raise L3KError("dirichlet mask must cover every local dof")
            d.dirichlet = dm.ctypes.data_as(capi.c_uint8_p)
        self._h = C.c_void_p()
        check(capi.load().l3k_mesh_create(ctx._h, C.byref(d), C.byref(self._h)))
        self.n_owned_dofs = part.n_owned_nodes * dofs_per_node
        self.n_ghost_dofs = part.n_ghost_nodes * dofs_per_node

    def __del__(self):
        if getattr(self, "_h", None) and capi is not None:
            capi.load().l3k_mesh_destroy(self._h)
            self._h = None


class Transfer:
    """Handle of l3k_transfer_create: the inter-order transfer of ONE level pair of a mesh that may be partitioned (include/l3k.h),
    beside solve.PMultigrid's single-rank pairs.  fine, coarse: DeviceMesh'es of this rank's elements at two orders on one context;
    elem_map (int64, host or device, or None = identity; match_elements makes it) names the coarse element of each fine one.  A
    vector of a level is its owned rows plus its ghost rows (the (1, n_ghost_dofs) result of a distributed operator's
    import_ghosts, or None on a mesh without ghosts).  The meshes and the map are kept alive here."""

    def __init__(self, fine, coarse, elem_map=None):
        import torch
        self.fine, self.coarse = fine, coarse
        self._map = None if elem_map is None else torch.as_tensor(elem_map, dtype=torch.int64).to(torch.device("cuda", fine.ctx.device)).contiguous()
        self._h = C.c_void_p()
        check(capi.load().l3k_transfer_create(fine.ctx._h, fine._h, coarse._h, None if self._map is None else self._map.data_ptr(),
                                              C.byref(self._h)))

    @property
    def info(self):
        """order_fine, order_coarse, n_owned_dofs_fine, n_ghost_dofs_fine, n_owned_dofs_coarse, n_ghost_dofs_coarse"""
        import types
        i = capi.TransferInfo()
        check(capi.load().l3k_transfer_info_get(self._h, C.byref(i)))
        return types.SimpleNamespace(**{name: getattr(i, name) for name, _ in capi.TransferInfo._fields_})

    @staticmethod
    def _vec(t, n, name, optional=False):
        if t is None and (optional or n == 0):
            return None
        if t is None or t.numel() < n or (not optional and t.numel() != n) or not t.is_contiguous():
            raise L3KError(f"{name} must be a contiguous tensor over {n} dofs")
        return C.c_void_p(t.data_ptr())

    def prolong(self, xc, xc_ghost, xf, add=False, frozen=None):
        """xf <- P xc, or xf += P xc, on the owned fine rows (l3k_transfer_prolong); xc_ghost: the imported ghost rows of xc;
        frozen: owned fine rows with frozen == 0 are left alone"""
        i = self.info
        check(capi.load().l3k_transfer_prolong(
            self._h, self._vec(xc, i.n_owned_dofs_coarse, "xc"), self._vec(xc_ghost, i.n_ghost_dofs_coarse, "xc_ghost", True),
            self._vec(xf, i.n_owned_dofs_fine, "xf"), int(bool(add)),
            None if frozen is None else self._vec(frozen, i.n_owned_dofs_fine, "frozen")))
        return xf

    def restrict(self, rf, rc, rc_ghost):
        """rc, rc_ghost <- this rank's share of P^T rf (l3k_transfer_restrict); the coarse level's export_add of rc_ghost into rc
        completes the product"""
        i = self.info
        check(capi.load().l3k_transfer_restrict(
            self._h, self._vec(rf, i.n_owned_dofs_fine, "rf"), self._vec(rc, i.n_owned_dofs_coarse, "rc"),
            self._vec(rc_ghost, i.n_ghost_dofs_coarse, "rc_ghost", True)))
        return rc

    def close(self):
        if getattr(self, "_h", None) and capi is not None:
            capi.load().l3k_transfer_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # (module globals may be gone at interpreter shutdown)
            pass


def _ptr(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def _blob(kernel_params):
    if kernel_params is None:
        return None, 0, None
    arr = np.ascontiguousarray(kernel_params, dtype=np.float64)
    return arr.ctypes.data_as(C.c_void_p), arr.nbytes, arr


def _sides(face_elem, face_side):
    fe = np.ascontiguousarray(face_elem, dtype=np.int64)
    fs = np.ascontiguousarray(face_side, dtype=np.uint8)
    if fe.shape != fs.shape or fe.ndim != 1:
        raise L3KError("face_elem and face_side must be 1-D arrays of the same length")
    return fe, fs


class BoundaryTerm:
    """A boundary equation kernel on a list of element sides: assembleProblem(kernel, boundary_ids) of the reference
    (algsys/MatrixFreeSystem.hpp:58-68).  Attach it to a MatrixFreeSystem, or use apply / diag_rhs directly."""

    def __init__(self, mesh, kernel_id, face_elem, face_side, kernel_params=None, asm_opts=(1, 0, 0), field_inds=None,
                 n_rhs=1):
        self.mesh, self.ctx, self.kernel_id, self.n_rhs = mesh, mesh.ctx, kernel_id, n_rhs
        self.info = kernel_info(kernel_id)
        blob, nbytes, self._keep = _blob(kernel_params)
        opts = capi.AsmOpts(*asm_opts)
        fi = None if field_inds is None else (C.c_int * len(field_inds))(*field_inds)
        fe, fs = _sides(face_elem, face_side)
        self.n_faces = fe.size
        self._h = C.c_void_p()
        check(capi.load().l3k_bnd_create(self.ctx._h, mesh._h, kernel_id, blob, nbytes, C.byref(opts), fi, n_rhs, fe.size,
                                         fe.ctypes.data_as(capi.c_int64_p), fs.ctypes.data_as(capi.c_uint8_p),
                                         C.byref(self._h)))
        self._fields = None

    def __del__(self):
        if getattr(self, "_h", None) and capi is not None:
            capi.load().l3k_bnd_destroy(self._h)
            self._h = None

    def set_fields(self, fields):
        if fields is not None and (fields.dim() != 2 or not fields.is_contiguous()):
            raise L3KError("fields must be a contiguous (n_fields, n_local_nodes) tensor")
        self._fields = fields
        check(capi.load().l3k_bnd_set_fields(self._h, _ptr(fields), 0 if fields is None else fields.shape[1]))

    def set_time(self, t):
        check(capi.load().l3k_bnd_set_time(self._h, float(t)))

    def apply(self, X, Y, alpha=1.0, which=2, XG=None, YG=None):
        """Y += alpha * A_b X"""
        nc, ldx = MatrixFreeSystem._cols(X)
        _, ldy = MatrixFreeSystem._cols(Y)
        ldxg = MatrixFreeSystem._cols(XG)[1] if XG is not None else 0
        ldyg = MatrixFreeSystem._cols(YG)[1] if YG is not None else 0
        check(capi.load().l3k_bnd_apply(self._h, which, _ptr(X), ldx, _ptr(XG), ldxg, _ptr(Y), ldy, _ptr(YG), ldyg, nc,
                                        alpha))
        return Y

    def diag_rhs(self, diag, rhs, dirichlet_vals=None, which=2, diag_ghost=None, rhs_ghost=None):
        """diag += diag(A_b), rhs += B_b^T W (f_b - B_b g) (accumulating; no Dirichlet finalisation)"""
        g = dirichlet_vals
        ldg = 0 if g is None else g.shape[1]
        ldrg = 0 if rhs_ghost is None else rhs_ghost.shape[1]
        check(capi.load().l3k_bnd_diag_rhs(self._h, which, _ptr(g), ldg, _ptr(diag), _ptr(rhs), rhs.shape[1],
                                           _ptr(diag_ghost), _ptr(rhs_ghost), ldrg))
        return diag, rhs

    def local_assemble(self, first=0, count=None, want_K=True, want_F=True):
        """assembleLocalSystem on the sides [first, first+count) of the list, in the order the term was given
        (l3k_bnd_local_assemble; hexes): the local system of the whole element from the side quadrature.  Returns
        (K [count, Nd, Nd] row-major, bitwise symmetric, F [count, n_rhs, Nd])."""
        import torch
        count = self.n_faces - first if count is None else count
        Nd = (self.mesh.part.order + 1) ** 3 * self.info["n_unknowns"]
        n = max(count, 0)
        K = torch.empty((n, Nd, Nd), dtype=torch.float64, device="cuda") if want_K else None
        F = torch.empty((n, self.n_rhs, Nd), dtype=torch.float64, device="cuda") if want_F else None
        check(capi.load().l3k_bnd_local_assemble(self._h, first, count, _ptr(K), _ptr(F)))
        return K, F

    def side_systems(self, first=0, count=None, want_K=True, want_F=True):
        """assembleLocalSystem on the sides [first, first+count) of the list, in the order the term was given
        (l3k_asm_side_systems; hexes and quads): the local system of the whole element from the side quadrature.  Returns
        (K [count, Nd, Nd] row-major, bitwise symmetric, F [count, n_rhs, Nd]), Nd = (p+1)^dim U."""
        import torch
        count = self.n_faces - first if count is None else count
        Nd = (self.mesh.part.order + 1) ** self.mesh.part.dim * self.info["n_unknowns"]
        n = max(count, 0)
        K = torch.empty((n, Nd, Nd), dtype=torch.float64, device="cuda") if want_K else None
        F = torch.empty((n, self.n_rhs, Nd), dtype=torch.float64, device="cuda") if want_F else None
        check(capi.load().l3k_asm_side_systems(self._h, first, count, _ptr(K), _ptr(F)))
        return K, F

    def assemble_global(self, row_ptr, col_ind, values, rhs=None, first=0, count=None, skip_dirichlet=False, workspace_bytes=0):
        """The boundary overload of assembleGlobalSystem for the sides [first, first+count) of the list
        (l3k_bnd_assemble_global; hexes): side systems formed and summed into `values` (over the CSR graph row_ptr int64 /
        col_ind int32) and `rhs` [n_rhs, n_local_dofs]; additive.  Returns the number of entries outside the graph."""
        count = self.n_faces - first if count is None else count
        missing = C.c_int64(0)
        check(capi.load().l3k_bnd_assemble_global(self._h, first, count, _ptr(row_ptr), _ptr(col_ind), _ptr(values), _ptr(rhs),
                                                  0 if rhs is None else rhs.stride(0) if rhs.dim() == 2 else rhs.numel(),
                                                  int(skip_dirichlet), workspace_bytes, C.byref(missing)))
        return missing.value


def integrate(mesh, residual_id, fields=None, kernel_params=None, asm_opts=(1, 0, 0), time=0.0, square=False,
              face_elem=None, face_side=None):
    """evalLocalIntegral (post/Integral.hpp:54-111): this rank's integral of a residual kernel over all elements, or over
    the listed element sides.  fields: contiguous (n_fields, n_local_nodes) device tensor.  Returns a numpy array
    [n_equations]; multi-rank callers all-reduce it (computeIntegral :113-128)."""
    info = residual_info(residual_id)
    blob, nbytes, keep = _blob(kernel_params)
    opts = capi.AsmOpts(*asm_opts)
    if fields is not None and (fields.dim() != 2 or not fields.is_contiguous()):
        raise L3KError("fields must be a contiguous (n_fields, n_local_nodes) tensor")
    out = np.zeros(info["n_equations"])
    if face_elem is None:
        nf, fe_p, fs_p = -1, None, None
    else:
        fe, fs = _sides(face_elem, face_side)
        nf, fe_p, fs_p = fe.size, fe.ctypes.data_as(capi.c_int64_p), fs.ctypes.data_as(capi.c_uint8_p)
    check(capi.load().l3k_integrate(mesh.ctx._h, mesh._h, residual_id, blob, nbytes, C.byref(opts), _ptr(fields),
                                    0 if fields is None else fields.shape[1], float(time), int(square), nf, fe_p, fs_p,
                                    out.ctypes.data_as(capi.c_double_p)))
    return out


def values_at_nodes(mesh, residual_id, dof_inds, values, fields=None, kernel_params=None, time=0.0, face_elem=None,
                    face_side=None):
    """computeValuesAtNodes (algsys/ComputeValuesAtNodes.hpp) on one rank -- the engine of setDirichletBCValues / setValues:
    evaluates the residual kernel at the nodes of the listed element sides (or of all elements), averages the
    contributions per dof and writes them into `values` (1-D device tensor over the local dofs); other entries keep their
    content.  Returns `values`."""
    import torch
    info = residual_info(residual_id)
    if len(dof_inds) != info["n_equations"]:
        raise L3KError("one dof index per equation of the kernel")
    blob, nbytes, keep = _blob(kernel_params)
    di = (C.c_int * len(dof_inds))(*dof_inds)
    s = torch.zeros_like(values)
    c = torch.zeros_like(values)
    if face_elem is None:
        nf, fe_p, fs_p = -1, None, None
    else:
        fe, fs = _sides(face_elem, face_side)
        nf, fe_p, fs_p = fe.size, fe.ctypes.data_as(capi.c_int64_p), fs.ctypes.data_as(capi.c_uint8_p)
    lib = capi.load()
    check(lib.l3k_values_at_nodes(mesh.ctx._h, mesh._h, residual_id, blob, nbytes, _ptr(fields),
                                  0 if fields is None else fields.shape[1], float(time), nf, fe_p, fs_p, di, _ptr(s), _ptr(c)))
    check(lib.l3k_average_values(mesh.ctx._h, _ptr(s), _ptr(c), values.numel(), _ptr(values)))
    return values


def update_solution(mesh, X, sol_inds, fields, sol_man_inds, XG=None):
    """MatrixFreeSystem::updateSolution (algsys/MatrixFreeSystem.hpp:1231-1273): the solution's per-node dofs `sol_inds` of every
    column of X (ncols, n_owned_dofs) -- ghost rows from XG (ncols, n_ghost_dofs), the imported values -- into the fields
    `sol_man_inds` (one per (index, column), index-major) of the SoA field storage `fields` (n_fields, n_local_nodes): what a
    kernel's FieldAccess reads at the next assembly (time stepping, Newton iterations)."""
    nc, ldx = MatrixFreeSystem._cols(X)
    if fields.dim() != 2 or not fields.is_contiguous():
        raise L3KError("fields must be a contiguous (n_fields, n_local_nodes) tensor")
    if len(sol_man_inds) != len(sol_inds) * nc:
        raise L3KError("Source and destination indices lengths must match")  # MatrixFreeSystem.hpp:1237-1238
    si = (C.c_int * len(sol_inds))(*[int(i) for i in sol_inds])
    di = (C.c_int * len(sol_man_inds))(*[int(i) for i in sol_man_inds])
    check(capi.load().l3k_update_solution(mesh.ctx._h, mesh._h, _ptr(X), ldx, _ptr(XG), 0 if XG is None else XG.shape[1], nc,
                                          len(sol_inds), si, di, _ptr(fields), fields.shape[1], fields.shape[0]))
    return fields


def norm_l2(mesh, residual_id, fields=None, kernel_params=None, asm_opts=(1, 0, 0), time=0.0, face_elem=None,
            face_side=None, group=None):
    """computeNormL2 (post/NormL2.hpp:31-62): sqrt of the integral of the squared residual with doubled quadrature
    orders; all-reduced over `group` when torch.distributed is initialised."""
    doubled = (2 * asm_opts[0], 2 * asm_opts[1], asm_opts[2])
    sq = integrate(mesh, residual_id, fields, kernel_params, doubled, time, True, face_elem, face_side)
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
        import torch
        t = torch.from_numpy(sq)
        if dist.get_backend(group) == "nccl":
            t = t.cuda()
        dist.all_reduce(t, group=group)
        sq = t.cpu().numpy()
    return np.sqrt(sq)


def element_node_split(order, dim=3):
    """(primary, internal) element-local node indices of a hex (dim = 3: ix + n iy + n^2 iz, n = order + 1) or a quad (dim = 2:
    ix + n iy) of `order`, each ascending: the internal nodes have all of their indices in 1 .. order-1
    (mesh/ElementTraits.hpp:37-59)."""
    if dim not in (2, 3):
        raise L3KError(f"element_node_split: dim = {dim}; it is 2 (quads) or 3 (hexes)")
    n = order + 1
    idx = np.arange(n ** dim)
    inner = np.ones(idx.shape, dtype=bool)
    for d in range(dim):
        i = (idx // n ** d) % n
        inner &= (i >= 1) & (i <= order - 1)
    return idx[~inner], idx[inner]


def condensed_graph(elem_nodes, order, dofs_per_node, field_inds):
    """CSR sparsity (row_ptr int64, col_ind int32, columns ascending) over the local dofs that couples the primary dofs of every
    element with each other: the graph of the condensed system (the rows of internal dofs are empty).  Built at node level
    (one entry per coupled node pair), then expanded to the dofs of the fields."""
    elem_nodes = np.asarray(elem_nodes).astype(np.int64)
    fi = np.sort(np.asarray(field_inds, dtype=np.int64))
    U, dpn = len(fi), int(dofs_per_node)
    primary, _ = element_node_split(order)
    n_nodes = int(elem_nodes.max()) + 1 if elem_nodes.size else 0
    en = elem_nodes[:, primary]
    key = np.unique((en[:, :, None] * n_nodes + en[:, None, :]).ravel())
    ra, cb = key // max(n_nodes, 1), key % max(n_nodes, 1)
    deg = np.bincount(ra, minlength=n_nodes).astype(np.int64)
    node_cols = (cb[:, None] * dpn + fi[None, :]).ravel()  # per node: its neighbour dofs, ascending
    seg_start = U * (np.cumsum(deg) - deg)
    seg_len = U * deg
    # rows (a, f) for f in fi, ascending in the dof a dpn + f; each holds node a's segment
    row_len = np.zeros((n_nodes, dpn), dtype=np.int64)
    row_len[:, fi] = seg_len[:, None]
    row_ptr = np.concatenate([[0], np.cumsum(row_len.ravel())]).astype(np.int64)
    starts, lens = np.repeat(seg_start, U), np.repeat(seg_len, U)
    total = int(lens.sum())
    base = np.repeat(starts - (np.cumsum(lens) - lens), lens)
    col_ind = node_cols[base + np.arange(total)] if total else np.zeros(0, np.int64)
    return row_ptr, col_ind.astype(np.int32)


class MatrixFreeSystem:
    """algsys::MatrixFreeSystem for one rank: kernel + mesh -> operator.  apply() is Operator::apply
    (Y <- alpha*A*X + beta*Y, algsys/MatrixFreeSystem.hpp:34-41,1038)."""

    def __init__(self, mesh, kernel_id, kernel_params=None, asm_opts=(1, 0, 0), field_inds=None, n_rhs=1):
        self.mesh, self.ctx, self.kernel_id, self.n_rhs = mesh, mesh.ctx, kernel_id, n_rhs
        self.info = kernel_info(kernel_id)
        blob = None
        nbytes = 0
        if kernel_params is not None:
            arr = np.ascontiguousarray(kernel_params, dtype=np.float64)
            blob, nbytes = arr.ctypes.data_as(C.c_void_p), arr.nbytes
        opts = capi.AsmOpts(*asm_opts)
        fi = None
        if field_inds is not None:
            fi = (C.c_int * len(field_inds))(*field_inds)
        self.field_inds = list(range(self.info["n_unknowns"])) if field_inds is None else [int(f) for f in field_inds]
        self._h = C.c_void_p()
        check(capi.load().l3k_mf_create(self.ctx._h, mesh._h, kernel_id, blob, nbytes, C.byref(opts), fi, n_rhs,
                                        C.byref(self._h)))
        self._fields = None
        self._boundary_terms = []

    def __del__(self):
        if getattr(self, "_h", None) and capi is not None:
            capi.load().l3k_mf_destroy(self._h)
            self._h = None

    def attach_boundary(self, term):
        """Registers a BoundaryTerm: apply / apply_elems / diag_rhs include it from now on."""
        check(capi.load().l3k_mf_attach_boundary(self._h, term._h))
        self._boundary_terms.append(term)  # keeps the term alive as long as the system

    def assemble_boundary(self, on=True):
        """With on, local_assemble, assemble_global, condense_local, condense_global and recover_internal work on
        K_e + sum K_s, F_e + sum F_s over the attached sides of each element (l3k_mf_assemble_boundary; hexes).  Off by
        default: the assembled and condensed calls then ignore the attached terms."""
        check(capi.load().l3k_mf_assemble_boundary(self._h, int(bool(on))))

    # post::FieldAccess: SoA (n_fields, n_local_nodes) device tensor, kept alive here
    def set_fields(self, fields):
        if fields is not None and (fields.dim() != 2 or not fields.is_contiguous()):
            raise L3KError("fields must be a contiguous (n_fields, n_local_nodes) tensor")
        self._fields = fields
        check(capi.load().l3k_mf_set_fields(self._h, _ptr(fields), 0 if fields is None else fields.shape[1]))

    def set_time(self, t):
        check(capi.load().l3k_mf_set_time(self._h, float(t)))

    def route(self, which=2, ncols=1, with_energy=False):
        """One line naming the kernel (template, variant, lanes, LDS, grid) the element launch of apply_elems(which, ...,
        ncols columns) takes right now -- decided by the launcher's own code (l3k_mf_route)."""
        buf = C.create_string_buffer(512)
        check(capi.load().l3k_mf_route(self._h, which, ncols, int(with_energy), buf, len(buf)))
        return buf.value.decode()

    @staticmethod
    def _cols(t):
        if t.dim() != 2 or t.stride(1) != 1:
            raise L3KError("multivectors are (ncols, ld) tensors with unit stride along rows")
        return t.shape[0], (t.stride(0) if t.shape[0] > 1 else t.shape[1])

    def apply(self, X, Y, alpha=1.0, beta=0.0):
        nc, ldx = self._cols(X)
        nc2, ldy = self._cols(Y)
        if nc != nc2:
            raise L3KError("X and Y must have the same number of columns")  # MatrixFreeSystem.hpp:1035
        check(capi.load().l3k_mf_apply(self._h, _ptr(X), ldx, _ptr(Y), ldy, nc, alpha, beta))
        return Y

    # split-phase pieces (used by DistributedOperator)
    def apply_energy(self, X, Y, S):
        """Y <- A X (one column) and S[1] <- <X, A X> in one pass (l3k_mf_apply_energy): S is the PCG's device scalar
        block (8 doubles)."""
        check(capi.load().l3k_mf_apply_energy(self._h, _ptr(X), _ptr(Y), _ptr(S)))
        return Y

    def energy_begin(self, S):
        check(capi.load().l3k_mf_energy_begin(self._h, _ptr(S)))

    def energy_end(self, X):
        """True if S[1] now holds this rank's share of <X, A X> (else take the dot product)."""
        fused = C.c_int(0)
        check(capi.load().l3k_mf_energy_end(self._h, _ptr(X), C.byref(fused)))
        return bool(fused.value)

    def scale(self, Y, beta):
        nc, ldy = self._cols(Y)
        check(capi.load().l3k_mf_scale(self._h, _ptr(Y), ldy, nc, beta))

    def apply_elems(self, which, X, XG, Y, YG, alpha, beta):
        """beta must be the value scale() was called with (see l3k_mf_scale in include/l3k.h)."""
        nc, ldx = self._cols(X)
        _, ldy = self._cols(Y)
        # (the stride between the columns, not the number of ghost rows: the ghost rows may be a view behind the owned rows)
        ldxg = self._cols(XG)[1] if XG is not None else 0
        ldyg = self._cols(YG)[1] if YG is not None else 0
        check(capi.load().l3k_mf_apply_elems(self._h, which, _ptr(X), ldx, _ptr(XG), ldxg, _ptr(Y), ldy, _ptr(YG), ldyg,
                                             nc, alpha, beta))

    def dirichlet_rows(self, X, Y, alpha):
        nc, ldx = self._cols(X)
        _, ldy = self._cols(Y)
        check(capi.load().l3k_mf_dirichlet_rows(self._h, _ptr(X), ldx, _ptr(Y), ldy, nc, alpha))

    def pack_rows(self, src, idx, dst):
        nc, ld = self._cols(src)
        check(capi.load().l3k_pack_rows(self.ctx._h, _ptr(src), ld, nc, _ptr(idx), idx.numel(), _ptr(dst)))

    def unpack_add_rows(self, src, idx, dst):
        nc, ld = self._cols(dst)
        check(capi.load().l3k_unpack_add_rows(self.ctx._h, _ptr(src), idx.numel(), _ptr(idx), _ptr(dst), ld, nc))

    def diag_rhs(self, dirichlet_vals=None, which=2, diag=None, rhs=None, diag_ghost=None, rhs_ghost=None,
                 finalize=True):
        """computeDiagAndRhs (algsys/MatrixFreeSystem.hpp:888-941): diag(A) and the rhs with Dirichlet lifting.
        dirichlet_vals: (n_rhs, n_local_dofs) tensor or None (= 0).  Returns (diag [n_owned], rhs (n_rhs, n_owned));
        accumulates into the given tensors (the caller zeroes them), allocates zeroed ones otherwise."""
        import torch
        n_owned, n_ghost = self.mesh.n_owned_dofs, self.mesh.n_ghost_dofs
        dev = "cuda"
        if diag is None:
            diag = torch.zeros(n_owned, dtype=torch.float64, device=dev)
        if rhs is None:
            rhs = torch.zeros((self.n_rhs, n_owned), dtype=torch.float64, device=dev)
        if n_ghost and diag_ghost is None:
            diag_ghost = torch.zeros(n_ghost, dtype=torch.float64, device=dev)
            rhs_ghost = torch.zeros((self.n_rhs, n_ghost), dtype=torch.float64, device=dev)
        g = dirichlet_vals
        ldg = 0 if g is None else g.shape[1]
        check(capi.load().l3k_mf_diag_rhs(self._h, which, _ptr(g), ldg, _ptr(diag), _ptr(rhs), rhs.shape[1],
                                          _ptr(diag_ghost), _ptr(rhs_ghost), max(n_ghost, 1), int(finalize)))
        return diag, rhs

    def dirichlet_finalize(self, dirichlet_vals, diag, rhs):
        """diag = 1, rhs = g on the owned Dirichlet rows (the last step of computeDiagAndRhs, after the export)"""
        g = dirichlet_vals
        check(capi.load().l3k_mf_dirichlet_finalize(self._h, _ptr(g), 0 if g is None else g.shape[1], _ptr(diag), _ptr(rhs),
                                                    rhs.shape[1]))

    def local_assemble(self, first=0, count=None, want_K=True, want_F=True, want_checksum=False):
        """assembleLocalSystem for elements [first, first+count) (algsys/AssembleLocalSystem.hpp:234-256).
        Returns (K [count, Nd, Nd] row-major, F [count, n_rhs, Nd] i.e. column-major Nd x n_rhs per element, checksum)."""
        import torch
        count = self.mesh.part.n_elems - first if count is None else count
        Nd = (self.mesh.part.order + 1) ** 3 * self.info["n_unknowns"]
        K = torch.empty((count, Nd, Nd), dtype=torch.float64, device="cuda") if want_K else None
        F = torch.zeros((count, self.n_rhs, Nd), dtype=torch.float64, device="cuda") if want_F else None
        cs = torch.empty(count, dtype=torch.float64, device="cuda") if want_checksum else None
        check(capi.load().l3k_local_assemble(self._h, first, count, _ptr(K), _ptr(F), _ptr(cs)))
        return K, F, cs

    def element_systems(self, first=0, count=None, want_K=True, want_F=True):
        """assembleLocalSystem for the elements [first, first+count) (l3k_asm_element_systems; hexes and quads).  Returns
        (K [count, Nd, Nd] row-major, bitwise symmetric, F [count, n_rhs, Nd]), Nd = (p+1)^dim U."""
        import torch
        count = self.mesh.part.n_elems - first if count is None else count
        Nd = (self.mesh.part.order + 1) ** self.mesh.part.dim * self.info["n_unknowns"]
        n = max(count, 0)
        K = torch.empty((n, Nd, Nd), dtype=torch.float64, device="cuda") if want_K else None
        F = torch.zeros((n, self.n_rhs, Nd), dtype=torch.float64, device="cuda") if want_F else None
        check(capi.load().l3k_asm_element_systems(self._h, first, count, _ptr(K), _ptr(F)))
        return K, F

    def local_assemble_into(self, K, first=0, count=None):
        """The element matrices of [first, first + count) into the caller's tensor K [count, Nd, Nd] (row-major, bitwise symmetric)."""
        count = K.shape[0] if count is None else count
        Nd = (self.mesh.part.order + 1) ** 3 * self.info["n_unknowns"]
        if tuple(K.shape[1:]) != (Nd, Nd) or K.shape[0] < count or not K.is_contiguous() or str(K.dtype) != "torch.float64":
            raise L3KError(f"local_assemble_into: K must be a contiguous float64 tensor [>= {count}, {Nd}, {Nd}]")
        check(capi.load().l3k_local_assemble(self._h, first, count, _ptr(K), None, None))
        return K

    def assembled_scatter(self, K, F, row_ptr, col_ind, values, rhs, first=0, skip_dirichlet=False):
        """scatterLocalSystem for the batch [first, first + len(K)) (algsys/ScatterLocalSystem.hpp:24-54): K [count, Nd, Nd]
        and F [count, n_rhs, Nd] as local_assemble returns them, summed into `values` (over the caller's CSR graph
        row_ptr int64 / col_ind int32, device tensors) and `rhs` [n_rhs, n_local_dofs].  Returns the number of entries
        that were not in the graph."""
        import ctypes as C
        count = (K if K is not None else F).shape[0]
        missing = C.c_int64(0)
        check(capi.load().l3k_assembled_scatter(self._h, first, count, _ptr(K), _ptr(F), _ptr(row_ptr), _ptr(col_ind), _ptr(values),
                                                _ptr(rhs), 0 if rhs is None else rhs.stride(0) if rhs.dim() == 2 else rhs.numel(),
                                                int(skip_dirichlet), C.byref(missing)))
        return missing.value

    def local_assemble_tiled(self, first=0, count=None):
        """K_e of the elements [first, first + count) in the tiled layout of l3k_local_assemble_tiled: a tensor
        [count, U, U, n, n, n, n, n, n] indexed [e, u, u', bx', bz, bx, by, by', bz']."""
        import torch
        count = self.mesh.part.n_elems - first if count is None else count
        n, U = self.mesh.part.order + 1, self.info["n_unknowns"]
        Kt = torch.empty((count, U, U, n, n, n, n, n, n), dtype=torch.float64, device="cuda")
        check(capi.load().l3k_local_assemble_tiled(self._h, first, count, _ptr(Kt)))
        return Kt

    def assemble_global(self, row_ptr, col_ind, values, rhs=None, first=0, count=None, skip_dirichlet=False, workspace_bytes=0):
        """assembleGlobalSystem for the elements [first, first + count) (algsys/AssembleGlobalSystem.hpp:20-53): element systems
        formed and summed into `values` (over the CSR graph row_ptr int64 / col_ind int32) and `rhs` [n_rhs, n_local_dofs] inside
        the library, assembly and scatter of consecutive sub-batches overlapped on two streams.  Returns the number of entries
        outside the graph."""
        import ctypes as C
        count = self.mesh.part.n_elems - first if count is None else count
        missing = C.c_int64(0)
        check(capi.load().l3k_assemble_global(self._h, first, count, _ptr(row_ptr), _ptr(col_ind), _ptr(values), _ptr(rhs),
                                              0 if rhs is None else rhs.stride(0) if rhs.dim() == 2 else rhs.numel(),
                                              int(skip_dirichlet), workspace_bytes, C.byref(missing)))
        return missing.value

    def condense_local(self, first=0, count=None, want_S=True, want_G=True):
        """Static condensation of the element-internal dofs (StaticCondensationManager::condenseSystem,
        algsys/StaticCondensationManager.hpp:322-350) for elements [first, first+count): S [count, Nbd, Nbd] = K_bb - K_bi K_ii^-1 K_ib
        (row-major, bitwise symmetric) and G [count, n_rhs, Nbd] = F_b - K_bi K_ii^-1 F_i over the primary dofs of each element
        (element_node_split(order)[0], node-major)."""
        import torch
        count = self.mesh.part.n_elems - first if count is None else count
        primary, _ = element_node_split(self.mesh.part.order)
        Nbd = len(primary) * self.info["n_unknowns"]
        S = torch.empty((count, Nbd, Nbd), dtype=torch.float64, device="cuda") if want_S else None
        G = torch.empty((count, self.n_rhs, Nbd), dtype=torch.float64, device="cuda") if want_G else None
        check(capi.load().l3k_condense_local(self._h, first, count, _ptr(S), _ptr(G)))
        return S, G

    def condense_global(self, row_ptr, col_ind, values, rhs=None, first=0, count=None, skip_dirichlet=False, workspace_bytes=0):
        """Condensed assembleGlobalSystem for the elements [first, first + count): element systems formed, condensed and their
        S_e / g_e summed into `values` (over the CSR graph row_ptr int64 / col_ind int32, e.g. condensed_graph) and `rhs`
        [n_rhs, n_local_dofs] inside the library.  Returns the number of entries outside the graph."""
        import ctypes as C
        count = self.mesh.part.n_elems - first if count is None else count
        missing = C.c_int64(0)
        check(capi.load().l3k_condense_global(self._h, first, count, _ptr(row_ptr), _ptr(col_ind), _ptr(values), _ptr(rhs),
                                              0 if rhs is None else rhs.stride(0) if rhs.dim() == 2 else rhs.numel(),
                                              int(skip_dirichlet), workspace_bytes, C.byref(missing)))
        return missing.value

    def recover_internal(self, X, first=0, count=None):
        """StaticCondensationManager::recoverSolution for the elements [first, first + count): X [n_rhs, n_local_dofs] holds the
        solution on the primary dofs; its element-internal dofs are overwritten with K_ii^-1 (F_i - K_ib x_b).  The element systems
        are formed again: the system's fields and time must be those it was condensed with."""
        count = self.mesh.part.n_elems - first if count is None else count
        ldx = (X.stride(0) if X.shape[0] > 1 else X.shape[1]) if X.dim() == 2 else X.numel()  # (a single row may carry stride 0)
        check(capi.load().l3k_condensed_recover(self._h, first, count, _ptr(X), ldx))
        return X

    def new_ghost_buffer(self, ncols, like):
        import torch
        return torch.zeros((ncols, max(self.mesh.n_ghost_dofs, 1)), dtype=torch.float64, device=like.device)

    def sparsity_graph(self, kind="full"):
        """The CSR graph of this system's dofs on its mesh, built on the device (SparsityGraph): kind "full" is what
        assemble_global writes into, "condensed" what condense_global does; CsrOperator takes its tensors as they are."""
        return SparsityGraph(self.mesh, self.field_inds, kind)


class SparsityGraph:
    """The CSR sparsity graph of a DeviceMesh over its local dofs, built on the device (l3k_graph_create / l3k_graph_fill;
    computeLocalGraph, algsys/SparsityGraph.hpp:26-81): the dofs node * dofs_per_node + field_inds[u] of every element coupled
    with each other (kind "full"), or those of the element's primary nodes only (kind "condensed", hexes).  field_inds: strictly
    ascending, None = all dofs of the node.  row_ptr int64 [n + 1] and col_ind int32 [nnz] are torch tensors on the mesh's
    device, columns ascending within a row; `info` holds n, nnz, n_empty_rows, max_row_len, n_rows_scratch, workspace_bytes,
    max_elems_per_node and lds_key_capacity (l3k_graph_info)."""

    KINDS = {"full": 0, "condensed": 1}

    def __init__(self, mesh, field_inds=None, kind="full"):
        import types
        self.mesh, self.ctx = mesh, mesh.ctx
        if kind not in self.KINDS:
            raise L3KError(f"SparsityGraph: kind is 'full' or 'condensed', not {kind!r}")
        fi = None if field_inds is None else (C.c_int * len(field_inds))(*[int(f) for f in field_inds])
        self._h = C.c_void_p()
        check(capi.load().l3k_graph_create(mesh._h, 0 if fi is None else len(fi), fi, self.KINDS[kind], C.byref(self._h)))
        i = capi.GraphInfo()
        check(capi.load().l3k_graph_info_get(self._h, C.byref(i)))
        self.info = types.SimpleNamespace(**{name: getattr(i, name) for name, _ in capi.GraphInfo._fields_})
        self.n = self.info.n
        self.row_ptr, self.col_ind = self.fill()

    def fill(self, row_ptr=None, col_ind=None):
        """Writes the graph into row_ptr int64 [n + 1] and col_ind int32 [nnz] (allocated here if not given); returns both."""
        import torch
        dev = torch.device("cuda", self.ctx.device)
        row_ptr = torch.empty(self.info.n + 1, dtype=torch.int64, device=dev) if row_ptr is None else row_ptr
        col_ind = torch.empty(self.info.nnz, dtype=torch.int32, device=dev) if col_ind is None else col_ind
        if row_ptr.dtype != torch.int64 or col_ind.dtype != torch.int32 or row_ptr.numel() < self.info.n + 1 or \
                col_ind.numel() < self.info.nnz or not (row_ptr.is_contiguous() and col_ind.is_contiguous()):
            raise L3KError("SparsityGraph.fill: row_ptr is a contiguous int64 tensor of n + 1 entries, col_ind an int32 one of nnz")
        check(capi.load().l3k_graph_fill(self._h, _ptr(row_ptr), _ptr(col_ind) if col_ind.numel() else None))
        return row_ptr, col_ind

    def __del__(self):
        if getattr(self, "_h", None) and capi is not None:
            capi.load().l3k_graph_destroy(self._h)
            self._h = None


class CsrOperator:
    """A square CSR matrix on the device in front of the solver (l3k_csr_create): row_ptr int64 [n + 1], col_ind int32 strictly
    ascending within a row, values float64 -- the arrays assemble_global / condense_global fill.  Nothing is copied: the three
    tensors are kept alive here, and `values` may be rewritten between calls (the graph may not).  Creation validates the graph
    on the device and refuses one through which an apply could gather out of bounds.  n_owned_dofs = n, so solve.pcg and
    solve.ChebyshevPreconditioner take it where they take a MatrixFreeSystem.  Applies and solves are bitwise reproducible on
    any context.  lanes_per_row: 0 = chosen from the mean row length, else 4, 16 or 64."""

    def __init__(self, ctx, row_ptr, col_ind, values, lanes_per_row=0):
        import torch
        if row_ptr.dtype != torch.int64 or col_ind.dtype != torch.int32 or values.dtype != torch.float64:
            raise L3KError("CsrOperator: row_ptr is int64, col_ind int32 and values float64")
        if row_ptr.dim() != 1 or row_ptr.numel() < 1 or not (row_ptr.is_contiguous() and col_ind.is_contiguous() and values.is_contiguous()):
            raise L3KError("CsrOperator: row_ptr [n + 1], col_ind [nnz] and values [nnz] are contiguous 1-D tensors")
        if col_ind.numel() != values.numel() or int(row_ptr[-1].item()) != col_ind.numel():
            raise L3KError("CsrOperator: col_ind and values must have row_ptr[n] entries each")
        self.ctx, self.row_ptr, self.col_ind, self.values = ctx, row_ptr, col_ind, values
        self.n = self.n_owned_dofs = row_ptr.numel() - 1
        self._h = C.c_void_p()
        check(capi.load().l3k_csr_create(ctx._h, self.n, _ptr(row_ptr), _ptr(col_ind), _ptr(values), int(lanes_per_row),
                                         C.byref(self._h)))

    def __del__(self):
        if getattr(self, "_h", None) and capi is not None:
            capi.load().l3k_csr_destroy(self._h)
            self._h = None

    def info(self):
        """n, nnz, n_empty_rows, max_row_len, mean_row_len (of the non-empty rows), lanes_per_row (l3k_csr_info)"""
        import types
        i = capi.CsrInfo()
        check(capi.load().l3k_csr_info_get(self._h, C.byref(i)))
        return types.SimpleNamespace(**{name: getattr(i, name) for name, _ in capi.CsrInfo._fields_})

    def apply(self, X, Y, alpha=1.0, beta=0.0):
        """Y <- alpha A X + beta Y; X, Y: (ncols, ld) multivectors or 1-D vectors over the n rows (l3k_csr_apply)"""
        if X.dim() == 1 and Y.dim() == 1:
            X, Y2 = X[None, :], Y[None, :]
        else:
            Y2 = Y
        nc, ldx = MatrixFreeSystem._cols(X)
        nc2, ldy = MatrixFreeSystem._cols(Y2)
        if nc != nc2 or X.shape[1] < self.n or Y2.shape[1] < self.n:
            raise L3KError("X and Y must have the same number of columns and at least n rows")
        check(capi.load().l3k_csr_apply(self._h, _ptr(X), ldx, _ptr(Y2), ldy, nc, alpha, beta))
        return Y

    def apply_energy(self, X, Y, S):
        """Y <- A X (one column) and S[1] <- <X, A X> in one pass (l3k_csr_apply_energy): S is the PCG's scalar block (8 doubles)"""
        if X.numel() != self.n or Y.numel() != self.n or S.numel() < 8 or not (X.is_contiguous() and Y.is_contiguous()):
            raise L3KError("X and Y are contiguous vectors over the n rows, S has 8 entries")
        check(capi.load().l3k_csr_apply_energy(self._h, _ptr(X), _ptr(Y), _ptr(S)))
        return Y

    def _diag(self, want_diag, want_minv, damping, threshold):
        import torch
        out = [torch.empty(self.n, dtype=torch.float64, device=self.values.device) if w else None for w in (want_diag, want_minv)]
        check(capi.load().l3k_csr_diag(self._h, _ptr(out[0]), float(damping), float(threshold), _ptr(out[1])))
        return out

    def diag(self):
        """The stored diagonal, 0 where a row has none (l3k_csr_diag)"""
        return self._diag(True, False, 1.0, 0.0)[0]

    def jacobi_inverse(self, damping=1.0, threshold=0.0):
        """sign(a_ii) damping / max(|a_ii|, threshold) on the non-empty rows, 0 on the empty ones, which the PCG then leaves
        alone (l3k_csr_diag)"""
        return self._diag(False, True, damping, threshold)[1]

    def dirichlet(self, mask, bc_vals, rhs):
        """DirichletBCAlgebraic::apply in place (l3k_csr_dirichlet): mask uint8 [n]; bc_vals, rhs: (ncols, ld) or 1-D.  Rewrites
        self.values and rhs; raises, with nothing changed, if a masked row stores no diagonal entry."""
        import torch
        if mask.dtype != torch.uint8 or mask.numel() != self.n or not mask.is_contiguous():
            raise L3KError("mask must be a contiguous uint8 tensor over the n rows")
        g, r = (bc_vals[None, :], rhs[None, :]) if rhs.dim() == 1 else (bc_vals, rhs)
        nc, ldg = MatrixFreeSystem._cols(g)
        nc2, ldr = MatrixFreeSystem._cols(r)
        if nc != nc2 or g.shape[1] < self.n or r.shape[1] < self.n:
            raise L3KError("Number of RHSs must be equal to the number of prescribed values")  # bcs/DirichletBC.hpp:86
        check(capi.load().l3k_csr_dirichlet(self._h, _ptr(self.values), _ptr(mask), _ptr(g), ldg, _ptr(r), ldr, nc))
        return rhs

    def dirichlet_local(self, mask, bc_vals_local, rhs, n_owned):
        """The rank-local Dirichlet step with the owner rule on the local matrix of a partitioned system, in place
        (l3k_csr_dirichlet_dist): the operator is over the local dofs [owned | ghost], the first n_owned rows are owned; mask uint8
        [n], bc_vals_local and rhs (ncols, ld) or 1-D over the LOCAL dofs (ghost values imported by the caller).  A flagged owned row
        becomes the identity row with rhs = g, a flagged ghost row an all-zero row with rhs = 0.  DistributedCsrOperator(self, halo)
        then applies the ranks' matrices as one; the ghost rows of rhs still have to be export-added into their owners' rows."""
        import torch
        if mask.dtype != torch.uint8 or mask.numel() != self.n or not mask.is_contiguous():
            raise L3KError("mask must be a contiguous uint8 tensor over the n rows")
        g, r = (bc_vals_local[None, :], rhs[None, :]) if rhs.dim() == 1 else (bc_vals_local, rhs)
        nc, ldg = MatrixFreeSystem._cols(g)
        nc2, ldr = MatrixFreeSystem._cols(r)
        if nc != nc2 or g.shape[1] < self.n or r.shape[1] < self.n:
            raise L3KError("Number of RHSs must be equal to the number of prescribed values")  # bcs/DirichletBC.hpp:86
        check(capi.load().l3k_csr_dirichlet_dist(self._h, _ptr(self.values), _ptr(mask), _ptr(g), ldg, _ptr(r), ldr, nc, int(n_owned)))
        return rhs


class _AssembledOperator(CsrOperator):
    """The CsrOperator of a closed AssembledSystem: the l3k_csr handle belongs to the system (which is kept alive here), the
    tensors are views of the system's arrays."""

    def __init__(self, system, handle):
        self.ctx, self.row_ptr, self.col_ind, self.values = system.ctx, system.row_ptr, system.col_ind, system.values
        self.n = self.n_owned_dofs = system.n
        self.system = system
        self._h = C.c_void_p(handle)

    def __del__(self):  # (not the owner of the handle)
        self._h = None


class DistributedCsrOperator:
    """The assembled or condensed matrix of a partitioned mesh in front of the solver (l3k_csr_dist_*), in the sub-assembled form:
    `local` is this rank's CsrOperator over its local dofs [owned | ghost] -- the matrix of its own elements -- and the global
    matrix, the sum of the ranks' local ones, is never formed; vectors hold the owned rows only and the exchanges of `halo` (a
    distributed.NativeHalo) run inside every apply.  AssembledSystem(..., halo=...).end() returns one; it can also be built from any
    CsrOperator over local dofs (arrays filled by assemble_global / condense_global on a partitioned hex mesh, after
    dirichlet_local) plus the halo.  n = n_owned_dofs: the owned dofs.  solve.pcg_distributed takes it as its `op` (with minv from
    jacobi_inverse, and with precond=dict(...) for Chebyshev): its host loop takes <p, A p> from apply(..., energy=s), and with
    native=True the whole iteration runs inside the library (l3k_csr_dist_pcg_solve).  apply, diag and jacobi_inverse are
    collective.  Applies are bitwise reproducible."""

    def __init__(self, local, halo, n_owned=None, _handle=None):
        lib = capi.load()
        self.local, self.halo, self.ctx = local, halo, local.ctx
        self.n_ghost = int(lib.l3k_halo_n_ghost_dofs(halo._h))
        self.n = self.n_owned_dofs = local.n - self.n_ghost if n_owned is None else int(n_owned)
        self._own = _handle is None
        self._h = C.c_void_p(_handle)
        if self._own:
            check(lib.l3k_csr_dist_create(local._h, halo._h, self.n, C.byref(self._h)))

    def __del__(self):
        if getattr(self, "_h", None) and capi is not None:
            if self._own:
                capi.load().l3k_csr_dist_destroy(self._h)
            self._h = None

    def _rows(self, ptr, count):
        import torch
        dev = torch.device("cuda", self.ctx.device)
        if count == 0:
            return torch.empty(0, dtype=torch.int32, device=dev)

        class _Mem:
            pass
        m = _Mem()
        m.owner = self
        m.__cuda_array_interface__ = {"shape": (int(count),), "typestr": "<i4", "data": (int(ptr), False), "version": 2, "strides": None}
        return torch.as_tensor(m, device=dev)

    @property
    def info(self):
        """n_owned, n_ghost, n_interior_rows, n_border_rows, n_ghost_rows and the three ascending row lists interior_rows,
        border_rows, ghost_rows as int32 device tensors (views of the operator's lists: l3k_csr_dist_info)"""
        import types
        i = capi.CsrDistInfo()
        check(capi.load().l3k_csr_dist_info_get(self._h, C.byref(i)))
        return types.SimpleNamespace(n_owned=i.n_owned, n_ghost=i.n_ghost, n_interior_rows=i.n_interior_rows,
                                     n_border_rows=i.n_border_rows, n_ghost_rows=i.n_ghost_rows,
                                     interior_rows=self._rows(i.d_interior_rows, i.n_interior_rows),
                                     border_rows=self._rows(i.d_border_rows, i.n_border_rows),
                                     ghost_rows=self._rows(i.d_ghost_rows, i.n_ghost_rows))

    def apply(self, X, Y, alpha=1.0, beta=0.0, energy=None):
        """Y <- alpha A X + beta Y on the owned rows; X, Y: (ncols, ld) multivectors or 1-D vectors over the owned rows
        (l3k_csr_dist_apply; collective).  energy: the PCG's device scalar block S (8 doubles); for one column with alpha = 1 and
        beta = 0, S[1] receives this rank's share of <X, A X> from the same launches (l3k_csr_dist_apply_energy) and
        self.energy_fused says that it did -- the protocol of distributed.DistributedOperator.apply."""
        if X.dim() == 1 and Y.dim() == 1:
            X, Y2 = X[None, :], Y[None, :]
        else:
            Y2 = Y
        nc, ldx = MatrixFreeSystem._cols(X)
        nc2, ldy = MatrixFreeSystem._cols(Y2)
        if nc != nc2 or X.shape[1] < self.n or Y2.shape[1] < self.n:
            raise L3KError("X and Y must have the same number of columns and at least n_owned rows")
        self.energy_fused = energy is not None and nc == 1 and alpha == 1.0 and beta == 0.0
        if self.energy_fused:
            if energy.numel() < 8 or not energy.is_contiguous():
                raise L3KError("energy is the PCG's scalar block: a contiguous tensor of 8 doubles")
            check(capi.load().l3k_csr_dist_apply_energy(self._h, _ptr(X), _ptr(Y2), _ptr(energy)))
        else:
            check(capi.load().l3k_csr_dist_apply(self._h, _ptr(X), ldx, _ptr(Y2), ldy, nc, alpha, beta))
        return Y

    def apply_energy(self, X, Y, S):
        """Y <- A X (one column over the owned rows) and S[1] <- this rank's share of <X, A X> (l3k_csr_dist_apply_energy;
        collective): S is the PCG's scalar block (8 doubles); no other slot of it is written"""
        if X.numel() != self.n or Y.numel() != self.n or S.numel() < 8 or not (X.is_contiguous() and Y.is_contiguous()):
            raise L3KError("X and Y are contiguous vectors over the owned rows, S has 8 entries")
        check(capi.load().l3k_csr_dist_apply_energy(self._h, _ptr(X), _ptr(Y), _ptr(S)))
        return Y

    def _diag(self, want_diag, want_minv, damping, threshold):
        import torch
        dev = torch.device("cuda", self.ctx.device)
        out = [torch.empty(self.n, dtype=torch.float64, device=dev) if w else None for w in (want_diag, want_minv)]
        check(capi.load().l3k_csr_dist_diag(self._h, _ptr(out[0]), float(damping), float(threshold), _ptr(out[1])))
        return out

    def diag(self):
        """The diagonal of the global matrix on the owned rows (l3k_csr_dist_diag; collective)"""
        return self._diag(True, False, 1.0, 0.0)[0]

    def jacobi_inverse(self, damping=1.0, threshold=0.0):
        """sign(a_ii) damping / max(|a_ii|, threshold) of the global diagonal on the owned rows, 0 on the empty ones, which the PCG
        then leaves alone (l3k_csr_dist_diag; collective)"""
        return self._diag(False, True, damping, threshold)[1]

    def import_ghosts(self, V):
        """comm::Import of a multivector (ncols, n_owned): its (ncols, max(n_ghost, 1)) ghost rows (l3k_halo_import)"""
        import torch
        ng = max(self.n_ghost, 1)
        ghost = torch.zeros((V.shape[0], ng), dtype=torch.float64, device=V.device)
        check(capi.load().l3k_halo_import(self.halo._h, _ptr(V), V.stride(0), V.shape[0], _ptr(ghost), ng))
        return ghost

    def export_add(self, ghost, owned):
        """comm::Export: every ghost row added into its owner's row of `owned` (l3k_halo_export_add)"""
        if ghost.numel() == 0:  # (a rank without ghosts still takes part; the halo takes no NULL vector)
            import torch
            ghost = torch.zeros((owned.shape[0], 1), dtype=torch.float64, device=owned.device)
        check(capi.load().l3k_halo_export_add(self.halo._h, _ptr(ghost), ghost.stride(0), owned.shape[0], _ptr(owned), owned.stride(0)))
        return owned


class AssembledSystem:
    """algsys::AssembledSystem for one rank, on hexes and on quads (l3k_asm_*): begin() / add(term) / end() are beginAssembly /
    assembleProblem(domain or boundary kernel) / endAssembly.  The object owns the CSR arrays of the full sparsity graph of
    field_inds (strictly ascending; None = all dofs of the node: the union of the terms' dofs), the right-hand sides
    [n_rhs, n] and, on quads, the sub-batch workspace (workspace_bytes, 0 = 1 GiB; hexes use the terms' own pipelines with that size);
    row_ptr, col_ind, values and rhs are torch views of them, not copies, made on access.  end() applies the mesh's Dirichlet mask with the prescribed values and returns a CsrOperator over the
    same arrays, which solve.pcg and solve.ChebyshevPreconditioner take.  Without a halo a partitioned mesh is refused.

    condensation="element_boundary" (quads; CondensationPolicy::ElementBoundary of the reference, l3k_asm_create_condensed): the
    matrix lives on the condensed graph (the primary dofs of every element coupled, the rows of internal dofs empty), the object
    keeps the internal rows of every element, end() eliminates them, and recover(x) fills the internal dofs of a solution.

    halo (a distributed.NativeHalo of this rank's part, l3k_asm_create_dist): the system of one rank of a partitioned mesh, in the
    sub-assembled form -- the arrays hold the local matrix over the local dofs [owned | ghost] and travel nowhere.  begin() and add()
    are rank-local; end(g_owned) is collective, takes the prescribed values over the OWNED dofs and returns a
    DistributedCsrOperator, which solve.pcg_distributed takes; rhs[:, :n_owned] is then the owned right-hand side (the ghost part
    has been added to its owners and is 0); recover(x_owned) is collective and returns the owned dofs.  The flags of a ghost dof
    in the mesh's Dirichlet mask must equal its owner's, as on the matrix-free path."""

    STATES = ("new", "open", "closed")
    CONDENSATION = ("none", "element_boundary")

    def __init__(self, mesh, field_inds=None, n_rhs=1, workspace_bytes=0, condensation="none", halo=None):
        condensation = "none" if condensation is None else condensation
        if condensation not in self.CONDENSATION:
            raise L3KError(f"AssembledSystem: condensation = {condensation!r}; it is one of {self.CONDENSATION}")
        self.mesh, self.ctx, self.n_rhs, self.condensation, self.halo = mesh, mesh.ctx, n_rhs, condensation, halo
        fi = None if field_inds is None else (C.c_int * len(field_inds))(*[int(f) for f in field_inds])
        self._h = C.c_void_p()
        if halo is not None:
            check(capi.load().l3k_asm_create_dist(mesh._h, halo._h, 0 if fi is None else len(fi), fi, n_rhs, workspace_bytes,
                                                  int(condensation != "none"), C.byref(self._h)))
        else:
            create = capi.load().l3k_asm_create if condensation == "none" else capi.load().l3k_asm_create_condensed
            check(create(mesh._h, 0 if fi is None else len(fi), fi, n_rhs, workspace_bytes, C.byref(self._h)))
        i = self._info()
        self.n, self.nnz = i.n, i.nnz
        self.n_owned = mesh.n_owned_dofs if halo is not None else i.n
        self.n_fields = mesh.dofs_per_node if field_inds is None else len(field_inds)

    def __del__(self):
        if getattr(self, "_h", None) and capi is not None:
            capi.load().l3k_asm_destroy(self._h)
            self._h = None

    def _info(self):
        i = capi.AsmInfo()
        check(capi.load().l3k_asm_info_get(self._h, C.byref(i)))
        return i

    # The four arrays as torch views, built afresh on every access: a view keeps the system alive (its memory is the system's), the
    # system keeps no view -- torch pins the exporting object from C, where the cycle collector could not see a cycle back to self
    @property
    def row_ptr(self):
        i = self._info()
        return self._view(i.d_row_ptr, (i.n + 1,), "<i8")

    @property
    def col_ind(self):
        i = self._info()
        return self._view(i.d_col_ind, (i.nnz,), "<i4")

    @property
    def values(self):
        i = self._info()
        return self._view(i.d_values, (i.nnz,), "<f8")

    @property
    def rhs(self):
        i = self._info()
        return self._view(i.d_rhs, (i.n_rhs, i.ldr), "<f8")[:, :i.n]

    def _view(self, ptr, shape, typestr):
        """A torch tensor over device memory the object owns (no copy; the tensor keeps `self` alive)"""
        import torch
        dtype = {"<i8": torch.int64, "<i4": torch.int32, "<f8": torch.float64}[typestr]
        dev = torch.device("cuda", self.ctx.device)
        if int(np.prod(shape)) == 0:
            return torch.empty(shape, dtype=dtype, device=dev)

        class _Mem:
            pass
        m = _Mem()
        m.owner = self
        m.__cuda_array_interface__ = {"shape": tuple(int(x) for x in shape), "typestr": typestr, "data": (int(ptr), False),
                                      "version": 2, "strides": None}
        return torch.as_tensor(m, device=dev)

    @property
    def info(self):
        """n, nnz, n_missing (entries outside the graph: 0 by construction), ldr, n_rhs and state ("new", "open", "closed")"""
        import types
        i = self._info()
        return types.SimpleNamespace(n=i.n, nnz=i.nnz, n_missing=i.n_missing, ldr=i.ldr, n_rhs=i.n_rhs, state=self.STATES[i.state])

    def begin(self):
        """beginAssembly: values and rhs <- 0, the system is open (allowed in any state)"""
        check(capi.load().l3k_asm_begin(self._h))
        return self

    def add(self, term, first=0, count=None):
        """assembleProblem: the element systems of a MatrixFreeSystem's elements, or the side systems of a BoundaryTerm's sides,
        [first, first + count) summed into values and rhs"""
        if isinstance(term, BoundaryTerm):
            count = term.n_faces - first if count is None else count
            check(capi.load().l3k_asm_add_boundary(self._h, term._h, first, count))
        elif isinstance(term, MatrixFreeSystem):
            count = term.mesh.part.n_elems - first if count is None else count
            check(capi.load().l3k_asm_add_domain(self._h, term._h, first, count))
        else:
            raise L3KError("AssembledSystem.add takes a MatrixFreeSystem or a BoundaryTerm")
        return self

    def end(self, dirichlet_vals=None):
        """endAssembly: the mesh's Dirichlet mask applied with the prescribed values dirichlet_vals [n_rhs, >= n] (None:
        homogeneous); returns the CsrOperator over the object's arrays"""
        g = dirichlet_vals
        if g is not None:
            g = g[None, :] if g.dim() == 1 else g
            nc, ldg = MatrixFreeSystem._cols(g)
            if nc != self.n_rhs:
                raise L3KError("Number of RHSs must be equal to the number of prescribed values")  # bcs/DirichletBC.hpp:86
        check(capi.load().l3k_asm_end(self._h, _ptr(g), 0 if g is None else ldg))
        if self.halo is not None:
            return DistributedCsrOperator(_AssembledOperator(self, self._info().csr), self.halo, _handle=self._dist_info().dist)
        return _AssembledOperator(self, self._info().csr)

    def _dist_info(self):
        i = capi.AsmDistInfo()
        check(capi.load().l3k_asm_dist_info_get(self._h, C.byref(i)))
        return i

    @property
    def cond_info(self):
        """condensed, n_primary_nodes and n_internal_nodes per element, n_elems, store_bytes and n_failed (the elements whose
        internal block failed the pivot test of the last end()); all 0 on a system without condensation"""
        import types
        i = capi.AsmCondInfo()
        check(capi.load().l3k_asm_cond_info_get(self._h, C.byref(i)))
        return types.SimpleNamespace(**{name: getattr(i, name) for name, _ in capi.AsmCondInfo._fields_})

    def recover(self, x):
        """recoverSolution: the internal dofs of x [n] or [n_rhs, >= n] (float64, on the device, contiguous rows) from its solved
        primary dofs, in place; a closed condensed system.  With a halo (collective): x holds the owned dofs, [n_owned] or
        [n_rhs, n_owned]; the ghost dofs are imported, and the owned dofs with the internal ones filled come back as a new tensor"""
        if self.halo is not None:
            import torch
            xo = x[None, :] if x.dim() == 1 else x
            if xo.shape != (self.n_rhs, self.n_owned):
                raise L3KError(f"AssembledSystem.recover: x is over the {self.n_owned} owned dofs of {self.n_rhs} right-hand sides")
            X = torch.zeros((self.n_rhs, max(self.n, 1)), dtype=torch.float64, device=x.device)
            X[:, :self.n_owned] = xo
            check(capi.load().l3k_asm_recover(self._h, _ptr(X), X.shape[1]))
            out = X[:, :self.n_owned].contiguous()
            return out[0] if x.dim() == 1 else out
        X = x[None, :] if x.dim() == 1 else x
        nc, ldx = MatrixFreeSystem._cols(X)
        if nc != self.n_rhs:
            raise L3KError(f"AssembledSystem.recover: x has {nc} columns, the system n_rhs = {self.n_rhs}")
        check(capi.load().l3k_asm_recover(self._h, _ptr(X), ldx))
        return x

    def schur_updates(self, first=0, count=None):
        """(W, w): K_bi K_ii^-1 K_ib [count, Nb, Nb] and K_bi K_ii^-1 F_i [count, n_rhs, Nb] of the elements [first, first + count),
        Nb = n_primary_nodes * fields, from the store of a closed condensed system"""
        import torch
        ci = self.cond_info
        count = ci.n_elems - first if count is None else count
        nb = ci.n_primary_nodes * self.n_fields
        dev = torch.device("cuda", self.ctx.device)
        W = torch.empty((max(count, 0), nb, nb), dtype=torch.float64, device=dev)
        w = torch.empty((max(count, 0), self.n_rhs, nb), dtype=torch.float64, device=dev)
        check(capi.load().l3k_asm_schur_updates(self._h, first, count, _ptr(W), _ptr(w)))
        return W, w


class MultiTermSystem:
    """algsys::MatrixFreeSystem as the sum of its assembleProblem calls (l3k_mfs_*; algsys/MatrixFreeSystem.hpp:24-89): any number
    of MatrixFreeSystem and BoundaryTerm terms over the rows of `mesh`, each on `mesh` itself or on a DeviceMesh over the same
    nodes that holds some of the elements (DeviceMesh(ctx, partition.element_subset(part, elems), dofs_per_node, the same mask);
    ElevatedMesh.subset(domain_ids) for the domains of a mesh file).  add(term) ..., finalize(), then the calls of a
    MatrixFreeSystem with its names and arguments: code that drives the split-phase pieces takes either.  solve.pcg and
    solve.ChebyshevPreconditioner take the object as they take a MatrixFreeSystem.  The terms are kept alive here."""

    def __init__(self, mesh, n_rhs=1):
        self.mesh, self.ctx, self.n_rhs = mesh, mesh.ctx, n_rhs
        self.terms = []
        self._h = C.c_void_p()
        check(capi.load().l3k_mfs_create(mesh._h, n_rhs, C.byref(self._h)))

    def __del__(self):
        if getattr(self, "_h", None) and capi is not None:
            capi.load().l3k_mfs_destroy(self._h)
            self._h = None

    def add(self, term):
        """assembleProblem(kernel, domain ids / boundary ids): a MatrixFreeSystem (without attached boundary terms) or a
        BoundaryTerm joins the sum; refused after finalize()"""
        if isinstance(term, BoundaryTerm):
            check(capi.load().l3k_mfs_add_boundary(self._h, term._h))
        elif isinstance(term, MatrixFreeSystem):
            check(capi.load().l3k_mfs_add_domain(self._h, term._h))
        else:
            raise L3KError("MultiTermSystem.add takes a MatrixFreeSystem or a BoundaryTerm")
        self.terms.append(term)
        return self

    def finalize(self):
        """The coverage mask of the terms and the number of active rows (l3k_mfs_finalize); opens apply, diag_rhs and the solvers"""
        check(capi.load().l3k_mfs_finalize(self._h))
        return self

    @property
    def info(self):
        """n_terms, n_rows (owned dofs), n_active_rows, n_dirichlet_rows, n_rhs, finalized"""
        import types
        i = capi.MfsInfo()
        check(capi.load().l3k_mfs_info_get(self._h, C.byref(i)))
        return types.SimpleNamespace(**{name: getattr(i, name) for name, _ in capi.MfsInfo._fields_})

    def active(self):
        """uint8 device tensor over the local dofs: 1 where a term has an entry"""
        import torch
        out = torch.empty(self.mesh.n_owned_dofs + self.mesh.n_ghost_dofs, dtype=torch.uint8, device=torch.device("cuda", self.ctx.device))
        check(capi.load().l3k_mfs_active(self._h, _ptr(out)))
        return out

    _cols = staticmethod(MatrixFreeSystem._cols)

    def apply(self, X, Y, alpha=1.0, beta=0.0):
        nc, ldx = self._cols(X)
        nc2, ldy = self._cols(Y)
        if nc != nc2:
            raise L3KError("X and Y must have the same number of columns")  # MatrixFreeSystem.hpp:1035
        check(capi.load().l3k_mfs_apply(self._h, _ptr(X), ldx, _ptr(Y), ldy, nc, alpha, beta))
        return Y

    def apply_energy(self, X, Y, S):
        """Y <- A X (one column) and S[1] <- <X, A X> (l3k_mfs_apply_energy): S is the PCG's device scalar block (8 doubles)"""
        check(capi.load().l3k_mfs_apply_energy(self._h, _ptr(X), _ptr(Y), _ptr(S)))
        return Y

    def scale(self, Y, beta):
        nc, ldy = self._cols(Y)
        check(capi.load().l3k_mfs_scale(self._h, _ptr(Y), ldy, nc, beta))

    def apply_elems(self, which, X, XG, Y, YG, alpha, beta):
        nc, ldx = self._cols(X)
        _, ldy = self._cols(Y)
        ldxg = self._cols(XG)[1] if XG is not None else 0
        ldyg = self._cols(YG)[1] if YG is not None else 0
        check(capi.load().l3k_mfs_apply_elems(self._h, which, _ptr(X), ldx, _ptr(XG), ldxg, _ptr(Y), ldy, _ptr(YG), ldyg,
                                              nc, alpha, beta))

    def dirichlet_rows(self, X, Y, alpha):
        nc, ldx = self._cols(X)
        _, ldy = self._cols(Y)
        check(capi.load().l3k_mfs_dirichlet_rows(self._h, _ptr(X), ldx, _ptr(Y), ldy, nc, alpha))

    def diag_rhs(self, dirichlet_vals=None, which=2, diag=None, rhs=None, diag_ghost=None, rhs_ghost=None, finalize=True):
        """computeDiagAndRhs summed over the terms: the arguments and results of MatrixFreeSystem.diag_rhs"""
        import torch
        n_owned, n_ghost = self.mesh.n_owned_dofs, self.mesh.n_ghost_dofs
        dev = torch.device("cuda", self.ctx.device)
        if diag is None:
            diag = torch.zeros(n_owned, dtype=torch.float64, device=dev)
        if rhs is None:
            rhs = torch.zeros((self.n_rhs, n_owned), dtype=torch.float64, device=dev)
        if n_ghost and diag_ghost is None:
            diag_ghost = torch.zeros(n_ghost, dtype=torch.float64, device=dev)
            rhs_ghost = torch.zeros((self.n_rhs, n_ghost), dtype=torch.float64, device=dev)
        g = dirichlet_vals
        check(capi.load().l3k_mfs_diag_rhs(self._h, which, _ptr(g), 0 if g is None else g.shape[1], _ptr(diag), _ptr(rhs),
                                           rhs.shape[1], _ptr(diag_ghost), _ptr(rhs_ghost), max(n_ghost, 1), int(finalize)))
        return diag, rhs

    def jacobi_inverse(self, diag, damping=1.0, threshold=0.0):
        """sign(d) damping / max(|d|, threshold) on the active owned rows, 0 on the rows no term covers (l3k_mfs_jacobi_inverse): the
        PCG leaves x as it is there"""
        import torch
        if diag.numel() != self.mesh.n_owned_dofs or not diag.is_contiguous():
            raise L3KError("diag must be a contiguous tensor over the owned dofs")
        out = torch.empty_like(diag)
        check(capi.load().l3k_mfs_jacobi_inverse(self._h, _ptr(diag), float(damping), float(threshold), _ptr(out)))
        return out

    def new_ghost_buffer(self, ncols, like):
        import torch
        return torch.zeros((ncols, max(self.mesh.n_ghost_dofs, 1)), dtype=torch.float64, device=like.device)
