"""A dense numpy restatement of the assembled system on a partitioned mesh in the SUB-ASSEMBLED form: every rank r
keeps the matrix A_r of its own elements and sides over its local dofs [owned | ghost], the global matrix is

    A = sum_r R_r^T A_r R_r          (R_r: the rows of the whole mesh -> the local dofs of rank r)

and the algebraic Dirichlet conditions are applied rank by rank with an OWNER RULE: a flagged owned row becomes the identity row
with rhs = g, a flagged ghost row an all-zero row with rhs = 0, an unflagged row gives rhs_i -= a_ij g_j over its flagged columns,
which are then zeroed; the ghost rows of rhs are export-added into their owners' rows afterwards.  Summed over the ranks this is
DirichletBCAlgebraic::apply (bcs/DirichletBC.hpp:82-150) on the global matrix -- tests/test_asm_dist_cpu.py shows it against
tests/csr_ref.py's step on the whole mesh -- and these functions are the reference of tests/test_gpu_asm_dist.py.

Element matrices: tests/quad_asm_ref.py on quads (Diffusion2D, Adiabatic2D), the oracle's on hexes.  Everything is float64 and dense;
the meshes are small."""
import numpy as np

import oracle_lib as O
import quad_asm_ref as QA
from l3ster_amd import partition, system


# ------------------------------------------------------------------------------------------------------------- the cases
class Case:
    """A whole mesh and its parts.  whole / parts: the host meshes; idx[r][local node] = the node's row in the whole mesh; U dofs
    per node; mask: the whole mesh's Dirichlet flags, bool [nodes * U]; sides / part_sides[r]: (face_elem, face_side) of the boundary
    term on the whole mesh / on rank r's elements; elem_of[r][local element] = its index in the whole mesh."""

    def local_mask(self, r):
        return self.mask.reshape(-1, self.U)[self.idx[r]].reshape(-1)

    def local_dofs(self, r):
        """the whole-mesh dof of every local dof of rank r"""
        return (self.idx[r][:, None] * self.U + np.arange(self.U)[None, :]).reshape(-1)

    def n_owned(self, r):
        return self.parts[r].n_owned_nodes * self.U

    def gather(self, per_rank):
        """whole-mesh [ncols, n] array from the ranks' (ncols, n_owned) arrays; every row must arrive exactly once"""
        n = self.whole.n_local_nodes * self.U
        ncols = np.atleast_2d(np.asarray(per_rank[0])).shape[0]
        out, seen = np.zeros((ncols, n)), np.zeros(n, dtype=np.int64)
        for r in range(len(self.parts)):
            rows = self.local_dofs(r)[:self.n_owned(r)]
            out[:, rows] = np.atleast_2d(np.asarray(per_rank[r]))[:, :rows.size]
            seen[rows] += 1
        assert np.array_equal(seen, np.ones_like(seen))
        return out

    def scatter(self, whole_vec, r):
        """rank r's owned rows of a whole-mesh [ncols, n] array"""
        return np.ascontiguousarray(np.atleast_2d(whole_vec)[:, self.local_dofs(r)[:self.n_owned(r)]])


def quad_case(ne=(5, 4), p=3, world=4, perturb=0.1, device=None):
    """SquarePartition(ne, p) cut by rcb_partition: Diffusion2D (U = 3), T flagged on the sides x = 0 and x = 1, Adiabatic2D on the
    sides y = 0 and y = 1"""
    q = Case()
    q.dim, q.p, q.U, q.world, q.kpar = 2, p, 3, world, None
    q.whole = system.SquarePartition(ne, p, perturb=perturb)
    pv = partition.rcb_partition(q.whole.elem_verts, world)
    q.parts = [partition.PartitionedMesh(q.whole.elem_nodes, q.whole.elem_verts, None, pv, r, world, p, device=device) for r in range(world)]
    q.idx = [m.node_grid_id[:m.n_local_nodes].astype(np.int64) for m in q.parts]  # (a PartitionedMesh's ids: the whole mesh's rows)
    q.elem_of = [np.asarray(m.elem_global, dtype=np.int64) for m in q.parts]
    q.mask = q.whole.dirichlet_mask(q.U, sides=(2, 3)).astype(bool)
    q.sides = q.whole.boundary_sides([0, 1])
    q.part_sides = [partition.local_sides(m, *q.sides) for m in q.parts]
    return q


def cube_case(ne=(4, 2, 2), p=2, parts=(2, 1, 1), perturb=0.1):
    """CubePartition(ne, p, parts): Diffusion3D with the parameters kpar (U = 4), T flagged on the whole boundary, Adiabatic3D on the side of index 1"""
    q = Case()
    q.dim, q.p, q.U, q.world, q.kpar = 3, p, 4, int(np.prod(parts)), [0.7, 1.3]
    q.whole = system.CubePartition(ne, p, perturb=perturb)
    q.parts = [system.CubePartition(ne, p, parts, r, perturb=perturb) for r in range(q.world)]
    at = np.full(int(q.whole.node_grid_id.max()) + 1, -1, dtype=np.int64)
    at[q.whole.node_grid_id] = np.arange(q.whole.n_local_nodes)
    q.idx = [at[m.node_grid_id] for m in q.parts]
    where = {q.whole.elem_verts[e].tobytes(): e for e in range(q.whole.n_elems)}  # (the perturbation does not depend on the parts)
    q.elem_of = [np.array([where[m.elem_verts[e].tobytes()] for e in range(m.n_elems)], dtype=np.int64) for m in q.parts]
    q.mask = q.whole.dirichlet_mask(q.U).astype(bool)
    q.sides = q.whole.boundary_sides([1])
    q.part_sides = [m.boundary_sides([1]) for m in q.parts]
    return q


# --------------------------------------------------------------------------------------------------- local dense systems
def elem_dofs(part, e, U):
    return (part.elem_nodes[e].astype(np.int64)[:, None] * U + np.arange(U)[None, :]).reshape(-1)


def element_rhs(q, e_whole):
    """a right-hand side of element e of the WHOLE mesh, [Nd]: the built-in kernels have none, so the tests bring their own --
    drawn from the element's index in the whole mesh, the same on whichever rank holds the element"""
    Nd = (q.p + 1) ** q.dim * q.U
    return np.random.default_rng(1000 + int(e_whole)).uniform(-1, 1, Nd)


def local_system(q, part, sides, elem_of, with_rhs=True):
    """(A [n, n], rhs [n], pattern bool [n, n]) of one mesh (the whole one or a part) over its local dofs: the domain kernel on every
    element, the boundary kernel on the listed sides, summed through elem_nodes; pattern: the full sparsity graph (the dofs of every
    element coupled with each other)"""
    n = part.n_local_nodes * q.U
    A, rhs, pattern = np.zeros((n, n)), np.zeros(n), np.zeros((n, n), dtype=bool)
    nq = system.n_qps1d(q.p, 1, 0)  # (the default assembly options of the device terms)
    dom = QA.diffusion2d() if q.dim == 2 else None
    bnd = QA.adiabatic2d() if q.dim == 2 else None
    for e in range(part.n_elems):
        d = elem_dofs(part, e, q.U)
        if q.dim == 2:
            K = QA.element_system(dom, q.p, nq, part.elem_verts[e])[0]
        else:
            K = O.assemble_local(O.KERNEL_DIFFUSION3D, q.p, nq, 1, part.elem_verts[e], None, q.kpar)[0]
        A[np.ix_(d, d)] += K
        pattern[np.ix_(d, d)] = True
        if with_rhs:
            rhs[d] += element_rhs(q, elem_of[e])
    for e, s in zip(*sides):
        d = elem_dofs(part, e, q.U)
        if q.dim == 2:
            A[np.ix_(d, d)] += QA.side_system(bnd, int(s), q.p, nq, part.elem_verts[e])[0]
        else:
            A[np.ix_(d, d)] += O.assemble_local_side(int(s), O.KERNEL_ADIABATIC3D, q.p, nq, 1, part.elem_verts[e])[0]
    return A, rhs, pattern


def csr_of(A, pattern):
    """(row_ptr int64, col_ind int32, values) of a dense matrix on a pattern (columns ascending; pattern entries that are 0 stay)"""
    rows, cols = np.nonzero(pattern)
    row_ptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=A.shape[0]))]).astype(np.int64)
    return row_ptr, cols.astype(np.int32), A[rows, cols]


def dense_of(row_ptr, col_ind, values, n=None):
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    n = row_ptr.size - 1 if n is None else n
    A = np.zeros((row_ptr.size - 1, n))
    A[np.repeat(np.arange(row_ptr.size - 1), np.diff(row_ptr)), np.asarray(col_ind, dtype=np.int64)] = values
    return A


# ------------------------------------------------------------------------------------------------------ the three pieces
def row_classes(row_ptr, col_ind, n_owned):
    """(interior, border, ghost): ascending int32 row lists.  Interior: an owned row with every column < n_owned (an empty owned row
    is interior); border: an owned row with at least one ghost column; ghost: a row >= n_owned"""
    row_ptr, col_ind = np.asarray(row_ptr, dtype=np.int64), np.asarray(col_ind, dtype=np.int64)
    n = row_ptr.size - 1
    has_ghost = np.zeros(n, dtype=bool)
    rows = np.repeat(np.arange(n), np.diff(row_ptr))
    has_ghost[rows[col_ind >= n_owned]] = True
    owned = np.arange(n) < n_owned
    return tuple(np.flatnonzero(sel).astype(np.int32) for sel in (owned & ~has_ghost, owned & has_ghost, ~owned))


def dirichlet_owner_rule(A, rhs, mask, g, n_owned):
    """The rank-local Dirichlet step on a dense local matrix: mask bool [n], g [ncols, n] over the LOCAL dofs, rhs [ncols, n].
    Returns (A', rhs')."""
    A, rhs, g = A.copy(), np.atleast_2d(rhs).astype(np.float64).copy(), np.atleast_2d(g)
    mask = np.asarray(mask).astype(bool)
    free = ~mask
    rhs[:, free] -= (A[np.ix_(free, mask)] @ g[:, mask].T).T
    A[:, mask] = 0.0
    A[mask, :] = 0.0
    owned_flagged = np.flatnonzero(mask[:n_owned])
    A[owned_flagged, owned_flagged] = 1.0
    rhs[:, mask] = 0.0
    rhs[:, owned_flagged] = g[:, owned_flagged]
    return A, rhs


def sum_of_ranks(q, mats):
    """sum_r R_r^T A_r R_r, dense over the whole mesh's dofs"""
    n = q.whole.n_local_nodes * q.U
    A = np.zeros((n, n))
    for r, Ar in enumerate(mats):
        d = q.local_dofs(r)
        A[np.ix_(d, d)] += Ar  # (the local dofs of a rank are distinct rows of the whole mesh)
    return A


def export_add(q, vecs):
    """the ranks' local [ncols, n_local] vectors summed into the whole mesh's rows: what the export leaves in the owners' rows"""
    n = q.whole.n_local_nodes * q.U
    out = np.zeros((np.atleast_2d(vecs[0]).shape[0], n))
    for r, v in enumerate(vecs):
        out[:, q.local_dofs(r)] += np.atleast_2d(v)
    return out


def prescribed_values(q):
    """T = x at the flagged dofs of the whole mesh, 0 elsewhere, [1, n]"""
    x = q.whole.node_coords()[:, 0]
    g = np.zeros((q.whole.n_local_nodes, q.U))
    g[:, 0] = x
    return np.where(q.mask, g.reshape(-1), 0.0)[None, :]
