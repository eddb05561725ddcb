"""CPU restatement of the p-multigrid preconditioner (include/l3k.h: l3k_pmg_*) in numpy / torch, dense: the 1-D transfer table, the
global prolongation of a level pair with the ownership rule of the device (owner = the lowest fine element that contains the node),
its masked form, the symmetric V-cycle with solve.chebyshev_reference as the smoother of every level, and a PCG on top.  The level
operators come from the oracle's mesh-level apply, as dense matrices (column by column) where a test wants the matrix of M^-1 and
as callables otherwise."""
import numpy as np
import torch

import oracle_lib as O
from helpers import oracle_mesh
from l3ster_amd import solve, system


def gll_nodes(n):
    """the n Gauss-Lobatto-Legendre nodes from numpy's Legendre series: +-1 and the roots of P_{n-1}' (independent of the library)"""
    inner = np.polynomial.legendre.Legendre.basis(n - 1).deriv().roots() if n > 2 else np.zeros(0)
    x = np.concatenate([[-1.0], np.sort(inner.real), [1.0]])
    return 0.5 * (x - x[::-1])  # (symmetrised)


def interp_1d(p_from, p_to):
    """T[i][j] = l_j(x_i): the order-p_from GLL Lagrange basis at the GLL nodes of order p_to, product form"""
    xf, xt = gll_nodes(p_from + 1), gll_nodes(p_to + 1)
    T = np.ones((p_to + 1, p_from + 1))
    for j in range(p_from + 1):
        for k in range(p_from + 1):
            if k != j:
                T[:, j] *= (xt - xf[k]) / (xf[j] - xf[k])
    return T


def owners(fine_part):
    """owner[node] = the lowest element that contains the node"""
    own = np.full(fine_part.n_owned_nodes, np.iinfo(np.int64).max, dtype=np.int64)
    for e in range(fine_part.n_elems - 1, -1, -1):
        own[fine_part.elem_nodes[e].astype(np.int64)] = e
    return own


def node_prolongation(fine_part, coarse_part, elem_map=None):
    """The node-level P (fine nodes x coarse nodes, dense): row `node` holds the coarse basis functions of the OWNING element at the
    node.  Every component of a node moves alike: the dof-level matrix is kron(P_nodes, I_U)."""
    T = interp_1d(coarse_part.order, fine_part.order)
    Pe = T
    for _ in range(fine_part.dim - 1):
        Pe = np.kron(T, Pe)  # local index = ix + n iy + n^2 iz: the slowest direction leads
    own = owners(fine_part)
    Pn = np.zeros((fine_part.n_owned_nodes, coarse_part.n_owned_nodes))
    for e in range(fine_part.n_elems):
        ec = e if elem_map is None else int(elem_map[e])
        fn, cn = fine_part.elem_nodes[e].astype(np.int64), coarse_part.elem_nodes[ec].astype(np.int64)
        mine = own[fn] == e
        Pn[np.ix_(fn[mine], cn)] = Pe[mine]
    return Pn


def prolongation(fine_part, coarse_part, U, elem_map=None, mask_f=None, mask_c=None):
    """The global P over the dofs (dense).  mask_f / mask_c (byte masks over the dofs): rows / columns zeroed."""
    P = np.kron(node_prolongation(fine_part, coarse_part, elem_map), np.eye(U))
    if mask_f is not None:
        P[np.asarray(mask_f, bool)] = 0.0
    if mask_c is not None:
        P[:, np.asarray(mask_c, bool)] = 0.0
    return P


class Level:
    """One level: apply(v, out) (torch), minv (torch), and the smoother's numbers"""

    def __init__(self, apply, minv, lambda_max, cond_est, degree, mask=None, part=None):
        self.apply, self.minv, self.lambda_max, self.cond_est, self.degree = apply, minv, lambda_max, cond_est, degree
        self.mask, self.part = mask, part

    def smooth(self, r):
        return solve.chebyshev_reference(self.apply, self.minv, r, self.lambda_max, self.cond_est, self.degree)


def vcycle(levels, Ps, r, l=0):
    """z = cycle(l, r) of include/l3k.h; Ps[l]: the masked P between the levels l (fine) and l + 1, a torch matrix"""
    L = levels[l]
    z = L.smooth(r)
    if l + 1 == len(levels):
        return z
    live, zero, az = L.minv != 0, torch.zeros_like(r), torch.empty_like(r)
    L.apply(z, az)
    d = torch.where(live, r - az, zero)
    e = Ps[l] @ vcycle(levels, Ps, Ps[l].T @ d, l + 1)
    z = z + torch.where(live, e, zero)
    L.apply(z, az)
    d = torch.where(live, r - az, zero)
    return z + L.smooth(d)


def pcg(levels, Ps, b, x, tol, **kw):
    """Hestenes-Stiefel PCG with the V-cycle as the preconditioner (solve.cg: the loop of l3k_pcg_solve_cheb)"""
    return solve.cg(levels[0].apply, b, x, tol=tol, precond=lambda r: vcycle(levels, Ps, r), **kw)


# --------------------------------------------------------------------------------------------------------- the test problems
def diffusion_level(ne, p, dim=3, dense=False, perturb=0.1, U=None):
    """Diffusion3D (U = 4) or Diffusion2D (U = 3) on a perturbed ne^dim mesh of order p, T fixed on all sides, from the oracle:
    dict(part, mask, apply, minv, diag, rhs[, A])"""
    if dim == 3:
        U = U or 4
        part = system.CubePartition(ne, p, perturb=perturb)
        kid, kpar = 0, [1.0, 0.0]
    else:
        U = U or 3
        part = system.SquarePartition(ne, p, perturb=perturb)
        kid, kpar = 2, None
    mask = part.dirichlet_mask(U)
    xyz = part.node_coords()
    g = np.zeros((part.n_local_nodes, U))
    g[:, 0] = xyz[:, 0]  # T = x on the boundary
    g = (g.reshape(-1) * mask)[None, :]
    om = O.MeshView(dim, p, p + 1, part.elem_nodes, part.elem_verts, part.n_local_nodes, U, np.arange(U), mask, None)
    diag, rhs = O.mf_diag_rhs(om, kid, 1, np.asfortranarray(g.T), kparams=kpar)
    out = dict(part=part, mask=mask, diag=diag, rhs=rhs[:, 0].copy(), minv=solve.jacobi_inverse(torch.as_tensor(diag)), U=U, g=g,
               kernel_id=kid, kparams=kpar)
    if dense:
        n = len(diag)
        A = np.ascontiguousarray(O.mf_apply(om, kid, np.eye(n), kparams=kpar))
        assert np.abs(A - A.T).max() <= 1e-12 * np.abs(A).max()
        At = torch.as_tensor(0.5 * (A + A.T))
        out.update(A=At.numpy(), apply=lambda v, o: o.copy_(At @ v))
    else:
        out["apply"] = lambda v, o: o.copy_(torch.as_tensor(O.mf_apply(om, kid, v.numpy().reshape(-1, 1), kparams=kpar)[:, 0]))
    return out


def lambda_max_dense(A, minv):
    """the largest eigenvalue of D^-1 A"""
    d = np.sqrt(np.asarray(minv))
    return float(np.linalg.eigvalsh(d[:, None] * A * d[None, :])[-1])


def power_lambda(apply, minv, iters=30):
    """the power method on D^-1 A from solve.power_start_vector (a deterministic stand-in where no dense matrix is formed)"""
    x = solve.power_start_vector(minv.numel())
    y, lam = torch.empty_like(x), 0.0
    for _ in range(iters):
        x = x / x.norm()
        apply(x, y)
        y = minv * y
        lam = float(torch.dot(x, y))
        x = y.clone()
    return lam


SMOOTH = dict(degree=3, cond_est=20.0)  # every level but the last
COARSE = dict(degree=8, cond_est=400.0)  # the last level: the coarse solve, a fixed polynomial


def hierarchy(ne, orders, dim=3, dense=False, perturb=0.1):
    """(levels, Ps, data): the restated hierarchy of one mesh at `orders` (finest first) with the smoothers SMOOTH / COARSE and
    lambda_max = 1.1 x the extreme eigenvalue (dense) or the power method's estimate"""
    data = [diffusion_level(ne, p, dim, dense, perturb) for p in orders]
    levels = []
    for i, d in enumerate(data):
        lam = 1.1 * (lambda_max_dense(d["A"], d["minv"].numpy()) if dense else power_lambda(d["apply"], d["minv"]))
        o = COARSE if i + 1 == len(data) else SMOOTH
        levels.append(Level(d["apply"], d["minv"], lam, o["cond_est"], o["degree"], d["mask"], d["part"]))
    Ps, maps = [], []
    for f, c in zip(data[:-1], data[1:]):
        m = system.match_elements(f["part"], c["part"])
        maps.append(m)
        Ps.append(torch.as_tensor(prolongation(f["part"], c["part"], f["U"], m, f["mask"], c["mask"])))
    return levels, Ps, data, maps
