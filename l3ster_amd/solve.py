"""Jacobi-preconditioned conjugate gradients around the matrix-free operator.

The reference delegates the iteration to Trilinos Belos ("Block CG", solve/BelosSolvers.hpp:116-122) with its own native
Jacobi preconditioner (solve/NativePreconditioners.hpp:36-96); Belos is a third-party dependency that is not under
/root/reference, so the CG arithmetic is restated from the published algorithm (Hestenes-Stiefel PCG) and parity is
pinned end to end (solution / error thresholds), not iterate by iterate.  Vector updates and dot
products are torch ops (plumbing); the operator apply -- the hot path -- is the HIP kernel behind `apply`.
"""
import ctypes as C
import inspect

import torch
import torch.distributed as dist


def jacobi_inverse(diag, damping=1.0, threshold=0.0):
    """NativeJacobiImpl::init (solve/NativePreconditioners.hpp:75-96): sign(d)*damping / max(|d|, threshold)."""
    sign = torch.where(diag < 0, -torch.ones_like(diag), torch.ones_like(diag))
    return sign * damping / torch.clamp(diag.abs(), min=threshold)


class IterSolveResult:
    def __init__(self, tol, num_iters, converged):
        self.tol, self.num_iters, self.converged = tol, num_iters, converged

    def __repr__(self):
        return f"IterSolveResult(tol={self.tol:.3e}, num_iters={self.num_iters}, converged={self.converged})"


def cg(apply, b, x, minv=None, tol=1e-6, max_iters=10_000, residual_scaling="none", group=None, throw_on_fail=True,
       precond=None):
    """Solves A x = b for one column (1-D tensors over the OWNED rows of this rank); x holds the initial guess and the
    result.  apply(p, out) computes out <- A p.  Options mirror IterSolverOpts (solve/SolverInterface.hpp:26-37):
    residual_scaling in {"none", "initial", "rhs"}.  `group`: torch.distributed group for the dot products of a
    partitioned vector (None = single rank).  `precond`: a callable z = precond(r) in place of the diagonal minv (a
    symmetric positive definite M^-1, e.g. chebyshev_reference behind a lambda)."""
    if precond is not None and minv is not None:
        raise ValueError("give minv or precond, not both")
    prec = precond if precond is not None else (lambda r: r * minv) if minv is not None else None

    def dot(u, v):
        s = torch.dot(u, v)
        if group is not None or (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1):
            dist.all_reduce(s, op=dist.ReduceOp.SUM, group=group)
        return s.item()

    r = torch.empty_like(b)
    apply(x, r)
    r = b - r
    rr0 = dot(r, r) ** 0.5
    scale = {"none": 1.0, "initial": rr0 if rr0 > 0 else 1.0, "rhs": max(dot(b, b) ** 0.5, 1e-300)}[residual_scaling]
    z = prec(r) if prec is not None else r.clone()
    p = z.clone()
    rz = dot(r, z)
    ap = torch.empty_like(b)
    res = rr0 / scale
    it = 0
    while res > tol and it < max_iters:
        apply(p, ap)
        alpha = rz / dot(p, ap)
        x.add_(p, alpha=alpha)
        r.sub_(ap, alpha=alpha)
        res = dot(r, r) ** 0.5 / scale
        it += 1
        if res <= tol:
            break
        z = prec(r) if prec is not None else r
        rz_new = dot(r, z)
        p.mul_(rz_new / rz).add_(z)
        rz = rz_new
    converged = res <= tol
    if throw_on_fail and not converged:
        raise RuntimeError("Solver failed to converge")  # solve/BelosSolvers.hpp:103
    return IterSolveResult(res, it, converged)


def chebyshev_coefficients(lambda_max, lambda_min, degree):
    """c0 and the (a_k, b_k) of the recurrence below, in the arithmetic of the library's host routine
    (csrc/host/chebyshev.hpp): the same doubles."""
    theta, delta = (lambda_max + lambda_min) / 2.0, (lambda_max - lambda_min) / 2.0
    sigma = theta / delta
    rho, steps = 1.0 / sigma, []
    for _ in range(1, degree):
        rho_new = 1.0 / (2.0 * sigma - rho)
        steps.append((rho_new * rho, 2.0 * rho_new / delta))
        rho = rho_new
    return 1.0 / theta, steps


def chebyshev_reference(apply, minv, r, lambda_max, cond_est, degree):
    """z = p(D^-1 A) D^-1 r in torch ops: the Chebyshev iteration with Jacobi scaling that Ifpack2ChebyshevPreconditioner
    (solve/Ifpack2Preconditioners.hpp:26-36,107-131) stands for, as l3k_cheb_apply runs it (include/l3k.h): lambda_min =
    lambda_max / cond_est, w = z = D^-1 r / theta, then degree - 1 steps w = a w + b D^-1 (r - A z), z += w.  Rows with
    minv == 0 are frozen: w = z = 0.  apply(v, out) computes out <- A v."""
    if degree < 1 or not cond_est > 1:
        raise ValueError("degree >= 1 and cond_est > 1")
    c0, steps = chebyshev_coefficients(lambda_max, lambda_max / cond_est, degree)
    live, zero = minv != 0, torch.zeros_like(r)
    w = torch.where(live, c0 * (minv * r), zero)
    z = w.clone()
    az = torch.empty_like(r)
    for a, b in steps:
        apply(z, az)
        w = torch.where(live, a * w + b * (minv * (r - az)), zero)
        z = torch.where(live, z + w, zero)
    return z


def power_start_vector(n, device="cpu"):
    """The start vector of the power method in l3k_cheb_create before its normalisation (include/l3k.h): lowbias32 of the
    row index mapped to [-1, 1), bit for bit (uint32 arithmetic carried in int64)."""
    m32 = 0xFFFFFFFF
    h = torch.arange(n, dtype=torch.int64, device=device) & m32
    h = h ^ (h >> 16)
    h = (h * 0x7FEB352D) & m32  # (int64 products wrap modulo 2^64: the low 32 bits are those of the uint32 product)
    h = h ^ (h >> 15)
    h = (h * 0x846CA68B) & m32
    h = h ^ (h >> 16)
    return h.to(torch.float64) * 2.0 ** -31 - 1.0


def _overlap(u, v, n):
    """Do the n doubles at u and at v share memory?"""
    return abs(u.data_ptr() - v.data_ptr()) < 8 * n


def _entry(system, name):
    """(the entry point `name` for this kind of system, its number of rows): l3k_<name> for a MatrixFreeSystem,
    l3k_csr_<name> for a system.CsrOperator, l3k_mfs_<name> for a system.MultiTermSystem -- the same loops inside the library on
    each operator"""
    from . import capi
    from .system import CsrOperator, MultiTermSystem
    if isinstance(system, CsrOperator):
        return getattr(capi.load(), "l3k_csr_" + name), system.n
    if isinstance(system, MultiTermSystem):
        if name == "pcg_solve_pmg":
            raise capi.L3KError("p-multigrid is not provided for a MultiTermSystem")
        return getattr(capi.load(), "l3k_mfs_" + name), system.mesh.n_owned_dofs
    return getattr(capi.load(), "l3k_" + name), system.mesh.n_owned_dofs


class ChebyshevPreconditioner:
    """Handle of l3k_cheb_create / l3k_csr_cheb_create: the Chebyshev-Jacobi preconditioner of a single-rank MatrixFreeSystem
    or of a system.CsrOperator (options of Ifpack2ChebyshevOpts; its diag_threshold is jacobi_inverse's threshold).  `minv` (1-D device tensor
    over the owned dofs) and the system are kept alive here.  lambda_max=None: estimated by max_power_iters steps of the
    power method and multiplied by boost_factor."""

    def __init__(self, system, minv, degree=1, cond_est=30., max_power_iters=10, boost_factor=1.1, lambda_max=None):
        from . import capi
        self.system, self.minv = system, minv
        create, self.n = _entry(system, "cheb_create")
        if minv is None or minv.numel() != self.n or not minv.is_contiguous():
            raise capi.L3KError("minv must be a contiguous tensor over the owned dofs of the system")
        opts = capi.ChebOpts(int(degree), float(cond_est), int(max_power_iters), float(boost_factor),
                             0.0 if lambda_max is None else float(lambda_max))
        self._h = C.c_void_p()
        capi.check(create(system._h, C.c_void_p(minv.data_ptr()), C.byref(opts), C.byref(self._h)))

    @property
    def info(self):
        """lambda_max, lambda_min, lambda_est, degree, power_iters, applies_per_call (l3k_cheb_info)"""
        import types
        from . import capi
        i = capi.ChebInfo()
        capi.check(capi.load().l3k_cheb_info_get(self._h, C.byref(i)))
        return types.SimpleNamespace(**{name: getattr(i, name) for name, _ in capi.ChebInfo._fields_})

    def apply(self, r, z):
        """z <- p(D^-1 A) D^-1 r (l3k_cheb_apply); r, z: distinct 1-D device tensors over the owned dofs.  z goes through
        l3k_mf_apply, which refuses a vector that is not aligned as the system's kernel needs it."""
        from . import capi
        n = self.n
        if r.numel() != n or z.numel() != n or not (r.is_contiguous() and z.is_contiguous()):
            raise capi.L3KError("r and z must be contiguous tensors over the owned dofs of the system")
        if _overlap(r, z, n):  # (the first kernel writes z before the steps read r: the result would be silently wrong)
            raise capi.L3KError("r and z must be distinct vectors that do not overlap")
        capi.check(capi.load().l3k_cheb_apply(self._h, C.c_void_p(r.data_ptr()), C.c_void_p(z.data_ptr())))
        return z

    def close(self):
        if getattr(self, "_h", None):
            from . import capi
            capi.load().l3k_cheb_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # (module globals may be gone at interpreter shutdown)
            pass


class PMultigrid:
    """Handle of l3k_pmg_create: the p-multigrid preconditioner of a single-rank MatrixFreeSystem (include/l3k.h).  `levels`, finest
    first: (MatrixFreeSystem, ChebyshevPreconditioner created on it, elem_map or None) -- the same elements at strictly decreasing
    orders; elem_map (int64, host or device; system.match_elements makes it) names the element of this level for each element of
    the level before and is ignored on the first level.  The systems, smoothers and maps are kept alive here."""

    def __init__(self, levels):
        from . import capi
        levels = [tuple(l) + (None,) * (3 - len(l)) for l in levels]
        if len(levels) < 2:
            raise capi.L3KError(f"PMultigrid needs at least two levels, got {len(levels)}")
        self.levels = levels
        self.system = levels[0][0]
        dev = levels[0][1].minv.device
        self._maps = [None if m is None or i == 0 else torch.as_tensor(m, dtype=torch.int64).to(dev).contiguous()
                      for i, (_, _, m) in enumerate(levels)]
        arr = (capi.PmgLevel * len(levels))()
        for a, (sys_l, cheb, _), m in zip(arr, levels, self._maps):
            a.mf, a.smoother, a.d_elem_map = sys_l._h, cheb._h, None if m is None else m.data_ptr()
        self._h = C.c_void_p()
        capi.check(capi.load().l3k_pmg_create(self.system.mesh.ctx._h, len(levels), arr, C.byref(self._h)))

    def info(self):
        """n_levels and per level order, n_dofs, applies_per_cycle (l3k_pmg_info)"""
        import types
        from . import capi
        i = capi.PmgInfo()
        capi.check(capi.load().l3k_pmg_info_get(self._h, C.byref(i)))
        n = i.n_levels
        return types.SimpleNamespace(n_levels=n, order=list(i.order[:n]), n_dofs=list(i.n_dofs[:n]),
                                     applies_per_cycle=list(i.applies_per_cycle[:n]))

    def _vec(self, t, level, name):
        from . import capi
        n = self.levels[level][0].mesh.n_owned_dofs
        if t.numel() != n or not t.is_contiguous():
            raise capi.L3KError(f"{name} must be a contiguous tensor over the {n} owned dofs of level {level}")
        return C.c_void_p(t.data_ptr())

    def _level(self, coarse_level):
        from . import capi
        if not 1 <= coarse_level < len(self.levels):
            raise capi.L3KError(f"coarse_level {coarse_level} outside [1, {len(self.levels)})")

    def prolong(self, coarse_level, xc, xf, add=False):
        """xf <- P xc, or xf += P xc, between the levels coarse_level and coarse_level - 1 (l3k_pmg_prolong)"""
        from . import capi
        self._level(coarse_level)
        capi.check(capi.load().l3k_pmg_prolong(self._h, coarse_level, self._vec(xc, coarse_level, "xc"),
                                               self._vec(xf, coarse_level - 1, "xf"), int(bool(add))))
        return xf

    def restrict(self, coarse_level, rf, rc):
        """rc <- P^T rf (l3k_pmg_restrict)"""
        from . import capi
        self._level(coarse_level)
        capi.check(capi.load().l3k_pmg_restrict(self._h, coarse_level, self._vec(rf, coarse_level - 1, "rf"),
                                                self._vec(rc, coarse_level, "rc")))
        return rc

    def apply(self, r, z):
        """z <- M^-1 r, one symmetric V-cycle (l3k_pmg_apply); r, z: distinct vectors of level 0"""
        from . import capi
        pr, pz = self._vec(r, 0, "r"), self._vec(z, 0, "z")
        if _overlap(r, z, r.numel()):
            raise capi.L3KError("r and z must be distinct vectors that do not overlap")
        capi.check(capi.load().l3k_pmg_apply(self._h, pr, pz))
        return z

    def close(self):
        if getattr(self, "_h", None):
            from . import capi
            capi.load().l3k_pmg_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # (module globals may be gone at interpreter shutdown)
            pass


def _operator_mesh(op):
    """the DeviceMesh under a distributed operator (NativeDistributedOperator.mf, DistributedOperator.backend)"""
    mf = getattr(op, "mf", None) or op.backend
    return mf.mesh


class DistributedPMultigrid:
    """The p-multigrid preconditioner of a PARTITIONED system: the cycle of l3k_pmg_apply (include/l3k.h) run from here on the
    exported pieces, as pcg_distributed runs the Chebyshev iteration -- the hierarchy of a partitioned run lives above the C ABI.
    `levels`, finest first: (op, minv, smoother, elem_map) with
      op        a NativeDistributedOperator or DistributedOperator over this rank's owned rows of the level,
      minv      the level's inverse diagonal over its owned rows (rows with minv == 0 are frozen),
      smoother  a dict of ChebyshevPreconditioner's options (degree, cond_est, max_power_iters, boost_factor, lambda_max) or an
                object whose .info has lambda_max, lambda_min and degree; without lambda_max the distributed power method of
                pcg_distributed estimates it, through `reduce`,
      elem_map  the element of this level for each element of the level before (system.match_elements on the two parts of this
                rank; None = identity; ignored on the first level).
    `reduce(view)`: sums a small device tensor over the ranks in place (None: torch.distributed when initialised, else
    nothing); pcg_distributed hands over its own.  The smoothers are l3k_cheb_first / _step around op.apply, the residual is
    l3k_pmg_residual, the transfers are system.Transfer with the coarse level's import_ghosts before each prolongation and its
    export_add after each restriction; the last level is its smoother alone.  Per level pair a cycle adds one coarse import and
    one coarse export-add to the exchanges of the applies.  All vectors of all levels are allocated here."""

    def __init__(self, levels, reduce=None):
        from . import capi
        from .system import Transfer
        levels = [tuple(l) + (None,) * (4 - len(l)) for l in levels]
        if len(levels) < 2:
            raise capi.L3KError(f"DistributedPMultigrid needs at least two levels, got {len(levels)}")
        self.levels, self.op, self.minv, self._reduce, self._coeffs = levels, levels[0][0], levels[0][1], reduce, None
        self._ctx = _operator_mesh(self.op).ctx
        self._vecs, self.transfers = [], [None]
        for i, (op, minv, smoother, emap) in enumerate(levels):
            n = _operator_mesh(op).n_owned_dofs
            if minv is None or smoother is None or minv.numel() != n or not minv.is_contiguous():
                raise capi.L3KError(f"DistributedPMultigrid: level {i} needs minv, a contiguous tensor over its {n} owned dofs, "
                                    "and its smoother")
            if _operator_mesh(op).ctx is not self._ctx:
                raise capi.L3KError(f"DistributedPMultigrid: level {i} lives on another context")
            names = ("d", "e", "w", "az") if i == 0 else ("r", "z", "d", "e", "w", "az")
            self._vecs.append({k: torch.zeros(n, dtype=torch.float64, device=minv.device) for k in names})
            if i:
                self.transfers.append(Transfer(_operator_mesh(levels[i - 1][0]), _operator_mesh(op), emap))
                ng = max(_operator_mesh(op).n_ghost_dofs, 1)
                self._vecs[i]["rg"] = torch.zeros((1, ng), dtype=torch.float64, device=minv.device)

    def setup(self, reduce=None):
        """The Chebyshev coefficients of every level (collective where a level has no lambda_max: the power method reduces its
        two dot products over the ranks); done once, on the first apply at the latest."""
        if self._coeffs is None:
            red = reduce or self._reduce or _default_reduce
            self._coeffs = [_distributed_chebyshev(sm, op, minv, red) for op, minv, sm, _ in self.levels]
        return self

    def _smooth(self, l, r, z):  # z <- S_l r (l3k_cheb_apply: zero initial guess)
        from . import capi
        lib, h = capi.load(), self._ctx._h
        (op, minv, _, _), v, (c0, steps) = self.levels[l], self._vecs[l], self._coeffs[l]
        n = minv.numel()
        capi.check(lib.l3k_cheb_first(h, _vp(r), _vp(minv), c0, _vp(v["w"]), _vp(z), n, None))
        for ca, cb in steps:
            op.apply(z[None, :], v["az"][None, :])
            capi.check(lib.l3k_cheb_step(h, _vp(r), _vp(v["az"]), _vp(minv), ca, cb, _vp(v["w"]), _vp(z), n, None))

    def _residual(self, l, r, z):  # d <- r - A_l z on the live rows, 0 on the frozen ones
        from . import capi
        (op, minv, _, _), v = self.levels[l], self._vecs[l]
        op.apply(z[None, :], v["az"][None, :])
        capi.check(capi.load().l3k_pmg_residual(self._ctx._h, _vp(v["d"]), _vp(r), _vp(v["az"]), _vp(minv), minv.numel()))

    def _cycle(self, l, r, z):
        self._smooth(l, r, z)
        if l + 1 == len(self.levels):
            return
        v, c, T, cop = self._vecs[l], self._vecs[l + 1], self.transfers[l + 1], self.levels[l + 1][0]
        self._residual(l, r, z)
        T.restrict(v["d"], c["r"], c["rg"])
        cop.export_add(c["rg"], c["r"][None, :])
        self._cycle(l + 1, c["r"], c["z"])
        T.prolong(c["z"], cop.import_ghosts(c["z"][None, :]), z, add=True, frozen=self.levels[l][1])
        self._residual(l, r, z)
        self._smooth(l, v["d"], v["e"])
        z.add_(v["e"])  # (e is 0 on the frozen rows: the smoother stores it so)

    def apply(self, r, z):
        """z <- M^-1 r, one symmetric V-cycle; r, z: distinct contiguous vectors over this rank's owned dofs of level 0"""
        from . import capi
        n = self.minv.numel()
        if r.numel() != n or z.numel() != n or not (r.is_contiguous() and z.is_contiguous()):
            raise capi.L3KError("r and z must be contiguous tensors over the owned dofs of level 0")
        if n and _overlap(r, z, n):
            raise capi.L3KError("r and z must be distinct vectors that do not overlap")
        self.setup()
        self._cycle(0, r, z)
        return z


def _default_reduce(view):
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        dist.all_reduce(view, op=dist.ReduceOp.SUM)


def jacobi_inverse_native(ctx, diag, damping=1.0, threshold=0.0):
    """NativeJacobiImpl::init through the C ABI (l3k_jacobi_inverse)."""
    from . import capi
    out = torch.empty_like(diag)
    capi.check(capi.load().l3k_jacobi_inverse(ctx._h, C.c_void_p(diag.data_ptr()), diag.numel(), float(damping),
                                              float(threshold), C.c_void_p(out.data_ptr())))
    return out


_SCALING = {"none": 0, "initial": 1, "rhs": 2}


def _vp(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def _checked(results, throw_on_fail):
    if throw_on_fail and not all(r.converged for r in results):
        raise RuntimeError("Solver failed to converge")  # solve/BelosSolvers.hpp:103
    return results


def _from_c(results, throw_on_fail):
    """capi.CgResult's as IterSolveResult's; raises if one of them did not converge"""
    return _checked([IterSolveResult(r.achieved_tol, r.iterations, bool(r.converged)) for r in results], throw_on_fail)


def pcg(system, b, x, minv=None, tol=1e-6, max_iters=10_000, residual_scaling="none", check_every=1, throw_on_fail=True,
        precond=None):
    """Jacobi-PCG entirely behind the C ABI (l3k_pcg_solve): apply, fused vector updates and reductions run on the
    context's stream, the host only reads 32 bytes per convergence check.  Single rank; `system` is a
    l3ster_amd.system.MatrixFreeSystem or a system.CsrOperator (an assembled or condensed matrix: l3k_csr_pcg_solve, the
    same iteration on the CSR apply), b / x / minv 1-D device tensors over its owned dofs (the operator's rows).  `precond`: a
    ChebyshevPreconditioner of this system (it carries its own minv) -> l3k_pcg_solve_cheb, a PMultigrid whose finest
    level is this MatrixFreeSystem (one V-cycle per iteration; rows frozen by its finest smoother keep x) -> l3k_pcg_solve_pmg,
    or a factored TriangularPreconditioner of this CsrOperator (SGS or ILU(0); its empty rows keep x) -> l3k_csr_pcg_solve_tri;
    a multivector b then solves its columns one after the other, as l3k_pcg_solve_cols does."""
    from . import capi
    opts = capi.CgOpts(float(tol), int(max_iters), _SCALING[residual_scaling], int(check_every))
    if precond is not None:
        if minv is not None:
            raise capi.L3KError("give minv or precond (which carries its own minv), not both")
        if precond.system is not system:
            raise capi.L3KError("the preconditioner was created for another system")
        solve_cheb, n = _entry(system, "pcg_solve_pmg" if isinstance(precond, PMultigrid) else
                               "pcg_solve_tri" if isinstance(precond, TriangularPreconditioner) else "pcg_solve_cheb")
        cols = [(b, x)] if b.dim() == 1 else list(zip(b, x))
        if x.shape != b.shape or any(bc.stride(0) != 1 or xc.stride(0) != 1 or bc.numel() != n for bc, xc in cols):
            raise capi.L3KError("b and x must be tensors of one shape over the owned dofs with unit stride along rows")
        if any(_overlap(bc, xc, n) for bc, xc in cols):
            raise capi.L3KError("b and x must not share memory")
        res_c = (capi.CgResult * len(cols))()
        for (bc, xc), res in zip(cols, res_c):
            capi.check(solve_cheb(system._h, _vp(bc), _vp(xc), precond._h, C.byref(opts), C.byref(res)))
        out = _from_c(res_c, throw_on_fail)
        return out[0] if b.dim() == 1 else out
    if b.dim() == 2:  # a multivector (ncols, ld) of right-hand sides: the columns one after the other (l3k_pcg_solve_cols)
        nc = b.shape[0]
        if x.shape != b.shape or b.stride(1) != 1 or x.stride(1) != 1:
            raise capi.L3KError("b and x must be (ncols, ld) tensors of one shape with unit stride along rows")
        res_c = (capi.CgResult * nc)()
        capi.check(_entry(system, "pcg_solve_cols")[0](system._h, _vp(b), b.stride(0) if nc > 1 else b.shape[1], _vp(x),
                                          x.stride(0) if nc > 1 else x.shape[1], nc, _vp(minv), C.byref(opts), res_c))
        return _from_c(res_c, throw_on_fail)
    res = capi.CgResult()
    capi.check(_entry(system, "pcg_solve")[0](system._h, _vp(b), _vp(x), _vp(minv), C.byref(opts), C.byref(res)))
    return _from_c([res], throw_on_fail)[0]


class GmresWorkspace:
    """Handle of l3k_gmres_create: the workspace of restarted GMRES(restart_length) on n rows -- the basis, w, z, u, the Hessenberg
    matrix, the partial sums -- on the device of `ctx`.  restart_length above n is lowered to n; max_bytes: 0 = no guard, otherwise
    creation refuses a workspace above it and names the bytes needed.  One workspace serves any number of solves of its n.
    collective=True (l3k_gmres_create_dist): the workspace of one rank of gmres_distributed -- n is the rank's owned rows, may be 0,
    and does not lower restart_length, which every rank gives alike."""

    def __init__(self, ctx, n, restart_length=250, max_bytes=0, collective=False):
        from . import capi
        if int(restart_length) < 1:
            raise capi.L3KError(f"GmresWorkspace: restart_length = {restart_length} must be at least 1")
        if int(n) < (0 if collective else 1):
            raise capi.L3KError(f"GmresWorkspace: n = {n} must be at least {0 if collective else 1}")
        self.ctx = ctx
        self._h = C.c_void_p()
        create = capi.load().l3k_gmres_create_dist if collective else capi.load().l3k_gmres_create
        capi.check(create(ctx._h, int(n), int(restart_length), int(max_bytes), C.byref(self._h)))
        i = self.info
        self.n, self.restart_length = i.n, i.restart_length

    @property
    def info(self):
        """n, ld, restart_length, bytes (l3k_gmres_info)"""
        import types
        from . import capi
        i = capi.GmresInfo()
        capi.check(capi.load().l3k_gmres_info_get(self._h, C.byref(i)))
        return types.SimpleNamespace(**{name: getattr(i, name) for name, _ in capi.GmresInfo._fields_})

    def close(self):
        if getattr(self, "_h", None):
            from . import capi
            capi.load().l3k_gmres_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # (module globals may be gone at interpreter shutdown)
            pass


class GmresSolveResult(IterSolveResult):
    """IterSolveResult with what l3k_gmres_result adds: restarts, breakdown, estimate (the last residual estimate of the
    recurrence, scaled as tol) and orth_loss (the largest max_j |<v_j, w>| / ||w|| left by the two projections)."""

    def __init__(self, tol, num_iters, converged, restarts, breakdown, estimate, orth_loss):
        super().__init__(tol, num_iters, converged)
        self.restarts, self.breakdown, self.estimate, self.orth_loss = restarts, breakdown, estimate, orth_loss

    def __repr__(self):
        return (f"GmresSolveResult(tol={self.tol:.3e}, num_iters={self.num_iters}, converged={self.converged}, "
                f"restarts={self.restarts}, breakdown={self.breakdown}, estimate={self.estimate:.3e}, orth_loss={self.orth_loss:.3e})")


def gmres(system, b, x, minv=None, precond=None, tol=1e-6, max_iters=10_000, residual_scaling="none", check_every=1,
          restart_length=250, max_restarts=39, workspace=None, throw_on_fail=True):
    """Restarted GMRES(restart_length) behind the C ABI (l3k_gmres_solve; the reference's Gmres, solve/BelosSolvers.hpp:124-130, with
    max_restarts and restart_length of solve/SolverInterface.hpp:26-37): right preconditioning, classical Gram-Schmidt with one
    re-orthogonalisation, everything on the context's stream.  Single rank.  `system`, b, x, minv and precond as in pcg -- the
    operator need not be symmetric or definite: this is the Krylov solver for a system.CsrOperator that CG cannot serve.  Rows
    with minv == 0 (or frozen by the preconditioner's minv) keep x; the reported tol is the true residual over the other rows.
    `workspace`: a GmresWorkspace over the system's rows to reuse (its restart_length holds); None: one is created for this call
    with min(restart_length, max_iters, n) basis vectors.  A 2-D b solves its columns one after the other on one workspace.
    Returns a GmresSolveResult (a list of them for a 2-D b)."""
    from . import capi
    if precond is not None and minv is not None:
        raise capi.L3KError("give minv or precond (which carries its own minv), not both")
    if precond is not None and precond.system is not system:
        raise capi.L3KError("the preconditioner was created for another system")
    if int(restart_length) < 1:
        raise capi.L3KError(f"restart_length = {restart_length} must be at least 1")
    name = ("gmres_solve" if precond is None else "gmres_solve_pmg" if isinstance(precond, PMultigrid) else
            "gmres_solve_tri" if isinstance(precond, TriangularPreconditioner) else "gmres_solve_cheb")
    from .system import MultiTermSystem
    if name == "gmres_solve_pmg" and isinstance(system, MultiTermSystem):
        raise capi.L3KError("p-multigrid is not provided for a MultiTermSystem")
    entry, n = _entry(system, name)
    cols = [(b, x)] if b.dim() == 1 else list(zip(b, x))
    if x.shape != b.shape or any(bc.stride(0) != 1 or xc.stride(0) != 1 or bc.numel() != n for bc, xc in cols):
        raise capi.L3KError("b and x must be tensors of one shape over the owned dofs with unit stride along rows")
    if any(_overlap(bc, xc, n) for bc, xc in cols):
        raise capi.L3KError("b and x must not share memory")
    if minv is not None and (minv.numel() != n or not minv.is_contiguous()):
        raise capi.L3KError("minv must be a contiguous tensor over the owned dofs of the system")
    if workspace is not None and workspace.n != n:
        raise capi.L3KError(f"the workspace was created for n = {workspace.n}, the system has {n} rows")
    opts = capi.GmresOpts(float(tol), int(max_iters), _SCALING[residual_scaling], int(check_every), int(max_restarts))
    ctx = system.ctx if hasattr(system, "ctx") else system.mesh.ctx
    ws = workspace if workspace is not None else GmresWorkspace(ctx, n, max(1, min(int(restart_length), int(max_iters), n)))
    res_c = (capi.GmresResult * len(cols))()
    try:
        for (bc, xc), res in zip(cols, res_c):
            capi.check(entry(ws._h, system._h, _vp(bc), _vp(xc), precond._h if precond is not None else _vp(minv), C.byref(opts),
                             C.byref(res)))
    finally:
        if ws is not workspace:
            ws.close()
    out = _checked([GmresSolveResult(r.achieved_tol, r.iterations, bool(r.converged), r.restarts, bool(r.breakdown), r.estimate,
                                     r.orth_loss) for r in res_c], throw_on_fail)
    return out[0] if b.dim() == 1 else out


def pcg_distributed(op, ctx, b, x, minv=None, tol=1e-6, max_iters=10_000, residual_scaling="none", group=None,
                    throw_on_fail=True, allreduce=None, check_every=1, precond=None, native=False):
    """The same iteration for a partitioned system: `op.apply(X, Y)` is a DistributedOperator over this rank's owned
    rows; the fused l3k_cg_* kernels keep the scalars in a device block that is all-reduced between them (two small
    all-reduces per iteration, as Belos does).

    `precond`: a DistributedPMultigrid whose level 0 is `op` (it carries its minv): one V-cycle per iteration, the loop of
    l3k_pcg_solve_pmg; or the Chebyshev-Jacobi preconditioner over minv (required then) in place of the diagonal one: a dict of
    ChebyshevPreconditioner's options (degree, cond_est, max_power_iters, boost_factor, lambda_max) or an object whose
    .info has lambda_max, lambda_min and degree (a ChebyshevPreconditioner's numbers on another operator).  The
    iteration is then that of l3k_pcg_solve_cheb with the exported pieces (l3k_cheb_first / _step, l3k_cg_update_rx /
    _update_p): the inner applies go through op.apply and need no reduction, the outer scalars and -- without
    lambda_max -- <x, y> and <y, y> of the power method go through the same reduction hook.  The power method starts
    from power_start_vector over this rank's rows.

    native=True: the whole iteration inside the library (l3k_csr_dist_pcg_solve / l3k_pcg_solve_dist): `op` is a
    system.DistributedCsrOperator or a distributed.NativeDistributedOperator, the reductions are l3k_halo_allreduce_sum over the
    ranks of its halo -- `group` and `allreduce` must be None -- and the host reads 32 bytes per convergence check.  `precond`:
    None, a dict of Chebyshev options (the power method then runs inside the library too), a DistributedChebyshev of `op`, or an
    object whose .info has lambda_max, lambda_min and degree.  A DistributedPMultigrid stays on the host loop (native=False).
    Every rank returns the same IterSolveResult."""
    from . import capi
    if native:
        if group is not None or allreduce is not None:
            raise capi.L3KError("pcg_distributed(native=True) reduces over the ranks of the operator's halo inside the library: "
                                "group and allreduce must be None")
        if isinstance(precond, DistributedPMultigrid):
            raise capi.L3KError("pcg_distributed(native=True) has no p-multigrid: a DistributedPMultigrid runs on the host loop "
                                "(native=False)")
        opts = capi.CgOpts(float(tol), int(max_iters), _SCALING[residual_scaling], int(check_every))
        return _pcg_distributed_native(op, b, x, minv, opts, precond, throw_on_fail)
    pmg = precond if isinstance(precond, DistributedPMultigrid) else None
    if pmg is not None:
        if pmg.op is not op:
            raise capi.L3KError("pcg_distributed: the p-multigrid hierarchy was built on another operator: its level 0 must be op")
        if minv is not None and minv is not pmg.minv:
            raise capi.L3KError("pcg_distributed: give the hierarchy's own minv of level 0, or none")
        minv = pmg.minv
    if precond is not None and minv is None:
        raise capi.L3KError("pcg_distributed(precond=...) needs minv: the preconditioner is a polynomial in D^-1 A")
    lib, check, h, n = capi.load(), capi.check, ctx._h, b.numel()
    s = torch.zeros(8, dtype=torch.float64, device=b.device)
    multi = dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1
    fuse_energy = "energy" in inspect.signature(op.apply).parameters
    it = 0

    def reduce(view):
        if allreduce is not None:  # pluggable (the threaded multi-rank emulation of the tests)
            allreduce(view)
        elif multi:
            dist.all_reduce(view, op=dist.ReduceOp.SUM, group=group)

    def apply_energy(p, ap):  # ap = A p, reduced s[1] = <p, A p>
        nonlocal fuse_energy
        if fuse_energy:  # <p, A p> from the element kernels' quadrature stage where they can (l3k_mf_energy_*)
            op.apply(p[None, :], ap[None, :], energy=s)
            if it == 0:
                # element-wise shares (fused) and row-wise shares (dot product) of <p, A p> do not add up across ranks:
                # every rank must take the same route.  Decided once -- it depends on the launch sizes only.
                n_not = torch.tensor([0.0 if op.energy_fused else 1.0], dtype=torch.float64, device=b.device)
                reduce(n_not)
                fuse_energy = n_not.item() == 0.0
            elif not op.energy_fused:
                raise RuntimeError("the element kernels stopped accumulating <p, A p>")
        else:
            op.apply(p[None, :], ap[None, :])
        if not fuse_energy:
            check(lib.l3k_cg_dot_pap(h, _vp(p), _vp(ap), n, _vp(s)))
        reduce(s[1:2])

    def start():  # with the reduced <r, r> of the initial residual in s[3]: (residual scale, scaled residual)
        bb = torch.dot(b, b).reshape(1)
        reduce(bb)
        rr0 = s[3].item() ** 0.5
        scale = {"none": 1.0, "initial": rr0 if rr0 > 0 else 1.0, "rhs": max(bb.item() ** 0.5, 1e-300)}[residual_scaling]
        return scale, rr0 / scale

    if precond is None:  # the iteration of l3k_pcg_solve
        r, p, ap = torch.empty_like(b), torch.empty_like(b), torch.empty_like(b)
        op.apply(x[None, :], r[None, :])
        check(lib.l3k_cg_init(h, _vp(r), _vp(b), _vp(p), _vp(minv), n, _vp(s)))
        reduce(s[2:4])
        s[0] = s[2]
        scale, res = start()
        while res > tol and it < max_iters:
            apply_energy(p, ap)
            check(lib.l3k_cg_update_z(h, _vp(r), _vp(ap), _vp(minv), n, _vp(s)))  # (r holds z = M^-1 r: l3k.h)
            reduce(s[2:4])
            check(lib.l3k_cg_update_px(h, _vp(p), _vp(x), _vp(r), n, _vp(s)))
            it += 1
            if it % check_every == 0 or it == max_iters:  # (the only host synchronisation of the iteration)
                res = s[3].item() ** 0.5 / scale
    else:  # the iteration of l3k_pcg_solve_cheb; with a hierarchy: of l3k_pcg_solve_pmg
        r, z, p, ap, w = (torch.empty_like(b) for _ in range(5))
        if pmg is not None:
            pmg.setup(reduce)
        else:
            c0, steps = _distributed_chebyshev(precond, op, minv, reduce)

        def cheb():  # z = M^-1 r, reduced s[2] = <r, z> (the last kernel of the application leaves the local sum)
            if pmg is not None:  # one V-cycle; <r, z> is a dot product behind it
                pmg.apply(r, z)
                s[2] = torch.dot(r, z)
                reduce(s[2:3])
                return
            check(lib.l3k_cheb_first(h, _vp(r), _vp(minv), c0, _vp(w), _vp(z), n, _vp(None if steps else s)))
            for k, (ca, cb) in enumerate(steps):
                op.apply(z[None, :], ap[None, :])  # (ap is free here: it holds A z)
                check(lib.l3k_cheb_step(h, _vp(r), _vp(ap), _vp(minv), ca, cb, _vp(w), _vp(z), n,
                                        _vp(s if k == len(steps) - 1 else None)))
            reduce(s[2:3])

        op.apply(x[None, :], r[None, :])
        r.copy_(torch.where(minv != 0, b - r, torch.zeros_like(b)))  # (frozen rows: out of the residual from the start)
        s[3] = torch.dot(r, r)
        reduce(s[3:4])
        scale, res = start()
        if res > tol and it < max_iters:
            cheb()
            p.copy_(z)
            s[0] = s[2]
        while res > tol and it < max_iters:
            apply_energy(p, ap)
            check(lib.l3k_cg_update_rx(h, _vp(x), _vp(r), _vp(p), _vp(ap), _vp(minv), n, _vp(s)))
            reduce(s[3:4])
            it += 1
            if it % check_every == 0 or it == max_iters:  # (the only host synchronisation of the iteration)
                res = s[3].item() ** 0.5 / scale
            if res <= tol or it >= max_iters:  # (x is final: no preconditioner application for a direction nobody takes)
                break
            cheb()
            check(lib.l3k_cg_update_p(h, _vp(p), _vp(z), n, _vp(s)))
    return _checked([IterSolveResult(res, it, res <= tol)], throw_on_fail)[0]


def _distributed_chebyshev(precond, op, minv, reduce):
    """(c0, [(a_k, b_k)]) of pcg_distributed's preconditioner; runs the power method on D^-1 A through op.apply where no
    lambda_max is given (<x, y> and <y, y> reduced across the ranks)."""
    info = getattr(precond, "info", None)
    if info is not None:
        return chebyshev_coefficients(info.lambda_max, info.lambda_min, info.degree)
    o = _chebyshev_options(precond)
    lam = o["lambda_max"]
    if lam is None:
        lam = o["boost_factor"] * _distributed_lambda_est(op, minv, reduce, o["max_power_iters"])
    return chebyshev_coefficients(lam, lam / o["cond_est"], o["degree"])


def _chebyshev_options(precond):
    """a dict of ChebyshevPreconditioner's options completed with their defaults and checked"""
    o = dict(degree=1, cond_est=30.0, max_power_iters=10, boost_factor=1.1, lambda_max=None)
    unknown = set(precond) - set(o)
    if unknown:
        raise ValueError(f"unknown Chebyshev options {sorted(unknown)}")
    o.update(precond)
    if o["degree"] < 1 or not o["cond_est"] > 1 or not o["boost_factor"] >= 1:
        raise ValueError("Chebyshev options: degree >= 1, cond_est > 1, boost_factor >= 1")
    if o["lambda_max"] is None and o["max_power_iters"] < 1:
        raise ValueError("max_power_iters < 1 and no lambda_max given")
    return o


def _distributed_lambda_est(op, minv, reduce, max_power_iters=10):
    """The eigenvalue estimate of the host loop: max_power_iters steps of the power method on D^-1 A through op.apply from
    power_start_vector over this rank's rows, <x, y> and <y, y> reduced across the ranks."""
    live = minv != 0
    y = torch.where(live, power_start_vector(minv.numel(), minv.device), torch.zeros_like(minv))
    t = torch.zeros(2, dtype=torch.float64, device=minv.device)
    t[1] = torch.dot(y, y)
    reduce(t[1:2])
    ax = torch.empty_like(minv)
    for _ in range(max_power_iters):
        xv = y * (1.0 / torch.sqrt(t[1]))
        op.apply(xv[None, :], ax[None, :])
        y = torch.where(live, minv * ax, torch.zeros_like(minv))
        t[0], t[1] = torch.dot(xv, y), torch.dot(y, y)
        reduce(t)
    est = t[0].item()
    if not (est > 0 and est < float("inf")):
        raise RuntimeError(f"the power method on D^-1 A gave the eigenvalue estimate {est}: it must be finite and positive")
    return est


def _native_operator(op):
    """(kind, handles) of an operator the collective entry points take: ("csr", (l3k_csr_dist,)) for a
    system.DistributedCsrOperator, ("mf", (l3k_mf, l3k_halo)) for a matrix-free operator on a distributed.NativeHalo"""
    from . import capi
    from .system import DistributedCsrOperator
    if isinstance(op, DistributedCsrOperator):
        return "csr", (op._h,)
    mf, halo = getattr(op, "mf", None), getattr(op, "halo", None)
    if mf is not None and getattr(halo, "_h", None) and getattr(mf, "_h", None):
        return "mf", (mf._h, halo._h)
    raise capi.L3KError("the collective solve inside the library takes a system.DistributedCsrOperator or a "
                        "distributed.NativeDistributedOperator (a MatrixFreeSystem on a NativeHalo)")


class DistributedChebyshev:
    """Handle of l3k_csr_dist_cheb_create / l3k_cheb_create_dist: the Chebyshev-Jacobi preconditioner of a partitioned operator
    (a system.DistributedCsrOperator, or a distributed.NativeDistributedOperator), with the power method and its reductions inside
    the library.  Creation and apply are collective; options as ChebyshevPreconditioner's.  `op` and `minv` are kept alive here."""

    def __init__(self, op, minv, degree=1, cond_est=30., max_power_iters=10, boost_factor=1.1, lambda_max=None):
        from . import capi
        kind, handles = _native_operator(op)
        self.op, self.system, self.minv = op, op, minv
        if minv is None or not minv.is_contiguous():
            raise capi.L3KError("minv must be a contiguous tensor over the owned dofs of the operator")
        opts = capi.ChebOpts(int(degree), float(cond_est), int(max_power_iters), float(boost_factor),
                             0.0 if lambda_max is None else float(lambda_max))
        create = capi.load().l3k_csr_dist_cheb_create if kind == "csr" else capi.load().l3k_cheb_create_dist
        self._h = C.c_void_p()
        capi.check(create(*handles, _vp(minv), C.byref(opts), C.byref(self._h)))

    info = ChebyshevPreconditioner.info
    close = ChebyshevPreconditioner.close
    __del__ = ChebyshevPreconditioner.__del__

    def apply(self, r, z):
        """z <- p(D^-1 A) D^-1 r over the owned rows (l3k_cheb_apply; collective)"""
        from . import capi
        if _overlap(r, z, r.numel()):
            raise capi.L3KError("r and z must be distinct vectors that do not overlap")
        capi.check(capi.load().l3k_cheb_apply(self._h, _vp(r), _vp(z)))
        return z


def _pcg_distributed_native(op, b, x, minv, opts, precond, throw_on_fail):
    """pcg_distributed(native=True): l3k_csr_dist_pcg_solve / l3k_pcg_solve_dist"""
    from . import capi
    kind, handles = _native_operator(op)
    n = b.numel()
    if x.numel() != n or not (b.is_contiguous() and x.is_contiguous()) or (n and _overlap(b, x, n)):
        raise capi.L3KError("b and x must be distinct contiguous vectors over the owned dofs")
    cheb = None
    if precond is not None:
        if minv is None:
            raise capi.L3KError("pcg_distributed(precond=...) needs minv: the preconditioner is a polynomial in D^-1 A")
        if isinstance(precond, DistributedChebyshev):
            cheb = precond
        elif isinstance(precond, dict):
            cheb = DistributedChebyshev(op, minv, **_chebyshev_options(precond))
        else:  # another preconditioner's numbers on this operator: no power method
            i = precond.info
            cheb = DistributedChebyshev(op, minv, degree=i.degree, cond_est=i.lambda_max / i.lambda_min, lambda_max=i.lambda_max)
        minv = cheb.minv
    solve = capi.load().l3k_csr_dist_pcg_solve if kind == "csr" else capi.load().l3k_pcg_solve_dist
    res = capi.CgResult()
    try:
        capi.check(solve(*handles, _vp(b), _vp(x), _vp(minv), cheb._h if cheb is not None else None, C.byref(opts), C.byref(res)))
    finally:
        if cheb is not None and cheb is not precond:
            cheb.close()
    return _from_c([res], throw_on_fail)[0]


def gmres_distributed(op, ctx, b, x, minv=None, precond=None, workspace=None, restart_length=250, tol=1e-6, max_iters=10_000,
                      residual_scaling="none", check_every=1, max_restarts=39, throw_on_fail=True):
    """gmres for a partitioned system, the whole iteration inside the library (l3k_csr_dist_gmres_solve / l3k_gmres_solve_dist):
    `op` is a system.DistributedCsrOperator or a distributed.NativeDistributedOperator, b / x / minv this rank's owned rows (empty
    on a rank that owns nothing).  Every reducing pass -- <b, b>, <r, r> at the head of a cycle, the three passes of a step -- is
    followed by one l3k_halo_allreduce_sum_n over the ranks of the operator's halo, so every rank takes the same decisions and
    returns the same GmresSolveResult.  Collective: every rank calls it with the same options and restart_length.  `precond`: None
    (Jacobi with minv, or no preconditioner without), a DistributedChebyshev of `op`, or a dict of its options (minv required then;
    the object is made and dropped by the call).  `workspace`: a GmresWorkspace(ctx, n_owned, restart_length, collective=True) to
    reuse; None: one of min(restart_length, max_iters) basis vectors is created for this call.  The p-multigrid and the triangular
    preconditioners have no collective form."""
    from . import capi
    kind, handles = _native_operator(op)
    n = b.numel()
    if x.numel() != n or not (b.is_contiguous() and x.is_contiguous()) or (n and _overlap(b, x, n)):
        raise capi.L3KError("b and x must be distinct contiguous vectors over the owned dofs")
    if minv is not None and (minv.numel() != n or not minv.is_contiguous()):
        raise capi.L3KError("minv must be a contiguous tensor over the owned dofs of the operator")
    if int(restart_length) < 1:
        raise capi.L3KError(f"restart_length = {restart_length} must be at least 1")
    cheb = None
    if precond is not None:
        if isinstance(precond, DistributedChebyshev):
            cheb = precond
        elif isinstance(precond, dict):
            if minv is None:
                raise capi.L3KError("gmres_distributed(precond=dict(...)) needs minv: the preconditioner is a polynomial in D^-1 A")
            cheb = DistributedChebyshev(op, minv, **_chebyshev_options(precond))
        else:
            raise capi.L3KError("gmres_distributed takes a DistributedChebyshev or a dict of its options as precond: the p-multigrid "
                                "and the triangular preconditioners have no collective form")
        if minv is not None and minv is not cheb.minv and minv.data_ptr() != cheb.minv.data_ptr():
            raise capi.L3KError("give the preconditioner's own minv, or none")
    opts = capi.GmresOpts(float(tol), int(max_iters), _SCALING[residual_scaling], int(check_every), int(max_restarts))
    ws = workspace
    res = capi.GmresResult()
    try:
        if ws is None:
            ws = GmresWorkspace(ctx, n, max(1, min(int(restart_length), int(max_iters))), collective=True)
        solve = capi.load().l3k_csr_dist_gmres_solve if kind == "csr" else capi.load().l3k_gmres_solve_dist
        capi.check(solve(ws._h, *handles, _vp(b), _vp(x), None if cheb is not None else _vp(minv), cheb._h if cheb is not None else None,
                         C.byref(opts), C.byref(res)))
    finally:
        if ws is not None and ws is not workspace:
            ws.close()
        if cheb is not None and cheb is not precond:
            cheb.close()
    return _checked([GmresSolveResult(res.achieved_tol, res.iterations, bool(res.converged), res.restarts, bool(res.breakdown),
                                      res.estimate, res.orth_loss)], throw_on_fail)[0]


class CholeskySolver:
    """Handle of l3k_chol_create: the sparse direct solver on a single-rank system.CsrOperator -- the one AssembledSystem.end()
    returns included -- where the reference uses Amesos2 (Klu2 / Lapack, solve/Amesos2Solvers.hpp:18-32).  Band Cholesky: the
    matrix is taken as symmetric positive definite (what the assembled path produces once the Dirichlet conditions are applied);
    only its lower triangle, after a reverse Cuthill-McKee ordering, is read.  Creation runs the symbolic phase on the host and
    refuses a structurally unsymmetric graph and a factor above max_bytes (0 = 8 GiB); block = 0 (chosen), 32 or 64.  factor()
    reads A's current values: a time loop assembles again and calls it again.  Rows of A that store nothing (the internal dofs of
    a condensed system) are left alone.  Factor and solve are bitwise reproducible.  A is kept alive here."""

    def __init__(self, A, max_bytes=0, block=0):
        from . import capi
        from .system import CsrOperator, DistributedCsrOperator
        if isinstance(A, DistributedCsrOperator):
            raise capi.L3KError("CholeskySolver: a DistributedCsrOperator is refused: the direct solver works on the matrix of one "
                                "rank; solve a partitioned system with solve.pcg_distributed")
        if not isinstance(A, CsrOperator):
            raise capi.L3KError("CholeskySolver takes a system.CsrOperator (AssembledSystem.end() returns one)")
        self.A, self.n = A, A.n
        self._h = C.c_void_p()
        opts = capi.CholOpts(int(max_bytes), int(block))
        capi.check(capi.load().l3k_chol_create(A._h, C.byref(opts), C.byref(self._h)))

    @property
    def info(self):
        """n, n_active, n_blocks, block, max_height, factor_bytes, factor_flops, update_flops, n_bad_pivots, first_bad_row,
        factored (l3k_chol_info)"""
        import types
        from . import capi
        i = capi.CholInfo()
        capi.check(capi.load().l3k_chol_info_get(self._h, C.byref(i)))
        return types.SimpleNamespace(**{name: getattr(i, name) for name, _ in capi.CholInfo._fields_})

    def factor(self):
        """The numeric factorisation of A's current values (l3k_chol_factor); raises "matrix is not positive definite" with the
        counts in .info"""
        from . import capi
        capi.check(capi.load().l3k_chol_factor(self._h))
        return self

    def solve(self, b, x=None):
        """x <- A^-1 b on the rows of A that store entries; b, x: 1-D vectors over the n rows or (ncols, ld >= n) multivectors
        with contiguous rows, x = None: in place of b (l3k_chol_solve).  The other rows of x keep their values."""
        from . import capi
        x = b if x is None else x
        B, X = (b[None, :], x[None, :]) if b.dim() == 1 and x.dim() == 1 else (b, x)
        if B.dim() != 2 or X.dim() != 2 or B.shape[0] != X.shape[0] or B.shape[1] < self.n or X.shape[1] < self.n:
            raise capi.L3KError("b and x must have the same number of columns and at least n rows")
        if B.dtype != torch.float64 or X.dtype != torch.float64 or B.stride(1) != 1 or X.stride(1) != 1:
            raise capi.L3KError("b and x are float64 with contiguous rows")
        ldb = B.stride(0) if B.shape[0] > 1 else max(B.shape[1], 1)
        ldx = X.stride(0) if X.shape[0] > 1 else max(X.shape[1], 1)
        capi.check(capi.load().l3k_chol_solve(self._h, C.c_void_p(B.data_ptr()), ldb, C.c_void_p(X.data_ptr()), ldx, B.shape[0]))
        return x

    def close(self):
        if getattr(self, "_h", None):
            from . import capi
            capi.load().l3k_chol_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # (module globals may be gone at interpreter shutdown)
            pass


class TriangularPreconditioner:
    """Handle of l3k_tri_create: symmetric Gauss-Seidel (kind="sgs") or ILU(0) (kind="ilu0") on a single-rank system.CsrOperator,
    where the reference uses Ifpack2 (Ifpack2SGSOpts / Ifpack2IluKOpts, solve/Ifpack2Preconditioners.hpp:97-101,134-157).  Both are
    level-scheduled sparse triangular solves in A's pattern; `damping` is the SSOR factor of SGS, the two thresholds modify the
    diagonal before ILU(0) factors, fuse_rows = 0 leaves the launch plan to the library (include/l3k.h).  Creation is symbolic
    only; factor() reads A's current values: a time loop assembles again and calls it again.  Rows of A that store nothing are
    frozen: apply writes 0 there and a solve keeps x.  Pass the factored object as precond= to solve.pcg / solve.gmres.  Results
    are bitwise reproducible.  A is kept alive here."""

    KINDS = {"sgs": 0, "ilu0": 1}

    def __init__(self, A, kind="ilu0", damping=1.0, absolute_threshold=0.0, relative_threshold=1.0, fuse_rows=0):
        from . import capi
        from .system import CsrOperator, DistributedCsrOperator
        if isinstance(A, DistributedCsrOperator):
            raise capi.L3KError("TriangularPreconditioner: a DistributedCsrOperator is refused: the triangular solves work on the "
                                "matrix of one rank")
        if not isinstance(A, CsrOperator):
            raise capi.L3KError("TriangularPreconditioner takes a system.CsrOperator (AssembledSystem.end() returns one)")
        if kind not in self.KINDS:
            raise capi.L3KError(f"TriangularPreconditioner: kind = {kind!r}; it is 'sgs' or 'ilu0'")
        self.system, self.n, self.kind = A, A.n, kind
        self._h = C.c_void_p()
        opts = capi.TriOpts(self.KINDS[kind], float(damping), float(absolute_threshold), float(relative_threshold), int(fuse_rows))
        capi.check(capi.load().l3k_tri_create(A._h, C.byref(opts), C.byref(self._h)))

    @property
    def info(self):
        """n, n_active, nnz, kind, lanes_per_row, n_levels_lower, n_levels_upper, max_level_rows, n_launches_lower,
        n_launches_upper, bytes, n_bad_pivots, first_bad_row, factored (l3k_tri_info)"""
        import types
        from . import capi
        i = capi.TriInfo()
        capi.check(capi.load().l3k_tri_info_get(self._h, C.byref(i)))
        return types.SimpleNamespace(**{name: getattr(i, name) for name, _ in capi.TriInfo._fields_})

    def factor(self):
        """The numeric phase on A's current values (l3k_tri_factor); raises with the number of zero or non-finite pivots and the
        first one's row, which .info keeps"""
        from . import capi
        capi.check(capi.load().l3k_tri_factor(self._h))
        return self

    def _call(self, fn, u, v):
        from . import capi
        n = self.n
        if u.numel() != n or v.numel() != n or not (u.is_contiguous() and v.is_contiguous()) or u.dtype != torch.float64 or v.dtype != torch.float64:
            raise capi.L3KError("the vectors must be contiguous float64 tensors over the rows of the operator")
        capi.check(fn(self._h, C.c_void_p(u.data_ptr()), C.c_void_p(v.data_ptr())))
        return v

    def apply(self, r, z):
        """z <- M^-1 r (l3k_tri_apply); r, z: distinct 1-D device tensors over the rows"""
        from . import capi
        return self._call(capi.load().l3k_tri_apply, r, z)

    def solve_lower(self, r, y):
        """the first half of apply (l3k_tri_solve_lower)"""
        from . import capi
        return self._call(capi.load().l3k_tri_solve_lower, r, y)

    def solve_upper(self, y, z):
        """the second half of apply, for SGS with the diagonal scaling in front (l3k_tri_solve_upper)"""
        from . import capi
        return self._call(capi.load().l3k_tri_solve_upper, y, z)

    def values(self):
        """ILU(0): the factor in A's pattern, a new device tensor of nnz doubles (l3k_tri_values)"""
        from . import capi
        out = torch.empty_like(self.system.values)
        capi.check(capi.load().l3k_tri_values(self._h, C.c_void_p(out.data_ptr())))
        return out

    def close(self):
        if getattr(self, "_h", None):
            from . import capi
            capi.load().l3k_tri_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # (module globals may be gone at interpreter shutdown)
            pass


def direct_solve(A, b, x, max_bytes=0):
    """The reference's solver.solve(A, b, x) with a direct solver: symbolic phase, numeric factorisation and solve in one call.
    Keep a CholeskySolver instead where the matrix, or its graph, serves more than one solve."""
    solver = CholeskySolver(A, max_bytes)
    try:
        solver.factor().solve(b, x)
    finally:
        solver.close()
    return x
