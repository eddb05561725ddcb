"""The triangular preconditioners on the device CSR operator (l3k_tri_*, solve.TriangularPreconditioner): SGS and ILU(0), against
the longdouble restatement of tests/tri_ref.py.

Factors and solves are held to the two DERIVED bounds of tri_ref (factor_bound, solve_bound: first-order backward errors with the
number of roundings counted, nothing tuned on the device's output).  Iteration counts are held EQUAL to the restatement's, run on
the CPU inside the test with the same preconditioner; every such case asserts that the restatement's own estimates at the stopping
step and at the step before lie a factor >= 1.5 from the tolerance (stopping_margin), which the device's rounding (1e-10 relative
at the most) cannot bridge.  Where the tolerance is this file's choice it is the geometric mean of two consecutive estimates that
are a factor >= 2.25 apart (for PCG, whose residuals do not fall monotonically: with every earlier residual a factor 1.5 above it
too, and in the float64 run of the restatement as well as in the longdouble one).  Case (e) prescribes all three unknowns of
Diffusion2D on all four sides: with Dirichlet values on two sides and adiabatic walls the restatement's PCG residuals with ILU(0)
never fall by 2.25 in one of the first 100 steps, so no tolerance with both margins exists there.  Case (a) fixes 1e-6 |b|; its right-hand side is this file's choice, made so that the margins hold.

The damped SGS solve of case (h) gets three more roundings than solve_bound counts for its right-hand side: c = (2 - omega) /
omega costs two and c * a_ii one, all exact at omega = 1."""
import ctypes as C

import numpy as np
import pytest
import torch

import gmres_ref as G
import tri_ref as R
from l3ster_amd import capi, solve, system
from tri_ref import EPS, LD

pytestmark = pytest.mark.gpu
_CTX, _CACHE = [], {}
KINDS = ("sgs", "ilu0")


def ctx(k=0):
    while len(_CTX) <= k:
        torch.cuda.set_device(0)
        _CTX.append(system.Context(0, torch.cuda.current_stream().cuda_stream))
    return _CTX[k]


def dev(a, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


def host(t):
    return t.cpu().numpy()


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


class Mat:
    """a matrix of tri_ref (A, P) as a CsrOperator; `csr` overrides the arrays (a batch of blocks)"""

    def __init__(self, A, P, lanes=0, context=None, csr=None):
        self.A, self.P = A, P
        self.csr = csr or R.to_csr(A, P)
        self.row_ptr, self.col_ind, self.values = dev(self.csr[0], torch.int64), dev(self.csr[1], torch.int32), dev(self.csr[2])
        self.n = len(self.csr[0]) - 1
        self.op = system.CsrOperator(context or ctx(), self.row_ptr, self.col_ind, self.values, lanes)

    def dense(self, values):
        """values in the pattern of the operator as the dense array(s) of tri_ref"""
        if self.A.ndim == 3:
            r, c = np.nonzero(self.P)
            out = np.zeros(self.A.shape)
            out[:, r, c] = values.reshape(self.A.shape[0], -1)
            return out
        return R.from_csr(self.csr[0], self.csr[1], values)[0]

    def vec(self, v):
        return v.reshape(self.A.shape[0], -1) if self.A.ndim == 3 else v

    def __call__(self, v):
        return self.A.astype(v.dtype) @ v


def ratio(err, bound, where=None):
    e, b = (err, bound) if where is None else (err[..., where], bound[..., where])
    return float(np.max(e / np.maximum(b, 1e-300)))


def check_factor(M, T, absolute=0.0, relative=1.0, label=""):
    F = M.dense(host(T.values()))
    B = R.block(M.P)
    err, bound = R.factor_bound(R.thresholded(M.A, M.P, absolute, relative), F, M.P)
    print(f"{label} factor: max err / bound = {ratio(err, bound, B):.3f}")
    assert np.isfinite(F).all() and (err[..., B] <= bound[..., B]).all()
    return F


def check_solves(M, T, kind, F, r, omega=1.0, extra_upper=0, label=""):
    """the two pieces inside solve_bound, apply = upper(lower) bit for bit, 0 on the empty rows; returns z"""
    n, active = M.n, R.active_rows(M.P)
    y, z, z2 = (torch.full((n,), 7.0, dtype=torch.float64, device="cuda") for _ in range(3))
    rd = dev(r)
    T.solve_lower(rd, y)
    T.solve_upper(y, z)
    T.apply(rd, z2)
    assert torch.equal(z, z2)
    Tl, Tu, s = R.triangles(F if kind == "ilu0" else M.A, M.P, kind, omega)
    yh, zh = M.vec(host(y)), M.vec(host(z))
    for name, Tm, out, rhs, extra in (("lower", Tl, yh, M.vec(r), 0), ("upper", Tu, zh, s * yh.astype(LD), extra_upper)):
        err, bound = R.solve_bound(Tm, out, rhs, active)
        bound = bound * ((Tm != 0).sum(-1) + 3 + extra) / ((Tm != 0).sum(-1) + 3)
        print(f"{label} {kind} {name}: max err / bound = {ratio(err, bound):.3f}")
        assert np.isfinite(out).all() and (err <= bound).all()
        assert not out[..., ~active].any()
    return z


def rel_scale(b):
    return np.sqrt(np.sum(b.astype(LD) ** 2))


def true_residual(M, b, x, live=None):
    r = b.astype(LD) - M(x.astype(LD))
    r = r if live is None else np.where(live, r, LD(0))
    return float(np.sqrt(np.sum(r * r)) / rel_scale(b))


def margins(history, tol, floor=1.5, two_sided=True):
    below, above = G.stopping_margin(history, tol)
    print(f"margins (below, above): {below:.4f} {above:.4f}, asserted >= {floor}")
    assert below >= floor and (above >= floor or not two_sided), (below, above)


def precond_of(M, kind, **kw):
    """(device preconditioner or minv tensor, restatement callable)"""
    if kind == "jacobi":
        d = np.where(R.active_rows(M.P), np.diag(M.A), 1.0)
        minv = np.where(R.active_rows(M.P), 1.0 / d, 0.0)
        return dev(minv), lambda v: v * minv.astype(v.dtype)
    return solve.TriangularPreconditioner(M.op, kind, **kw).factor(), R.Preconditioner(M.A, M.P, kind, kw.get("damping", 1.0))


def run_pcg(M, b, x0, pre, **kw):
    x = dev(x0)
    arg = dict(minv=pre) if isinstance(pre, torch.Tensor) else dict(precond=pre)
    return solve.pcg(M.op, dev(b), x, residual_scaling="rhs", throw_on_fail=False, **arg, **kw), host(x)


def run_gmres(M, b, x0, pre, m, **kw):
    x = dev(x0)
    arg = dict(minv=pre) if isinstance(pre, torch.Tensor) else dict(precond=pre)
    return solve.gmres(M.op, dev(b), x, residual_scaling="rhs", restart_length=m, throw_on_fail=False, **arg, **kw), host(x)


# ------------------------------------------------------------------------------------------------ (a) the reference's matrix
def spd():
    return cached("spd", lambda: Mat(*R.spd_matrix(100)))


def spd_rhs():
    """b = A x* with x* uniform in (-1, 1): at 1e-6 |b| the restatement's margins are 1.6 .. 26 for SGS and 1.8 .. 1.9 for Jacobi"""
    xs = np.random.default_rng(5).uniform(-1, 1, 100)
    return xs, spd().A @ xs


def test_a_reference_matrix_plan_and_exact_lu():
    M = spd()
    T = solve.TriangularPreconditioner(M.op, "ilu0").factor()
    i = T.info
    assert (i.n, i.n_active, i.nnz, i.kind, i.factored, i.n_bad_pivots, i.first_bad_row) == (100, 100, 298, 1, 1, 0, -1)
    assert (i.n_levels_lower, i.n_levels_upper, i.max_level_rows, i.n_launches_lower, i.n_launches_upper) == (100, 100, 1, 1, 1)
    assert i.lanes_per_row == M.op.info().lanes_per_row and i.bytes >= 298 * 8 + 4 * 100 * 8
    F = check_factor(M, T, label="(a)")
    Lm, U = R.lu_nopivot(M.A)
    assert np.abs(F - (np.tril(Lm, -1) + U)).max() <= 4 * EPS  # (ILU(0) of a tridiagonal matrix is its LU: entries of size <= 2)
    r = np.cos(0.7 * np.arange(100))
    for kind in KINDS:
        Tk = T if kind == "ilu0" else solve.TriangularPreconditioner(M.op, "sgs").factor()
        check_solves(M, Tk, kind, F, r, label="(a)")


@pytest.mark.parametrize("solver", ["pcg", "gmres"])
def test_a_reference_matrix_iteration_counts(solver):
    """ILU(0) = A: one iteration; SGS and Jacobi: the restatement's counts (4 and 11)"""
    M = spd()
    xs, b = spd_rhs()
    expected = {"ilu0": 1, "sgs": 4, "jacobi": 11}
    for kind in ("ilu0", "sgs", "jacobi"):
        pre, ref_pre = precond_of(M, kind)
        if solver == "pcg":
            ref = cached(("a", solver, kind), lambda: R.pcg(M, b, np.zeros(100), ref_pre, tol=1e-6))
            res, x = run_pcg(M, b, np.zeros(100), pre, tol=1e-6)
        else:
            ref = cached(("a", solver, kind), lambda: G.gmres(M, b, np.zeros(100), 100, prec=ref_pre, tol=1e-6, residual_scaling=2, dtype=LD))
            res, x = run_gmres(M, b, np.zeros(100), pre, 250, tol=1e-6)
        print(f"(a) {solver} {kind}: device {res.num_iters} iterations to {res.tol:.3e}; restatement {ref['iterations']} to {ref['achieved_tol']:.3e}")
        margins(ref["history"], 1e-6, two_sided=kind != "ilu0")
        assert res.converged and res.num_iters == ref["iterations"] == expected[kind]
        assert abs(res.tol - true_residual(M, b, x)) <= 1e-12 and np.abs(x - xs).max() <= 1e-5
        if kind == "ilu0":
            assert res.tol <= 1e-14


# ------------------------------------------------------------------------------------------------ (b) levels wider than one grid
@pytest.mark.parametrize("lanes", [4, 16, 64])
def test_b_levels_wider_than_one_grid_pass(lanes):
    """70 000 independent chains of 3 rows: 3 levels of 70 000 rows, above the 65 536 / 16 384 / 4 096 rows of one grid pass"""
    nc = 70_000
    B, P = cached("chains", lambda: R.chains(nc))
    M = Mat(B, P, lanes, csr=R.chains_csr(B, P))
    assert M.n == 210_000 and M.op.info().lanes_per_row == lanes and nc > 1024 * 256 // lanes
    r = np.cos(0.37 * np.arange(M.n)) + 0.2
    for kind in KINDS:
        T = solve.TriangularPreconditioner(M.op, kind).factor()
        i = T.info
        assert (i.n_levels_lower, i.n_levels_upper, i.max_level_rows, i.n_launches_lower, i.n_launches_upper) == (3, 3, nc, 3, 3)
        F = check_factor(M, T, label=f"(b) L={lanes}") if kind == "ilu0" else None
        check_solves(M, T, kind, F, r, label=f"(b) L={lanes}")


# ------------------------------------------------------------------------------------------------ (c) many dependent steps per row
@pytest.mark.parametrize("lanes", [4, 16, 64])
def test_c_full_band(lanes):
    """half-width 70, n = 400: 141 entries per row, 70 sequential k per row, more entries than lanes; ILU(0) is the band LU"""
    A, P = cached("band", lambda: R.band(400, 70))
    M = Mat(A, P, lanes)
    T = solve.TriangularPreconditioner(M.op, "ilu0").factor()
    assert T.info.n_levels_lower == 400 and T.info.n_launches_lower == 1
    F = check_factor(M, T, label=f"(c) L={lanes}")
    Lm, U = cached("band lu", lambda: R.lu_nopivot(A))
    # the same bound against the dense LU: |L U - A| of the device's factor is inside it, and the dense LU reproduces A exactly
    err, bound = R.factor_bound(np.asarray(np.tril(Lm) @ U, dtype=LD), F, P)
    assert (err[P] <= bound[P]).all()
    assert np.abs(F - (np.tril(Lm, -1) + U)).max() <= 1e-12 * np.abs(U).max()  # (diagonally dominant: the growth is bounded)
    r = np.sin(0.3 * np.arange(400)) + 0.1
    for kind in KINDS:
        Tk = T if kind == "ilu0" else solve.TriangularPreconditioner(M.op, "sgs").factor()
        check_solves(M, Tk, kind, F, r, label=f"(c) L={lanes}")


# ------------------------------------------------------------------------------------------------ (d) the grid
def grid(k=0):
    return cached(("grid", k), lambda: Mat(*R.grid(24), context=ctx(k)))


def test_d_grid_plans_and_equal_bits():
    M = grid()
    r = np.cos(0.1 * np.arange(M.n))
    L = M.op.info().lanes_per_row
    outs = []
    for k, fuse in ((0, 1), (0, 0), (0, 1_000_000), (1, 0)):
        Mk = grid(k)
        for kind in KINDS:
            T = solve.TriangularPreconditioner(Mk.op, kind, fuse_rows=fuse).factor()
            i = T.info
            assert (i.n_levels_lower, i.n_levels_upper, i.max_level_rows) == (47, 47, 24)
            plan = R.launch_plan(R.levels(M.P)[0], fuse or 256 // L)
            assert i.n_launches_lower == i.n_launches_upper == len(plan)
            if fuse == 1:
                assert len(plan) == 47 and sum(f for _, _, f in plan) == 2  # 45 level launches, two fused runs of one level
            if fuse == 1_000_000:
                assert len(plan) == 1
            F = check_factor(Mk, T, label=f"(d) fuse_rows={fuse}") if kind == "ilu0" else None
            z = check_solves(Mk, T, kind, F, r, label=f"(d) fuse_rows={fuse} context {k}")
            outs.append((kind, z, None if F is None else T.values()))
    for kind, z, f in outs[2:]:
        first = outs[0] if kind == "sgs" else outs[1]
        assert torch.equal(z, first[1]) and (f is None or torch.equal(f, first[2]))


# ------------------------------------------------------------------------------------------------ (f) GMRES(30) on the grid
@pytest.mark.parametrize("kind,near", [("ilu0", 10), ("sgs", 14), ("jacobi", 2)])
def test_f_gmres_on_the_grid(kind, near):
    M = grid()
    xs = np.cos(0.1 * np.arange(M.n))
    b = M.A @ xs
    pre, ref_pre = precond_of(M, kind)
    h = G.gmres(M, b, np.zeros(M.n), 30, prec=ref_pre, tol=0.0, max_iters=near + 12, residual_scaling=2, dtype=LD)["history"]
    tol, _ = R.choose_tol(h, near)
    ref = G.gmres(M, b, np.zeros(M.n), 30, prec=ref_pre, tol=tol, residual_scaling=2, dtype=LD)
    margins(ref["history"], tol)
    res, x = run_gmres(M, b, np.zeros(M.n), pre, 30, tol=tol)
    print(f"(f) {kind}: tol {tol:.3e}, device {res.num_iters} / {res.restarts}, restatement {ref['iterations']} / {ref['restarts']}")
    assert res.converged and res.num_iters == ref["iterations"] >= near and res.restarts == ref["restarts"]
    assert abs(res.tol - true_residual(M, b, x)) <= 1e-12


# ------------------------------------------------------------------------------------------------ (e) assembled systems
def assembled(condensation):
    def make():
        c, U = ctx(), 3
        part = system.SquarePartition(6, 3)
        # T = x and q = (1, 0), the solution of the reference's Diffusion2D test, prescribed on all four sides
        mask = part.dirichlet_mask(U, unknowns=(0, 1, 2), sides=(0, 1, 2, 3))
        mesh = system.DeviceMesh(c, part, U, mask)
        mf = system.MatrixFreeSystem(mesh, system.KERNEL_DIFFUSION2D)
        n = part.n_local_nodes * U
        exact = np.stack([part.node_coords()[:, 0], np.ones(part.n_local_nodes), np.zeros(part.n_local_nodes)], axis=1).reshape(-1)
        g = dev(np.where(mask != 0, exact, 0.0))
        asm = system.AssembledSystem(mesh, condensation=condensation)
        op = asm.begin().add(mf).end(g[None, :])
        A, P = R.from_csr(host(asm.row_ptr), host(asm.col_ind), host(asm.values))
        M = Mat.__new__(Mat)
        M.A, M.P, M.csr, M.n, M.op = A, P, (host(asm.row_ptr), host(asm.col_ind), host(asm.values)), asm.n, op
        return asm, M, host(asm.rhs[0]).copy()
    return cached(("asm", condensation), make)


@pytest.mark.parametrize("condensation", ["none", "element_boundary"])
def test_e_assembled_systems(condensation):
    """6 x 6 quads of order 3, Diffusion2D, Dirichlet values on all four sides: the plain system and the condensed one (empty
    internal rows)"""
    asm, M, b = assembled(condensation)
    active = R.active_rows(M.P)
    assert (condensation == "none") == bool(active.all()) and np.abs(M.A - M.A.T).max() <= 1e-12 * np.abs(M.A).max()
    rng = np.random.default_rng(2)
    r = rng.standard_normal(M.n)
    x0 = np.where(active, 0.0, rng.standard_normal(M.n))
    # (the Jacobi count is only compared with: float64 suffices, and its matrix products go through the BLAS)
    jac_ref = R.pcg(M, b, x0, precond_of(M, "jacobi")[1], live=active, tol=1e-9, max_iters=3000, dtype=np.float64)
    for kind in KINDS:
        T, ref_pre = precond_of(M, kind)
        assert T.info.n_active == active.sum() and T.info.n == M.n
        F = check_factor(M, T, label=f"(e) {condensation}") if kind == "ilu0" else None
        check_solves(M, T, kind, F, r, label=f"(e) {condensation}")
        # The residuals of PCG do not fall monotonically, and rounding moves them: the tolerance is placed where the restatement
        # stops at the same step with margins >= 1.5 in longdouble AND in float64
        h = R.pcg(M, b, x0, ref_pre, live=active, tol=0.0, max_iters=40)["history"]
        h64 = R.pcg(M, b, x0, R.Preconditioner(M.A, M.P, kind, dtype=np.float64), live=active, tol=0.0, max_iters=40, dtype=np.float64)["history"]
        print(f"(e) {condensation} {kind}: restatement residuals " + " ".join(f"{e:.2e}" for e in h))
        print(f"(e) {condensation} {kind}: ... in float64       " + " ".join(f"{e:.2e}" for e in h64))
        tol, its = R.choose_tol(h, near=8, also=[h64])
        margins(h, tol)
        margins(h64, tol)
        res, x = run_pcg(M, b, x0, T, tol=tol)
        n_jac = next(k + 1 for k, e in enumerate(jac_ref["history"]) if e <= tol)
        print(f"(e) {condensation} {kind}: tol {tol:.3e}, device {res.num_iters}, restatement {its}, Jacobi restatement {n_jac}")
        assert res.converged and res.num_iters == its < n_jac
        assert np.array_equal(x[~active].view(np.int64), x0[~active].view(np.int64))  # the empty rows keep x bit for bit
        assert abs(res.tol - true_residual(M, b, x, active)) <= 1e-10  # (the recurrence's residual against the true one)
        if condensation != "none" and kind == "ilu0":
            sol = dev(np.where(active, x, 0.0))
            asm.recover(sol)
            torch.cuda.synchronize()
            full = host(sol)
            assert np.array_equal(full[active], x[active]) and np.abs(full[~active]).max() > 0 and np.isfinite(full).all()


# ------------------------------------------------------------------------------------------------ (g) zero pivot
def test_g_zero_pivot():
    M = Mat(np.ones((2, 2)), np.ones((2, 2), dtype=bool))
    lib, T = capi.load(), solve.TriangularPreconditioner(M.op, "ilu0")
    assert lib.l3k_tri_factor(T._h) == -2 and "1 pivots are zero or not finite, the first at row 1" in lib.l3k_last_error().decode()
    i = T.info
    assert (i.n_bad_pivots, i.first_bad_row, i.factored) == (1, 1, 0)
    f = host(T.values())
    assert np.isfinite(f).all() and np.array_equal(f, [1.0, 1.0, 1.0, 1.0])
    r, z = dev([1.0, 2.0]), dev([0.0, 0.0])
    cres, gres = capi.CgResult(), capi.GmresResult()
    ws = solve.GmresWorkspace(ctx(), 2, 2)
    for rc in (lib.l3k_tri_apply(T._h, r.data_ptr(), z.data_ptr()), lib.l3k_tri_solve_lower(T._h, r.data_ptr(), z.data_ptr()),
               lib.l3k_tri_solve_upper(T._h, r.data_ptr(), z.data_ptr()),
               lib.l3k_csr_pcg_solve_tri(M.op._h, r.data_ptr(), z.data_ptr(), T._h, None, C.byref(cres)),
               lib.l3k_csr_gmres_solve_tri(ws._h, M.op._h, r.data_ptr(), z.data_ptr(), T._h, None, C.byref(gres))):
        assert rc == -1 and "l3k_tri_factor has not run, or its last run failed" in lib.l3k_last_error().decode()
    assert not z.any()
    S = solve.TriangularPreconditioner(M.op, "sgs")
    M.values.copy_(dev([1.0, 1.0, 1.0, 0.0]))
    assert lib.l3k_tri_factor(S._h) == -2 and "1 diagonal entries are zero or not finite, the first at row 1" in lib.l3k_last_error().decode()
    M.values.copy_(dev([1.0, 1.0, 1.0, float("inf")]))
    assert lib.l3k_tri_factor(S._h) == -2 and (S.info.n_bad_pivots, S.info.first_bad_row) == (1, 1)
    # good values: the same objects work
    M.values.copy_(dev([4.0, 1.0, 2.0, 3.0]))
    M.A = np.array([[4.0, 1.0], [2.0, 3.0]])
    for kind, obj in (("ilu0", T), ("sgs", S)):
        obj.factor()
        assert (obj.info.n_bad_pivots, obj.info.first_bad_row, obj.info.factored) == (0, -1, 1)
        F = check_factor(M, obj, label="(g)") if kind == "ilu0" else None
        check_solves(M, obj, kind, F, np.array([1.0, 2.0]), label="(g)")
    assert np.array_equal(host(T.values()), [4.0, 1.0, 0.5, 2.5])


# ------------------------------------------------------------------------------------------------ (h) thresholds and damping
def test_h_thresholds_and_damping():
    M = grid()
    r = np.cos(0.1 * np.arange(M.n))
    plain = solve.TriangularPreconditioner(M.op, "ilu0").factor().values()
    for at, rt in ((0.5, 1.0), (0.0, 1.25), (0.5, 1.25)):
        T = solve.TriangularPreconditioner(M.op, "ilu0", absolute_threshold=at, relative_threshold=rt).factor()
        F = check_factor(M, T, at, rt, label=f"(h) thresholds {at} {rt}")
        assert F[0, 0] == at + rt * 6.25 and not torch.equal(T.values(), plain)
        # the derived checks are the two bounds; against the restatement's own numbers only a gross error is looked for (a threshold
        # in the wrong place moves entries by O(1))
        ref = R.ilu0(M.A, M.P, at, rt)[0]
        assert np.abs(F - ref)[M.P].max() <= 1e-10 * np.abs(ref).max()
        pre = R.Preconditioner(M.A, M.P, "ilu0", absolute=at, relative=rt)
        z = check_solves(M, T, "ilu0", F, r, label="(h)")
        assert np.abs(host(z) - pre(r)).max() <= 1e-10 * np.abs(pre(r)).max()
    T = solve.TriangularPreconditioner(M.op, "sgs", damping=1.3).factor()
    z = check_solves(M, T, "sgs", None, r, omega=1.3, extra_upper=3, label="(h) damping 1.3")
    zr = R.Preconditioner(M.A, M.P, "sgs", 1.3)(r)
    z1 = R.Preconditioner(M.A, M.P, "sgs", 1.0)(r)
    assert np.abs(host(z) - zr).max() <= 1e-10 * np.abs(zr).max()  # (a gross-error check, as above) ...
    assert np.abs(zr - z1).max() >= 1e-3 * np.abs(zr).max()         # ... which tells omega = 1.3 from omega = 1


# ------------------------------------------------------------------------------------------------ (i) time loop and refusals
def test_i_time_loop_and_equal_bits():
    A, P = R.grid(24)
    M = Mat(A, P)
    r = dev(np.cos(0.1 * np.arange(M.n)))
    for kind in KINDS:
        T = solve.TriangularPreconditioner(M.op, kind)
        M.values.copy_(dev(M.csr[2]))
        z1, z2, z3 = (torch.empty_like(r) for _ in range(3))
        T.factor().apply(r, z1)
        f1 = T.values().clone() if kind == "ilu0" else None
        T.factor().apply(r, z2)
        assert torch.equal(z1, z2) and (f1 is None or torch.equal(f1, T.values()))
        M.values.mul_(dev(1.0 + 0.25 * np.sin(np.arange(len(M.csr[2])))))  # assembled again: new values in the same graph
        M2 = Mat.__new__(Mat)
        M2.A, M2.P, M2.csr, M2.n = R.from_csr(M.csr[0], M.csr[1], host(M.values))[0], P, (M.csr[0], M.csr[1], host(M.values)), M.n
        if kind == "sgs":  # SGS reads the off-diagonal entries live: without a new factor only the diagonal is stale
            T.apply(r, z3)
            assert not torch.equal(z3, z1)
        T.factor()
        F = check_factor(M2, T, label="(i) new values") if kind == "ilu0" else None
        z = check_solves(M2, T, kind, F, host(r), label="(i) new values")
        assert not torch.equal(z, z1)
        fresh = solve.TriangularPreconditioner(M.op, kind).factor()
        assert torch.equal(fresh.apply(r, z3), z) and (kind == "sgs" or torch.equal(fresh.values(), T.values()))


def test_i_refusals():
    lib, c = capi.load(), ctx()
    M = grid()
    h = C.c_void_p()

    def refused(rc, text):
        assert rc == -1 and text in lib.l3k_last_error().decode(), lib.l3k_last_error().decode()

    def opts(kind=1, damping=1.0, fuse=0):
        return C.byref(capi.TriOpts(kind, damping, 0.0, 1.0, fuse))

    P = R.grid(5)[1].copy()
    P[7, 7] = False
    nodiag = Mat(np.where(P, 1.0, 0.0), P)
    refused(lib.l3k_tri_create(nodiag.op._h, opts(), C.byref(h)), "l3k_tri_create: the active row 7 has no stored diagonal entry")
    refused(lib.l3k_tri_create(M.op._h, opts(kind=2), C.byref(h)), "l3k_tri_create: kind = 2")
    for w in (0.0, 2.0, -1.0, 2.5):
        refused(lib.l3k_tri_create(M.op._h, opts(kind=0, damping=w), C.byref(h)), "outside (0, 2)")
    refused(lib.l3k_tri_create(M.op._h, opts(fuse=-1), C.byref(h)), "fuse_rows = -1 is negative")
    refused(lib.l3k_tri_create(None, opts(), C.byref(h)), "l3k_tri_create: null argument")
    refused(lib.l3k_tri_create(M.op._h, opts(), None), "l3k_tri_create: null argument")
    with pytest.raises(capi.L3KError, match="kind = 'ilu'"):
        solve.TriangularPreconditioner(M.op, "ilu")
    with pytest.raises(capi.L3KError, match="takes a system.CsrOperator"):
        solve.TriangularPreconditioner(object())
    T, S = solve.TriangularPreconditioner(M.op, "ilu0"), solve.TriangularPreconditioner(M.op, "sgs").factor()
    v = torch.zeros(M.n + 8, dtype=torch.float64, device="cuda")
    refused(lib.l3k_tri_apply(T._h, v.data_ptr(), v.data_ptr() + 64), "l3k_tri_apply: nothing to solve with")
    T.factor()
    for name in ("l3k_tri_apply", "l3k_tri_solve_lower", "l3k_tri_solve_upper"):
        fn = getattr(lib, name)
        refused(fn(T._h, v.data_ptr(), v.data_ptr() + 8 * 8), name + ": the input and the output vector overlap")
        refused(fn(T._h, v.data_ptr() + 8 * (M.n - 1), v.data_ptr()), name + ": the input and the output vector overlap")
        refused(fn(T._h, None, v.data_ptr()), name + ": null argument")
        refused(fn(None, v.data_ptr(), v.data_ptr()), name + ": null argument")
    refused(lib.l3k_tri_values(S._h, v.data_ptr()), "l3k_tri_values: an SGS preconditioner has no factor values")
    refused(lib.l3k_tri_values(T._h, None), "l3k_tri_values: null argument")
    refused(lib.l3k_tri_info_get(T._h, None), "l3k_tri_info_get: null argument")
    refused(lib.l3k_tri_factor(None), "l3k_tri_factor: null argument")
    assert not v.any()
    # a tri of another operator
    twin = system.CsrOperator(c, M.row_ptr, M.col_ind, M.values)
    b, x = torch.ones(M.n, dtype=torch.float64, device="cuda"), torch.zeros(M.n, dtype=torch.float64, device="cuda")
    cres, gres = capi.CgResult(), capi.GmresResult()
    ws = solve.GmresWorkspace(c, M.n, 5)
    refused(lib.l3k_csr_pcg_solve_tri(twin._h, b.data_ptr(), x.data_ptr(), T._h, None, C.byref(cres)),
            "l3k_csr_pcg_solve_tri: the preconditioner was created for another system")
    refused(lib.l3k_csr_gmres_solve_tri(ws._h, twin._h, b.data_ptr(), x.data_ptr(), T._h, None, C.byref(gres)),
            "l3k_csr_gmres_solve_tri: the preconditioner was created for another system")
    refused(lib.l3k_csr_pcg_solve_tri(M.op._h, b.data_ptr(), x.data_ptr(), None, None, C.byref(cres)), "l3k_csr_pcg_solve_tri: null argument")
    refused(lib.l3k_csr_gmres_solve_tri(ws._h, M.op._h, b.data_ptr(), x.data_ptr(), None, None, C.byref(gres)), "l3k_csr_gmres_solve_tri: null argument")
    for fn in (solve.pcg, solve.gmres):
        with pytest.raises(capi.L3KError, match="created for another system"):
            fn(twin, b, x, precond=T)
    assert not x.any()
