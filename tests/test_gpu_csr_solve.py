"""Solves on the device CSR operator: the assembled system (assemble_global -> dirichlet -> jacobi_inverse -> pcg) and the condensed one
(condense_global -> dirichlet -> pcg -> recover_internal) on the perturbed cube of test_gpu_condensation.py, the Chebyshev-Jacobi
preconditioner on a CSR operator, several right-hand sides, reproducibility, and the CSR apply against the matrix-free one.

Bounds: the iteration count is held to the longdouble PCG of cg_ref on the dense copy of the same matrix (+-1), achieved_tol to
the true residual of the returned x (1e-12), and the error against a direct solve to the perturbation bound
||x - x*|| / ||x*|| <= cond(A) (||b - A x|| / ||b|| + n EPS) -- n EPS stands for the direct solve's own backward error."""
import numpy as np
import pytest
import torch

import cg_ref
from cg_ref import EPS, LD
from l3ster_amd import solve, system

pytestmark = pytest.mark.gpu
KID, U, KPAR = system.KERNEL_DIFFUSION3D, 4, [0.7, 1.3]
TOL = 1e-12
_CASES = {}


def dev(a, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


def full_graph(part):
    import scipy.sparse as sp
    dofs = (part.elem_nodes.astype(np.int64)[:, :, None] * U + np.arange(U)).reshape(part.n_elems, -1)
    nd = dofs.shape[1]
    n = part.n_local_nodes * U
    G = sp.coo_matrix((np.ones(part.n_elems * nd * nd), (np.repeat(dofs, nd, axis=1).ravel(), np.tile(dofs, (1, nd)).ravel())),
                      shape=(n, n)).tocsr()
    G.sort_indices()
    return G.indptr.astype(np.int64), G.indices.astype(np.int32)


def dense_of(op):
    import scipy.sparse as sp
    return sp.csr_matrix((op.values.cpu().numpy(), op.col_ind.cpu().numpy(), op.row_ptr.cpu().numpy()), shape=(op.n, op.n)).toarray()


def case(ne, p):
    """The setup of test_gpu_condensation.py::test_condensed_solve_and_recovery_match_full_solve, and on it the assembled system
    with its Dirichlet conditions applied, as a CsrOperator, a dense copy and a direct solve.  Once per module."""
    if (ne, p) in _CASES:
        return _CASES[ne, p]
    torch.cuda.set_device(0)
    ctx = system.Context(0, torch.cuda.current_stream().cuda_stream)  # (not in deterministic mode)
    part = system.CubePartition(ne, p, perturb=0.15)
    mask = part.dirichlet_mask(U)
    mf = system.MatrixFreeSystem(system.DeviceMesh(ctx, part, U, mask), KID, KPAR, asm_opts=(1, 0, 0), n_rhs=1)
    n = part.n_local_nodes * U
    dmask = np.asarray(mask).astype(bool).ravel()[:n]
    g = np.where(dmask, np.sin(np.arange(n) * 0.37), 0.0)
    row_ptr, col_ind = full_graph(part)
    RP, CI = torch.as_tensor(row_ptr, device="cuda"), torch.as_tensor(col_ind, device="cuda")
    vals = torch.zeros(len(col_ind), dtype=torch.float64, device="cuda")
    rhs = torch.zeros((1, n), dtype=torch.float64, device="cuda")
    assert mf.assemble_global(RP, CI, vals, rhs, skip_dirichlet=False) == 0
    op = system.CsrOperator(ctx, RP, CI, vals)
    M, G = dev(dmask.astype(np.uint8), torch.uint8), dev(g[None, :])
    op.dirichlet(M, G, rhs)
    minv = op.jacobi_inverse()
    A = dense_of(op)
    assert np.abs(A - A.T).max() <= 1e-12 * np.abs(A).max()
    b = rhs[0].cpu().numpy()
    c = dict(ctx=ctx, part=part, mf=mf, n=n, dmask=dmask, g=g, M=M, G=G, op=op, minv=minv, b=rhs[0], A=A, b_host=b,
             x_direct=np.linalg.solve(A, b), cond=float(np.linalg.cond(A)))
    _CASES[ne, p] = c
    return c


def true_residual(A, b, x, rows=slice(None)):
    r = (b.astype(LD) - A.astype(LD) @ x.astype(LD))[rows]
    return float(np.sqrt(np.sum(r * r)) / np.sqrt(np.sum(b.astype(LD) ** 2)))


def rel(x, ref):
    return float(np.linalg.norm(x - ref) / np.linalg.norm(ref))


def test_assembled_system_pcg():
    c = case(3, 2)
    n, A, b = c["n"], c["A"], c["b_host"]
    assert n == 1372
    assert np.array_equal(A[c["dmask"]], np.eye(n)[c["dmask"]]) and np.array_equal(b[c["dmask"]], c["g"][c["dmask"]])
    x = torch.zeros(n, dtype=torch.float64, device="cuda")
    res = solve.pcg(c["op"], c["b"], x, c["minv"], tol=TOL, residual_scaling="rhs")
    xh = x.cpu().numpy()
    # the iteration count of the same recurrence in longdouble on the dense copy of the same matrix
    minv = c["minv"].cpu().numpy()
    assert np.array_equal(minv, cg_ref.jacobi_inverse_ref(np.diag(A)))
    _, _, steps, init = cg_ref.pcg_ref(A, b, np.zeros(n), minv, res.num_iters + 5)
    bb = float(np.sqrt(np.sum(b.astype(LD) ** 2)))
    hist = [float(np.sqrt(init["rr"])) / bb] + [float(np.sqrt(s["rr"])) / bb for s in steps]
    ref_iters = next(k for k, r in enumerate(hist) if r <= TOL)
    true = true_residual(A, b, xh)
    err = rel(xh, c["x_direct"])
    print(f"assembled: iterations device {res.num_iters} longdouble {ref_iters}, achieved {res.tol:.3e}, true residual {true:.3e}, "
          f"error against the direct solve {err:.3e}, bound {c['cond'] * (true + n * EPS):.3e} (cond {c['cond']:.3e})")
    assert res.converged and abs(res.num_iters - ref_iters) <= 1
    assert abs(true - res.tol) <= 1e-12
    assert err <= c["cond"] * (true + n * EPS)
    c["x_assembled"] = xh


@pytest.mark.parametrize("ne,p", [(3, 2), (2, 4)])
def test_condensed_system_pcg_and_recovery(ne, p):
    c = case(ne, p)
    n, mf, part = c["n"], c["mf"], c["part"]
    xa = torch.zeros(n, dtype=torch.float64, device="cuda")
    ra = solve.pcg(c["op"], c["b"], xa, c["minv"], tol=TOL, residual_scaling="rhs")
    assert ra.converged
    x_asm = xa.cpu().numpy()
    row_ptr, col_ind = system.condensed_graph(part.elem_nodes, p, U, np.arange(U))
    RP, CI = torch.as_tensor(row_ptr, device="cuda"), torch.as_tensor(col_ind, device="cuda")
    vals = torch.zeros(len(col_ind), dtype=torch.float64, device="cuda")
    rhs = torch.zeros((1, n), dtype=torch.float64, device="cuda")
    assert mf.condense_global(RP, CI, vals, rhs) == 0
    op = system.CsrOperator(c["ctx"], RP, CI, vals)
    op.dirichlet(c["M"], c["G"], rhs)
    minv = op.jacobi_inverse()
    empty = np.diff(row_ptr) == 0
    _, internal = system.element_node_split(p)
    i_dofs = np.unique((part.elem_nodes[:, internal].astype(np.int64)[:, :, None] * U + np.arange(U)).ravel())
    assert empty.sum() == op.info().n_empty_rows == len(i_dofs) and empty[i_dofs].all()
    assert not minv.cpu().numpy()[empty].any() and minv.cpu().numpy()[~empty].all()
    # frozen rows keep what they start with: sentinels, untouched until the recovery overwrites them
    x0 = np.where(empty, 1000.0 + np.arange(n), 0.0)
    X = dev(x0[None, :])
    res = solve.pcg(op, rhs[0], X[0], minv, tol=TOL, residual_scaling="rhs")
    assert res.converged
    xc = X.cpu().numpy()[0]
    assert np.array_equal(xc[empty], x0[empty])
    S, f = dense_of(op), rhs[0].cpu().numpy()
    live = np.flatnonzero(~empty)
    true = true_residual(S, f, xc, live)
    assert abs(true - res.tol) <= 1e-12
    mf.recover_internal(X)
    torch.cuda.synchronize()
    x = X.cpu().numpy()[0]
    cond = float(np.linalg.cond(S[np.ix_(live, live)]))
    err, bound = rel(x, x_asm), cond * (true + n * EPS)
    print(f"condensed ne {ne} p {p}: iterations {res.num_iters} (assembled {ra.num_iters}), true residual {true:.3e}, against the "
          f"assembled solve {err:.3e} (primary dofs {rel(x[live], x_asm[live]):.3e}), bound {bound:.3e} (cond {cond:.3e})")
    assert np.isfinite(x).all() and err <= bound


def test_chebyshev_on_a_csr_operator():
    c = case(3, 2)
    op, minv, n = c["op"], c["minv"], c["n"]
    cheb = solve.ChebyshevPreconditioner(op, minv, degree=3, cond_est=30.0)
    info = cheb.info
    assert info.power_iters == 10 and info.applies_per_call == 2 and 0.0 < info.lambda_est < info.lambda_max
    r = dev(np.random.default_rng(8).standard_normal(n))
    z = torch.empty_like(r)
    cheb.apply(r, z)
    want = solve.chebyshev_reference(lambda v, out: op.apply(v, out), minv, r, info.lambda_max, 30.0, 3)
    err = float((z - want).norm() / want.norm())
    print(f"CSR Chebyshev degree 3: device against the torch restatement {err:.3e}")
    assert err <= 1e-13 and float(z.norm()) > 0.0
    xj, xc = torch.zeros_like(c["b"]), torch.zeros_like(c["b"])
    rj = solve.pcg(op, c["b"], xj, minv, tol=TOL, residual_scaling="rhs")
    rc = solve.pcg(op, c["b"], xc, precond=cheb, tol=TOL, residual_scaling="rhs")
    true = true_residual(c["A"], c["b_host"], xc.cpu().numpy())
    err = rel(xc.cpu().numpy(), c["x_direct"])
    print(f"outer iterations Chebyshev {rc.num_iters}, Jacobi {rj.num_iters}; error {err:.3e}, bound {c['cond'] * (true + n * EPS):.3e}")
    assert rc.converged and rj.converged and rc.num_iters < rj.num_iters
    assert err <= c["cond"] * (true + n * EPS)
    assert rel(xc.cpu().numpy(), xj.cpu().numpy()) <= c["cond"] * (true + true_residual(c["A"], c["b_host"], xj.cpu().numpy()) + n * EPS)
    # a preconditioner of another operator is refused
    other = system.CsrOperator(c["ctx"], op.row_ptr, op.col_ind, op.values)
    with pytest.raises(system.L3KError, match="the preconditioner was created for another system"):
        solve.pcg(other, c["b"], torch.zeros_like(xc), precond=cheb)
    import ctypes as C
    lib, result, x0 = system.capi.load(), system.capi.CgResult(), torch.zeros_like(xc)
    assert lib.l3k_csr_pcg_solve_cheb(other._h, C.c_void_p(c["b"].data_ptr()), C.c_void_p(x0.data_ptr()), cheb._h, None, C.byref(result)) == -1
    assert lib.l3k_last_error().decode() == "l3k_csr_pcg_solve_cheb: the preconditioner was created for another system"
    assert not x0.any()


def test_columns_equal_single_solves_and_solves_are_reproducible():
    c = case(3, 2)
    op, minv, n, b = c["op"], c["minv"], c["n"], c["b"]
    ld = n + 4
    B = torch.zeros((3, ld), dtype=torch.float64, device="cuda")
    B[0, :n], B[1, :n], B[2, :n] = b, 2.0 * b, dev(np.cos(np.arange(n) * 0.11))
    X = torch.zeros_like(B)
    out = solve.pcg(op, B, X, minv, tol=TOL, residual_scaling="rhs")
    assert len(out) == 3 and all(r.converged for r in out)
    for k in range(3):
        xs, xs2 = torch.zeros(n, dtype=torch.float64, device="cuda"), torch.zeros(n, dtype=torch.float64, device="cuda")
        bk = B[k, :n].contiguous()
        r1 = solve.pcg(op, bk, xs, minv, tol=TOL, residual_scaling="rhs")
        r2 = solve.pcg(op, bk, xs2, minv, tol=TOL, residual_scaling="rhs")
        assert torch.equal(xs, xs2) and (r1.num_iters, r1.tol) == (r2.num_iters, r2.tol)  # two solves: bit for bit
        assert torch.equal(X[k, :n], xs) and (out[k].num_iters, out[k].tol) == (r1.num_iters, r1.tol)
    assert not X[:, n:].any()


def test_csr_apply_agrees_with_the_matrix_free_apply_on_the_free_dofs():
    c = case(3, 2)
    mf, n = c["mf"], c["n"]
    RP, CI = c["op"].row_ptr, c["op"].col_ind
    vals = torch.zeros(CI.numel(), dtype=torch.float64, device="cuda")
    assert mf.assemble_global(RP, CI, vals, None, skip_dirichlet=True) == 0
    op = system.CsrOperator(c["ctx"], RP, CI, vals)
    x = dev(np.random.default_rng(4).standard_normal(n))
    y_mf, y_csr = torch.empty_like(x), torch.empty_like(x)
    mf.apply(x[None, :], y_mf[None, :])
    op.apply(x, y_csr)
    free = dev(~c["dmask"], torch.bool)
    err = float((y_mf[free] - y_csr[free]).norm() / y_mf[free].norm())
    print(f"CSR apply against the matrix-free apply on the free dofs: {err:.3e}")
    assert err <= 1e-11 and not y_csr[~free].any()
