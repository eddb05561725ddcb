"""The p-multigrid preconditioner on the device (l3k_pmg_*, l3k_pcg_solve_pmg) against the CPU restatement of tests/pmg_ref.py: the
transfer kernels against the dense P and P^T of the ownership rule, Dirichlet masks, element maps, the grid-stride walk, the
V-cycle and the PCG on it, quads, and the error paths.  Shapes are the smallest with shared faces, edges and vertices and more
than one owner decision (2 x 2 x 2 and 3 x 2 x 2 elements)."""
import ctypes as C

import numpy as np
import pytest
import torch

import pmg_ref as R
from l3ster_amd import capi, solve, system

pytestmark = pytest.mark.gpu
D3, D2, ADV = system.KERNEL_DIFFUSION3D, system.KERNEL_DIFFUSION2D, system.KERNEL_ADVECTION3D
ORDER_PAIRS = [(2, 1), (3, 1), (4, 2), (6, 3), (8, 4)]
_CTX, _PAIRS, _H = {}, {}, {}


def ctx(deterministic=False):
    if deterministic not in _CTX:
        torch.cuda.set_device(0)
        c = system.Context(0, torch.cuda.current_stream().cuda_stream)
        if deterministic:
            c.set_deterministic(True)
        _CTX[deterministic] = c
    return _CTX[deterministic]


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(np.asarray(b)), 1e-300))


def transfer_level(c, part, U, mask):
    """an operator and a (never applied) smoother on `part`: what a level needs where only the transfers are called"""
    kid, kpar = (ADV, [1.0]) if U == 1 else (D2, None) if part.dim == 2 else (D3, [1.0, 0.0])
    mf = system.MatrixFreeSystem(system.DeviceMesh(c, part, U, mask), kid, kpar)
    minv = torch.ones(part.n_owned_nodes * U, dtype=torch.float64, device="cuda")
    return mf, solve.ChebyshevPreconditioner(mf, minv, degree=1, lambda_max=1.0)


def make_part(ne, p, perturb):
    return system.SquarePartition(ne, p, perturb=perturb) if len(ne) == 2 else system.CubePartition(ne, p, perturb=perturb)


def pair(ne, pf, pc, U, deterministic=False, masks=False, perturb=0.1, permute=False, bad_map=False):
    """A level pair on the device and its node-level dense P on the host"""
    key = (ne, pf, pc, U, deterministic, masks, perturb, permute)
    if key in _PAIRS and not bad_map:
        return _PAIRS[key]
    c = ctx(deterministic)
    fine, coarse = make_part(ne, pf, perturb), make_part(ne, pc, perturb)
    if permute:
        perm = np.random.default_rng(8).permutation(coarse.n_elems)
        coarse.elem_nodes, coarse.elem_verts = coarse.elem_nodes[perm], coarse.elem_verts[perm]
    emap = system.match_elements(fine, coarse)
    if bad_map:
        emap = np.arange(fine.n_elems, dtype=np.int64) if emap is None else emap.copy()
        emap[[1, 2]] = emap[[2, 1]]
    mf_mask = fine.dirichlet_mask(U) if masks else None
    mc_mask = coarse.dirichlet_mask(U) if masks else None
    lf, lc = transfer_level(c, fine, U, mf_mask), transfer_level(c, coarse, U, mc_mask)
    pm = solve.PMultigrid([lf + (None,), lc + (emap,)])
    out = dict(pm=pm, fine=fine, coarse=coarse, U=U, emap=emap, mask_f=mf_mask, mask_c=mc_mask,
               Pn=R.node_prolongation(fine, coarse, emap), nf=fine.n_owned_nodes * U, nc=coarse.n_owned_nodes * U)
    if not bad_map:
        _PAIRS[key] = out
    return out


def P_times(q, xc):
    """dense P x_c with the masks of the pair (every component alike)"""
    U = q["U"]
    xc = np.where(q["mask_c"].astype(bool), 0.0, xc) if q["mask_c"] is not None else xc
    out = (q["Pn"] @ xc.reshape(-1, U)).reshape(-1)
    return np.where(q["mask_f"].astype(bool), 0.0, out) if q["mask_f"] is not None else out


def Pt_times(q, rf):
    U = q["U"]
    rf = np.where(q["mask_f"].astype(bool), 0.0, rf) if q["mask_f"] is not None else rf
    out = (q["Pn"].T @ rf.reshape(-1, U)).reshape(-1)
    return np.where(q["mask_c"].astype(bool), 0.0, out) if q["mask_c"] is not None else out


def vectors(q, seed=1):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(q["nc"]), rng.standard_normal(q["nf"])


# ------------------------------------------------------------------------------------------------ 1. the transfers
@pytest.mark.parametrize("U", [1, 4])
@pytest.mark.parametrize("pf,pc", ORDER_PAIRS)
@pytest.mark.parametrize("ne", [(2, 2, 2), (3, 2, 2)])
def test_transfers_equal_the_dense_matrices(ne, pf, pc, U):
    """x_f = P x_c and r_c = P^T r_f against the dense matrices of the ownership rule, relative L2 <= 1e-12 (the element-level bar:
    a transfer is one element's sweeps, no mesh-level accumulation of rounding beyond the 2^dim owners of a coarse node); the
    prolongation bit for bit on two runs; <P^T r, v> = <r, P v> with the device's own two kernels"""
    q = pair(ne, pf, pc, U)
    xc, rf = vectors(q)
    d_xc, d_rf = dev(xc), dev(rf)
    xf = [torch.full((q["nf"],), 7.0, dtype=torch.float64, device="cuda") for _ in range(2)]
    for t in xf:
        q["pm"].prolong(1, d_xc, t)
    e_p = rel(xf[0].cpu().numpy(), P_times(q, xc))
    d_rc = torch.full((q["nc"],), float("nan"), dtype=torch.float64, device="cuda")  # (zeroed by the call)
    q["pm"].restrict(1, d_rf, d_rc)
    e_r = rel(d_rc.cpu().numpy(), Pt_times(q, rf))
    lhs, rhs = float(torch.dot(d_rc, d_xc)), float(torch.dot(d_rf, xf[0]))
    print(f"{ne} {pf}->{pc} U={U}: prolongation {e_p:.2e}, restriction {e_r:.2e}, adjoint {abs(lhs - rhs):.2e}")
    assert e_p <= 1e-12 and e_r <= 1e-12
    assert torch.equal(xf[0], xf[1])
    assert abs(lhs - rhs) <= 1e-12 * float(d_rf.norm()) * float(d_xc.norm())
    # x_f += P x_c
    acc = dev(rf)
    q["pm"].prolong(1, d_xc, acc, add=True)
    assert rel(acc.cpu().numpy(), rf + P_times(q, xc)) <= 1e-12


@pytest.mark.parametrize("pf,pc,U", [(4, 2, 4), (3, 1, 1)])
def test_restriction_is_bitwise_reproducible_on_a_deterministic_context(pf, pc, U):
    q = pair((3, 2, 2), pf, pc, U, deterministic=True)
    _, rf = vectors(q, 2)
    d_rf = dev(rf)
    out = [torch.empty(q["nc"], dtype=torch.float64, device="cuda") for _ in range(2)]
    for t in out:
        q["pm"].restrict(1, d_rf, t)
    assert torch.equal(out[0], out[1])
    assert rel(out[0].cpu().numpy(), Pt_times(q, rf)) <= 1e-12


@pytest.mark.parametrize("pf,pc", [(3, 1), (4, 2), (8, 4)])
def test_prolongation_is_exact_for_polynomials_of_the_coarse_degree(pf, pc):
    """unperturbed mesh (affine elements): a polynomial of total degree <= p_c at the coarse nodes arrives as itself at the fine ones"""
    q = pair((3, 2, 2), pf, pc, 1, perturb=0.0)
    f = lambda x: (0.3 + x[:, 0] - 0.7 * x[:, 1] + 0.4 * x[:, 2]) ** pc
    xf = torch.empty(q["nf"], dtype=torch.float64, device="cuda")
    q["pm"].prolong(1, dev(f(q["coarse"].node_coords())), xf)
    want = f(q["fine"].node_coords())
    err = rel(xf.cpu().numpy(), want)
    print(f"{pf}->{pc}: polynomial of degree {pc}: {err:.2e}")
    assert err <= 1e-12


@pytest.mark.parametrize("ne,pf,pc", [((2, 2, 2), 4, 2), ((3, 2, 2), 3, 1)])
def test_dirichlet_masks_and_what_must_not_be_read(ne, pf, pc):
    q = pair(ne, pf, pc, 4, masks=True)
    mf, mc = q["mask_f"].astype(bool), q["mask_c"].astype(bool)
    assert mf.any() and mc.any()
    xc, rf = vectors(q, 3)
    xc_nan, rf_nan = xc.copy(), rf.copy()
    xc_nan[mc] = np.nan  # a masked coarse dof
    rf_nan[mf] = np.nan  # a masked fine dof
    xf = torch.empty(q["nf"], dtype=torch.float64, device="cuda")
    q["pm"].prolong(1, dev(xc_nan), xf)
    got = xf.cpu().numpy()
    assert np.isfinite(got).all() and np.abs(got[mf]).max() == 0.0
    assert rel(got, P_times(q, xc)) <= 1e-12
    rc = torch.empty(q["nc"], dtype=torch.float64, device="cuda")
    q["pm"].restrict(1, dev(rf_nan), rc)
    got = rc.cpu().numpy()
    assert np.isfinite(got).all() and np.abs(got[mc]).max() == 0.0
    assert rel(got, Pt_times(q, rf)) <= 1e-12


def test_restriction_reads_every_fine_node_once():
    """a node on a shared face is read by its owner only: with r_f = 1 the sum of P^T r_f is the number of fine nodes (P's rows sum
    to 1), not the number of (element, node) pairs"""
    q = pair((3, 2, 2), 4, 2, 1)
    rc = torch.empty(q["nc"], dtype=torch.float64, device="cuda")
    q["pm"].restrict(1, torch.ones(q["nf"], dtype=torch.float64, device="cuda"), rc)
    assert abs(float(rc.sum()) - q["nf"]) <= 1e-10 * q["nf"]


@pytest.mark.parametrize("pf,pc", [(4, 2), (3, 1)])
def test_element_map(pf, pc):
    a, b = pair((3, 2, 2), pf, pc, 4), pair((3, 2, 2), pf, pc, 4, permute=True)
    assert b["emap"] is not None
    xc, rf = vectors(a, 4)
    # (the coarse NODE numbering does not depend on the order of the elements: the same vectors serve both)
    outs = []
    for q in (a, b):
        xf = torch.empty(q["nf"], dtype=torch.float64, device="cuda")
        rc = torch.empty(q["nc"], dtype=torch.float64, device="cuda")
        q["pm"].prolong(1, dev(xc), xf)
        q["pm"].restrict(1, dev(rf), rc)
        outs.append((xf.cpu().numpy(), rc.cpu().numpy()))
    assert np.array_equal(outs[0][0], outs[1][0])
    assert rel(outs[1][1], outs[0][1]) <= 1e-12
    with pytest.raises(capi.L3KError, match=r"fine element 1 and its coarse partner have different vertices"):
        pair((3, 2, 2), pf, pc, 4, bad_map=True)


def test_more_elements_than_workgroups():
    """the grid-stride walk: with one wave per CU in the tuning a launch has CUs / 4 workgroups; the mesh has more elements"""
    c = ctx()
    g = max(1, torch.cuda.get_device_properties(0).multi_processor_count // 4)
    ne = next((a, b, 4) for a in range(1, 64) for b in range(1, a + 1) if g < 4 * a * b < 3 * g and (4 * a * b) % g)
    with c.tuning(waves_per_cu=1):
        q = pair(ne, 2, 1, 4)
        assert q["fine"].n_elems > g
        xc, rf = vectors(q, 5)
        xf = torch.empty(q["nf"], dtype=torch.float64, device="cuda")
        rc = torch.empty(q["nc"], dtype=torch.float64, device="cuda")
        q["pm"].prolong(1, dev(xc), xf)
        q["pm"].restrict(1, dev(rf), rc)
        assert rel(xf.cpu().numpy(), P_times(q, xc)) <= 1e-12 and rel(rc.cpu().numpy(), Pt_times(q, rf)) <= 1e-12


def test_quads_transfer_parity():
    q = pair((3, 3), 4, 2, 3, masks=True)
    xc, rf = vectors(q, 6)
    xf = torch.empty(q["nf"], dtype=torch.float64, device="cuda")
    rc = torch.empty(q["nc"], dtype=torch.float64, device="cuda")
    q["pm"].prolong(1, dev(xc), xf)
    q["pm"].restrict(1, dev(rf), rc)
    assert rel(xf.cpu().numpy(), P_times(q, xc)) <= 1e-12 and rel(rc.cpu().numpy(), Pt_times(q, rf)) <= 1e-12


# ------------------------------------------------------------------------------------------------ 2. the cycle and the PCG
def hierarchy(ne, orders, dim=3):
    """the restated hierarchy (oracle operators as callables) and its twin on the device with the same lambda_max per level"""
    key = (ne, orders, dim)
    if key in _H:
        return _H[key]
    levels, Ps, data, maps = R.hierarchy(ne, orders, dim)
    c = ctx()
    dl = []
    for i, (L, d) in enumerate(zip(levels, data)):
        mf = system.MatrixFreeSystem(system.DeviceMesh(c, d["part"], d["U"], d["mask"]), d["kernel_id"], d["kparams"])
        diag, rhs = mf.diag_rhs(dev(d["g"]))
        minv = solve.jacobi_inverse_native(c, diag)
        cheb = solve.ChebyshevPreconditioner(mf, minv, degree=L.degree, cond_est=L.cond_est, lambda_max=L.lambda_max)
        dl.append((mf, cheb, maps[i - 1] if i else None))
        if i == 0:
            b = rhs[0].contiguous()
    _H[key] = dict(levels=levels, Ps=Ps, data=data, dev=dl, pm=solve.PMultigrid(dl), b=b, n=data[0]["diag"].size)
    return _H[key]


@pytest.mark.parametrize("orders", [(4, 2, 1), (6, 3, 1)])
def test_vcycle_matches_the_restatement(orders):
    H = hierarchy(2, orders)
    info = H["pm"].info()
    assert info.order == list(orders) and info.n_dofs == [d["diag"].size for d in H["data"]]
    assert info.applies_per_cycle == [2 * (R.SMOOTH["degree"] - 1) + 2] * 2 + [R.COARSE["degree"] - 1]
    rng = np.random.default_rng(21)
    u, v = rng.standard_normal(H["n"]), rng.standard_normal(H["n"])
    zu, zv = (torch.empty(H["n"], dtype=torch.float64, device="cuda") for _ in range(2))
    H["pm"].apply(dev(u), zu)
    H["pm"].apply(dev(v), zv)
    want = R.vcycle(H["levels"], H["Ps"], torch.as_tensor(u)).numpy()
    err = rel(zu.cpu().numpy(), want)
    sym = abs(float(torch.dot(dev(u), zv)) - float(torch.dot(zu, dev(v)))) / (np.linalg.norm(u) * float(zv.norm()))
    print(f"orders {orders}: V-cycle against the restatement {err:.2e}, device symmetry {sym:.2e}")
    assert err <= 1e-11
    assert sym <= 1e-11


def test_pcg_with_pmultigrid():
    """3^3 elements of order 4, Diffusion3D, levels 4 -> 2 -> 1.  Stopping test of all three solves (device Jacobi, device
    p-multigrid, restatement): the solver's default, residual_scaling="none", i.e. the plain norm |r| <= 1e-10.  Measured on the
    device: Jacobi 573 iterations, p-multigrid 74, the restatement 74, the two device solutions 1.3e-9 of |x| apart.
    Why not residual_scaling="rhs", which tests/test_pmg_cpu.py uses for its iteration counts: |b| = 18.8 here, so |r| <= 1e-10 |b|
    stops both solves 18.8 times earlier, and the two solutions are then 2.4e-8 of |x| apart -- above the 1e-8 this test must
    hold.  That distance is the error a solve stopped at that residual is left with (the Jacobi solve's, mostly), not an error of
    the preconditioner; the plain norm is the tighter of the two tests, and with it the bound holds with a factor 7 to spare."""
    H = hierarchy(3, (4, 2, 1))
    mf, cheb0, n, b = H["dev"][0][0], H["dev"][0][1], H["n"], H["b"]
    kw = dict(tol=1e-10)
    xj, xm = (torch.zeros(n, dtype=torch.float64, device="cuda") for _ in range(2))
    rj = solve.pcg(mf, b, xj, cheb0.minv, **kw)
    rm = solve.pcg(mf, b, xm, precond=H["pm"], **kw)
    x_ref = torch.zeros(n, dtype=torch.float64)
    rr = R.pcg(H["levels"], H["Ps"], torch.as_tensor(H["data"][0]["rhs"]), x_ref, **kw)
    diff = float((xm - xj).norm() / xj.norm())
    print(f"3^3 order 4: iterations Jacobi {rj.num_iters}, p-multigrid device {rm.num_iters}, restatement {rr.num_iters}; "
          f"|x_pmg - x_jacobi| / |x_jacobi| = {diff:.2e}, against the restatement {rel(xm.cpu().numpy(), x_ref.numpy()):.2e}")
    assert rj.converged and rm.converged and rr.converged
    assert diff <= 1e-8
    assert abs(rm.num_iters - rr.num_iters) <= 1
    assert rm.num_iters < rj.num_iters
    # max_iters and check_every as in l3k_pcg_solve_cheb
    x = torch.zeros(n, dtype=torch.float64, device="cuda")
    r3 = solve.pcg(mf, b, x, precond=H["pm"], max_iters=3, throw_on_fail=False, **kw)
    assert r3.num_iters == 3 and not r3.converged
    x = torch.zeros(n, dtype=torch.float64, device="cuda")
    r5 = solve.pcg(mf, b, x, precond=H["pm"], check_every=5, **kw)
    assert r5.converged and r5.num_iters % 5 == 0 and rm.num_iters <= r5.num_iters < rm.num_iters + 5
    with pytest.raises(capi.L3KError, match="created for another system"):
        solve.pcg(H["dev"][1][0], b, x, precond=H["pm"], **kw)


def test_pcg_frozen_rows_keep_x():
    """rows frozen by level 0's smoother (minv == 0): x keeps its value there, the others are solved for"""
    H = hierarchy(2, (4, 2, 1))
    (mf, cheb0, _), n, c = H["dev"][0], H["n"], ctx()
    minv = cheb0.minv.clone()
    frozen = torch.zeros(n, dtype=torch.bool, device="cuda")
    frozen[5::11] = True
    minv[frozen] = 0.0
    i0 = cheb0.info
    cheb = solve.ChebyshevPreconditioner(mf, minv, degree=i0.degree, cond_est=R.SMOOTH["cond_est"], lambda_max=i0.lambda_max)
    pm = solve.PMultigrid([(mf, cheb, None)] + H["dev"][1:])
    x = dev(np.random.default_rng(9).standard_normal(n))
    x0 = x.clone()
    res = solve.pcg(mf, H["b"], x, precond=pm, tol=1e-9, residual_scaling="rhs")
    assert res.converged and torch.equal(x[frozen], x0[frozen]) and not torch.equal(x[~frozen], x0[~frozen])
    z = torch.empty(n, dtype=torch.float64, device="cuda")
    pm.apply(x0, z)
    assert float(z[frozen].abs().max()) == 0.0 and float(z.abs().max()) > 0.0


def test_quads_pcg_with_pmultigrid():
    H = hierarchy(3, (4, 2, 1), dim=2)
    mf, cheb0, n, b = H["dev"][0][0], H["dev"][0][1], H["n"], H["b"]
    kw = dict(tol=1e-10)
    xj, xm = (torch.zeros(n, dtype=torch.float64, device="cuda") for _ in range(2))
    rj = solve.pcg(mf, b, xj, cheb0.minv, **kw)
    rm = solve.pcg(mf, b, xm, precond=H["pm"], **kw)
    u = np.random.default_rng(22).standard_normal(n)
    z = torch.empty(n, dtype=torch.float64, device="cuda")
    H["pm"].apply(dev(u), z)
    err = rel(z.cpu().numpy(), R.vcycle(H["levels"], H["Ps"], torch.as_tensor(u)).numpy())
    print(f"quads 3^2 order 4: iterations Jacobi {rj.num_iters}, p-multigrid {rm.num_iters}; V-cycle against the restatement {err:.2e}")
    assert err <= 1e-11
    assert rj.converged and rm.converged and rm.num_iters < rj.num_iters
    assert float((xm - xj).norm() / xj.norm()) <= 1e-8


# ------------------------------------------------------------------------------------------------ 3. errors
def test_error_paths():
    lib, c = capi.load(), ctx()
    q = pair((2, 2, 2), 4, 2, 4)
    pm, (f, fc, _), (co, cc, _) = q["pm"], q["pm"].levels[0], q["pm"].levels[1]
    out, res = C.c_void_p(), capi.CgResult()

    def create(levels, n=None, context=None):
        arr = (capi.PmgLevel * len(levels))()
        for a, (mf, cheb, m) in zip(arr, levels):
            a.mf, a.smoother, a.d_elem_map = mf and mf._h, cheb and cheb._h, m
        return lib.l3k_pmg_create((context or c)._h, len(levels) if n is None else n, arr, C.byref(out))

    def refused(rc, text):
        assert rc == -1 and text in lib.l3k_last_error().decode(), lib.l3k_last_error().decode()

    refused(create([(f, fc, None), (co, None, None)]), "null argument")
    refused(create([(f, fc, None)]), "n_levels must lie in 2 .. 8")
    other = system.Context(0, torch.cuda.current_stream().cuda_stream)
    refused(create([(f, fc, None), (co, cc, None)], context=other), "another context")
    refused(create([(f, cc, None), (co, cc, None)]), "smoother of level 0 was created for another system")
    refused(create([(co, cc, None), (f, fc, None)]), "decrease strictly")
    refused(create([(f, fc, None), (f, fc, None)]), "decrease strictly")
    part = system.CubePartition((2, 2, 2), 4, parts=(2, 1, 1), rank=1, perturb=0.1)  # (rank 0 owns the shared nodes)
    assert part.n_ghost_nodes > 0
    gm = system.MatrixFreeSystem(system.DeviceMesh(c, part, 4, None), D3, [1.0, 0.0])
    refused(create([(gm, fc, None), (co, cc, None)]), "ghost nodes")
    other_mesh = pair((3, 2, 2), 2, 1, 4)["pm"].levels[1]
    refused(create([(f, fc, None), (other_mesh[0], other_mesh[1], None)]), "not one mesh at two orders")
    far = torch.full((q["fine"].n_elems,), 99, dtype=torch.int64, device="cuda")
    refused(create([(f, fc, None), (co, cc, far.data_ptr())]), "fine element 0 is mapped outside the coarse mesh")
    twice = torch.zeros(q["fine"].n_elems, dtype=torch.int64, device="cuda")
    refused(create([(f, fc, None), (co, cc, twice.data_ptr())]), "fine element 1 is mapped to a coarse element that an earlier one")
    v = torch.zeros(q["nf"] + 8, dtype=torch.float64, device="cuda")
    refused(lib.l3k_pmg_apply(pm._h, v.data_ptr(), v.data_ptr() + 32), "r and z overlap")
    for level in (0, 2, -1):
        refused(lib.l3k_pmg_prolong(pm._h, level, v.data_ptr(), v.data_ptr(), 0), "outside [1, 2)")
        refused(lib.l3k_pmg_restrict(pm._h, level, v.data_ptr(), v.data_ptr()), "outside [1, 2)")
    refused(lib.l3k_pcg_solve_pmg(co._h, v.data_ptr(), v.data_ptr(), pm._h, None, C.byref(res)), "created for another system")
    refused(lib.l3k_pcg_solve_pmg(f._h, None, v.data_ptr(), pm._h, None, C.byref(res)), "null argument")
    with pytest.raises(capi.L3KError, match="distinct vectors"):
        pm.apply(v[:q["nf"]], v[:q["nf"]])
