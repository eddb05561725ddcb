"""system.MultiTermSystem (l3k_mfs_*): the matrix-free sum of several terms over one set of rows, where a term on some of the
elements is an ordinary MatrixFreeSystem on a DeviceMesh of partition.element_subset(...) over the same nodes.

References: the reference's tests/MultiDomainTest.cpp restated (1), sums of single-term calls of the library (2, 4, 6), the dense
sum of P_e^T K_e P_e x built in numpy from the library's own element matrices (3), the assembled system with the direct solver (5).
Bars: 1e-6 is the reference's own (MultiDomainTest.cpp, eps); 1e-11 relative L2 is the project's mesh-level bar; 1e-8
the reference's cross-path bar.  Kernels the library has no instance of come from plugin.compile_kernel."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from l3ster_amd import capi, gmsh, partition, solve, system
from l3ster_amd.capi import L3KError

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MULTIDOM = os.path.join(ROOT, "tests", "golden", "gmsh_ascii4_square_multidom.msh")
D3, D3VAR, D2 = system.KERNEL_DIFFUSION3D, system.KERNEL_DIFFUSION3D_VAR, system.KERNEL_DIFFUSION2D
U = 4
ALPHA, BETA = 0.7, -0.3

SET_SRC = """
struct MultiDomSet {
    static constexpr l3k::KernelParams params{.dimension = 2, .n_equations = 1, .n_unknowns = 1};
    double set_value = 0.;
    template <typename In, typename Out> L3K_HD void operator()(const In&, Out& out) const {
        auto& [operators, rhs] = out;
        auto& [A0, Ax, Ay] = operators;
        A0(0, 0) = 1.;
        for (int r = 0; r < rhs.cols(); ++r)
            rhs(0, r) = set_value + 1000. * r;
    }
};"""


@pytest.fixture(scope="module")
def ctx():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    torch.cuda.set_device(0)
    return system.Context(0, torch.cuda.current_stream().cuda_stream)


@pytest.fixture(scope="module")
def det_ctx():
    torch.cuda.set_device(0)
    c = system.Context(0, torch.cuda.current_stream().cuda_stream)
    c.set_deterministic(True)
    return c


@pytest.fixture(scope="module")
def set_id():
    from l3ster_amd import plugin
    return plugin.compile_kernel("MultiDomSet", SET_SRC, kernel_id=1361, shapes=[(2, 3, 1), (2, 3, 2)])


@pytest.fixture(scope="module")
def var6_id():
    """Diffusion3DVar at order 6, which the library has no instance of"""
    from l3ster_amd import plugin
    return plugin.compile_kernel("MultiTermVar6", "struct MultiTermVar6 : ::l3k::kernels::Diffusion3DVar {};", kernel_id=1362,
                                 shapes=[(6, 7, 1)])


@pytest.fixture(scope="module")
def var2d_id():
    """Diffusion2DVar at order 3, which the library has no instance of"""
    from l3ster_amd import plugin
    return plugin.compile_kernel("MultiTermVar2D", "struct MultiTermVar2D : ::l3k::kernels::Diffusion2DVar {};", kernel_id=1363,
                                 shapes=[(3, 4, 1)])


def dev(a, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


def rel_l2(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(np.asarray(b)))


def random_vectors(n, seed, count=2):
    rng = np.random.default_rng(seed)
    return [rng.uniform(-1.0, 1.0, (1, n)) for _ in range(count)]


def diffusivity(part):
    """A smooth positive nodal field (1, n_local_nodes) for the variable-diffusivity kernels"""
    c = part.node_coords()
    return dev(1.0 + 0.3 * c[:, 0] + 0.2 * c[:, 1] * c[:, 1] + 0.1 * c[:, 2])[None, :].contiguous()


def var_term(mesh, kid, field):
    t = system.MatrixFreeSystem(mesh, kid)
    t.set_fields(field)
    return t


def coverage(parts_and_fields, n_nodes, dpn):
    """numpy restatement of the coverage mask: (elem_nodes of the term, its field_inds) pairs"""
    act = np.zeros((n_nodes, dpn), dtype=np.uint8)
    for elem_nodes, fi in parts_and_fields:
        for f in fi:
            act[np.asarray(elem_nodes).reshape(-1), f] = 1
    return act.reshape(-1)


# ------------------------------------------------------------------------------------------ 1. MultiDomainTest restated
def test_multidomain_four_kernels_on_four_domains(ctx, set_id):
    """tests/MultiDomainTest.cpp: the committed four-domain square at order 2, dofs_per_node = 4; term i has A0(0,0) = 1 and
    rhs = (i + 1, i + 1001) on dof i of domain i.  diag / rhs, the masked Jacobi inverse, PCG to 1e-10 per column from x = -7."""
    m = gmsh.read_mesh(MULTIDOM)
    mesh = system.ElevatedMesh(ctx, m.verts, m.conn, 2, m.bnd_conn, m.bnd_id, m.elem_domain)
    domains = np.unique(m.elem_domain)
    assert domains.size == 4
    rows = system.DeviceMesh(ctx, mesh, U)
    S = system.MultiTermSystem(rows, n_rhs=2)
    cover = []
    for i, d in enumerate(domains):
        sub = mesh.subset([d])
        assert 0 < sub.n_elems < mesh.n_elems
        S.add(system.MatrixFreeSystem(system.DeviceMesh(ctx, sub, U), set_id, kernel_params=[i + 1.0], field_inds=[i], n_rhs=2))
        cover.append((sub.elem_nodes, [i]))
    S.finalize()
    active = coverage(cover, mesh.n_local_nodes, U)
    assert 0 < active.sum() < active.size  # a dof lives on part of the mesh only
    assert np.array_equal(S.active().cpu().numpy(), active)
    info = S.info
    assert (info.n_terms, info.n_rows, info.n_active_rows, info.n_dirichlet_rows, info.n_rhs, info.finalized) == \
        (4, active.size, int(active.sum()), 0, 2, 1)
    diag, rhs = S.diag_rhs()
    minv = S.jacobi_inverse(diag)
    x = torch.full((2, active.size), -7.0, dtype=torch.float64, device="cuda")
    res = solve.pcg(S, rhs, x, minv, tol=1e-10, residual_scaling="initial")
    assert all(r.converged for r in res)
    x = x.cpu().numpy().reshape(2, -1, U)
    on = active.reshape(-1, U).astype(bool)
    for i in range(4):
        err = max(np.abs(x[0][on[:, i], i] - (i + 1)).max(), np.abs(x[1][on[:, i], i] - (i + 1001)).max())
        print(f"domain {int(domains[i])}, dof {i}: {int(on[:, i].sum())} nodes, max error {err:.2e}, {res[0].num_iters} + {res[1].num_iters} iterations")
        assert err < 1e-6
    assert np.all(x[:, ~on] == -7.0)  # bit for bit: no term covers these dofs
    assert np.all(minv.cpu().numpy()[~active.astype(bool)] == 0.0)


# ------------------------------------------------------------------------------------------ 2. two kernels on the same elements
def two_kernel_case(ctx, p, second):
    part = system.CubePartition(3, p, perturb=0.1)
    mask = part.dirichlet_mask(U, unknowns=(0,), sides=(0, 1))
    mesh = system.DeviceMesh(ctx, part, U, mask)
    a, b = system.MatrixFreeSystem(mesh, D3, [0.7, 1.3]), var_term(mesh, second, diffusivity(part))
    S = system.MultiTermSystem(mesh).add(a).add(b).finalize()
    return part, mask, mesh, a, b, S


def check_sum_of_applies(S, terms, mask, n, seed, label):
    x, y0 = random_vectors(n, seed)
    X, Y0 = dev(x), dev(y0)
    Y = S.apply(X, Y0.clone(), ALPHA, BETA)
    ref = BETA * y0
    for t in terms:
        Yt = torch.zeros_like(X)
        if isinstance(t, system.BoundaryTerm):
            t.apply(X, Yt, ALPHA)
            ref = ref + Yt.cpu().numpy()
        else:
            t.apply(X, Yt, ALPHA, 0.0)
            ref = ref + Yt.cpu().numpy() - ALPHA * x * mask[None, :n]  # (every single apply adds alpha x on the Dirichlet rows)
    ref = ref + ALPHA * x * mask[None, :n]  # ... the sum adds it once
    err = rel_l2(Y.cpu().numpy(), ref)
    print(f"{label}: sum against the single applies, relative L2 {err:.2e}")
    assert err <= 1e-11
    return Y


@pytest.mark.parametrize("p", [4, 6])
def test_two_kernels_on_the_same_elements(ctx, var6_id, p):
    """Diffusion3D and Diffusion3DVar on all dofs of 3^3 perturbed hexes: alpha = 0.7, beta = -0.3, Dirichlet on two sides.  A term
    that still wrote the element-internal rows would overwrite the other's: O(1) there."""
    part, mask, mesh, a, b, S = two_kernel_case(ctx, p, D3VAR if p == 4 else var6_id)
    assert "sumfactFastKernel" in a.route()  # the kernel the benchmark runs, whose lone route writes exclusive rows
    n = mesh.n_owned_dofs
    check_sum_of_applies(S, [a, b], mask, n, 7 + p, f"order {p}")
    # each term still works alone, fused stores and all, after running inside the sum
    x, y0 = random_vectors(n, 3)
    ya = a.apply(dev(x), dev(y0), ALPHA, BETA).cpu().numpy()
    S.apply(dev(x), dev(y0), ALPHA, BETA)
    assert rel_l2(a.apply(dev(x), dev(y0), ALPHA, BETA).cpu().numpy(), ya) <= 1e-13


# ------------------------------------------------------------------------------------------ 3. two domains
def split_case(ctx, part, k, kid_a, kid_b, field, dpn=U, mask=None, opts=None):
    """rows, the sum of kid_a on the elements [0, k) and kid_b on [k, n) as two subset meshes, and the two whole-mesh terms"""
    mask = part.dirichlet_mask(dpn, unknowns=(0,), sides=(0, 1)) if mask is None else mask
    rows = system.DeviceMesh(ctx, part, dpn, mask)
    lo = partition.element_subset(part, np.arange(0, k))
    hi = partition.element_subset(part, np.arange(k, part.n_elems))

    def make(mesh, kid):
        t = system.MatrixFreeSystem(mesh, kid, [0.7, 1.3] if kid == D3 else None)
        if t.info["n_fields"]:
            t.set_fields(field)
        return t
    terms = [make(system.DeviceMesh(ctx, lo, dpn, mask), kid_a), make(system.DeviceMesh(ctx, hi, dpn, mask), kid_b)]
    whole = [make(rows, kid_a), make(rows, kid_b)]
    S = system.MultiTermSystem(rows).add(terms[0]).add(terms[1]).finalize()
    return rows, mask, S, terms, whole, (lo, hi)


def dense_apply(part, mask, K_lo, K_hi, k, x, y0, dpn):
    """alpha sum_e P_e^T K_e P_e x + beta y0 with the Dirichlet semantics of the apply (algsys/MatrixFreeSystem.hpp:421-537,
    1087-1098): masked entries of x read as 0, masked rows receive nothing but alpha x"""
    free = 1.0 - mask.astype(np.float64)
    xm, y = x * free, BETA * y0.copy()
    K = np.concatenate([K_lo, K_hi])
    assert K.shape[0] == part.n_elems and K_lo.shape[0] == k
    Ue = K.shape[1] // part.elem_nodes.shape[1]
    for e in range(part.n_elems):
        dofs = (part.elem_nodes[e].astype(np.int64)[:, None] * dpn + np.arange(Ue)[None, :]).reshape(-1)
        y[dofs] += ALPHA * free[dofs] * (K[e] @ xm[dofs])
    return y + ALPHA * x * mask


def test_two_domains_hexes_vs_dense_numpy(ctx):
    part, k = system.CubePartition(3, 4, perturb=0.1), 10
    rows, mask, S, terms, whole, _ = split_case(ctx, part, k, D3, D3VAR, diffusivity(part))
    n = rows.n_owned_dofs
    K_lo = whole[0].local_assemble(0, k, want_F=False)[0].cpu().numpy()
    K_hi = whole[1].local_assemble(k, part.n_elems - k, want_F=False)[0].cpu().numpy()
    x, y0 = random_vectors(n, 11)
    y = S.apply(dev(x), dev(y0), ALPHA, BETA).cpu().numpy()[0]
    err = rel_l2(y, dense_apply(part, mask, K_lo, K_hi, k, x[0], y0[0], U))
    print(f"hexes, Diffusion3D on [0, {k}) + Diffusion3DVar on [{k}, {part.n_elems}): against the dense sum, relative L2 {err:.2e}")
    assert err <= 1e-11
    assert S.info.n_active_rows == n


def test_two_domains_of_one_kernel_are_the_whole_mesh(ctx):
    part, k = system.CubePartition(3, 4, perturb=0.1), 10
    rows, mask, S, terms, whole, _ = split_case(ctx, part, k, D3, D3, None)
    x, y0 = random_vectors(rows.n_owned_dofs, 12)
    y = S.apply(dev(x), dev(y0), ALPHA, BETA).cpu().numpy()
    err = rel_l2(y, whole[0].apply(dev(x), dev(y0), ALPHA, BETA).cpu().numpy())
    print(f"hexes, one kernel on two parts against the whole mesh: relative L2 {err:.2e}")
    assert err <= 1e-11


def test_two_domains_quads(ctx, var2d_id):
    part, k, dpn = system.SquarePartition((5, 4), 3, perturb=0.1), 7, 3
    mask = part.dirichlet_mask(dpn, unknowns=(0,), sides=(2, 3))
    rows, mask, S, terms, whole, _ = split_case(ctx, part, k, D2, var2d_id, diffusivity(part), dpn=dpn, mask=mask)
    n = rows.n_owned_dofs
    K_lo = whole[0].element_systems(0, k, want_F=False)[0].cpu().numpy()
    K_hi = whole[1].element_systems(k, part.n_elems - k, want_F=False)[0].cpu().numpy()
    x, y0 = random_vectors(n, 13)
    y = S.apply(dev(x), dev(y0), ALPHA, BETA).cpu().numpy()[0]
    err = rel_l2(y, dense_apply(part, mask, K_lo, K_hi, k, x[0], y0[0], dpn))
    print(f"quads, Diffusion2D on [0, {k}) + Diffusion2DVar on [{k}, {part.n_elems}): against the dense sum, relative L2 {err:.2e}")
    assert err <= 1e-11
    rows, mask, S, terms, whole, _ = split_case(ctx, part, k, D2, D2, None, dpn=dpn, mask=mask)
    y = S.apply(dev(x), dev(y0), ALPHA, BETA).cpu().numpy()
    err = rel_l2(y, whole[0].apply(dev(x), dev(y0), ALPHA, BETA).cpu().numpy())
    print(f"quads, one kernel on two parts against the whole mesh: relative L2 {err:.2e}")
    assert err <= 1e-11


# ------------------------------------------------------------------------------------------ 4. dof subsets and a boundary term
def test_dof_subsets_and_a_boundary_term(ctx):
    """Six dofs per node: Mass3D on the dofs [0, 1] of the elements [0, 20), Advection3D on dof [2] of the elements [12, 27) (they
    overlap on [12, 20)), Robin3D on the dofs [1, 2, 3, 4] of the sides x = 1; dof 5 is covered by nothing."""
    p, dpn = 2, 6
    part = system.CubePartition(3, p, perturb=0.1)
    mask = part.dirichlet_mask(dpn, unknowns=(0,), sides=(0,))
    rows = system.DeviceMesh(ctx, part, dpn, mask)
    lo, hi = partition.element_subset(part, np.arange(0, 20)), partition.element_subset(part, np.arange(12, 27))
    t_vec = system.MatrixFreeSystem(system.DeviceMesh(ctx, lo, dpn, mask), system.KERNEL_MASS3D, field_inds=[0, 1])
    t_sc = system.MatrixFreeSystem(system.DeviceMesh(ctx, hi, dpn, mask), system.KERNEL_ADVECTION3D, field_inds=[2])
    c = part.node_coords()
    t_sc.set_fields(dev(np.stack([0.2 + c[:, 0], 0.1 * c[:, 1], 0.3 - c[:, 2] * c[:, 0]])))
    t_bnd = system.BoundaryTerm(rows, system.KERNEL_ROBIN3D, *part.boundary_sides([5]), field_inds=[1, 2, 3, 4])
    terms = [t_vec, t_sc, t_bnd]
    S = system.MultiTermSystem(rows)
    for t in terms:
        S.add(t)
    S.finalize()
    n = rows.n_owned_dofs
    check_sum_of_applies(S, terms, mask, n, 21, "dof subsets + boundary term")
    fe, _ = part.boundary_sides([5])
    active = coverage([(lo.elem_nodes, [0, 1]), (hi.elem_nodes, [2]), (part.elem_nodes[fe], [1, 2, 3, 4])], part.n_local_nodes, dpn)
    assert np.array_equal(S.active().cpu().numpy(), active)
    # diag / rhs: the sums of the single-term calls (no finalisation), then the Dirichlet rows once
    diag, rhs = S.diag_rhs(finalize=False)
    d_ref, r_ref = torch.zeros_like(diag), torch.zeros_like(rhs)
    for t in terms:
        if isinstance(t, system.BoundaryTerm):
            t.diag_rhs(d_ref, r_ref)
        else:
            t.diag_rhs(diag=d_ref, rhs=r_ref, finalize=False)
    assert rel_l2(diag.cpu().numpy(), d_ref.cpu().numpy()) <= 1e-11 and rel_l2(rhs.cpu().numpy(), r_ref.cpu().numpy()) <= 1e-11
    diag, rhs = S.diag_rhs()
    on = mask[:n].astype(bool)
    assert np.all(diag.cpu().numpy()[on] == 1.0) and np.all(rhs.cpu().numpy()[0][on] == 0.0)
    minv = S.jacobi_inverse(diag).cpu().numpy().reshape(-1, dpn)
    assert np.all(minv[:, 5] == 0.0) and np.all(minv.reshape(-1)[active.astype(bool)] != 0.0)
    assert np.all(minv.reshape(-1)[~active.astype(bool)] == 0.0)


# ------------------------------------------------------------------------------------------ 5. solve
def test_solve_against_the_assembled_system(ctx):
    """The sum of case 3 solved by PCG with Jacobi and with Chebyshev degree 3, against the AssembledSystem of the same whole-mesh
    terms over the same element ranges, solved by the band Cholesky."""
    part, k = system.CubePartition(3, 2, perturb=0.1), 10
    mask = part.dirichlet_mask(U, unknowns=(0,), sides=(0, 1))
    rows = system.DeviceMesh(ctx, part, U, mask)
    lo, hi = partition.element_subset(part, np.arange(0, k)), partition.element_subset(part, np.arange(k, part.n_elems))
    a = system.MatrixFreeSystem(system.DeviceMesh(ctx, lo, U, mask), D3, [0.7, 1.3])
    b = system.MatrixFreeSystem(system.DeviceMesh(ctx, hi, U, mask), D3, [2.0, 0.5])
    S = system.MultiTermSystem(rows).add(a).add(b).finalize()
    aw, bw = system.MatrixFreeSystem(rows, D3, [0.7, 1.3]), system.MatrixFreeSystem(rows, D3, [2.0, 0.5])
    asm = system.AssembledSystem(rows)
    asm.begin()
    asm.add(aw, 0, k).add(bw, k, part.n_elems - k)
    op = asm.end()
    n = rows.n_owned_dofs
    x_ref = torch.zeros(n, dtype=torch.float64, device="cuda")
    solve.direct_solve(op, asm.rhs[0], x_ref)
    x_ref = x_ref.cpu().numpy()
    diag, rhs = S.diag_rhs()
    minv = S.jacobi_inverse(diag)
    x = torch.zeros(n, dtype=torch.float64, device="cuda")
    res = solve.pcg(S, rhs[0], x, minv, tol=1e-12, residual_scaling="rhs", max_iters=20000)
    err = rel_l2(x.cpu().numpy(), x_ref)
    print(f"Jacobi PCG on the sum: {res.num_iters} iterations, against the direct solve of the assembled system {err:.2e}")
    assert res.converged and err <= 1e-8
    cheb = solve.ChebyshevPreconditioner(S, minv, degree=3)
    x = torch.zeros(n, dtype=torch.float64, device="cuda")
    res_c = solve.pcg(S, rhs[0].contiguous(), x, tol=1e-12, residual_scaling="rhs", max_iters=20000, precond=cheb)
    err = rel_l2(x.cpu().numpy(), x_ref)
    print(f"Chebyshev(3) PCG on the sum: {res_c.num_iters} iterations, {err:.2e}")
    assert res_c.converged and err <= 1e-8 and res_c.num_iters <= res.num_iters
    # <x, A x> of apply_energy is the dot product behind the apply
    s = torch.zeros(8, dtype=torch.float64, device="cuda")
    X = dev(random_vectors(n, 5, 1)[0])
    Y = S.apply_energy(X, torch.empty_like(X), s)
    assert abs(float(s[1]) - float((X * Y).sum())) <= 1e-12 * abs(float(s[1]))


# ------------------------------------------------------------------------------------------ 6. classes and ghosts
def test_element_classes_and_ghost_buffers(ctx):
    """Rank 1 of a 2 x 1 x 1 partition: interior then border equals all, and the two halves of the interior equal the interior, with
    the ghost import / export buffers of the split-phase calls.  Bar: the pieces add the same products in another order, so they agree
    to rounding: 1e-12 of the largest entry."""
    part = system.CubePartition((4, 3, 3), 4, parts=(2, 1, 1), rank=1, perturb=0.1)
    assert part.n_ghost_nodes > 0 and 0 < part.n_interior_elems < part.n_elems
    mask = part.dirichlet_mask(U, unknowns=(0,), sides=(0, 1))
    rows = system.DeviceMesh(ctx, part, U, mask)
    k = part.n_interior_elems // 2 + 1  # both subsets hold interior and border elements
    idx = np.arange(part.n_elems)
    lo = partition.element_subset(part, np.concatenate([idx[:k], idx[part.n_interior_elems:part.n_interior_elems + 3]]))
    hi = partition.element_subset(part, np.setdiff1d(idx, lo.elem_index))
    assert 0 < lo.n_interior_elems < lo.n_elems and 0 < hi.n_interior_elems < hi.n_elems
    a = system.MatrixFreeSystem(system.DeviceMesh(ctx, lo, U, mask), D3, [0.7, 1.3])
    b = var_term(system.DeviceMesh(ctx, hi, U, mask), D3VAR, diffusivity(part))
    S = system.MultiTermSystem(rows).add(a).add(b).finalize()
    no, ng = rows.n_owned_dofs, rows.n_ghost_dofs
    x = part.synthetic_vector(U)
    X, XG = dev(x[:, :no]), dev(x[:, no:])

    def run(classes):
        Y = torch.zeros((1, no), dtype=torch.float64, device="cuda")
        YG = torch.zeros((1, ng), dtype=torch.float64, device="cuda")
        for which in classes:
            S.apply_elems(which, X, XG, Y, YG, ALPHA, 0.0)
        return np.concatenate([Y.cpu().numpy(), YG.cpu().numpy()], axis=1)
    y_all, y_int = run([2]), run([0])
    assert np.abs(y_all[:, no:]).max() > 0 and np.abs(y_int).max() > 0
    scale = np.abs(y_all).max()
    d1 = np.abs(run([0, 1]) - y_all).max() / scale
    d2 = np.abs(run([3, 4]) - y_int).max() / scale
    print(f"interior + border against all: {d1:.2e}; halves of the interior against the interior: {d2:.2e}")
    assert d1 <= 1e-12 and d2 <= 1e-12
    with pytest.raises(L3KError, match="single-rank"):
        S.apply(X, torch.zeros_like(X))


# ------------------------------------------------------------------------------------------ 7. determinism
def test_deterministic_context_gives_identical_bits(det_ctx):
    part, mask, mesh, a, b, S = two_kernel_case(det_ctx, 4, D3VAR)
    n = mesh.n_owned_dofs
    x, y0 = random_vectors(n, 31)
    y1 = S.apply(dev(x), dev(y0), ALPHA, BETA).cpu().numpy()
    y2 = S.apply(dev(x), dev(y0), ALPHA, BETA).cpu().numpy()
    assert np.array_equal(y1, y2) and np.abs(y1).max() > 0
    check_sum_of_applies(S, [a, b], mask, n, 32, "deterministic")
    diag, rhs = S.diag_rhs()
    minv = S.jacobi_inverse(diag)
    sols = []
    for _ in range(2):
        sol = torch.zeros(n, dtype=torch.float64, device="cuda")
        # (60 iterations of a solve that needs thousands at this order: the bits are the subject, not the limit)
        res = solve.pcg(S, rhs[0], sol, minv, tol=1e-30, residual_scaling="initial", max_iters=60, throw_on_fail=False)
        assert res.num_iters == 60 and 0 < res.tol < 1
        sols.append((sol.cpu().numpy(), res.tol))
    assert sols[0][1] == sols[1][1] and np.array_equal(sols[0][0], sols[1][0]) and np.abs(sols[0][0]).max() > 0


# ------------------------------------------------------------------------------------------ 8. coverage past one grid
def test_coverage_with_the_grid_capped_below_the_work(ctx):
    """With one wave per CU in the tuning the project's grid rule (stridedGrid) caps a launch at CUs / 4 workgroups of 256 threads;
    on 8 x 6 x 6 hexes of order 4 each of the two terms of the two-domain construction of case 3 has more (element, node) items
    (140 * 125 and 148 * 125) than that grid has threads, and so have the rows the count walks: every thread of the coverage and
    counting kernels strides.  The mask is the numpy one, and the one of the uncapped grid."""
    part, k = system.CubePartition((8, 6, 6), 4), 140
    cap = torch.cuda.get_device_properties(0).multi_processor_count // 4 * 256
    assert k * 125 > cap and (part.n_elems - k) * 125 > cap
    dpn = 5
    mask = part.dirichlet_mask(dpn, unknowns=(0,), sides=(0, 1))
    rows = system.DeviceMesh(ctx, part, dpn, mask)
    lo, hi = partition.element_subset(part, np.arange(0, k)), partition.element_subset(part, np.arange(k, part.n_elems))
    a = system.MatrixFreeSystem(system.DeviceMesh(ctx, lo, dpn, mask), D3)
    b = system.MatrixFreeSystem(system.DeviceMesh(ctx, hi, dpn, mask), system.KERNEL_ADVECTION3D, field_inds=[4])
    masks = []
    for tune in (dict(waves_per_cu=1), dict()):
        with ctx.tuning(**tune):
            S = system.MultiTermSystem(rows).add(a).add(b).finalize()
        masks.append(S.active().cpu().numpy())
        assert S.info.n_active_rows == int(masks[-1][:rows.n_owned_dofs].sum())
    want = coverage([(lo.elem_nodes, [0, 1, 2, 3]), (hi.elem_nodes, [4])], part.n_local_nodes, dpn)
    assert 0 < want.sum() < want.size
    assert np.array_equal(masks[0], want) and np.array_equal(masks[1], want)


# ------------------------------------------------------------------------------------------ 9. refusals
def test_refusals(ctx):
    part = system.CubePartition(2, 2)
    mask = part.dirichlet_mask(U, unknowns=(0,), sides=(0,))
    rows = system.DeviceMesh(ctx, part, U, mask)
    S = system.MultiTermSystem(rows, n_rhs=1)
    lib = capi.load()

    def refused(term, match):
        add = lib.l3k_mfs_add_boundary if isinstance(term, system.BoundaryTerm) else lib.l3k_mfs_add_domain
        assert add(S._h, term._h) == -1
        assert match in lib.l3k_last_error().decode(), lib.l3k_last_error().decode()
        assert S.info.n_terms == 0

    other_nodes = system.CubePartition((2, 2, 1), 2)
    refused(system.MatrixFreeSystem(system.DeviceMesh(ctx, other_nodes, U, other_nodes.dirichlet_mask(U, sides=(0,))), D3), "not a mesh over the same nodes")
    other_order = system.CubePartition(2, 1)
    refused(system.MatrixFreeSystem(system.DeviceMesh(ctx, other_order, U), D3), "order 1, the rows dim 3 and order 2")
    refused(system.MatrixFreeSystem(system.DeviceMesh(ctx, part, 5, part.dirichlet_mask(5, sides=(0,))), D3), "dofs_per_node = 5, the rows 4")
    flipped = mask.copy()
    dof = 4 * 7 + 2
    flipped[dof] ^= 1
    refused(system.MatrixFreeSystem(system.DeviceMesh(ctx, part, U, flipped), D3), f"first at dof {dof} (node 7, dof 2 of the node)")
    refused(system.MatrixFreeSystem(system.DeviceMesh(ctx, part, U), D3), f"first at dof {int(np.nonzero(mask)[0][0])} ")  # no mask = all zero
    with_bnd = system.MatrixFreeSystem(rows, D3)
    bnd = system.BoundaryTerm(rows, system.KERNEL_ROBIN3D, *part.boundary_sides([5]))
    with_bnd.attach_boundary(bnd)
    refused(with_bnd, "add them with l3k_mfs_add_boundary")
    S2 = system.MultiTermSystem(rows, n_rhs=2)
    assert lib.l3k_mfs_add_domain(S2._h, system.MatrixFreeSystem(rows, D3)._h) == -1 and "n_rhs = 1, the system 2" in lib.l3k_last_error().decode()

    term = system.MatrixFreeSystem(rows, D3)
    S.add(term).add(bnd)
    n = rows.n_owned_dofs
    X = dev(random_vectors(n, 1, 1)[0])
    Y = torch.full((1, n), 3.25, dtype=torch.float64, device="cuda")

    def apply_refused(S, X, Y, match):
        nc = X.shape[0]
        rc = lib.l3k_mfs_apply(S._h, X.data_ptr(), X.stride(0) if nc > 1 else n, Y.data_ptr(), Y.stride(0) if nc > 1 else n, nc, 1.0, 0.0)
        assert rc == -1 and match in lib.l3k_last_error().decode(), lib.l3k_last_error().decode()
        torch.cuda.synchronize()
        assert bool((Y == 3.25).all())  # untouched

    apply_refused(S, X, Y, "call l3k_mfs_finalize first")
    with pytest.raises(L3KError, match="l3k_mfs_finalize first"):
        S.diag_rhs()
    with pytest.raises(L3KError, match="l3k_mfs_finalize first"):
        S.active()
    S.finalize()
    assert lib.l3k_mfs_add_domain(S._h, term._h) == -1 and "finalized: no more terms" in lib.l3k_last_error().decode()
    assert lib.l3k_mfs_add_boundary(S._h, bnd._h) == -1 and "finalized: no more terms" in lib.l3k_last_error().decode()
    assert S.info.n_terms == 2
    X2 = torch.zeros((2, n), dtype=torch.float64, device="cuda")
    apply_refused(S, X2, torch.full((2, n), 3.25, dtype=torch.float64, device="cuda"), "number of columns (2) must be in [1, n_rhs = 1]")
    S.apply(X, Y)  # ... and the accepted call writes
    assert not bool((Y == 3.25).any())
    with pytest.raises(L3KError, match="takes a MatrixFreeSystem or a BoundaryTerm"):
        system.MultiTermSystem(rows).add(rows)


# ------------------------------------------------------------------------------------------ 10. C++ mirror
def test_cpp_mirror_gives_the_bits_of_the_python_route(det_ctx, tmp_path):
    """tests/cpp/multiterm_shim.cpp: l3k::MultiTermSystem over two l3k::ElementSubset meshes on a deterministic context -- one
    apply and one solve; the same steps through system.MultiTermSystem and partition.element_subset give the same bits."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe, out = str(tmp_path / "multiterm_shim"), str(tmp_path / "out.bin")
    cmd = [hipcc, "-std=c++20", "-O1", "--offload-arch=gfx950", f"-I{ROOT}/include", os.path.join(ROOT, "tests", "cpp", "multiterm_shim.cpp"),
           f"-L{ROOT}/l3ster_amd/lib", "-ll3k", f"-Wl,-rpath,{ROOT}/l3ster_amd/lib", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe, out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr
    cpp = np.fromfile(out, dtype=np.float64)
    part, k = system.CubePartition(3, 2, perturb=0.1), 10
    mask = part.dirichlet_mask(U, unknowns=(0,), sides=(0, 1))
    rows = system.DeviceMesh(det_ctx, part, U, mask)
    lo, hi = partition.element_subset(part, np.arange(0, k)), partition.element_subset(part, np.arange(k, part.n_elems))
    a = system.MatrixFreeSystem(system.DeviceMesh(det_ctx, lo, U, mask), D3, [0.7, 1.3])
    b = system.MatrixFreeSystem(system.DeviceMesh(det_ctx, hi, U, mask), D3, [2.0, 0.5])
    S = system.MultiTermSystem(rows).add(a).add(b).finalize()
    n = rows.n_owned_dofs
    i = np.arange(n, dtype=np.uint64)
    x = ((i * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)).astype(np.float64) * 2.0 ** -32 - 0.5
    y = ((i * np.uint64(2246822519)) & np.uint64(0xFFFFFFFF)).astype(np.float64) * 2.0 ** -32 - 0.5
    Y = S.apply(dev(x[None, :]), dev(y[None, :]), ALPHA, BETA)
    diag, rhs = S.diag_rhs()
    sol = torch.zeros(n, dtype=torch.float64, device="cuda")
    res = solve.pcg(S, rhs[0], sol, S.jacobi_inverse(diag), tol=1e-10, max_iters=5000, residual_scaling="initial")
    assert res.converged and cpp.shape == (2 * n,)
    assert np.abs(cpp[:n]).max() > 0 and np.array_equal(cpp[:n], Y.cpu().numpy()[0])
    assert np.abs(cpp[n:]).max() > 0 and np.array_equal(cpp[n:], sol.cpu().numpy())
