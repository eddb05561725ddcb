"""The hex post-processing kernels (integralDomainKernel, integralSideKernel, valuesAtNodesKernel of csrc/device/integral.hpp and
reducePartialsKernel of csrc/api_post.hip) against the dense numpy restatement of integral_ref.py, where they could be wrong
without the rest of the suite noticing: field derivatives on a distorted hex over the domain and each of the six sides at every
compiled shape of Diffusion3DError, nodal values with derivatives up to p = 6 (343 nodes for 256 threads), more partial sums
than one sweep of the reduction, a leading dimension larger than the node count, fields that include ghost nodes, and a probe
plugin that shows every input of a residual kernel on its own (point, time, normal).

Bars: results are compared as vectors, the error relative to the largest component of the expected vector, <= 1e-12 (the
restatement and the oracle agree to 1e-14, test_integral_ref_cpu.py).  Where a residual vanishes analytically its squared
integral must be <= 1e-20 x measure, a pointwise residual of 1e-10."""
import ctypes as C

import numpy as np
import pytest

import helpers
import integral_ref as R

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

BAR = 1e-12
KP = [0.7, 1.3]
REGIONS = [None, 0, 1, 2, 3, 4, 5]  # the domain and each side of a single element
U = 4
DOFS = [2, 0, 3, 1]


@pytest.fixture(scope="module")
def S():
    from l3ster_amd import system
    return system


@pytest.fixture(scope="module")
def ctx(S):
    torch.cuda.set_device(0)
    return S.Context(0, torch.cuda.current_stream().cuda_stream)


@pytest.fixture(scope="module")
def probe_id():
    from l3ster_amd import plugin
    return plugin.compile_kernel("HexProbeResidual", R.PROBE_SRC, kernel_id=1331, shapes=[(2, 3), (2, 5), (4, 5), (6, 7)],
                                 kind="residual")


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")


def _faces(region):
    return (None, None) if region is None else ([0], [region])


def _side_args(fe, fs):
    from l3ster_amd import capi
    if fe is None:
        return -1, None, None, None
    fe, fs = np.ascontiguousarray(fe, dtype=np.int64), np.ascontiguousarray(fs, dtype=np.uint8)
    return fe.size, fe.ctypes.data_as(capi.c_int64_p), fs.ctypes.data_as(capi.c_uint8_p), (fe, fs)


def raw_integrate(mesh, rid, fields, ldf, kparams, asm_opts, square, fe=None, fs=None, time=0.0, n_equations=4):
    """l3k_integrate with the leading dimension of `fields` given by the caller."""
    from l3ster_amd import capi
    kp = np.ascontiguousarray(kparams, dtype=np.float64)
    nf, fe_p, fs_p, keep = _side_args(fe, fs)
    out = np.zeros(n_equations)
    capi.check(capi.load().l3k_integrate(mesh.ctx._h, mesh._h, rid, kp.ctypes.data_as(C.c_void_p), kp.nbytes,
                                         C.byref(capi.AsmOpts(*asm_opts)), C.c_void_p(fields.data_ptr()), ldf, float(time),
                                         int(square), nf, fe_p, fs_p, out.ctypes.data_as(capi.c_double_p)))
    return out


def raw_values_at_nodes(mesh, rid, fields, ldf, kparams, dof_inds, fe=None, fs=None, time=0.0):
    """l3k_values_at_nodes alone: (sum, count) over the local dofs, before any averaging."""
    from l3ster_amd import capi
    kp = None if kparams is None else np.ascontiguousarray(kparams, dtype=np.float64)
    nf, fe_p, fs_p, keep = _side_args(fe, fs)
    n = mesh.part.n_local_nodes * mesh.dofs_per_node
    sc = torch.zeros((2, n), dtype=torch.float64, device="cuda")
    capi.check(capi.load().l3k_values_at_nodes(mesh.ctx._h, mesh._h, rid, None if kp is None else kp.ctypes.data_as(C.c_void_p),
                                               0 if kp is None else kp.nbytes, C.c_void_p(fields.data_ptr()), ldf, float(time), nf,
                                               fe_p, fs_p, (C.c_int * len(dof_inds))(*dof_inds), C.c_void_p(sc[0].data_ptr()),
                                               C.c_void_p(sc[1].data_ptr())))
    torch.cuda.synchronize()
    return sc[0].cpu().numpy(), sc[1].cpu().numpy()


def ref_integrate(part, fields, nq, residual, square, fe=None, fs=None, time=0.0):
    return R.integrate(part.elem_nodes, part.elem_verts, fields, part.order, nq, residual, square, fe, fs, time)


def ref_values_at_nodes(part, fields, residual, dof_inds, fe=None, fs=None, time=0.0, dofs_per_node=U):
    return R.values_at_nodes(part.elem_nodes, part.elem_verts, fields, part.order, residual, dof_inds, dofs_per_node,
                             part.n_local_nodes, fe, fs, time)


def coords(part):
    return R.node_coords(part.elem_nodes, part.elem_verts, part.order, part.n_local_nodes)


# --------------------------------------------------------------------------------------------------- 1. one distorted hex
@pytest.mark.parametrize("p,opts,nq", [(2, (2, 0, 0), 5), (4, (2, 0, 0), 9), (6, (1, 0, 0), 7), (6, (2, 0, 0), 13)])
def test_one_distorted_hex_random_fields(S, ctx, p, opts, nq):
    """Diffusion3DError on helpers.HEX (J^-1 is full and varies from point to point) with random fields: the domain and each
    of the six sides on its own, plain and squared, at every compiled shape.
    Measured worst relative error: 1.3e-15 at (2,5), 2.2e-15 at (4,9), 1.0e-14 at (6,7), 3.4e-15 at (6,13)."""
    part = helpers.SingleElementMesh(p, helpers.HEX)
    mesh = S.DeviceMesh(ctx, part, U)
    assert S.n_qps1d(p, *opts[:2]) == nq
    fields = np.random.default_rng(10 * p + nq).standard_normal((4, part.n_local_nodes))
    F = dev(fields)
    worst = 0.0
    for region in REGIONS:
        fe, fs = _faces(region)
        for square in (False, True):
            got = S.integrate(mesh, S.RESIDUAL_DIFFUSION3D_ERROR, F, kernel_params=KP, asm_opts=opts, square=square, face_elem=fe,
                              face_side=fs)
            err = R.rel_max(got, ref_integrate(part, fields, nq, R.diffusion3d_error(*KP), square, fe, fs))
            print(f"p={p} nq={nq} region={region} square={square}: {err:.2e}")
            worst = max(worst, err)
    print(f"p={p} nq={nq}: worst {worst:.2e}")
    assert worst <= BAR


@pytest.mark.parametrize("p", [2, 4])
def test_one_distorted_hex_polynomial_field(S, ctx, p):
    """T = x^2 + 3xy - 2yz + z^2, q = grad T sampled at the nodes is exact for p >= 2 on any hex (test_integral_ref_cpu.py):
    with k = 0.7, s = -2.8 the four residuals vanish, with s = 1.3 the first integrates to 4.1 x measure and the others to 0.
    Measured: squared integrals <= 1.7e-28 x measure at p = 2 and <= 4.1e-27 x measure at p = 4; 4.1 x measure to 6.9e-16 and 1.3e-14."""
    part = helpers.SingleElementMesh(p, helpers.HEX)
    mesh = S.DeviceMesh(ctx, part, U)
    opts, nq = (2, 0, 0), 2 * p + 1
    F = dev(R.poly_fields(coords(part)))
    worst_sq, worst_rel = 0.0, 0.0
    for region in REGIONS:
        fe, fs = _faces(region)
        measure = ref_integrate(part, None, nq, R.unit3d, False, fe, fs)[0]
        if p == 2:  # (the only order with a Unit3D shape at nq = 2p + 1)
            assert S.integrate(mesh, S.RESIDUAL_UNIT3D, asm_opts=opts, face_elem=fe, face_side=fs)[0] == pytest.approx(measure, rel=BAR)
        if region is None:
            assert measure == pytest.approx(22.0 / 3.0, rel=1e-14)
        sq = S.integrate(mesh, S.RESIDUAL_DIFFUSION3D_ERROR, F, kernel_params=[0.7, -2.8], asm_opts=opts, square=True, face_elem=fe,
                         face_side=fs)
        got = S.integrate(mesh, S.RESIDUAL_DIFFUSION3D_ERROR, F, kernel_params=KP, asm_opts=opts, face_elem=fe, face_side=fs)
        rel = R.rel_max(got, [4.1 * measure, 0.0, 0.0, 0.0])
        print(f"p={p} region={region}: squared {sq.max() / measure:.2e} x measure, 4.1 x measure to {rel:.2e}")
        worst_sq, worst_rel = max(worst_sq, sq.max() / measure), max(worst_rel, rel)
        assert np.all(sq >= 0)
    assert worst_sq <= 1e-20 and worst_rel <= BAR


# ------------------------------------------------------------------------------------------ 2. nodal values with derivatives
@pytest.fixture(scope="module")
def cubes(S):
    """CubePartition((ne,ne,ne), p, perturb=0.15) with one table of random fields and the restatement's sums and counts, per
    (ne, p).  The perturbation, 0.15 h sin(2 pi x) sin(2 pi y) sin(2 pi z) along (1, 1, 1), is zero at every vertex of the
    2 x 2 x 2 mesh: that mesh is undistorted and J^-1 diagonal on it, whatever `perturb` says.  The 3 x 3 x 3 mesh is distorted, with a
    J that is not symmetric."""
    out = {}
    for ne in (2, 3):
        for p in (2, 4, 6):
            part = S.CubePartition((ne,) * 3, p, perturb=0.15)
            assert (np.abs(part.elem_verts - S.CubePartition((ne,) * 3, p).elem_verts).max() > 0.03) == (ne == 3)
            fields = np.random.default_rng(200 + 10 * ne + p).standard_normal((4, part.n_local_nodes))
            sides = part.boundary_sides(range(6))
            want = {"domain": ref_values_at_nodes(part, fields, R.diffusion3d_error(*KP), DOFS),
                    "sides": ref_values_at_nodes(part, fields, R.diffusion3d_error(*KP), DOFS, *sides)}
            out[ne, p] = (part, fields, sides, want)
    return out


@pytest.mark.parametrize("p", [2, 4, 6])
@pytest.mark.parametrize("ne", [2, 3])
def test_nodal_values_with_derivatives(S, ctx, cubes, ne, p):
    """Diffusion3DError at the nodes into the dofs [2, 0, 3, 1]: all elements (p = 6: 343 nodes for the 256 threads of a
    workgroup) and the six physical sides together; sums and counts of l3k_values_at_nodes on their own, then the average
    through system.values_at_nodes, whose untouched entries keep their fill value.
    Measured worst relative error of the sums: 5e-16 (all orders, both meshes, both forms)."""
    part, fields, sides, want = cubes[ne, p]
    mesh = S.DeviceMesh(ctx, part, U)
    F = dev(fields)
    rid = S.RESIDUAL_DIFFUSION3D_ERROR
    for form, (fe, fs) in (("domain", (None, None)), ("sides", sides)):
        ws, wc = want[form]
        gs, gc = raw_values_at_nodes(mesh, rid, F, F.shape[1], KP, DOFS, fe, fs)
        assert np.array_equal(gc, wc) and np.array_equal(gc, np.round(gc))
        assert gc.max() == (8 if form == "domain" else 4)  # a vertex node inside the mesh; a vertex node on a cube edge (2 elements x 2 sides)
        err = R.rel_max(gs, ws)
        print(f"ne={ne} p={p} {form}: sums {err:.2e}")
        assert err <= BAR
        vals = torch.full((part.n_local_nodes * U,), 7.0, dtype=torch.float64, device="cuda")
        S.values_at_nodes(mesh, rid, DOFS, vals, fields=F, kernel_params=KP, face_elem=fe, face_side=fs)
        avg = np.where(wc > 0, ws / np.maximum(wc, 1), 7.0)
        got = vals.cpu().numpy()
        assert R.rel_max(got, avg) <= BAR
        assert np.all(got[wc == 0] == 7.0) and (form == "domain") == bool(np.all(wc > 0))


@pytest.mark.parametrize("ne", [2, 3])
def test_nodal_values_of_the_polynomial_field_vanish(S, ctx, cubes, ne):
    """p = 4, T and q = grad T as in test_one_distorted_hex_polynomial_field: the nodal residuals vanish to 1e-10, on all
    elements and on the six sides.  Measured: 3.9e-14 on 2 x 2 x 2, 8.3e-14 on 3 x 3 x 3."""
    part, _, sides, _ = cubes[ne, 4]
    mesh = S.DeviceMesh(ctx, part, U)
    F = dev(R.poly_fields(coords(part)))
    for fe, fs in ((None, None), sides):
        vals = torch.full((part.n_local_nodes * U,), 7.0, dtype=torch.float64, device="cuda")
        S.values_at_nodes(mesh, S.RESIDUAL_DIFFUSION3D_ERROR, DOFS, vals, fields=F, kernel_params=[0.7, -2.8], face_elem=fe, face_side=fs)
        got = vals.cpu().numpy()
        touched = got != 7.0
        assert touched.sum() == U * (part.n_local_nodes if fe is None else (4 * ne + 1) ** 3 - (4 * ne - 1) ** 3)
        print(f"ne={ne}: polynomial nodal residuals, {'domain' if fe is None else 'sides'}: {np.abs(got[touched]).max():.2e}")
        assert np.abs(got[touched]).max() <= 1e-10


# ------------------------------------------------------------------------- 3. more partial sums than one reduction sweep
def test_more_partial_sums_than_reduction_threads(S, ctx):
    """294 elements and 266 boundary sides: some of reducePartialsKernel's 256 threads take a second partial sum.  Two calls are
    bitwise equal (fixed summation order); a shuffled side list that holds one side twice counts it twice.
    Measured worst relative error: 9.7e-15 (domain), 5.7e-16 (sides)."""
    p, opts, nq = 2, (2, 0, 0), 5
    part = S.CubePartition((7, 7, 6), p, perturb=0.15)
    fe, fs = part.boundary_sides(range(6))
    assert part.n_elems == 294 and len(fe) == 266
    mesh = S.DeviceMesh(ctx, part, U)
    fields = np.random.default_rng(31).standard_normal((4, part.n_local_nodes))
    F = dev(fields)
    perm = np.random.default_rng(32).permutation(len(fe) + 1) % len(fe)  # side 0 of the list twice
    lists = {"domain": (None, None), "boundary": (fe, fs), "shuffled": (fe[perm], fs[perm])}
    worst = 0.0
    for name, (le, ls) in lists.items():
        for square in (False, True):
            got = S.integrate(mesh, S.RESIDUAL_DIFFUSION3D_ERROR, F, kernel_params=KP, asm_opts=opts, square=square, face_elem=le,
                              face_side=ls)
            again = S.integrate(mesh, S.RESIDUAL_DIFFUSION3D_ERROR, F, kernel_params=KP, asm_opts=opts, square=square, face_elem=le,
                                face_side=ls)
            np.testing.assert_array_equal(got, again)
            err = R.rel_max(got, ref_integrate(part, fields, nq, R.diffusion3d_error(*KP), square, le, ls))
            print(f"{name} square={square}: {err:.2e}")
            worst = max(worst, err)
    assert worst <= BAR
    # the doubled side is really in the sum: it changes the result far beyond the bar
    once = ref_integrate(part, fields, nq, R.diffusion3d_error(*KP), True, fe, fs)
    twice = ref_integrate(part, fields, nq, R.diffusion3d_error(*KP), True, fe[perm], fs[perm])
    assert R.rel_max(twice, once) > 1e-6


# --------------------------------------------------------------------------------------------------- 4. leading dimension
def test_leading_dimension_larger_than_the_node_count(S, ctx, cubes):
    """Fields stored as (F, n_local + 37), the padding filled with 1e300 (finite: the device units are built with finite-math
    flags): integrals are bitwise those of the tight layout; nodal sums, which are accumulated with atomics in no fixed order,
    agree to the bar, their counts exactly.  On the distorted 3 x 3 x 3 mesh."""
    part, fields, sides, want = cubes[3, 2]
    mesh = S.DeviceMesh(ctx, part, U)
    n, ld = part.n_local_nodes, part.n_local_nodes + 37
    padded = np.full((4, ld), 1e300)
    padded[:, :n] = fields
    tight, wide = dev(fields), dev(padded)
    rid = S.RESIDUAL_DIFFUSION3D_ERROR
    for fe, fs in ((None, None), sides):
        for square in (False, True):
            a = raw_integrate(mesh, rid, tight, n, KP, (2, 0, 0), square, fe, fs)
            b = raw_integrate(mesh, rid, wide, ld, KP, (2, 0, 0), square, fe, fs)
            np.testing.assert_array_equal(a, b)
            assert R.rel_max(b, ref_integrate(part, fields, 5, R.diffusion3d_error(*KP), square, fe, fs)) <= BAR
    for form, (fe, fs) in (("domain", (None, None)), ("sides", sides)):
        s0, c0 = raw_values_at_nodes(mesh, rid, tight, n, KP, DOFS, fe, fs)
        s1, c1 = raw_values_at_nodes(mesh, rid, wide, ld, KP, DOFS, fe, fs)
        assert np.array_equal(c0, c1) and np.array_equal(c1, want[form][1])
        assert R.rel_max(s1, s0) <= BAR and R.rel_max(s1, want[form][0]) <= BAR


# ----------------------------------------------------------------------------------------------------------- 5. ghost nodes
@pytest.mark.parametrize("ne", [(4, 2, 2), (6, 3, 3)])
def test_fields_with_ghost_nodes(S, ctx, ne):
    """Two ranks of CubePartition(ne, 2, (2,1,1), perturb=0.1), one after the other ((4,2,2) is undistorted, see `cubes`; (6,3,3) is not): the fields are one table indexed by node_grid_id, so
    both ranks and the unpartitioned mesh see one function, and the fields of the rank with ghost nodes include them.  The ranks'
    domain integrals add up to the restatement on the whole mesh, and so do the integrals over each rank's own boundary sides.
    Measured worst relative error: 7.8e-16 on (4,2,2), 3.2e-15 on (6,3,3)."""
    p, opts, nq = 2, (2, 0, 0), 5
    whole = S.CubePartition(ne, p, perturb=0.1)
    assert (np.abs(whole.elem_verts - S.CubePartition(ne, p).elem_verts).max() > 0.01) == (ne == (6, 3, 3))
    table = np.random.default_rng(51).standard_normal((4, int(whole.node_grid_id.max()) + 1))
    total = {(form, sq): np.zeros(4) for form in ("domain", "boundary") for sq in (False, True)}
    ghosts = 0
    for rank in (0, 1):
        part = S.CubePartition(ne, p, (2, 1, 1), rank, perturb=0.1)
        ghosts += part.n_ghost_nodes
        mesh = S.DeviceMesh(ctx, part, U)
        F = dev(table[:, part.node_grid_id])
        assert F.shape[1] == part.n_owned_nodes + part.n_ghost_nodes
        fe, fs = part.boundary_sides(range(6))
        for sq in (False, True):
            total["domain", sq] += S.integrate(mesh, S.RESIDUAL_DIFFUSION3D_ERROR, F, kernel_params=KP, asm_opts=opts, square=sq)
            total["boundary", sq] += S.integrate(mesh, S.RESIDUAL_DIFFUSION3D_ERROR, F, kernel_params=KP, asm_opts=opts, square=sq,
                                                 face_elem=fe, face_side=fs)
    assert ghosts > 0
    fields = table[:, whole.node_grid_id]
    wfe, wfs = whole.boundary_sides(range(6))
    for (form, sq), got in total.items():
        faces = (None, None) if form == "domain" else (wfe, wfs)
        err = R.rel_max(got, ref_integrate(whole, fields, nq, R.diffusion3d_error(*KP), sq, *faces))
        print(f"ghost {ne} {form} square={sq}: {err:.2e}")
        assert err <= BAR


# ------------------------------------------------------------------------------------------------- 6. a probe residual plugin
def test_probe_time_and_point(S, ctx, cubes, probe_id):
    """The probe shows (d f0/dx, d f0/dy, d f0/dz, f1 (1 + t), x + 2y + 4z, grad f0 . n, n_x + 2 n_y + 4 n_z, d f1/dz n_y): time
    0 against 0.75 in integrals (nq = 3 and nq = 5 at p = 2, nq = 5 at p = 4) and at the nodes; only the fourth entry moves, by
    the factor 1.75.  The domain integral has no normal (the last three stay 0); the domain form of the nodal values hands the
    kernel a zero normal, which gives 0 as well.  Measured worst relative error: 2.5e-15."""
    worst = 0.0
    for p, opts, nq in ((2, (1, 0, 0), 3), (2, (2, 0, 0), 5), (4, (1, 0, 0), 5)):
        part, fields, sides, _ = cubes[3, p]
        mesh = S.DeviceMesh(ctx, part, U)
        F = dev(fields[:2])
        for fe, fs in ((None, None), sides):
            got = {t: S.integrate(mesh, probe_id, F, asm_opts=opts, time=t, face_elem=fe, face_side=fs) for t in (0.0, 0.75)}
            for t in got:
                worst = max(worst, R.rel_max(got[t], ref_integrate(part, fields[:2], nq, R.probe3d, False, fe, fs, time=t)))
            assert got[0.75][3] != got[0.0][3] and abs(got[0.75][3] - 1.75 * got[0.0][3]) <= BAR * np.abs(got[0.0]).max()
            assert np.array_equal(np.delete(got[0.75], 3), np.delete(got[0.0], 3))
            if fe is None:
                assert np.all(got[0.0][5:] == 0.0)
            sq = S.integrate(mesh, probe_id, F, asm_opts=opts, time=0.75, square=True, face_elem=fe, face_side=fs)
            worst = max(worst, R.rel_max(sq, ref_integrate(part, fields[:2], nq, R.probe3d, True, fe, fs, time=0.75)))
    part, fields, sides, _ = cubes[3, 2]
    mesh = S.DeviceMesh(ctx, part, 8)
    F = dev(fields[:2])
    for fe, fs in ((None, None), sides):
        gs, gc = raw_values_at_nodes(mesh, probe_id, F, F.shape[1], None, list(range(8)), fe, fs, time=0.75)
        ws, wc = ref_values_at_nodes(part, fields[:2], R.probe3d, list(range(8)), fe, fs, time=0.75, dofs_per_node=8)
        assert np.array_equal(gc, wc)
        worst = max(worst, R.rel_max(gs, ws))
        if fe is None:
            assert np.all(gs.reshape(-1, 8)[:, 5:] == 0.0)
    print(f"probe, time and point: worst {worst:.2e}")
    assert worst <= BAR


def test_probe_closed_surface_and_divergence_theorem(S, ctx, cubes, probe_id):
    """The six sides of helpers.HEX close: the integral of n_x + 2 n_y + 4 n_z over them is 0 (each side's own share is not, and is
    the restatement's).  On the perturbed cube the flux of grad T, T = x^2 + 3xy - 2yz + z^2, through the boundary sides is the
    integral of laplace T = 4 over the unit cube.  Measured: closed surface 0.0 x area; flux 4 to 1e-15, volume 1 to 1e-15."""
    opts, nq = (2, 0, 0), 5
    part = helpers.SingleElementMesh(2, helpers.HEX)
    mesh = S.DeviceMesh(ctx, part, U)
    zero = torch.zeros((2, part.n_local_nodes), dtype=torch.float64, device="cuda")
    area = ref_integrate(part, None, nq, R.unit3d, False, [0] * 6, list(range(6)))[0]
    closed = S.integrate(mesh, probe_id, zero, asm_opts=opts, face_elem=[0] * 6, face_side=list(range(6)))
    print(f"closed surface: {closed[6] / area:.2e} x area")
    assert abs(closed[6]) <= BAR * area
    for side in range(6):
        got = S.integrate(mesh, probe_id, zero, asm_opts=opts, face_elem=[0], face_side=[side])
        want = ref_integrate(part, np.zeros((2, part.n_local_nodes)), nq, R.probe3d, False, [0], [side])
        assert R.rel_max(got, want) <= BAR and abs(want[6]) > 0.1
    for ne in (2, 3):
        cube, _, sides, _ = cubes[ne, 2]
        cmesh = S.DeviceMesh(ctx, cube, U)
        T = R.poly_fields(coords(cube))[0]
        flux = S.integrate(cmesh, probe_id, dev(np.stack([T, T])), asm_opts=opts, face_elem=sides[0], face_side=sides[1])
        volume = S.integrate(cmesh, S.RESIDUAL_UNIT3D, asm_opts=opts)[0]
        print(f"ne={ne}: flux of grad T {flux[5]:.15f}, volume {volume:.15f}")
        assert volume == pytest.approx(1.0, rel=BAR) and flux[5] == pytest.approx(4.0 * volume, rel=BAR)


def test_probe_on_each_side_at_order_six(S, ctx, probe_id):
    """Random fields on helpers.HEX at p = 6, nq = 7: each of the six sides and the domain on its own, integrals and nodal values (the
    domain form with its zero normal).  Measured worst relative error: 3.8e-15."""
    p, nq = 6, 7
    part = helpers.SingleElementMesh(p, helpers.HEX)
    mesh = S.DeviceMesh(ctx, part, 8)
    fields = np.random.default_rng(66).standard_normal((2, part.n_local_nodes))
    F = dev(fields)
    worst = 0.0
    for region in REGIONS:
        fe, fs = _faces(region)
        for square in (False, True):
            got = S.integrate(mesh, probe_id, F, time=0.25, square=square, face_elem=fe, face_side=fs)
            worst = max(worst, R.rel_max(got, ref_integrate(part, fields, nq, R.probe3d, square, fe, fs, time=0.25)))
        gs, gc = raw_values_at_nodes(mesh, probe_id, F, F.shape[1], None, list(range(8)), fe, fs, time=0.25)
        ws, wc = ref_values_at_nodes(part, fields, R.probe3d, list(range(8)), fe, fs, time=0.25, dofs_per_node=8)
        assert np.array_equal(gc, wc) and gc.sum() == 8 * (343 if region is None else 49)
        worst = max(worst, R.rel_max(gs, ws))
    print(f"probe at p = 6: worst {worst:.2e}")
    assert worst <= BAR
