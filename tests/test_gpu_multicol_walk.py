"""The MULTI-COLUMN variant of the single-wave element kernel (sumfactFastKernel<..., MULTI>, csrc/device/sumfact_fast.hpp) on meshes
with MORE BATCHES THAN WAVES.  The variant applies all columns of an element batch in one pass: the column loop sits inside the
persistent batch loop, the ticket of the next batch is drawn once per batch and consumed -- together with the prefetch of the next
element's node ids and Dirichlet flag -- in the pass of the last column only, and x, y and the ghost buffers move by col * ld.  It runs
for several columns wherever a wave holds several elements (orders 1-4 with nq = p + 1, Diffusion3DPoint p = 2 / nq = 5) and the
dof layout is dense, through an R-column instance or through the one-pass plan of the single-column instance.  The other tests of
this variant stay at or below 64 elements, so each wave takes one batch and leaves: the hand-over at the end of the batch loop, the
ticket arithmetic around the column loop, the flag of a later element and the tail batch after a walk do not run there.  Here
2 G < n_batches < 3 G, n_batches % G != 0 and N % EW != 0 (G = CUs * waves per CU, the full grid; EW elements per wave), on the
production grid and with l3k_tuning::waves_per_cu = 1 (G = CUs: a few thousand elements walk) -- asserted from the route line, so
that a change of routing turns these tests red instead of hollowing them out.  Every comparison with the oracle is made per element
and per column as well as in norm: a norm over 10^6 dofs can hide one wrong element.

Tolerances (tests/test_gpu_apply.py): relative L2 1e-11 against the oracle, 1e-12 route against route, bit for bit where stated."""
import os
import re
import time
import types

import numpy as np
import pytest

import oracle_lib as O
from helpers import oracle_mesh, rel_err
from l3ster_amd import system

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ALPHA, BETA = 1.5, -0.25
TOL, TOL_ROUTES = 1e-11, 1e-12
D3, VAR, ADV = system.KERNEL_DIFFUSION3D, system.KERNEL_DIFFUSION3D_VAR, system.KERNEL_ADVDIFF3D
POINT, ADVEC, DIVCURL = system.KERNEL_DIFFUSION3D_POINT, system.KERNEL_ADVECTION3D, system.KERNEL_DIVCURL3D
KPAR = {D3: [0.7, 1.0], ADV: [0.7, 1.3, 0.5], POINT: [0.8, 1.2], ADVEC: [0.05], DIVCURL: [0.6]}
NTHREADS = min(16, len(os.sched_getaffinity(0)))  # oracle threads
WALK = dict(waves_per_cu=1)  # the cheap way to a walk: one wave per CU


@pytest.fixture(scope="module")
def ctx():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    torch.cuda.set_device(0)
    return system.Context(0, torch.cuda.current_stream().cuda_stream)


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")


ROUTE = re.compile(r"sumfactFastKernel<p=(\d+),nq=(\d+),U=(\d+),F=(\d+)>.*: one wave per (\d+) element\(s\), .* (\d+) waves/CU x (\d+) CUs = "
                   r"grid (\d+), (static|dynamic) batches")


def parse_route(line):
    m = ROUTE.search(line)
    assert m, line
    p, nq, U, F, ew, waves_cu, cus, grid = (int(v) for v in m.groups()[:8])
    return types.SimpleNamespace(p=p, nq=nq, U=U, F=F, ew=ew, waves_cu=waves_cu, cus=cus, grid=grid, deal=m.group(9), full=waves_cu * cus)


def walk_dims(G, EW):
    """(a, b, c), a >= b >= c: the smallest mesh among the most cube-like ones with 2 G < ceil(N / EW) < 3 G, ceil(N / EW) % G != 0
    and N % EW != 0 -- every wave walks two batches, some a third, and the last batch is a partial one"""
    for spread in range(0, 64):  # a - c <= spread
        best = None
        for c in range(1, 96):
            for b in range(c, c + spread + 1):
                for a in range(b, c + spread + 1):
                    n = a * b * c
                    nb = -(-n // EW)
                    if 2 * G < nb < 3 * G and nb % G != 0 and n % EW != 0 and (best is None or n < best[0]):
                        best = (n, (a, b, c))
        if best:
            return best[1]
    raise AssertionError(f"no mesh for a grid of {G} waves of {EW} elements")


def assert_walk(line, n_elems, waves_per_cu=0):
    """the walk inequalities of a launch over n_elems elements, from its route line; returns the parsed line"""
    r = parse_route(line)
    nb = -(-n_elems // r.ew)
    assert r.grid == r.full, f"the launch does not fill the grid: {line}"
    assert 2 * r.full < nb < 3 * r.full and nb % r.full != 0 and n_elems % r.ew != 0, (n_elems, nb, line)
    if waves_per_cu:
        assert r.waves_cu == waves_per_cu and r.grid == waves_per_cu * r.cus, line
    else:
        assert r.waves_cu > 1, line  # the production grid: as many waves per CU as LDS and registers allow
    return r


def make_system(ctx, part, kid, vo=1, n_rhs=1, dirichlet=True, fields_seed=3):
    info = system.kernel_info(kid)
    U, F = info["n_unknowns"], info["n_fields"]
    mask = part.dirichlet_mask(U) if dirichlet else None  # unknown 0 on the six sides of the cube (benchmarks/Diffusion3D.hpp:39-41)
    mf = system.MatrixFreeSystem(system.DeviceMesh(ctx, part, U, mask), kid, KPAR.get(kid), asm_opts=(vo, 0, 0), n_rhs=n_rhs)
    fields = np.random.default_rng(fields_seed).uniform(-1, 1, (F, part.n_local_nodes)) if F else None
    if F:
        mf.set_fields(dev(fields))
    return mf, mask, fields


class Case:
    """one kernel shape on a mesh sized for a walk of `ncols`-column launches under the tuning `tune`: the mesh, the operands
    (host) and the system on `ctx`"""

    def __init__(self, ctx, kid, p, vo, ncols, n_rhs=None, tune=WALK, perturb=0.1, dims=None):
        info = system.kernel_info(kid)
        self.ctx, self.kid, self.p, self.vo, self.ncols, self.tune = ctx, kid, p, vo, ncols, dict(tune)
        self.U, self.F, self.nq = info["n_unknowns"], info["n_fields"], system.n_qps1d(p, vo)
        self.n_rhs = n_rhs or ncols
        assert (kid, p, self.nq, 1) in system.instances(), f"shape ({kid}, {p}, {self.nq}) is not compiled in"
        with ctx.tuning(**self.tune):
            if dims is None:
                # G and EW from the route line of this shape (the grid depends on the mesh only through min(n_batches, G))
                probe, _, _ = make_system(ctx, system.CubePartition(2, p), kid, vo, self.n_rhs)
                r = parse_route(probe.route(2, ncols))
                dims = walk_dims(r.full, r.ew)
            self.dims = dims
            self.part = part = system.CubePartition(dims, p, perturb=perturb)
            self.mf, self.mask, self.fields = make_system(ctx, part, kid, vo, self.n_rhs)
        self.n = part.n_local_nodes * self.U
        self.x = part.synthetic_vector(self.U, ncols=ncols)  # independent columns: a column mix-up does not cancel
        self.y0 = np.random.default_rng(1).uniform(-1, 1, self.x.shape)
        self.elem_dofs = elem_dofs(part, self.U)
        self._ref = {}

    def route(self, which=2, ncols=None):
        return self.mf.route(which, self.ncols if ncols is None else ncols)

    def assert_multi_walk(self, which=2):
        line = self.route(which)
        assert f"sumfactFastKernel<p={self.p},nq={self.nq},U={self.U},F={self.F}>" in line and " multi-column" in line, line
        assert "column by column" not in line and "one per column" not in line, line
        return assert_walk(line, self.part.n_elems, self.tune.get("waves_per_cu", 0))

    def oracle(self, alpha=ALPHA, beta=BETA):
        """alpha A x + beta y0 of all columns on the whole mesh (threaded); [n_dofs, ncols]"""
        if (alpha, beta) not in self._ref:
            om = oracle_mesh(self.part, self.nq, self.U, np.arange(self.U), self.mask, self.fields)
            t0 = time.perf_counter()
            self._ref[(alpha, beta)] = O.mf_apply(om, self.kid, self.x.T, np.asfortranarray(self.y0.T.copy()), alpha=alpha, beta=beta,
                                                  kparams=KPAR.get(self.kid), nthreads=NTHREADS)
            print(f"oracle: {self.part.n_elems} elements of order {self.p}, {self.ncols} columns on {NTHREADS} threads: {time.perf_counter() - t0:.1f} s")
        return self._ref[(alpha, beta)]

    def apply(self, alpha=ALPHA, beta=BETA, ncols=None):
        nc = self.ncols if ncols is None else ncols
        X, Y = dev(self.x[:nc]), dev(self.y0[:nc])
        self.mf.apply(X, Y, alpha, beta)
        torch.cuda.synchronize()
        assert np.array_equal(X.cpu().numpy(), self.x[:nc])
        return Y.cpu().numpy()


def elem_dofs(part, U):
    return (part.elem_nodes.astype(np.int64)[:, :, None] * U + np.arange(U)).reshape(part.n_elems, -1)


def check(got, ref, edofs, ew, what, tol=TOL):
    """got [ncols, n], ref [n, ncols]: the relative L2 error over everything, then per column max |got - ref| over the dofs of each
    element against tol * max |ref| of the column -- the worst element is named with its batch e // EW"""
    got, ref = np.asarray(got), np.asarray(ref).T
    assert got.shape == ref.shape, (got.shape, ref.shape)
    r = rel_err(got, ref)
    for c in range(got.shape[0]):
        per_elem = np.abs(got[c] - ref[c])[edofs].max(axis=1)
        w = int(np.argmax(per_elem))
        bound = tol * np.abs(ref[c]).max()
        print(f"{what}, column {c}: rel err (all columns) {r:.3e}; worst element {w} (batch {w // ew}): {per_elem[w]:.3e}, bound {bound:.3e}")
        n_bad = int((per_elem > bound).sum())
        first_bad = int(np.argmax(per_elem > bound)) if n_bad else -1
        assert n_bad == 0, (f"{what}, column {c}: {n_bad} of {len(per_elem)} elements beyond {bound:.3e}; worst element {w} (batch {w // ew}) "
                            f"max |err| {per_elem[w]:.3e}; first bad element {first_bad} (batch {first_bad // ew}); rel err {r:.3e}")
    assert r < tol, f"{what}: rel err {r:.3e}"


# ------------------------------------------------------------------------------------ 2. values against the oracle
SHAPES = [
    # kernel, p, value order (nq = vo * p + 1), columns, entry, grid
    (D3, 2, 1, 2, "instance", "production"),  # the 2-column instance: launchColumnsFast (3.6e4 elements on 2048 waves of 7)
    (D3, 4, 1, 3, "one-pass", "production"),  # Instance::apply_cols of the single-column instance (1e4 elements)
    (D3, 4, 1, 2, "one-pass", "walk"),
    (D3, 1, 1, 2, "one-pass", "walk"),  # 16 elements per wave
    (D3, 3, 1, 2, "one-pass", "walk"),  # 4
    (ADV, 2, 1, 2, "instance", "walk"),  # external fields (F = 3), fetched again in every column's pass
    (ADV, 4, 1, 2, "one-pass", "walk"),
    (VAR, 4, 1, 2, "one-pass", "walk"),
    (DIVCURL, 2, 1, 2, "one-pass", "walk"),  # odd numbers of unknowns: 8-byte stores on the exclusive rows
    (DIVCURL, 4, 1, 2, "one-pass", "walk"),
    (ADVEC, 2, 1, 2, "one-pass", "walk"),
    (ADVEC, 4, 1, 2, "one-pass", "walk"),
    (POINT, 2, 2, 2, "one-pass", "walk"),  # nq = 5 > p + 1
]


@pytest.mark.parametrize("kid,p,vo,ncols,entry,grid", SHAPES)
def test_walk_values_vs_oracle(ctx, kid, p, vo, ncols, entry, grid):
    """y <- alpha A x + beta y (perturbed mesh, Dirichlet on the cube sides, random y0 and fields, independent columns) of a launch in
    which every wave walks two or three batches, against the oracle on the same mesh: everything in norm, every element of every column"""
    nq = system.n_qps1d(p, vo)
    assert ((kid, p, nq, ncols) in system.instances()) == (entry == "instance"), (kid, p, nq, ncols, entry)
    c = Case(ctx, kid, p, vo, ncols, tune=WALK if grid == "walk" else {})
    with ctx.tuning(**c.tune):
        r = c.assert_multi_walk()
        print(f"{c.part.n_elems} elements {c.dims}, {-(-c.part.n_elems // r.ew)} batches on a grid of {r.grid}: {c.route()}")
        y = c.apply()
        assert {"launched", "multi-column", "dynamic"} <= system.last_fast_launch(), system.last_fast_launch()
    check(y, c.oracle(), c.elem_dofs, r.ew, f"kernel {kid} p = {p} nq = {nq}, {ncols} columns ({entry}, {grid} grid)")


# ------------------------------------------------------------------------------------ 3. the other routes as cross-checks
@pytest.fixture(scope="module")
def cases(ctx):
    """the cases with one wave per CU that several tests share, made once each and dropped -- systems, meshes, device memory -- when
    the file ends"""
    made = {}

    def get(kid, p, vo=1, ncols=2, n_rhs=None, perturb=0.1):
        key = (kid, p, vo, ncols, n_rhs, perturb)
        if key not in made:
            made[key] = Case(ctx, kid, p, vo, ncols, n_rhs=n_rhs, perturb=perturb)
        return made[key]

    yield get
    made.clear()


@pytest.mark.parametrize("kid,p", [(D3, 4), (DIVCURL, 2)])
def test_column_by_column_and_static_deal_agree(ctx, cases, kid, p):
    """the same operands through l3k_tuning::column_by_column (single-column launches) and through the static deal of the multi-column
    variant (batch + stride instead of tickets): route lines asserted, results equal to the one-pass result to 1e-12"""
    c = cases(kid, p)
    with ctx.tuning(**WALK):
        r = c.assert_multi_walk()
        assert r.deal == "dynamic"
        y = c.apply()
        with ctx.tuning(column_by_column=1):
            line = c.route()
            assert "column by column" in line and "multi-column" not in line and "sumfactFastKernel" in line, line
            y_cols = c.apply()
        with ctx.tuning(static_deal=1):
            line = c.route()
            assert "static batches" in line and " multi-column" in line, line
            assert_walk(line, c.part.n_elems, 1)
            y_static = c.apply()
        assert "dynamic batches" in c.route() and " multi-column" in c.route()
    assert rel_err(y_cols, y) < TOL_ROUTES and rel_err(y_static, y) < TOL_ROUTES, (rel_err(y_cols, y), rel_err(y_static, y))
    check(y_cols, c.oracle(), c.elem_dofs, r.ew, "column by column")
    check(y_static, c.oracle(), c.elem_dofs, r.ew, "static deal")


@pytest.mark.parametrize("p,multi", [(4, False), (2, True)])
def test_deterministic_mode_agrees(ctx, cases, p, multi):
    """a context in deterministic mode (one launch per colour; the one-pass plan is not taken, the 2-column instance keeps the
    multi-column variant): bit for bit reproducible, and equal to the one-pass result to 1e-12.  A cross-check: the launches of
    the deterministic context cover one colour each and are not asserted to walk; the one-pass launch it is compared with is."""
    c = cases(D3, p)
    with ctx.tuning(**WALK):
        c.assert_multi_walk()
        y = c.apply()
    ctxd = system.Context(0, torch.cuda.current_stream().cuda_stream)
    ctxd.set_deterministic(True)
    ctxd.set_tuning(**WALK)
    mf, _, _ = make_system(ctxd, c.part, D3, 1, 2)
    line = mf.route(2, 2)
    assert "deterministic" in line and "sumfactFastKernel" in line and (" multi-column" in line) == multi, line
    assert ("column by column" in line) == (not multi), line
    runs = []
    for _ in range(2):
        X, Y = dev(c.x), dev(c.y0)
        mf.apply(X, Y, ALPHA, BETA)
        torch.cuda.synchronize()
        runs.append(Y)
    assert torch.equal(runs[0], runs[1])
    assert rel_err(runs[0].cpu().numpy(), y) < TOL_ROUTES


def test_no_affine_and_multi_column_on_a_uniform_mesh(ctx, cases):
    """an unperturbed mesh: the single-column launch takes the affine variant (one Jacobian per element), l3k_tuning::no_affine takes it
    away (route asserted) and changes the result by rounding only; the multi-column variant, which never takes it, agrees with the
    affine single-column launches column by column, and with the oracle"""
    c = cases(D3, 4, perturb=0.0)
    with ctx.tuning(**WALK):
        line = c.route(ncols=1)
        assert " affine" in line and "multi-column" not in line, line
        cols_affine = np.concatenate([run_columns(c, [k]) for k in range(c.ncols)])
        with ctx.tuning(no_affine=1):
            line = c.route(ncols=1)
            assert " affine" not in line and "sumfactFastKernel" in line and "multi-column" not in line, line
            col0_plain = run_columns(c, [0])
        r = c.assert_multi_walk()
        assert " affine" not in c.route()
        y = c.apply()
    assert rel_err(col0_plain, cols_affine[:1]) < TOL_ROUTES
    assert rel_err(y, cols_affine) < TOL_ROUTES
    check(y, c.oracle(), c.elem_dofs, r.ew, "multi-column, uniform mesh")
    check(cols_affine, c.oracle(), c.elem_dofs, r.ew, "affine, column by column")


def run_columns(c, cols, alpha=ALPHA, beta=BETA):
    X, Y = dev(c.x[cols]), dev(c.y0[cols])
    c.mf.apply(X, Y, alpha, beta)
    torch.cuda.synchronize()
    return Y.cpu().numpy()


# ------------------------------------------------------------------------------------ 4. layout and range edges, at walking size
@pytest.fixture(scope="module")
def edge(cases):
    """Diffusion3D, order 4 (two elements per wave), created for three columns, on the mesh that walks with one wave per CU"""
    return cases(D3, 4, ncols=2, n_rhs=3)


def test_padded_unequal_leading_dimensions(ctx, edge):
    """ldx != ldy, both even and larger than the number of rows; the padding of both columns and a third, unused column keep their
    canary values bit for bit, x is not written"""
    c, n = edge, edge.n
    ldx, ldy = n + 6, n + 10
    assert n % 2 == 0
    Xb = torch.full((3, ldx), 7.25, dtype=torch.float64, device="cuda")
    Yb = torch.full((3, ldy), -3.5, dtype=torch.float64, device="cuda")
    Xb[:2, :n], Yb[:2, :n] = dev(c.x), dev(c.y0)
    X0 = Xb.clone()
    with ctx.tuning(**WALK):
        r = c.assert_multi_walk()
        c.mf.apply(Xb[:2, :n], Yb[:2, :n], ALPHA, BETA)
        torch.cuda.synchronize()
    assert torch.equal(Xb, X0)
    out = Yb.cpu().numpy()
    assert np.all(out[:2, n:] == -3.5) and np.all(out[2] == -3.5)
    check(out[:2, :n], c.oracle(), c.elem_dofs, r.ew, "padded leading dimensions")


def test_beta_zero_overwrites_nan(ctx, edge):
    """beta = 0 is an overwrite: NaN in y0 does not survive -- exclusive rows are stored without a read, the shell rows after l3k_mf_scale"""
    c = edge
    with ctx.tuning(**WALK):
        r = c.assert_multi_walk()
        X = dev(c.x)
        Y = torch.full_like(X, float("nan"))
        c.mf.apply(X, Y, ALPHA, 0.0)
        torch.cuda.synchronize()
    assert torch.isfinite(Y).all()
    check(Y.cpu().numpy(), c.oracle(ALPHA, 0.0), c.elem_dofs, r.ew, "beta = 0 over NaN")


def test_fewer_columns_than_n_rhs(ctx, edge):
    """a system created for three columns applied to two (one pass of the multi-column variant) and to one (the single-column kernel)"""
    c = edge
    assert c.mf.n_rhs == 3
    with ctx.tuning(**WALK):
        r = c.assert_multi_walk()
        y2 = c.apply()
        line = c.route(ncols=1)
        assert "multi-column" not in line and "sumfactFastKernel" in line, line
        y1 = c.apply(ncols=1)
    check(y2, c.oracle(), c.elem_dofs, r.ew, "2 of 3 columns")
    check(y1, c.oracle()[:, :1], c.elem_dofs, r.ew, "1 of 3 columns")


def test_element_sub_ranges_single_rank(ctx, edge):
    """l3k_mf_scale once, then the two halves of the interior (which = 3, 4: the second is the only launch with elem_begin != 0, and an
    odd element count makes the halves unequal; each half has more batches than waves, so part of the waves take a second one)
    against the one launch over everything"""
    c = edge
    N = c.part.n_interior_elems
    assert N == c.part.n_elems and N % 2 == 1
    out = []
    with ctx.tuning(**WALK):
        r = c.assert_multi_walk()
        for which in (3, 4):
            line = c.route(which)
            h = parse_route(line)
            assert " multi-column" in line and h.grid == h.full == r.full and -(-(N // 2) // h.ew) > h.full, line  # more than one batch for some waves of each half
        for sequence in ([2], [3, 4]):
            X, Y = dev(c.x), dev(c.y0)
            c.mf.scale(Y, BETA)
            for which in sequence:
                c.mf.apply_elems(which, X, None, Y, None, ALPHA, BETA)
            c.mf.dirichlet_rows(X, Y, ALPHA)
            torch.cuda.synchronize()
            out.append(Y.cpu().numpy())
    assert rel_err(out[1], out[0]) < TOL_ROUTES
    check(out[1], c.oracle(), c.elem_dofs, r.ew, "which = 3 + 4")


@pytest.fixture(scope="module")
def rank_case(ctx, edge):
    """rank 1 of a (2, 1, 1) partition whose local block is the walking mesh of `edge`: a rank with ghost nodes"""
    a, b, cc = edge.dims
    part = system.CubePartition((2 * a, b, cc), 4, parts=(2, 1, 1), rank=1, perturb=0.1)
    assert part.n_elems == edge.part.n_elems and part.n_ghost_nodes > 0 and 0 < part.n_interior_elems < part.n_elems
    with ctx.tuning(**WALK):
        mf, mask, _ = make_system(ctx, part, D3, 1, 2)
    U = 4
    no, ng = part.n_owned_nodes * U, part.n_ghost_nodes * U
    x = part.synthetic_vector(U, ncols=2)
    y0 = np.random.default_rng(2).uniform(-1, 1, (2, no))
    return types.SimpleNamespace(part=part, mf=mf, mask=mask, no=no, ng=ng, x=x, y0=y0, edofs=elem_dofs(part, U))


def _split_run(rc, sequence):
    """ghost rows in buffers of their own (ldxg = ldyg = n_ghost_dofs != n_owned_dofs): returns [y | y_ghost] (2, n_local_dofs)"""
    X, XG = dev(rc.x[:, :rc.no]), dev(rc.x[:, rc.no:])
    Y, YG = dev(rc.y0), torch.zeros((2, rc.ng), dtype=torch.float64, device="cuda")
    rc.mf.scale(Y, BETA)
    for which in sequence:
        rc.mf.apply_elems(which, X, XG, Y, YG, ALPHA, BETA)
    torch.cuda.synchronize()
    return np.concatenate([Y.cpu().numpy(), YG.cpu().numpy()], axis=1)


def test_split_ghost_buffers(ctx, rank_case):
    """MULTI x SPLIT: apply_elems(2) of a rank with ghosts, ghost rows in buffers of their own, against (a) the same call with the
    ghost rows directly behind the owned rows of each column (one leading dimension for both: the variant without the owned-or-ghost
    select) and (b) the oracle on the rank's local mesh with the ghost rows as ordinary rows.  The route line of l3k_mf_route is
    made without the operands and shows the ghost-buffer variant for every launch over border elements of such a mesh, so the
    variant each of the two calls really launched is taken from l3k_last_fast_launch."""
    rc = rank_case
    no, ng, nl = rc.no, rc.ng, rc.no + rc.ng
    assert no != ng and no % 2 == 0 and ng % 2 == 0
    with ctx.tuning(**WALK):
        line = rc.mf.route(2, 2)
        assert " split-ghost" in line and " multi-column" in line, line
        r = assert_walk(line, rc.part.n_elems, 1)
        line0 = rc.mf.route(0, 2)
        assert "split-ghost" not in line0 and " multi-column" in line0, line0
        split = _split_run(rc, [2])
        assert {"launched", "split-ghost", "multi-column"} <= system.last_fast_launch(), system.last_fast_launch()
        xc = dev(rc.x)
        yc = torch.zeros((2, nl), dtype=torch.float64, device="cuda")
        yc[:, :no] = dev(rc.y0)
        rc.mf.scale(yc[:, :no], BETA)
        rc.mf.apply_elems(2, xc[:, :no], xc[:, no:], yc[:, :no], yc[:, no:], ALPHA, BETA)
        launched = system.last_fast_launch()
        assert {"launched", "multi-column"} <= launched and "split-ghost" not in launched, launched
        torch.cuda.synchronize()
    assert np.abs(split[:, no:]).max() > 0.0  # the export buffer received something, in both columns
    assert np.abs(split[0, no:]).max() > 0.0 and np.abs(split[1, no:]).max() > 0.0
    assert rel_err(yc.cpu().numpy(), split) < TOL_ROUTES
    om = oracle_mesh(rc.part, 5, 4, np.arange(4), rc.mask)
    y0 = np.zeros((nl, 2), order="F")
    y0[:no] = rc.y0.T
    ref = O.mf_apply(om, D3, rc.x.T, y0, alpha=ALPHA, beta=BETA, kparams=KPAR[D3], do_dirichlet_rows=False, nthreads=NTHREADS)
    check(split, ref, rc.edofs, r.ew, "ghost rows in buffers of their own")
    check(yc.cpu().numpy(), ref, rc.edofs, r.ew, "ghost rows behind the owned rows")


def test_element_sub_ranges_partitioned_rank(ctx, rank_case):
    """interior (0) + border (1) launches of a rank with ghosts equal the launch over all its elements (2)"""
    with ctx.tuning(**WALK):
        for which in (0, 1):
            assert " multi-column" in rank_case.mf.route(which, 2)
        both, parts = _split_run(rank_case, [2]), _split_run(rank_case, [0, 1])
    assert rel_err(parts, both) < TOL_ROUTES


def test_apply_dist_two_columns_two_ranks():
    """l3k_mf_apply_dist with two columns on two ranks (threads, in-process transport), every rank's context with one wave per CU and
    halves of the interior that each have more batches than waves: against the oracle on the whole mesh"""
    from test_gpu_dist_cabi import check_against_whole, run_ranks
    from l3ster_amd.distributed import InprocGroup, NativeDistributedOperator, NativeHalo
    torch.cuda.set_device(0)
    p, U, ncols, parts = 4, 4, 2, (2, 1, 1)
    probe_ctx = system.Context(0, torch.cuda.current_stream().cuda_stream)
    probe_ctx.set_tuning(**WALK)
    probe, _, _ = make_system(probe_ctx, system.CubePartition(2, p), D3, 1, ncols)
    pr = parse_route(probe.route(2, ncols))
    a, b, cc = walk_dims(pr.full, pr.ew)
    ne = (2 * (a + 1), b, cc)  # a layer of border elements on top of an interior of the walking size
    group = InprocGroup(2)
    out = {}

    def body(rank):
        part = system.CubePartition(ne, p, parts, rank, perturb=0.1)
        c = system.Context(0, torch.cuda.current_stream().cuda_stream)
        c.set_tuning(**WALK)
        mf = system.MatrixFreeSystem(system.DeviceMesh(c, part, U, part.dirichlet_mask(U)), D3, KPAR[D3], n_rhs=ncols)
        for which in (3, 4):
            line = mf.route(which, ncols)
            h = parse_route(line)
            assert " multi-column" in line and h.waves_cu == 1 and h.grid == h.cus == pr.full, line
            assert -(-(part.n_interior_elems // 2) // h.ew) > h.grid, (part.n_interior_elems, line)  # more than one batch for some waves of each half
        if part.n_ghost_nodes > 0:  # (the lower rank owns the shared nodes: it has no border elements)
            assert " multi-column" in mf.route(1, ncols) and " split-ghost" in mf.route(1, ncols), mf.route(1, ncols)
        n_owned = part.n_owned_nodes * U
        X = dev(part.synthetic_vector(U, ncols=ncols)[:, :n_owned])
        Y = dev(part.synthetic_vector(U, seed=7, ncols=ncols)[:, :n_owned])
        op = NativeDistributedOperator(mf, NativeHalo(c, part, U, rank, 2, transport=group))
        for _ in range(2):  # (the import / export buffers are reused)
            Yc = Y.clone()
            op.apply(X, Yc, ALPHA, BETA)
        torch.cuda.current_stream().synchronize()
        out[rank] = (Yc.cpu().numpy(), part.node_grid_id[:part.n_owned_nodes].copy())

    run_ranks(2, body)
    whole = system.CubePartition(ne, p, perturb=0.1)
    x, y0 = whole.synthetic_vector(U, ncols=ncols), whole.synthetic_vector(U, seed=7, ncols=ncols)
    y_ref = O.mf_apply(oracle_mesh(whole, p + 1, U, np.arange(U), whole.dirichlet_mask(U)), D3, x.T, np.asfortranarray(y0.T.copy()),
                       alpha=ALPHA, beta=BETA, kparams=KPAR[D3], nthreads=NTHREADS)
    check_against_whole(out, whole, y_ref, ncols)
    # ... and row by row (a norm over the rank's rows can hide a few wrong ones)
    row_of = np.full(int(whole.node_grid_id.max()) + 1, -1, np.int64)
    row_of[whole.node_grid_id] = np.arange(whole.n_local_nodes)
    for rank, (y, gid) in out.items():
        ref = y_ref.reshape(whole.n_local_nodes, U, ncols)[row_of[gid]]
        got = y.reshape(ncols, len(gid), U).transpose(1, 2, 0)
        assert np.abs(got - ref).max() < TOL * np.abs(ref).max(), rank


def test_energy_armed_with_several_columns(ctx, edge):
    """l3k_mf_energy_begin, a two-column element launch, l3k_mf_energy_end: nothing was fused and s[1] stays 0 (the caller takes the
    dot product); a single-column l3k_mf_apply_energy afterwards still gives <x, A x>"""
    c = edge
    with ctx.tuning(**WALK):
        c.assert_multi_walk()
        X = dev(c.x)
        Y = torch.zeros_like(X)
        S = torch.full((8,), 7.0, dtype=torch.float64, device="cuda")
        c.mf.energy_begin(S)
        c.mf.apply_elems(2, X, None, Y, None, 1.0, 0.0)
        fused = c.mf.energy_end(X)
        torch.cuda.synchronize()
        s = S.cpu().numpy()
        assert not fused and s[1] == 0.0 and np.all(s[[0, 2, 3, 4, 5, 6, 7]] == 7.0), (fused, s)
        line = c.mf.route(2, 1, with_energy=True)
        assert " energy" in line and "multi-column" not in line, line
        Y1 = torch.full_like(X[:1], 3.0)
        c.mf.apply_energy(X[:1], Y1, S)
        Yr = torch.zeros_like(X[:1])
        c.mf.apply(X[:1], Yr)
        torch.cuda.synchronize()
    want = torch.dot(X[0], Yr[0]).item()
    assert float((Y1 - Yr).abs().max()) <= 1e-12 * float(Yr.abs().max())
    assert abs(float(S[1]) - want) <= 1e-12 * abs(want), (float(S[1]), want)


def test_misaligned_columns_are_refused(ctx, edge):
    """two columns with an odd leading dimension, or from a base that is 8 bytes off a 16-byte boundary: the "16-byte aligned" error
    from l3k_mf_apply_elems and from l3k_mf_apply, and nothing is launched -- not the scaling pass of l3k_mf_apply (beta != 1)
    either: the output is as it was"""
    c, n = edge, edge.n
    X, Y0 = dev(c.x), dev(c.y0)
    odd = torch.zeros((2, n + 1), dtype=torch.float64, device="cuda")
    flat = torch.zeros(2 * n + 2, dtype=torch.float64, device="cuda")
    off = flat[1:1 + 2 * n].view(2, n)
    assert off.data_ptr() % 16 == 8 and odd[:, :n].stride(0) % 2 == 1
    with ctx.tuning(**WALK):
        for what, Xa, Ya in [("odd ldx", odd[:, :n], None), ("odd ldy", X, odd[:, :n]), ("x off by 8 bytes", off, None),
                             ("y off by 8 bytes", X, off)]:
            if Ya is None:
                Xa.copy_(X)
                Ya = Y0.clone()
            else:
                Ya.copy_(Y0)
            before = Ya.clone()
            with pytest.raises(system.L3KError, match="16-byte aligned"):
                c.mf.apply_elems(2, Xa, None, Ya, None, ALPHA, BETA)
            with pytest.raises(system.L3KError, match="16-byte aligned"):
                c.mf.apply(Xa, Ya, ALPHA, BETA)
            torch.cuda.synchronize()
            assert torch.equal(Ya, before), what
