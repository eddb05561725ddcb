"""The order-6 one-wave-per-element kernel with its gather one element ahead (FastCfg::gather_ahead, device/sumfact_fast.hpp):
a wave requests the next element's node ids behind the x-pencil stage and its x rows behind the I^T-y stage of the current
element, so the first and the last element of a wave (prologue, epilogue), the walk in between, the switch to another XCD's
counter, the Dirichlet-flagged elements, the beta != 0 exclusive rows and the SPLIT / ENERGY variants each take code of their own.

Every case: Diffusion3D on a perturbed cube (perturb = 0.1), the one-wave kernel also on the smallest meshes (generic_below = 0),
against the CPU oracle on the same mesh and x; relative L2 <= 1e-11, the project's mesh-level tolerance.

The walking mesh is 12 x 11 x 11 = 1 452 elements, not 12^3 = 1 728: with one wave per CU on 256 CUs the XCD-chunked deal gives
every XCD ceil(n / 8) consecutive elements, and 1 728 = 8 * 216 leaves all eight chunks equal, so that a wave changes to another
XCD's counter only by the accident of timing.  1 452 = 7 * 182 + 178 is the nearest size with unequal chunks: the last XCD runs
dry four elements early and its waves continue on the next counter (about 5.7 elements per wave: prologue, steady state, epilogue)."""
import os

import numpy as np
import pytest

import oracle_lib as O
from helpers import oracle_mesh, rel_err
from l3ster_amd import system

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

U, KID, TOL = 4, system.KERNEL_DIFFUSION3D, 1e-11
WALK_NE = (12, 11, 11)
NTHREADS = min(16, len(os.sched_getaffinity(0)))


@pytest.fixture(scope="module")
def ctx():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    torch.cuda.set_device(0)
    c = system.Context(0, torch.cuda.current_stream().cuda_stream)
    c.set_tuning(generic_below=0)
    return c


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")


class Case:
    """One mesh with its device system, x, a non-zero y0 and the oracle's view of it (built once per mesh and mask)."""

    def __init__(self, ctx, ne, p, dirichlet=True):
        self.p = p
        self.part = system.CubePartition(ne, p, perturb=0.1)
        full = self.part.dirichlet_mask(U)
        self.mask = full if dirichlet else np.zeros_like(full)
        self.mf = system.MatrixFreeSystem(system.DeviceMesh(ctx, self.part, U, self.mask), KID)
        self.x = self.part.synthetic_vector(U)
        self.y0 = np.random.default_rng(5).uniform(-1, 1, self.x.shape)
        self.om = oracle_mesh(self.part, p + 1, U, np.arange(U), self.mask)

    def reference(self, alpha=1.0, beta=0.0):
        return O.mf_apply(self.om, KID, self.x.T, np.asfortranarray(self.y0.T.copy()), alpha=alpha, beta=beta, nthreads=NTHREADS)

    def error(self, alpha=1.0, beta=0.0):
        X, Y = dev(self.x), dev(self.y0)
        self.mf.apply(X, Y, alpha, beta)
        torch.cuda.synchronize()
        err = rel_err(Y.cpu().numpy().T, self.reference(alpha, beta))
        print(f"p={self.p} elems={self.part.n_elems} alpha={alpha} beta={beta}: rel L2 {err:.3e}")
        return err


def assert_order6_fast(line):
    assert "sumfactFastKernel<p=6,nq=7,U=4,F=0>" in line and "one wave per 1 element(s)" in line, line


@pytest.mark.parametrize("n", [1, 2, 3])
def test_elements_in_a_row(ctx, n):
    """1, 2 and 3 elements: a launch of one wave without a successor, of waves that are prologue and epilogue only (grid = number
    of elements: the ticket after a wave's first element is beyond the end), and -- with the static deal -- the same by stride"""
    c = Case(ctx, (n, 1, 1), 6)
    assert_order6_fast(c.mf.route())
    assert c.error() < TOL
    with ctx.tuning(static_deal=1):
        assert "static batches" in c.mf.route(), c.mf.route()
        assert c.error() < TOL


@pytest.fixture(scope="module")
def walk(ctx):
    return Case(ctx, WALK_NE, 6)


def grid_of(line):
    return int(line.split("= grid ")[1].split(",")[0])


@pytest.mark.parametrize("static", [0, 1])
def test_walk_one_wave_per_cu(ctx, walk, static):
    """every wave walks several elements: dynamic deal (XCD-chunked, unequal chunks: see the module docstring) and static deal"""
    with ctx.tuning(waves_per_cu=1, static_deal=static):
        line = walk.mf.route()
        assert_order6_fast(line)
        grid, n = grid_of(line), walk.part.n_elems
        assert "1 waves/CU" in line and grid % 8 == 0 and n >= 4 * grid, line  # at least four elements per wave
        if static:
            assert "static batches" in line, line
        else:
            assert "dynamic batches" in line and "XCD-chunked" in line, line
            chunk = -(-n // 8)
            assert 0 < n - 7 * chunk < chunk, (n, chunk)  # the last XCD's chunk is the shorter one
        assert walk.error() < TOL
        assert ("dynamic" in system.last_fast_launch()) == (not static), system.last_fast_launch()


def test_walk_beta_on_nonzero_y(ctx, walk):
    """beta = 0.5 on a non-zero y: the element-exclusive rows are read, scaled and stored by the element kernel itself"""
    with ctx.tuning(waves_per_cu=1):
        assert walk.error(alpha=1.0, beta=0.5) < TOL
        assert walk.error(alpha=-0.75, beta=0.5) < TOL


@pytest.mark.parametrize("dirichlet", [True, False])
def test_walk_dirichlet_sides(ctx, walk, dirichlet):
    """Dirichlet on all six sides (flagged and unflagged elements side by side in every wave's walk) and on none (no flagged element)"""
    c = walk if dirichlet else Case(ctx, WALK_NE, 6, dirichlet=False)
    assert bool(c.mask.any()) == dirichlet
    with ctx.tuning(waves_per_cu=1):
        assert c.error() < TOL
    assert c.error() < TOL  # the production grid: at most one element per wave


def test_split_ghost_buffers_two_parts(ctx):
    """SPLIT variant: the upper half of an 8 x 4 x 4 mesh cut in two (the rank with ghost nodes), ghost rows of x and y in buffers of
    their own, the element launches of the partitioned apply -- first interior half, border elements, second interior half --
    against the oracle on the rank's local mesh with the ghost rows as ordinary rows (no Dirichlet-row pass: that is the caller's)"""
    p = 6
    part = system.CubePartition((8, 4, 4), p, (2, 1, 1), 1, perturb=0.1)
    assert part.n_ghost_nodes > 0
    mask = part.dirichlet_mask(U)
    mf = system.MatrixFreeSystem(system.DeviceMesh(ctx, part, U, mask), KID)
    no, ng = part.n_owned_nodes * U, part.n_ghost_nodes * U
    assert no != ng
    x = part.synthetic_vector(U)
    alpha = 1.25
    om = oracle_mesh(part, p + 1, U, np.arange(U), mask)
    ref = O.mf_apply(om, KID, x.T, np.zeros((no + ng, 1), order="F"), alpha=alpha, beta=0.0, do_dirichlet_rows=False, nthreads=NTHREADS)
    for tune in (dict(), dict(waves_per_cu=1, static_deal=1)):
        with ctx.tuning(**tune):
            line = mf.route(1)
            assert_order6_fast(line)
            assert " split-ghost" in line, line
            X, XG = dev(x[:, :no]), dev(x[:, no:])
            Y, YG = torch.full((1, no), 3.0, dtype=torch.float64, device="cuda"), torch.zeros((1, ng), dtype=torch.float64, device="cuda")
            mf.scale(Y, 0.0)
            for which in (3, 1, 4):
                mf.apply_elems(which, X, XG, Y, YG, alpha, 0.0)
                # (ghost buffers of their own are passed to every launch: all three run the variant with the owned-or-ghost select)
                assert {"launched", "split-ghost"} <= system.last_fast_launch(), (which, system.last_fast_launch())
            torch.cuda.synchronize()
            got = np.concatenate([Y.cpu().numpy(), YG.cpu().numpy()], axis=1)
            assert np.abs(got[0, no:]).max() > 0.0
            err = rel_err(got.T, ref)
            print(f"split, tuning {tune}: rel L2 {err:.3e}")
            assert err < TOL


def test_fused_energy(ctx, walk):
    """ENERGY variant (the PCG's apply with <x, A x> accumulated by the element kernel): y and x^T A x against the oracle"""
    y_ref = walk.reference()
    want = float(np.dot(walk.x[0], y_ref[:, 0]))
    for tune in (dict(waves_per_cu=1), dict()):
        with ctx.tuning(**tune):
            line = walk.mf.route(2, 1, with_energy=True)
            assert_order6_fast(line)
            assert " energy" in line, line
            X, Y = dev(walk.x), dev(walk.y0)
            S = torch.full((8,), 7.0, dtype=torch.float64, device="cuda")
            walk.mf.apply_energy(X, Y, S)
            torch.cuda.synchronize()
            assert "energy" in system.last_fast_launch(), system.last_fast_launch()
            s = S.cpu().numpy()
            print(f"energy, tuning {tune}: x^T A x {s[1]:.15e} oracle {want:.15e} rel {abs(s[1] - want) / abs(want):.3e}")
            assert rel_err(Y.cpu().numpy().T, y_ref) < TOL
            assert abs(s[1] - want) <= TOL * abs(want)
            assert np.all(s[[0, 2, 3, 4, 5, 6, 7]] == 7.0)


@pytest.mark.parametrize("p,ne", [(4, (7, 6, 5)), (2, (9, 7, 5))])
def test_other_orders_unchanged(ctx, p, ne):
    """orders whose shapes keep the gather at the top of the element (several elements per wave): odd sizes, batches with idle teams"""
    c = Case(ctx, ne, p)
    with ctx.tuning(waves_per_cu=1):
        line = c.mf.route()
        assert f"sumfactFastKernel<p={p},nq={p + 1},U=4,F=0>" in line and "one wave per 1 element(s)" not in line, line
        assert c.error(alpha=1.5, beta=-0.25) < TOL
    assert c.error() < TOL
