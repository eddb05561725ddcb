"""The global-scratch (GS) element kernels on meshes with MORE ELEMENTS THAN WORKGROUPS.  Shapes whose per-element buffers exceed the
LDS (the NS3D plugin at p = 4 and p = 6) run sumfactApplyKernel / diagKernel / assembleCoeffKernel as persistent kernels: scratchGrid
launches g = min(elem_count, 2 * CUs) workgroups, each on its own slice of the context's scratch arena, and every workgroup walks the
elements eb, eb + g, eb + 2 g, ...  The other tests of these shapes stay below g elements, so the loop body runs once; here
2 g < N < 3 g and N % g != 0 (some workgroups take three elements, the others two) -- asserted, together with the route line, so
that a change of routing turns these tests red instead of hollowing them out.  Checked from the second iteration on: the barrier at
the end of the body, the re-zeroing of the diagonal accumulator, the re-load of the vertices and the connectivity, the batch-local
index of the coefficient records and the checksum slot, the position of the degenerate-element flag, the stride and the tail, and the
growth of the shared arena between launches that are not synchronised.  Every comparison is made per element as well as in norm: a
relative L2 norm over 5e5 dofs can hide one wrong element out of 1100."""
import copy
import os
import time

import numpy as np
import pytest

import oracle_lib as O
from helpers import oracle_mesh, rel_err

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

KID = 1013  # as tests/test_ns3d_plugin.py (same id, same shapes: one plugin library)
OPTS = (1, 1, 0)  # nq = 2 p
SOURCE = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "kernels", "ns3d.hpp")).read()
U = F = 7
ALPHA, BETA = 1.5, -0.25
TOL = 1e-11  # tests/test_ns3d_plugin.py::test_mesh_vs_oracle: this kernel on this route


@pytest.fixture(scope="module")
def ns3d():
    from l3ster_amd import plugin
    return plugin.compile_kernel("NS3D", SOURCE, KID, shapes=[(2, 4, 1), (4, 8, 1), (6, 12, 1)])


@pytest.fixture(scope="module")
def grid():
    """the number of persistent workgroups of a GS launch with at least that many elements: scratchGrid's formula"""
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return 2 * torch.cuda.get_device_properties(0).multi_processor_count


def walk_dims(g):
    """(a, b, c), a >= b >= c, with 2 g < a b c < 3 g and a b c % g != 0: the smallest such mesh among the most cube-like ones
    ((11, 10, 10), 1100 elements, for the 512 workgroups of a 256-CU part)"""
    for spread in range(1, 64):  # a - c <= spread
        best = None
        for c in range(1, 64):
            for b in range(c, c + spread + 1):
                for a in range(b, c + spread + 1):
                    n = a * b * c
                    if 2 * g < n < 3 * g and n % g != 0 and (best is None or n < best[0]):
                        best = (n, (a, b, c))
        if best:
            return best[1]
    raise AssertionError(f"no mesh for a grid of {g} workgroups")


def _ctx():
    from l3ster_amd import system
    return system.Context(0, torch.cuda.current_stream().cuda_stream)


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")


def _route_is_gs(mf, p):
    line = mf.route()
    assert "GLOBAL scratch" in line and f"sumfactApplyKernel<p={p},nq={2 * p},U=7,F=7" in line, line
    return line


class Case:
    """the mesh of one order, its fields and operands (host), and the device objects on a context"""

    def __init__(self, p, g):
        from l3ster_amd import system
        self.p, self.nq, self.g = p, 2 * p, g
        self.part = part = system.CubePartition(walk_dims(g), p, perturb=0.15)
        N = part.n_elems
        assert 2 * g < N < 3 * g and N % g != 0, (N, g)  # every workgroup walks two elements, N % g of them a third
        assert system.n_qps1d(p, *OPTS[:2]) == self.nq
        self.mask = part.dirichlet_mask(U, unknowns=(0, 1, 2))  # the three velocity components on all sides
        self.fields = np.random.default_rng(4).uniform(-1, 1, (F, part.n_local_nodes))
        self.x = part.synthetic_vector(U)
        self.y0 = np.random.default_rng(1).uniform(-1, 1, self.x.shape)
        self.gd = np.random.default_rng(6).uniform(-1, 1, (1, part.n_local_nodes * U)) * self.mask[None, :]
        self.elem_dofs = (part.elem_nodes.astype(np.int64)[:, :, None] * U + np.arange(U)).reshape(N, -1)

    def system(self, ctx, kid, dirichlet=True, part=None):
        from l3ster_amd import system
        mf = system.MatrixFreeSystem(system.DeviceMesh(ctx, part or self.part, U, self.mask if dirichlet else None), kid, asm_opts=OPTS)
        mf.set_fields(_dev(self.fields))
        return mf

    def oracle(self):
        return oracle_mesh(self.part, self.nq, U, np.arange(U), self.mask, self.fields)

    def check(self, got, ref, what):
        """got, ref over the local dofs: the relative L2 error, then max |got - ref| over the dofs of each element against
        1e-11 max |ref| -- the worst element is named with its place in the walk (workgroup e % g, iteration e // g)"""
        got, ref = np.asarray(got).reshape(-1), np.asarray(ref).reshape(-1)
        err = np.abs(got - ref)
        per_elem = err[self.elem_dofs].max(axis=1)
        w = int(np.argmax(per_elem))
        bound = TOL * np.abs(ref).max()
        r = rel_err(got, ref)
        print(f"{what}: rel err {r:.3e}; worst element {w} (workgroup {w % self.g}, iteration {w // self.g}): {per_elem[w]:.3e}, bound {bound:.3e}")
        n_bad = int((per_elem > bound).sum())
        first_bad = int(np.argmax(per_elem > bound)) if n_bad else -1
        assert n_bad == 0, (f"{what}: {n_bad} elements beyond {bound:.3e}; worst element {w} (workgroup {w % self.g}, iteration {w // self.g}) "
                            f"max |err| {per_elem[w]:.3e}; first bad element {first_bad} (workgroup {first_bad % self.g}, iteration "
                            f"{first_bad // self.g}); rel err {r:.3e}")
        assert r < TOL, f"{what}: rel err {r:.3e}"


_cases = {}


def case(p, g):
    if p not in _cases:
        _cases[p] = Case(p, g)
    return _cases[p]


@pytest.mark.parametrize("p", [4, 6])
def test_walk_apply_diag_rhs_vs_oracle(ns3d, grid, p):
    """y <- alpha A x + beta y (Dirichlet on the velocity components of all sides, random fields and y0), diag and the lifted rhs
    with random Dirichlet values on the whole mesh of 2 g < N < 3 g elements against the oracle: the whole vectors, in norm and per
    element.  The oracle alone on the CPU for the 1100 elements of a 256-CU part, measured on 8 threads: p = 4 (0.53 M dofs) apply
    0.1 s, diag + rhs 2.7 s; p = 6 (1.75 M dofs) apply 0.5 s, diag + rhs 25.5 s (0.1 s and 8.2 s beside the GPU, on every core the
    test may use) -- both legs stay under a minute, so p = 6, the only registered shape whose assembleCoeffKernel is GS, keeps its
    diag too.  The test prints the seconds of each oracle call."""
    c = case(p, grid)
    nthreads = len(os.sched_getaffinity(0))
    mf = c.system(_ctx(), ns3d)
    line = _route_is_gs(mf, p)
    X, Y = _dev(c.x), _dev(c.y0)
    mf.apply(X, Y, ALPHA, BETA)
    diag, rhs = mf.diag_rhs(_dev(c.gd))
    y, diag, rhs = Y.cpu().numpy()[0], diag.cpu().numpy(), rhs.cpu().numpy()[0]
    om = c.oracle()
    t0 = time.perf_counter()
    y_ref = O.mf_apply(om, O.KERNEL_NS3D, c.x.T, np.asfortranarray(c.y0.T.copy()), alpha=ALPHA, beta=BETA, nthreads=nthreads)
    t1 = time.perf_counter()
    d_ref, r_ref = O.mf_diag_rhs(om, O.KERNEL_NS3D, 1, np.asfortranarray(c.gd.T), nthreads=nthreads)
    t2 = time.perf_counter()
    print(f"p = {p}: {c.part.n_elems} elements on {grid} workgroups, {line}; oracle on {nthreads} threads: apply {t1 - t0:.1f} s, diag + rhs {t2 - t1:.1f} s")
    c.check(y, y_ref[:, 0], f"apply p = {p}")
    c.check(diag, d_ref, f"diag p = {p}")
    c.check(rhs, r_ref[:, 0], f"lifted rhs p = {p}")


def test_walk_streamed_assembly(ns3d, grid):
    """assembleCoeffKernel is GS at p = 6 only (5 F M^3 doubles: 143 KB at p = 4, 484 KB at p = 6).  Streaming mode (no K_e: 46 MB
    each) hands the whole range to one launch, so count = N > 2 g makes the coefficient kernel -- and the RHS-mode apply kernel with
    element-local output behind F_e -- walk.  There is no oracle K_e at this size (80 GFLOP per element), so: (1) checksums and F_e
    of the one launch against launches of at most g elements over the same range, which run the loop body once and are what
    test_ns3d_plugin.py pins -- F_e bit for bit (no atomics), checksums at the rtol of the streamed checksum there; (2) at the
    three walk positions and three more elements F_e against the oracle and the single-element K_e, whose checksum the big launch
    must reproduce, through its action on a vector against the oracle."""
    p, nq = 6, 12
    c = case(p, grid)
    g, N = grid, c.part.n_elems
    assert N > 2 * g and N % g != 0
    mf = c.system(_ctx(), ns3d, dirichlet=False)
    _route_is_gs(mf, p)
    _, F_big, cs_big = mf.local_assemble(0, N, want_K=False, want_F=True, want_checksum=True)
    F_big, cs_big = F_big.cpu(), cs_big.cpu()
    for first in range(0, N, g):
        n = min(g, N - first)
        _, F_c, cs_c = mf.local_assemble(first, n, want_K=False, want_F=True, want_checksum=True)
        F_c, cs_c = F_c.cpu(), cs_c.cpu()
        for i in range(n):
            e = first + i
            where = f"element {e} (workgroup {e % g}, iteration {e // g})"
            assert torch.equal(F_big[e], F_c[i]), f"F_e of {where}: max diff {(F_big[e] - F_c[i]).abs().max().item():.3e}"
            np.testing.assert_allclose(cs_big[e].item(), cs_c[i].item(), rtol=1e-11, err_msg=f"checksum of {where}")
    rng = np.random.default_rng(11)
    picks = [0, g + int(rng.integers(g)), N - 1] + [int(e) for e in rng.choice(np.arange(1, N - 1), 3, replace=False)]
    assert g <= picks[1] < 2 * g and picks[2] >= 2 * g
    for e in picks:
        where = f"element {e} (workgroup {e % g}, iteration {e // g})"
        nf = c.fields[:, c.part.elem_nodes[e]].T
        _, F_ref = O.diag_rhs_local(O.KERNEL_NS3D, p, nq, 1, c.part.elem_verts[e], None, None, nf)
        assert np.abs(F_big[e].numpy().T - F_ref).max() < 1e-12 * max(1.0, np.abs(F_ref).max()), where
        K, _, cs1 = mf.local_assemble(e, 1, want_F=False, want_checksum=True)
        np.testing.assert_allclose(cs_big[e].item(), cs1.cpu()[0].item(), rtol=1e-11, err_msg=f"checksum of {where}")
        K = K.cpu().numpy()[0]
        v = np.random.default_rng(e).uniform(-1, 1, (K.shape[1], 1))
        assert rel_err(K @ v, O.apply_local(O.KERNEL_NS3D, p, nq, c.part.elem_verts[e], v, nf)) < 1e-12, where


@pytest.mark.parametrize("where", ["second", "last"])
def test_walk_degenerate_element_is_reported(ns3d, grid, where):
    """one element with |J| <= 0 (two vertices exchanged) that a workgroup reaches in its second / its last iteration: the flag sits
    behind the records of the whole batch, a.workspace[elem_count * NQP * CS], whichever iteration sets it"""
    from l3ster_amd import system
    p = 6
    c = case(p, grid)
    g, N = grid, c.part.n_elems
    e = g + 5 if where == "second" else N - 1
    assert N > 2 * g and (g <= e < 2 * g if where == "second" else e >= 2 * g)
    bad = copy.copy(c.part)
    bad.elem_verts = c.part.elem_verts.copy()
    bad.elem_verts[e, [0, 1]] = bad.elem_verts[e, [1, 0]]
    mf = c.system(_ctx(), ns3d, dirichlet=False, part=bad)
    _route_is_gs(mf, p)
    with pytest.raises(system.L3KError, match="degenerate"):
        mf.local_assemble(0, N, want_K=False, want_F=False, want_checksum=True)
    # (and none is reported for the elements before it)
    _, _, cs = mf.local_assemble(0, e, want_K=False, want_F=False, want_checksum=True)
    assert torch.isfinite(cs).all()


def test_arena_grows_between_unsynchronised_launches(ns3d, grid):
    """One context, four launches back to back without a synchronisation: a p = 4 GS apply (the arena: g slices of 286 KB), a p = 6
    GS apply (g slices of 968 KB: contextScratch frees the arena and allocates a larger one while the first kernel may still run),
    the p = 4 apply again, a p = 4 diag + rhs (another slice size on the same arena).  Each result against the same call made
    alone on a fresh context (whose arena starts empty), at the tolerance of the oracle comparison, in norm and per element."""
    c4, c6 = case(4, grid), case(6, grid)

    def operands(c):
        return _dev(c.x), _dev(c.y0), _dev(c.gd)

    def alone(c, kind):
        mf = c.system(_ctx(), ns3d)
        _route_is_gs(mf, c.p)
        X, Y, G = operands(c)
        if kind == "apply":
            mf.apply(X, Y, ALPHA, BETA)
            torch.cuda.synchronize()
            return [Y.cpu().numpy()[0]]
        diag, rhs = mf.diag_rhs(G)
        torch.cuda.synchronize()
        return [diag.cpu().numpy(), rhs.cpu().numpy()[0]]

    ref4, ref6, refd = alone(c4, "apply"), alone(c6, "apply"), alone(c4, "diag")
    ctx = _ctx()  # scratch_bytes == 0: the first launch allocates the arena
    mf4, mf6 = c4.system(ctx, ns3d), c6.system(ctx, ns3d)
    _route_is_gs(mf4, 4), _route_is_gs(mf6, 6)
    X4, Y4a, G4 = operands(c4)
    X6, Y6, _ = operands(c6)
    Y4b = Y4a.clone()
    diag = torch.zeros(mf4.mesh.n_owned_dofs, dtype=torch.float64, device="cuda")
    rhs = torch.zeros((1, mf4.mesh.n_owned_dofs), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    mf4.apply(X4, Y4a, ALPHA, BETA)
    mf6.apply(X6, Y6, ALPHA, BETA)
    mf4.apply(X4, Y4b, ALPHA, BETA)
    mf4.diag_rhs(G4, diag=diag, rhs=rhs)
    torch.cuda.synchronize()
    c4.check(Y4a.cpu().numpy()[0], ref4[0], "1: p = 4 apply on the small arena")
    c6.check(Y6.cpu().numpy()[0], ref6[0], "2: p = 6 apply after the arena grew")
    c4.check(Y4b.cpu().numpy()[0], ref4[0], "3: p = 4 apply on the grown arena")
    c4.check(diag.cpu().numpy(), refd[0], "4: p = 4 diag on the grown arena")
    c4.check(rhs.cpu().numpy()[0], refd[1], "4: p = 4 lifted rhs on the grown arena")
