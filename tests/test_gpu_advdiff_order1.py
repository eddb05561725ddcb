"""The order-1 shape of the advection-diffusion kernel (the last level of a 4 -> 2 -> 1 p-multigrid hierarchy on it,
tools/bench_pmg.py) against the CPU oracle: whole-mesh apply, diagonal and lifted right-hand side.  Tolerance: relative L2 <= 1e-11
per mesh.  The mesh is the smallest with interior nodes in every direction and with odd extents."""
import numpy as np
import pytest

import oracle_lib as O
from helpers import oracle_mesh, rel_err
from l3ster_amd import system

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")


def test_advdiff_order_1_matches_the_oracle():
    kid, p, kpar = system.KERNEL_ADVDIFF3D, 1, [0.7, 1.3, 0.5]
    assert (kid, p, system.n_qps1d(p), 1) in system.instances()
    torch.cuda.set_device(0)
    ctx = system.Context(0, torch.cuda.current_stream().cuda_stream)
    info = system.kernel_info(kid)
    U, F = info["n_unknowns"], info["n_fields"]
    part = system.CubePartition((5, 4, 3), p, perturb=0.1)
    mask = part.dirichlet_mask(U)
    mf = system.MatrixFreeSystem(system.DeviceMesh(ctx, part, U, mask), kid, kpar)
    rng = np.random.default_rng(3)
    fields = rng.uniform(-1, 1, (F, part.n_local_nodes))
    mf.set_fields(dev(fields))
    om = oracle_mesh(part, system.n_qps1d(p), U, np.arange(U), mask, fields)
    x = part.synthetic_vector(U, ncols=1)
    y0 = rng.uniform(-1, 1, x.shape)
    want = O.mf_apply(om, kid, x.T, np.asfortranarray(y0.T.copy()), alpha=1.5, beta=-0.25, kparams=kpar)
    Y = dev(y0)
    mf.apply(dev(x), Y, 1.5, -0.25)
    assert rel_err(Y.cpu().numpy().T, want) < 1e-11
    g = np.where(mask != 0, rng.standard_normal(mask.size), 0.0)[None, :]
    diag, rhs = mf.diag_rhs(dev(g))
    d_ref, r_ref = O.mf_diag_rhs(om, kid, 1, np.asfortranarray(g.T), kparams=kpar)
    assert rel_err(diag.cpu().numpy(), d_ref) < 1e-11
    assert rel_err(rhs.cpu().numpy().T, r_ref) < 1e-11
