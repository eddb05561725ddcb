"""The single-rank GMRES keeps its bits: solve.gmres on tri("fast", 1000) of tests/test_gpu_gmres.py against
tests/golden/gmres_single_rank_bits.npz, recorded on an MI355X from the commit before the collective GMRES went in (the three pass
routes of DESIGN.md 4.25: restart lengths 5, 30 and 300; no preconditioner, Jacobi, Chebyshev degree 2).  The kernels sum in a fixed
order, so the bits of x and of every field of the result are a property of the code, not of the run.

    python tests/test_gpu_gmres_bits.py FILE.npz     records the fixture (how the committed one was made)"""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gmres_single_rank_bits.npz")
CASES = [("jacobi", 5), ("jacobi", 30), ("jacobi", 300), ("none", 30), ("cheb2", 30)]
FIELDS = ("tol", "estimate", "orth_loss", "num_iters", "restarts", "converged", "breakdown")


def single_rank_solves():
    """{name: array} of the bits (uint64) of x and of the result's fields, per case; gmres_distributed is not involved"""
    from l3ster_amd import solve
    from test_gpu_gmres import dev, fast_case
    T, b, minv, _ = fast_case()
    bd, md = dev(b), dev(minv)
    out = {}
    for precond, m in CASES:
        x = torch.zeros(T.n, dtype=torch.float64, device="cuda")
        kw = dict(minv=md) if precond == "jacobi" else {} if precond == "none" else dict(precond=solve.ChebyshevPreconditioner(T.op, md, degree=2))
        r = solve.gmres(T.op, bd, x, tol=1e-12, residual_scaling="rhs", restart_length=m, throw_on_fail=False, **kw)
        out[f"{precond}_{m}_x"] = x.cpu().numpy().view(np.uint64)
        out[f"{precond}_{m}_result"] = np.array([float(getattr(r, f)) for f in FIELDS]).view(np.uint64)
    return out


def test_single_rank_bits_are_those_of_the_parent():
    want, got = np.load(GOLDEN), single_rank_solves()
    assert sorted(want.files) == sorted(got)
    for name in want.files:
        if name.endswith("_result"):
            print(name, dict(zip(FIELDS, got[name].view(np.float64))))
        assert np.array_equal(want[name], got[name]), name
    assert all(got[f"{p}_{m}_result"].view(np.float64)[FIELDS.index("converged")] == 1.0 for p, m in CASES)


if __name__ == "__main__":
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [here, os.path.dirname(here)]
    np.savez(sys.argv[1], **single_rank_solves())
    print("recorded", sys.argv[1])
