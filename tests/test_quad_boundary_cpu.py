"""Boundary terms, integrals and values at nodes on quads, host side: the 2-D boundary / residual kernels in the registry and
their device shapes, and the numpy restatement of a quad side's operator (quad_side_ref.py) against the oracle.  No GPU."""
import numpy as np
import pytest

import oracle_lib as O
import quad_side_ref as Q
from l3ster_amd import build, system
from test_oracle_boundary import QUAD


def test_boundary_kernel_info_matches_oracle():
    info, ref = system.kernel_info(system.KERNEL_ADIABATIC2D), O.kernel_params(system.KERNEL_ADIABATIC2D)
    assert (info["dimension"], info["n_equations"], info["n_unknowns"], info["n_fields"]) == (ref["dim"], ref["E"], ref["U"], ref["F"])
    assert (info["dimension"], info["n_equations"], info["n_unknowns"]) == (2, 1, 3) and info["name"] == "adiabatic2d"


@pytest.mark.parametrize("rid,name", [(system.RESIDUAL_LINEAR2D_ERROR, "linear2d_error"), (system.RESIDUAL_UNIT2D, "unit2d"),
                                      (system.RESIDUAL_COORDX2D, "coordx2d")])
def test_residual_info_matches_oracle(rid, name):
    info, ref = system.residual_info(rid), O.residual_params(rid)
    assert (info["dimension"], info["n_equations"], info["n_fields"]) == (ref["dim"], ref["E"], ref["F"]) == (2, ref["E"], ref["F"])
    assert info["name"] == name and info["param_bytes"] == 0


def test_ids_match_the_oracle_constants():
    assert system.KERNEL_ADIABATIC2D == O.KERNEL_ADIABATIC2D == 5
    assert (system.RESIDUAL_LINEAR2D_ERROR, system.RESIDUAL_UNIT2D, system.RESIDUAL_COORDX2D) == (1, 3, 5)


def test_minimum_instances_listed():
    bnd, res = build.parse_side_instances()
    bnd = {(t.split("::")[-1], int(p), int(nq), int(r)) for t, p, nq, r in bnd}
    res = {(t.split("::")[-1], int(p), int(nq)) for t, p, nq in res}
    want_b = {("Adiabatic2D", p, p + 1, 1) for p in range(1, 7)} | {("Adiabatic2D", 2, 3, 2), ("Adiabatic2D", 4, 5, 2)}
    want_r = {("Linear2DError", 2, 5), ("Linear2DError", 4, 9), ("Linear2DError", 6, 13), ("Unit2D", 1, 6), ("Unit2D", 2, 3),
              ("Unit2D", 2, 5), ("Unit2D", 4, 9)} | {("CoordX2D", p, p + 1) for p in range(1, 7)}
    assert want_b <= bnd and want_r <= res


@pytest.mark.parametrize("p,nq", [(1, 2), (2, 3), (3, 5), (4, 5)])
@pytest.mark.parametrize("side", range(4))
def test_numpy_side_operator_matches_oracle(p, nq, side):
    kid, U = O.KERNEL_ADIABATIC2D, 3
    N = (p + 1) ** 2
    K, F = Q.side_system(Q.adiabatic2d, U, 1, p, nq, side, QUAD)
    x = np.random.default_rng(p + 7 * side).uniform(-1, 1, (N * U, 2))
    y = O.apply_local_side(side, kid, p, nq, QUAD, x)
    assert np.abs(K @ x - y).max() < 1e-13 * max(1.0, np.abs(y).max())
    diag, rhs = O.diag_rhs_local_side(side, kid, p, nq, 1, QUAD)
    assert np.abs(np.diag(K) - diag).max() < 1e-13 * max(1.0, np.abs(diag).max())
    assert np.abs(F[:, 0] - rhs[:, 0]).max() < 1e-13
    # only nodes of the side or next to it (through phi_k'(+-1)) take part; Adiabatic2D has no derivative term, so the side's own
    dn = np.abs(np.diag(K)).reshape(N, U).sum(axis=1)
    diag_nodes = np.flatnonzero(dn > 1e-13 * dn.max())
    idx = np.arange(N)
    on_side = [idx // (p + 1) == 0, idx // (p + 1) == p, idx % (p + 1) == 0, idx % (p + 1) == p][side]
    assert set(diag_nodes) <= set(np.flatnonzero(on_side))
