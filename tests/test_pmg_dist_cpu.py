"""The p-multigrid transfer on a partitioned mesh, on the CPU: the partitioned ownership rule restated in numpy
(tests/pmg_dist_ref.py) gives, assembled over the ranks, exactly the single-rank P of tests/pmg_ref.py -- one row per global fine
dof -- and "restrict, then export-add" is its transpose; the element pairing of two parts of one rank; the new entry points in
the header and the binding, and their refusals without a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pmg_dist_ref as RD
import pmg_ref as R
from l3ster_amd import capi, system

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NE, PARTS, WORLD = (4, 2, 2), (2, 1, 1), 2
NEW = ["l3k_transfer_create", "l3k_transfer_info_get", "l3k_transfer_prolong", "l3k_transfer_restrict", "l3k_transfer_destroy",
       "l3k_pmg_residual"]


def restated(pf, pc, perturb=0.1):
    fine = [system.CubePartition(NE, pf, PARTS, r, perturb=perturb) for r in range(WORLD)]
    coarse = [system.CubePartition(NE, pc, PARTS, r, perturb=perturb) for r in range(WORLD)]
    maps = [system.match_elements(f, c) for f, c in zip(fine, coarse)]
    Ps = [RD.rank_node_prolongation(f, c, m) for f, c, m in zip(fine, coarse, maps)]
    wf, wc = system.CubePartition(NE, pf, perturb=perturb), system.CubePartition(NE, pc, perturb=perturb)
    return fine, coarse, maps, Ps, wf, wc


@pytest.mark.parametrize("pf,pc", [(4, 2), (2, 1)])
def test_partitioned_rule_assembles_to_the_single_rank_prolongation(pf, pc):
    fine, coarse, maps, Ps, wf, wc = restated(pf, pc)
    assert all(f.n_ghost_nodes + c.n_ghost_nodes > 0 for f, c in zip(fine[1:], coarse[1:]))  # (a real rank boundary)
    P, rows = RD.assemble(fine, coarse, Ps, wf, wc)
    assert np.array_equal(rows, np.ones_like(rows))  # every global fine node: exactly one row
    # ... and a complete one: every owned fine node found its handler (the rows of an interpolation sum to 1)
    assert all(np.abs(Pr.sum(axis=1) - 1.0).max() <= 1e-13 for Pr in Ps)
    want = R.node_prolongation(wf, wc, system.match_elements(wf, wc))
    err = np.abs(P - want).max()
    print(f"orders {pf} -> {pc}: max |P assembled - P single rank| = {err:.2e}")
    assert err <= 1e-14
    # restrict, then export-add = the transpose
    rf = np.random.default_rng(5).standard_normal((wf.n_local_nodes, 3))
    got = RD.restrict_export_add(fine, coarse, Ps, wf, wc, rf)
    ref = want.T @ rf
    assert np.linalg.norm(got - ref) <= 1e-13 * np.linalg.norm(ref)


def test_ghost_fine_nodes_have_no_handler():
    part = system.CubePartition(NE, 2, PARTS, 1, perturb=0.1)
    own = RD.owners(part)
    assert part.n_ghost_nodes > 0
    assert np.all(own[part.n_owned_nodes:] == RD.SENTINEL) and np.all(own[:part.n_owned_nodes] < part.n_elems)


@pytest.mark.parametrize("pf,pc", [(4, 2), (6, 3)])
def test_match_elements_on_two_parts_of_one_rank(pf, pc):
    for rank in range(4):
        f = system.CubePartition((4, 4, 2), pf, (2, 2, 1), rank, perturb=0.1)
        c = system.CubePartition((4, 4, 2), pc, (2, 2, 1), rank, perturb=0.1)
        m = system.match_elements(f, c)
        m = np.arange(f.n_elems) if m is None else m
        assert np.array_equal(np.sort(m), np.arange(f.n_elems)) and np.array_equal(f.elem_verts, c.elem_verts[m])


def test_header_and_binding_expose_the_new_names():
    header = open(os.path.join(ROOT, "include", "l3k.h")).read()
    lib = capi.load()
    for name in NEW:
        assert re.search(r"^int\s+" + name + r"\(", header, re.M), name
        assert name in capi.SIGNATURES and hasattr(lib, name), name
    assert "l3k_transfer_info" in header and [n for n, _ in capi.TransferInfo._fields_] == [
        "order_fine", "order_coarse", "n_owned_dofs_fine", "n_ghost_dofs_fine", "n_owned_dofs_coarse", "n_ghost_dofs_coarse"]
    from l3ster_amd import solve
    assert hasattr(system, "Transfer") and hasattr(solve, "DistributedPMultigrid")
    assert "class Transfer" in open(os.path.join(ROOT, "include", "l3k", "operator.hpp")).read()


def test_null_handles_are_refused_with_the_calls_name():
    lib = capi.load()
    out, info = C.c_void_p(), capi.TransferInfo()
    calls = {
        "l3k_transfer_create": lambda: lib.l3k_transfer_create(None, None, None, None, C.byref(out)),
        "l3k_transfer_info_get": lambda: lib.l3k_transfer_info_get(None, C.byref(info)),
        "l3k_transfer_prolong": lambda: lib.l3k_transfer_prolong(None, None, None, None, 0, None),
        "l3k_transfer_restrict": lambda: lib.l3k_transfer_restrict(None, None, None, None),
        "l3k_pmg_residual": lambda: lib.l3k_pmg_residual(None, None, None, None, None, 4),
    }
    for name, call in calls.items():
        assert call() == -1, name
        assert lib.l3k_last_error().decode().startswith(f"{name}: null argument"), name
    assert out.value is None and lib.l3k_transfer_destroy(None) == 0
