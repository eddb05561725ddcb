"""The collective PCG of a partitioned system, on the CPU: the new entry points in the header, the library and the binding; what must
not have moved (L3K_VERSION, the transport table); the refusals of the Python layer that need no device; and the numpy restatement
tests/pcg_dist_ref.py -- the sum in rank order and the partitioned Jacobi-PCG over tests/asm_dist_ref.py's host matrices -- proved
against tests/cg_ref.py on the whole matrix.  No GPU: the reference of tests/test_gpu_pcg_dist.py."""
import os
import re

import numpy as np
import pytest

import asm_dist_ref as AD
import cg_ref
import pcg_dist_ref as PD
from l3ster_amd import capi, distributed, solve, system

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["l3k_halo_allreduce_sum", "l3k_csr_dist_apply_energy", "l3k_pcg_solve_dist", "l3k_csr_dist_pcg_solve", "l3k_cheb_create_dist",
       "l3k_csr_dist_cheb_create"]
_CASES = {}


def case(kind):
    if kind not in _CASES:
        q = AD.quad_case(device="cpu") if kind == "quad" else AD.cube_case()
        q.mats, q.b, q.A, q.b_whole = PD.closed_system(q)
        _CASES[kind] = q
    return _CASES[kind]


# ------------------------------------------------------------------------------------------------ header, library, binding
def test_header_library_and_binding_expose_the_six_names():
    header = open(os.path.join(ROOT, "include", "l3k.h")).read()
    lib = capi.load()
    for name in NEW:
        assert re.search(r"^int\s+" + name + r"\(", header, re.M), name
        assert name in capi.SIGNATURES and hasattr(lib, name), name
    for name in NEW[2:]:  # every solve cites the Belos call it stands in for
        assert "solve/BelosSolvers.hpp:116-122" in header[:header.index("int " + name + "(")].rsplit("/* ----", 1)[1]
    hpp = open(os.path.join(ROOT, "include", "l3k", "operator.hpp")).read()
    assert "pcgSolve" in hpp and "chebyshev(" in hpp and "l3k_pcg_solve_dist" in hpp and "l3k_csr_dist_pcg_solve" in hpp
    assert hasattr(distributed.NativeHalo, "allreduce") and hasattr(solve, "DistributedChebyshev")


def test_version_and_transport_table_have_not_moved():
    header = open(os.path.join(ROOT, "include", "l3k.h")).read()
    assert capi.load().l3k_version() == 101 and re.search(r"^#define L3K_VERSION 101$", header, re.M)
    assert [n for n, _ in capi.HaloTransport._fields_] == ["user", "group_begin", "send", "recv", "group_end", "destroy"]
    body = re.search(r"typedef struct l3k_halo_transport\s*\{(.*?)\}\s*l3k_halo_transport;", header, re.S).group(1)
    assert len([m for m in body.split(";") if m.strip()]) == 6


def test_null_handles_are_refused_with_the_calls_name():
    lib = capi.load()
    import ctypes as C
    out, res = C.c_void_p(0xdead), capi.CgResult()
    calls = {
        "l3k_halo_allreduce_sum": lambda: lib.l3k_halo_allreduce_sum(None, None, 1),
        "l3k_csr_dist_apply_energy": lambda: lib.l3k_csr_dist_apply_energy(None, None, None, None),
        "l3k_pcg_solve_dist": lambda: lib.l3k_pcg_solve_dist(None, None, None, None, None, None, None, C.byref(res)),
        "l3k_csr_dist_pcg_solve": lambda: lib.l3k_csr_dist_pcg_solve(None, None, None, None, None, None, C.byref(res)),
        "l3k_cheb_create_dist": lambda: lib.l3k_cheb_create_dist(None, None, None, None, C.byref(out)),
        "l3k_csr_dist_cheb_create": lambda: lib.l3k_csr_dist_cheb_create(None, None, None, C.byref(out)),
    }
    for name, call in calls.items():
        assert call() == -1 and name in lib.l3k_last_error().decode(), name
    assert out.value == 0xdead


# ------------------------------------------------------------------------------------------------ the Python refusals
def test_native_refuses_a_reduction_of_the_callers():
    with pytest.raises(capi.L3KError, match="native=True.*allreduce must be None"):
        solve.pcg_distributed(object(), None, None, None, native=True, allreduce=lambda view: None)
    with pytest.raises(capi.L3KError, match="native=True.*group"):
        solve.pcg_distributed(object(), None, None, None, native=True, group=object())


def test_native_refuses_the_p_multigrid_and_names_the_host_loop():
    pmg = object.__new__(solve.DistributedPMultigrid)
    with pytest.raises(capi.L3KError, match="host loop"):
        solve.pcg_distributed(object(), None, None, None, native=True, precond=pmg)


def test_native_refuses_an_operator_without_a_native_halo():
    import torch
    b, x = torch.zeros(4, dtype=torch.float64), torch.zeros(4, dtype=torch.float64)
    with pytest.raises(capi.L3KError, match="DistributedCsrOperator"):
        solve.pcg_distributed(object(), None, b, x, native=True)
    with pytest.raises(capi.L3KError, match="1 to 8"):
        distributed.NativeHalo.allreduce(object(), torch.zeros(9, dtype=torch.float64))


def test_the_default_route_is_the_host_loop():
    import inspect
    assert inspect.signature(solve.pcg_distributed).parameters["native"].default is False


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("world", [1, 2, 4])
@pytest.mark.parametrize("count", [1, 3, 8])
def test_sum_in_rank_order(world, count):
    rows = PD.order_dependent_rows(world, count)
    got = PD.sum_in_rank_order(rows)
    want = [float(rows[0, c]) for c in range(count)]
    for c in range(count):
        for r in range(1, world):
            want[c] = want[c] + float(rows[r, c])
    assert got.tolist() == want
    if world == 4:  # the inputs do tell one order from another
        assert any(got[c] != PD.sum_in_rank_order(rows[::-1])[c] for c in range(count))
    # the chain of reductions keeps every rank on the same total
    end = PD.chain(world, count, 20, rows)
    assert all(np.array_equal(end[r] - r, end[0]) for r in range(world))


@pytest.mark.parametrize("kind", ["quad", "cube"])
def test_partitioned_apply_is_the_whole_matrix(kind):
    q = case(kind)
    x = np.random.default_rng(3).uniform(-1, 1, q.A.shape[0])
    got = q.gather([v[None, :] for v in PD.dist_apply(q, q.mats, [q.scatter(x, r)[0] for r in range(q.world)])])[0]
    want = q.A @ x
    assert np.linalg.norm(got - want) <= 1e-13 * np.linalg.norm(want)
    xs = [q.scatter(x, r)[0] for r in range(q.world)]
    assert abs(PD.dist_dot(xs, xs) - x @ x) <= 1e-13 * (x @ x)


@pytest.mark.parametrize("kind", ["quad", "cube"])
def test_partitioned_pcg_takes_the_iterations_of_cg_ref(kind):
    q, tol = case(kind), 1e-10
    ranks = range(q.world)
    diag = PD.dist_diag(q, q.mats)
    assert np.allclose(q.gather([d[None, :] for d in diag])[0], np.diag(q.A), rtol=1e-13, atol=0)
    minv = [1.0 / d for d in diag]
    x, it, res = PD.pcg(q, q.mats, q.b, [np.zeros_like(v) for v in q.b], minv, tol, 5000)
    assert res <= tol and 0 < it < 5000
    # cg_ref on the whole matrix at working precision: the first step whose scaled residual meets the tolerance
    minv_w = 1.0 / np.diag(q.A)
    x_w, _, steps, _ = cg_ref.pcg_ref(q.A, q.b_whole, np.zeros_like(q.b_whole), minv_w, it + 5, dtype=np.float64)
    scale = np.linalg.norm(q.b_whole)
    first = next(j + 1 for j, s in enumerate(steps) if np.sqrt(float(s["rr"])) / scale <= tol)
    print(f"{kind}: {it} iterations on {q.world} ranks, {first} on the whole matrix, residual {res:.2e}")
    assert it == first
    x_all = q.gather([v[None, :] for v in x])[0]
    x_ref = np.linalg.solve(q.A, q.b_whole)
    assert np.linalg.norm(x_all - x_ref) <= 1e-8 * np.linalg.norm(x_ref)


def test_frozen_rows_keep_x_and_leave_the_residual():
    q = case("quad")
    diag = PD.dist_diag(q, q.mats)
    minv = [1.0 / d for d in diag]
    minv[0][:3] = 0.0
    x0 = [np.full_like(v, 0.25) for v in q.b]
    x, it, res = PD.pcg(q, q.mats, q.b, x0, minv, 1e-10, 5000)
    assert res <= 1e-10 and np.array_equal(x[0][:3], x0[0][:3])
