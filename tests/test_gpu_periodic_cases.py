"""l3k_periodic_match on the designed inputs of periodic_cases.py: every neighbour cell, the low and the high end of the grid, nodes
out of reach, distances exactly on the tolerance, ties, several listings of a node, every regime of the grid, ids from 2^31 and
4096 + 4096 nodes in long cell runs.  The cases live on a lattice on which every comparison of the matcher is exact, so the device
must equal the all-pairs restatement exactly (tests/test_periodic_cases_cpu.py checks the cases themselves, without a device).
And the inputs from which no grid can be made are refused before anything is launched or written."""
import ctypes as C

import numpy as np
import pytest

import periodic_cases as P
from l3ster_amd import capi, system

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    torch.cuda.set_device(0)
    return system.Context(0, torch.cuda.current_stream().cuda_stream)


def device_match(ctx, case):
    mesh = P.build_mesh(case)
    return system.periodic_match(ctx, mesh, mesh.src, mesh.dst, case.translation, case.tolerance)


@pytest.mark.parametrize("case", P.CASES, ids=repr)
def test_device_equals_brute_force(ctx, case):
    got, want = device_match(ctx, case), P.reference(case)
    assert got[0].dtype == np.uint32 and got[1].dtype == np.uint32
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), case
    assert got[2:] == tuple(int(v) for v in want[2:]), (got[2:], want[2:])
    assert np.all(np.diff(got[0].astype(np.int64)) > 0)  # ascending in the source node, one pair per node
    again = device_match(ctx, case)
    assert np.array_equal(again[0], got[0]) and np.array_equal(again[1], got[1]) and again[2:] == got[2:]
    if case.expect is not None:  # and the answer worked out on paper
        assert P.same_result(P.as_result(*case.expect), got)


@pytest.mark.parametrize("a,b", P.SAME_ANSWER)
def test_third_entries_are_ignored_in_2d(ctx, a, b):
    assert P.same_result(device_match(ctx, P.by_name(a)), device_match(ctx, P.by_name(b)))


def call_c_abi(ctx, case, pair_src, pair_dst, counts):
    mesh = P.build_mesh(case)
    en, ev = np.ascontiguousarray(mesh.elem_nodes, dtype=np.uint32), np.ascontiguousarray(mesh.elem_verts, dtype=np.float64)
    (se, ss), (de, ds) = mesh.src, mesh.dst
    t = np.array(case.translation, dtype=np.float64)
    p32, p64, p8, pdbl = capi.c_uint32_p, capi.c_int64_p, capi.c_uint8_p, capi.c_double_p
    return capi.load().l3k_periodic_match(
        ctx._h, mesh.dim, 1, en.shape[0], en.ctypes.data_as(p32), ev.ctypes.data_as(pdbl), se.size, se.ctypes.data_as(p64),
        ss.ctypes.data_as(p8), de.size, de.ctypes.data_as(p64), ds.ctypes.data_as(p8), t.ctypes.data_as(pdbl), float(case.tolerance),
        pair_src.ctypes.data_as(p32), pair_dst.ctypes.data_as(p32), *[C.byref(c) for c in counts])


@pytest.mark.parametrize("case,word", P.refused_inputs(), ids=repr)
def test_no_grid_is_refused_and_nothing_written(ctx, case, word):
    ps, pd = np.full(16, 99, np.uint32), np.full(16, 99, np.uint32)
    counts = [C.c_int64(-7) for _ in range(4)]
    assert call_c_abi(ctx, case, ps, pd, counts) == -1
    message = capi.load().l3k_last_error().decode()
    assert message.startswith("l3k_periodic_match: ") and word in message, message
    assert np.all(ps == 99) and np.all(pd == 99) and [c.value for c in counts] == [-7] * 4
    with pytest.raises(capi.L3KError, match=word):
        device_match(ctx, case)
    # the context is as good as before
    after = P.by_name("7-ids-and-identity-3d")
    ps, pd = np.full(16, 99, np.uint32), np.full(16, 99, np.uint32)
    assert call_c_abi(ctx, after, ps, pd, counts) == 0
    want = P.reference(after)
    n = counts[0].value
    assert n == want[0].size and np.array_equal(ps[:n], want[0]) and np.array_equal(pd[:n], want[1]) and np.all(ps[n:] == 99)
    assert [c.value for c in counts[1:]] == [int(v) for v in want[2:]]
