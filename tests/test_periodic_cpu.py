"""l3k_periodic_merge (host only) against the numpy restatement of periodic_ref.py: random pair sets with chains and components
of 2, 4 and 8 nodes, duplicate and self pairs, no pairs, a second merge; the numbering invariants; the closed-form node counts of
structured meshes made periodic; the refusals; and the names in the header, the binding and the library."""
import ctypes as C
import os

import numpy as np
import pytest

import periodic_ref as R
from l3ster_amd import capi, system

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def both(elem_nodes, n_nodes, n_noninternal, a, b):
    got = system.periodic_merge(elem_nodes, n_nodes, n_noninternal, a, b)
    want = R.merge(elem_nodes, n_nodes, n_noninternal, a, b)
    assert np.array_equal(got[0], want[0]) and got[0].dtype == np.uint32
    assert np.array_equal(got[1], want[1]) and got[1].dtype == np.uint32
    assert got[2:] == want[2:], (got[2:], want[2:])
    return got


def random_mesh(rng, n_elems=40, n_noninternal=90, per_elem=9, n_internal=2):
    """A connectivity in the numbering class of the library: random non-internal ids (every one used), then n_internal internal
    ids per element."""
    outer = rng.integers(0, n_noninternal, (n_elems, per_elem))
    outer.ravel()[rng.permutation(outer.size)[:n_noninternal]] = np.arange(n_noninternal)
    inner = n_noninternal + np.arange(n_elems * n_internal).reshape(n_elems, n_internal)
    return np.concatenate([outer, inner], axis=1).astype(np.uint32), n_noninternal + n_elems * n_internal


@pytest.mark.parametrize("seed", range(4))
def test_merge_random_components(seed):
    rng = np.random.default_rng(seed)
    en, n_nodes = random_mesh(rng)
    ids = rng.permutation(90)
    comps = [ids[0:2], ids[2:6], ids[6:14], ids[14:16], ids[16:24], ids[24:28]]  # sizes 2, 4, 8, 2, 8, 4
    a, b = [], []
    for k, c in enumerate(comps):
        if k % 2 == 0:  # a chain in random order
            a += c[:-1].tolist()
            b += c[1:].tolist()
        else:  # a star around a node that is not the lowest, plus an edge that closes a cycle
            hub = int(c.max())
            others = [int(v) for v in c if v != hub]
            a += [hub] * len(others) + [others[0]]
            b += others + [others[-1]]
    order = rng.permutation(len(a))
    a, b = np.array(a)[order], np.array(b)[order]
    flip = rng.integers(0, 2, a.size).astype(bool)
    a, b = np.where(flip, b, a), np.where(flip, a, b)
    new_en, node_map, n_out, n_nonint_out, n_comp = both(en, n_nodes, 90, a, b)
    assert n_comp == 6 and n_out == n_nodes - sum(len(c) - 1 for c in comps) and n_nonint_out == 90 - (n_nodes - n_out)
    for c in comps:
        assert np.unique(node_map[c]).size == 1
        assert node_map[c[0]] == node_map[c.min()]
    # the representative is the lowest id: the kept nodes keep their relative order
    kept = np.setdiff1d(np.arange(n_nodes), np.concatenate([np.setdiff1d(c, [c.min()]) for c in comps]))
    assert np.array_equal(node_map[kept], np.arange(n_out))
    # duplicates and self pairs change nothing
    a2 = np.concatenate([a, a[:5], b[:3], [7, 11]])
    b2 = np.concatenate([b, b[:5], a[:3], [7, 11]])
    again = both(en, n_nodes, 90, a2, b2)
    assert np.array_equal(again[0], new_en) and np.array_equal(again[1], node_map) and again[2:] == (n_out, n_nonint_out, n_comp)
    # numbering: non-internal ids below internal ones, internal ids contiguous per element and in the old order
    assert new_en[:, :9].max() < n_nonint_out
    assert np.array_equal(new_en[:, 9:], n_nonint_out + np.arange(80).reshape(40, 2))
    assert np.array_equal(np.unique(new_en), np.arange(n_out))
    # a second merge of the result with no pairs is the identity
    second = both(new_en, n_out, n_nonint_out, [], [])
    assert np.array_equal(second[0], new_en) and np.array_equal(second[1], np.arange(n_out)) and second[2:] == (n_out, n_nonint_out, 0)


def test_merge_without_pairs_is_the_identity():
    en, n_nodes = random_mesh(np.random.default_rng(9))
    before = en.copy()
    new_en, node_map, n_out, n_nonint_out, n_comp = both(en, n_nodes, 90, np.zeros(0, np.uint32), np.zeros(0, np.uint32))
    assert np.array_equal(en, before)  # the wrapper works on a copy
    assert np.array_equal(new_en, en) and np.array_equal(node_map, np.arange(n_nodes)) and (n_out, n_nonint_out, n_comp) == (n_nodes, 90, 0)
    only_self = both(en, n_nodes, 90, [3, 4], [3, 4])
    assert np.array_equal(only_self[0], en) and only_self[4] == 0
    empty = both(np.zeros((0, 4), np.uint32), 0, 0, [], [])
    assert empty[0].shape == (0, 4) and empty[2:] == (0, 0, 0)


def test_restatements_agree_with_the_library_tables():
    for dim in (2, 3):
        for p in (1, 2, 5):
            assert np.array_equal(R.side_nodes(dim, p), system.side_nodes(dim, p))
    for n in range(2, 10):
        # a few ulp of 1 either way; the match tests need the two to agree far below tolerance / 3 = 3e-13
        assert np.abs(R.gll(n) - system.gll_nodes(n)).max() < 1e-15
    part = system.SquarePartition((3, 2), 3, perturb=0.1)
    ids, loc = R.side_node_locations(part, *part.boundary_sides(range(4)))
    assert np.abs(loc - part.node_coords()[ids]).max() < 1e-15
    nm = np.array([0, 1, 0, 2, 1])
    x = np.arange(6.0).reshape(1, 6)
    assert np.array_equal(R.prolong(nm, x, 2), [[0, 1, 2, 3, 0, 1, 4, 5, 2, 3]])
    y = np.arange(10.0).reshape(1, 10)
    assert np.array_equal(R.restrict(nm, y, 2, 3), [[0 + 4, 1 + 5, 2 + 8, 3 + 9, 6, 7]])
    assert np.isclose((R.prolong(nm, x, 2) * y).sum(), (x * R.restrict(nm, y, 2, 3)).sum())


def periodic_pairs(part, axes):
    """High side -> low side of every listed axis of a structured partition of the unit square / cube, by the all-pairs match"""
    a, b = [], []
    for axis in axes:
        low = 2 * (part.dim - 1 - axis)
        t = np.zeros(3)
        t[axis] = -1.0
        ps, pd, n_unmatched, n_ambiguous, first = R.brute_force_match(part, part.boundary_sides([low + 1]), part.boundary_sides([low]), t)
        assert (n_unmatched, n_ambiguous, first) == (0, 0, -1)
        a.append(ps), b.append(pd)
    return np.concatenate(a), np.concatenate(b)


@pytest.mark.parametrize("ne,p,axes", [((5, 3), 1, (0,)), ((5, 3), 3, (0,)), ((4, 3), 2, (1,)), ((5, 3), 1, (0, 1)), ((4, 3), 4, (0, 1)),
                                       ((1, 2), 3, (0, 1))])
def test_closed_form_node_counts_quads(ne, p, axes):
    part = system.SquarePartition(ne, p)
    n_nodes = part.n_owned_nodes
    n_nonint = n_nodes - part.n_elems * (p - 1) ** 2
    R.check_numbering(part.elem_nodes, n_nodes, n_nonint, 2, p)
    a, b = periodic_pairs(part, axes)
    new_en, node_map, n_out, n_nonint_out, n_comp = both(part.elem_nodes, n_nodes, n_nonint, a, b)
    nx, ny = (ne[0] * p + (0 not in axes)), (ne[1] * p + (1 not in axes))
    assert n_out == nx * ny  # (nx p)(ny p + 1) periodic in x, (nx p)(ny p) in x and y
    R.check_numbering(new_en, n_out, n_nonint_out, 2, p, part.elem_nodes)
    if axes == (0, 1):  # the four corners are one node
        xy = part.node_coords()
        corners = np.nonzero(((xy[:, 0] < 1e-9) | (xy[:, 0] > 1 - 1e-9)) & ((xy[:, 1] < 1e-9) | (xy[:, 1] > 1 - 1e-9)))[0]
        assert corners.size == 4 and np.unique(node_map[corners]).size == 1
        assert n_comp == (ne[0] * p - 1) + (ne[1] * p - 1) + 1


@pytest.mark.parametrize("ne,p", [((3, 2, 2), 1), ((3, 2, 2), 3), ((1, 2, 2), 2)])
def test_closed_form_node_counts_fully_periodic_hexes(ne, p):
    part = system.CubePartition(ne, p)
    n_nodes = part.n_owned_nodes
    n_nonint = n_nodes - part.n_elems * (p - 1) ** 3
    a, b = periodic_pairs(part, (0, 1, 2))
    new_en, node_map, n_out, n_nonint_out, n_comp = both(part.elem_nodes, n_nodes, n_nonint, a, b)
    assert n_out == ne[0] * p * ne[1] * p * ne[2] * p
    R.check_numbering(new_en, n_out, n_nonint_out, 3, p, part.elem_nodes)
    xyz = part.node_coords()
    on = (xyz < 1e-9) | (xyz > 1 - 1e-9)
    corners = np.nonzero(on.all(axis=1))[0]
    assert corners.size == 8 and np.unique(node_map[corners]).size == 1
    # nodes merge exactly when they agree modulo 1 in every coordinate
    key = np.round(np.mod(xyz, 1.0) * 1e6).astype(np.int64) % 10 ** 6
    _, inverse = np.unique(key, axis=0, return_inverse=True)
    assert inverse.max() + 1 == n_out
    assert np.unique(np.stack([inverse.ravel(), node_map.astype(np.int64)], axis=1), axis=0).shape[0] == n_out


def test_merge_refusals():
    lib = capi.load()
    en = np.array([[0, 1, 2, 4], [1, 3, 2, 5]], dtype=np.uint32)
    a, b = np.array([0], np.uint32), np.array([3], np.uint32)
    node_map = np.full(6, 77, np.uint32)
    out = [C.c_int64(-5) for _ in range(3)]
    p32 = capi.c_uint32_p
    good = [6, 4, 1, a.ctypes.data_as(p32), b.ctypes.data_as(p32), 8, en.ctypes.data_as(p32), node_map.ctypes.data_as(p32),
            C.byref(out[0]), C.byref(out[1]), C.byref(out[2])]

    def refused(**change):
        args = list(good)
        for k, v in change.items():
            args[int(k[1:])] = v
        before = en.copy()
        assert lib.l3k_periodic_merge(*args) == -1
        assert "l3k_periodic_merge" in lib.l3k_last_error().decode()
        assert np.array_equal(en, before) and np.all(node_map == 77) and [o.value for o in out] == [-5] * 3  # nothing written

    internal, outside = np.array([4], np.uint32), np.array([6], np.uint32)
    refused(a3=internal.ctypes.data_as(p32)), refused(a4=internal.ctypes.data_as(p32))  # an element-internal node
    refused(a3=outside.ctypes.data_as(p32)), refused(a4=outside.ctypes.data_as(p32))
    refused(a0=5)  # an elem_nodes entry >= n_nodes
    refused(a3=None), refused(a4=None), refused(a6=None), refused(a7=None), refused(a8=None), refused(a9=None), refused(a10=None)
    refused(a0=-1), refused(a1=-1), refused(a1=7), refused(a2=-1), refused(a5=-1)
    assert lib.l3k_periodic_merge(*good) == 0
    assert en.tolist() == [[0, 1, 2, 3], [1, 0, 2, 4]] and node_map.tolist() == [0, 1, 2, 0, 3, 4]
    assert [o.value for o in out] == [5, 3, 1]
    with pytest.raises(capi.L3KError, match="l3k_periodic_merge"):
        system.periodic_merge(en, 5, 3, [4], [0])
    with pytest.raises(capi.L3KError):
        system.periodic_merge(en, 5, 3, [0, 1], [2])


def build_cpp_shim(out):
    """tests/cpp/periodic_shim.cpp against include/l3k/operator.hpp and the library"""
    import shutil
    import subprocess
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    cmd = [hipcc, "-std=c++20", "-O1", "--offload-arch=gfx950", f"-I{ROOT}/include", os.path.join(ROOT, "tests", "cpp", "periodic_shim.cpp"),
           f"-L{ROOT}/l3ster_amd/lib", "-ll3k", f"-Wl,-rpath,{ROOT}/l3ster_amd/lib", "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


def test_cpp_mirror_merges_on_the_host(tmp_path):
    import subprocess
    exe = build_cpp_shim(str(tmp_path / "periodic_shim"))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr


def test_names_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "l3k.h")).read()
    lib = capi.load()
    for name in ("l3k_periodic_match", "l3k_periodic_merge"):
        assert f"int {name}(" in header
        assert name in capi.SIGNATURES
        assert getattr(lib, name) is not None
    assert "#define L3K_VERSION 101" in header
    assert "bcs/PeriodicBC.hpp" in header and "BCDefinition.hpp:92-104" in header
    assert callable(system.periodic_match) and callable(system.periodic_merge) and callable(system.ElevatedMesh.periodic)
