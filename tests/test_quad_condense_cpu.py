"""CPU-side checks of static condensation on quads inside the assembled system: the node split against its closed forms, the numpy
helper of the GPU tests against itself (the global Schur complement over all internal dofs is the sum of the element ones), and the
new entry points in the header and in capi.py."""
import os
import re

import numpy as np
import pytest

import quad_condense_ref as QC
from l3ster_amd import capi, system

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("l3k_asm_create_condensed", "l3k_asm_cond_info_get", "l3k_asm_recover", "l3k_asm_schur_updates")


@pytest.mark.parametrize("p", range(1, 9))
def test_quad_node_split_closed_forms(p):
    prim, inner = system.element_node_split(p, dim=2)
    n = p + 1
    assert len(prim) == 4 * p and len(inner) == (p - 1) ** 2
    assert np.all(np.diff(prim) > 0) and np.all(np.diff(inner) > 0)
    assert sorted(np.concatenate([prim, inner])) == list(range(n * n))
    ix, iy = prim % n, prim // n
    assert np.all((ix == 0) | (ix == p) | (iy == 0) | (iy == p))
    ix, iy = inner % n, inner // n
    assert np.all((ix >= 1) & (ix <= p - 1) & (iy >= 1) & (iy <= p - 1))
    # the default stays the hex split
    hp, hi = system.element_node_split(p)
    hp3, hi3 = system.element_node_split(p, dim=3)
    assert len(hp) == n ** 3 - (p - 1) ** 3 and np.array_equal(hp, hp3) and np.array_equal(hi, hi3)
    with pytest.raises(system.L3KError, match="dim"):
        system.element_node_split(p, dim=1)


@pytest.mark.parametrize("p,U", [(2, 1), (3, 2), (4, 3)])
def test_global_schur_complement_is_the_sum_of_the_element_ones(p, U):
    """Random SPD element matrices on a 3 x 2 quad mesh: the internal dofs of different elements do not couple, so the Schur
    complement of the assembled matrix over all of them is the assembled sum of the element Schur complements"""
    part = system.SquarePartition((3, 2), p)
    rng = np.random.default_rng(10 * p + U)
    NN, R = (p + 1) ** 2, 2
    n = part.n_local_nodes * U
    A, f = np.zeros((n, n)), np.zeros((n, R))
    S_sum, g_sum = np.zeros((n, n)), np.zeros((n, R))
    pe, ie = QC.dof_split(p, U)
    for e in range(part.n_elems):
        B = rng.standard_normal((NN * U, NN * U))
        K, F = B @ B.T + NN * U * np.eye(NN * U), rng.standard_normal((NN * U, R))
        d = (part.elem_nodes[e].astype(np.int64)[:, None] * U + np.arange(U)[None, :]).reshape(-1)
        A[np.ix_(d, d)] += K
        f[d] += F
        S, g, _ = QC.schur_complement(K, F, pe, ie)
        S_sum[np.ix_(d[pe], d[pe])] += S
        g_sum[d[pe]] += g
    prim, inner = QC.mesh_split(part, U, range(U))
    assert len(inner) == part.n_elems * (p - 1) ** 2 * U and len(prim) + len(inner) == n
    S, g, cond = QC.schur_complement(A, f, prim, inner)
    assert np.abs(S - S_sum[np.ix_(prim, prim)]).max() <= QC.tol(cond, A)
    assert np.abs(g - g_sum[prim]).max() <= QC.tol(cond, A)
    # recovery gives back the internal part of the full solve
    x = np.linalg.solve(A, f)
    x_i = QC.recover(A, f, prim, inner, np.linalg.solve(S, g))
    assert np.abs(x_i - x[inner]).max() <= 1e-10 * np.abs(x).max()


def test_embed_places_a_term_in_the_systems_fields():
    K, F = np.arange(16.0).reshape(4, 4), np.arange(8.0).reshape(4, 2)
    Ks, Fs = QC.embed(K, F, 2, [4, 1], [0, 1, 2, 4])  # two nodes, unknowns -> slots 3 and 1
    d = [3, 1, 7, 5]
    assert np.array_equal(Ks[np.ix_(d, d)], K) and np.array_equal(Fs[d], F) and Ks.sum() == K.sum()


def test_cpp_mirror_compiles_and_links(tmp_path):
    """tests/cpp/quad_condense_shim.cpp against include/l3k/operator.hpp and the built library (it runs in the GPU tests)"""
    import shutil
    import subprocess
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    cmd = [hipcc, "-std=c++20", "-O1", "--offload-arch=gfx950", f"-I{ROOT}/include", os.path.join(ROOT, "tests", "cpp", "quad_condense_shim.cpp"),
           f"-L{ROOT}/l3ster_amd/lib", "-ll3k", f"-Wl,-rpath,{ROOT}/l3ster_amd/lib", "-o", str(tmp_path / "quad_condense_shim")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def test_header_and_bindings_declare_the_new_entry_points():
    header = open(os.path.join(ROOT, "include", "l3k.h")).read()
    assert "#define L3K_VERSION 101" in header
    for name in NEW + ("l3k_asm_create",):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
        assert m, name
        assert len(m.group(1).split(",")) == len(capi.SIGNATURES[name][1]), name
    assert re.search(r"\}\s*l3k_asm_cond_info\s*;", header)
    fields = [n for n, _ in capi.AsmCondInfo._fields_]
    assert fields == ["condensed", "n_primary_nodes", "n_internal_nodes", "n_elems", "store_bytes", "n_failed"]
    lib = capi.load()
    assert all(hasattr(lib, name) for name in NEW) and lib.l3k_version() == 101
