"""What of the matrix-free sum of several terms (l3k_mfs_*, system.MultiTermSystem, partition.element_subset) can be checked
without a device: the header against the bindings and the library, the layout of the info struct, the element subsets, the
refusals that come before any device call, and that the C++ mirror compiles and links."""
import ctypes as C
import os
import re
import shutil
import subprocess
import types

import numpy as np
import pytest

from l3ster_amd import capi, gmsh, partition, system

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MULTIDOM = os.path.join(ROOT, "tests", "golden", "gmsh_ascii4_square_multidom.msh")
NEW = ("l3k_mfs_create", "l3k_mfs_add_domain", "l3k_mfs_add_boundary", "l3k_mfs_finalize", "l3k_mfs_info_get", "l3k_mfs_active",
       "l3k_mfs_destroy", "l3k_mfs_apply", "l3k_mfs_scale", "l3k_mfs_apply_elems", "l3k_mfs_dirichlet_rows", "l3k_mfs_diag_rhs",
       "l3k_mfs_jacobi_inverse", "l3k_mfs_apply_energy", "l3k_mfs_pcg_solve", "l3k_mfs_pcg_solve_cols", "l3k_mfs_cheb_create",
       "l3k_mfs_pcg_solve_cheb")
# the split-phase calls take the arguments of their single-term twins
TWINS = {"l3k_mfs_apply": "l3k_mf_apply", "l3k_mfs_scale": "l3k_mf_scale", "l3k_mfs_apply_elems": "l3k_mf_apply_elems",
         "l3k_mfs_dirichlet_rows": "l3k_mf_dirichlet_rows", "l3k_mfs_diag_rhs": "l3k_mf_diag_rhs", "l3k_mfs_apply_energy": "l3k_mf_apply_energy",
         "l3k_mfs_pcg_solve": "l3k_pcg_solve", "l3k_mfs_pcg_solve_cols": "l3k_pcg_solve_cols", "l3k_mfs_cheb_create": "l3k_cheb_create",
         "l3k_mfs_pcg_solve_cheb": "l3k_pcg_solve_cheb"}


def test_header_bindings_and_library_agree():
    header = open(os.path.join(ROOT, "include", "l3k.h")).read()
    lib = capi.load()
    for name in NEW:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
        assert m, name
        assert len(m.group(1).split(",")) == len(capi.SIGNATURES[name][1]), name
        assert capi.SIGNATURES[name][0] is C.c_int and hasattr(lib, name), name
    for name, twin in TWINS.items():
        assert [a for a in capi.SIGNATURES[name][1]] == [a for a in capi.SIGNATURES[twin][1]], name

        def params(n):
            text = re.search(r"\bint\s+" + n + r"\s*\(([^;]*)\)\s*;", header).group(1)
            return [re.sub(r"\s+", " ", p).strip() for p in text.split(",")][1:]  # (the handle differs)
        assert params(name) == params(twin), name
    # every new entry point cites the reference lines it stands for
    section = header[header.index("matrix-free systems of several terms"):header.index("typedef struct l3k_mfs l3k_mfs;")]
    for cite in ("algsys/MatrixFreeSystem.hpp:24-89", ":789-802", ":876-885", ":888-941", ":1020-1140", "solve/NativePreconditioners.hpp:75-96",
                 "solve/BelosSolvers.hpp:116-122", "tests/MultiDomainTest.cpp"):
        assert cite in section, cite


def test_info_struct_layout():
    header = open(os.path.join(ROOT, "include", "l3k.h")).read()
    body = re.search(r"typedef struct\s*\{([^}]*)\}\s*l3k_mfs_info\s*;", header).group(1)
    names = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.split(None, 1)[1].split(",")]
    assert names == [n for n, _ in capi.MfsInfo._fields_] == ["n_terms", "n_rows", "n_active_rows", "n_dirichlet_rows", "n_rhs", "finalized"]
    assert [t for _, t in capi.MfsInfo._fields_] == [C.c_int64] * 4 + [C.c_int] * 2
    assert C.sizeof(capi.MfsInfo) == 40 and capi.MfsInfo.n_rhs.offset == 32 and capi.MfsInfo.finalized.offset == 36


def check_subset(part, sub, elems):
    elems = np.asarray(elems, dtype=np.int64)
    interior = elems < part.n_interior_elems
    want = np.concatenate([elems[interior], elems[~interior]])  # the order kept, interior first
    assert np.array_equal(sub.elem_index, want)
    assert (sub.n_elems, sub.n_interior_elems) == (elems.size, int(interior.sum()))
    assert np.array_equal(sub.elem_nodes, part.elem_nodes[want]) and sub.elem_nodes.dtype == part.elem_nodes.dtype
    assert np.array_equal(sub.elem_verts, part.elem_verts[want])
    assert sub.elem_nodes.flags.c_contiguous and sub.elem_verts.flags.c_contiguous
    for name in ("dim", "order", "n_owned_nodes", "n_ghost_nodes", "n_local_nodes", "global_node_base", "n_global_nodes"):
        assert getattr(sub, name) == getattr(part, name), name
    for name in ("node_grid_id", "node_boundary", "ghost_global_id", "send_nodes", "ghost_ranges", "nbr_rank"):
        if hasattr(part, name):
            assert getattr(sub, name) is getattr(part, name), name  # shared, not copied


def test_element_subset_on_a_cube_partition():
    part = system.CubePartition((4, 3, 3), 2, parts=(2, 1, 1), rank=1, perturb=0.1)
    assert 0 < part.n_interior_elems < part.n_elems and part.n_ghost_nodes > 0
    n_before = part.n_elems
    elems = [part.n_elems - 1, 3, part.n_interior_elems, 0, part.n_interior_elems - 1, 7]  # border and interior, unordered
    sub = partition.element_subset(part, elems)
    check_subset(part, sub, elems)
    assert np.array_equal(sub.elem_boundary, part.elem_boundary[sub.elem_index]) and part.n_elems == n_before
    assert np.array_equal(sub.dirichlet_mask(4), part.dirichlet_mask(4))  # node level: the parent's
    assert np.array_equal(sub.node_coords()[np.unique(sub.elem_nodes)], part.node_coords()[np.unique(sub.elem_nodes)])
    check_subset(part, partition.element_subset(part, np.arange(part.n_elems)), np.arange(part.n_elems))
    empty = partition.element_subset(part, [])
    assert (empty.n_elems, empty.n_interior_elems) == (0, 0) and empty.elem_nodes.shape == (0, 27)
    for bad in ([part.n_elems], [-1], [0, 5, part.n_elems + 3]):
        with pytest.raises(ValueError, match="outside"):
            partition.element_subset(part, bad)
    with pytest.raises(ValueError, match="twice"):
        partition.element_subset(part, [2, 5, 2])
    with pytest.raises(ValueError, match="integer"):
        partition.element_subset(part, [0.5])


def multidom_part():
    """The multi-domain square as the part an ElevatedMesh is, without its device calls: order 1, where the connectivity of the
    file is the node table"""
    m = gmsh.read_mesh(MULTIDOM)
    n = m.verts.shape[0]
    return m, types.SimpleNamespace(dim=2, order=1, n_elems=m.conn.shape[0], n_interior_elems=m.conn.shape[0], elem_nodes=m.conn.copy(),
                                    elem_verts=m.verts[m.conn.astype(np.int64)], n_owned_nodes=n, n_ghost_nodes=0, n_local_nodes=n,
                                    global_node_base=0, n_global_nodes=n, elem_domain=m.elem_domain, nbr_rank=[], send_nodes=[],
                                    ghost_ranges=[], face_elem=np.array([3, -1, 9], np.int64), face_side=np.array([0, 255, 2], np.uint8),
                                    elements_of=lambda ids: np.nonzero(np.isin(m.elem_domain, ids))[0])


def test_element_subset_on_the_multidomain_mesh():
    m, part = multidom_part()
    domains = np.unique(m.elem_domain)
    seen = []
    for d in domains:
        elems = part.elements_of([d])
        sub = partition.element_subset(part, elems)
        check_subset(part, sub, elems)
        assert np.all(sub.elem_domain == d) and sub.n_elems == int((m.elem_domain == d).sum())
        seen.append(sub.elem_index)
        # boundary elements follow their elements; those of absent elements are the side of none
        for f, e in enumerate(part.face_elem):
            if e >= 0 and e in elems:
                assert sub.elem_index[sub.face_elem[f]] == e and sub.face_side[f] == part.face_side[f]
            else:
                assert sub.face_elem[f] == -1 and sub.face_side[f] == 255
    assert np.array_equal(np.sort(np.concatenate(seen)), np.arange(part.n_elems))  # the domains tile the mesh
    assert system.ElevatedMesh.subset(part, domains[:2]).n_elems == int(np.isin(m.elem_domain, domains[:2]).sum())


def test_refusals_without_a_device():
    lib = capi.load()
    err = lambda: lib.l3k_last_error().decode()
    out = C.c_void_p()
    assert lib.l3k_mfs_create(None, 1, C.byref(out)) == -1 and "null argument" in err() and not out.value
    for fn, args in ((lib.l3k_mfs_add_domain, (None, None)), (lib.l3k_mfs_add_boundary, (None, None)), (lib.l3k_mfs_finalize, (None,)),
                     (lib.l3k_mfs_info_get, (None, None)), (lib.l3k_mfs_active, (None, None)),
                     (lib.l3k_mfs_apply, (None, None, 0, None, 0, 1, 1.0, 0.0)), (lib.l3k_mfs_scale, (None, None, 0, 1, 0.0)),
                     (lib.l3k_mfs_apply_elems, (None, 2, None, 0, None, 0, None, 0, None, 0, 1, 1.0, 0.0)),
                     (lib.l3k_mfs_dirichlet_rows, (None, None, 0, None, 0, 1, 1.0)),
                     (lib.l3k_mfs_diag_rhs, (None, 2, None, 0, None, None, 0, None, None, 0, 1)),
                     (lib.l3k_mfs_jacobi_inverse, (None, None, 1.0, 0.0, None)), (lib.l3k_mfs_apply_energy, (None, None, None, None)),
                     (lib.l3k_mfs_pcg_solve, (None, None, None, None, None, None)),
                     (lib.l3k_mfs_pcg_solve_cols, (None, None, 0, None, 0, 1, None, None, None)),
                     (lib.l3k_mfs_cheb_create, (None, None, None, None)), (lib.l3k_mfs_pcg_solve_cheb, (None, None, None, None, None, None))):
        assert fn(*args) == -1, fn.__name__
        assert "null argument" in err() or "bad argument" in err(), (fn.__name__, err())
    assert lib.l3k_mfs_destroy(None) == 0
    with pytest.raises(capi.L3KError, match="takes a MatrixFreeSystem or a BoundaryTerm"):
        system.MultiTermSystem.add(types.SimpleNamespace(_h=None, terms=[]), object())


def test_pcg_dispatch_knows_the_sum():
    from l3ster_amd import solve
    S = system.MultiTermSystem.__new__(system.MultiTermSystem)
    S.mesh = types.SimpleNamespace(n_owned_dofs=12)
    fn, n = solve._entry(S, "pcg_solve")
    assert n == 12 and fn is capi.load().l3k_mfs_pcg_solve
    assert solve._entry(S, "cheb_create")[0] is capi.load().l3k_mfs_cheb_create
    with pytest.raises(capi.L3KError, match="p-multigrid"):
        solve._entry(S, "pcg_solve_pmg")


def test_cpp_mirror_compiles_and_links(tmp_path):
    """tests/cpp/multiterm_shim.cpp against include/l3k/operator.hpp and the built library (it runs in the GPU tests)"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    cmd = [hipcc, "-std=c++20", "-O1", "--offload-arch=gfx950", f"-I{ROOT}/include", os.path.join(ROOT, "tests", "cpp", "multiterm_shim.cpp"),
           f"-L{ROOT}/l3ster_amd/lib", "-ll3k", f"-Wl,-rpath,{ROOT}/l3ster_amd/lib", "-o", str(tmp_path / "multiterm_shim")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
