"""The numpy restatement of the quad element and side systems (tests/quad_asm_ref.py) proved against the CPU oracle, and what
of the assembled-system object (l3k_asm_*, include/l3k.h) can be checked without a device: the symbols and prototypes, the layout
of l3k_asm_info, and the refusals that need no handle."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle_lib as O
import quad_asm_ref as Q
from l3ster_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# a distorted quad (vertex i + 2j), no two sides parallel
VERTS = np.array([[0.0, 0.1, 0.0], [1.3, -0.2, 0.0], [-0.15, 0.9, 0.0], [1.1, 1.25, 0.0]])


@pytest.mark.parametrize("p", [1, 2, 3, 4])
@pytest.mark.parametrize("R", [1, 2])
def test_element_system_vs_oracle(p, R):
    """Diffusion2D (kernel id 2): K to 1e-13 |K|max; F is identically zero on both sides (the kernel has no source)"""
    for nq in (p + 1, p + 3):
        K_ref, F_ref = O.assemble_local(O.KERNEL_DIFFUSION2D, p, nq, R, VERTS)
        K, F = Q.element_system(Q.diffusion2d(R), p, nq, VERTS)
        assert K.shape == K_ref.shape and F.shape == F_ref.shape == ((p + 1) ** 2 * 3, R)
        assert np.abs(K - K_ref).max() <= 1e-13 * np.abs(K_ref).max()
        assert not F.any() and not F_ref.any()


@pytest.mark.parametrize("p", [2, 4])
def test_element_system_with_a_field_vs_oracle(p):
    """Diffusion2DVar (kernel id 3): the interpolated field and its physical derivatives enter the operators"""
    nf = np.random.default_rng(p).uniform(0.5, 1.5, ((p + 1) ** 2, 1))
    K_ref, _ = O.assemble_local(O.KERNEL_DIFFUSION2D_VAR, p, p + 1, 1, VERTS, node_fields=nf)
    K, _ = Q.element_system(Q.diffusion2d_var(), p, p + 1, VERTS, node_fields=nf)
    assert np.abs(K - K_ref).max() <= 1e-13 * np.abs(K_ref).max()


@pytest.mark.parametrize("p", [1, 2, 3, 4])
@pytest.mark.parametrize("side", [0, 1, 2, 3])
def test_side_system_vs_oracle(p, side):
    """Adiabatic2D (kernel id 5) on every side: the outward normal and the line jacobian of the distorted quad"""
    K_ref, F_ref = O.assemble_local_side(side, O.KERNEL_ADIABATIC2D, p, p + 1, 1, VERTS)
    K, F = Q.side_system(Q.adiabatic2d(), side, p, p + 1, VERTS)
    assert K.shape == K_ref.shape == ((p + 1) ** 2 * 3,) * 2
    assert np.abs(K_ref).max() > 0
    assert np.abs(K - K_ref).max() <= 1e-13 * np.abs(K_ref).max()
    assert not F.any() and not F_ref.any()


def test_source_term_reaches_F():
    """A kernel with a point-dependent source: F = sum_q w jac B^T f is not zero, and is linear in the source"""
    def kernel(scale):
        def k(vals, ders, point, normal, time):
            A0, A1, A2, _ = Q.diffusion2d()(vals, ders, point, normal, time)
            f = np.zeros((4, 1))
            f[0, 0] = scale * (1.0 + point[0] + 2.0 * point[1] + time)
            return A0, A1, A2, f
        return k
    K1, F1 = Q.element_system(kernel(1.0), 2, 3, VERTS, time=0.5)
    K2, F2 = Q.element_system(kernel(2.0), 2, 3, VERTS, time=0.5)
    assert np.abs(F1).max() > 0 and np.allclose(F2, 2.0 * F1, rtol=1e-14, atol=0) and np.array_equal(K1, K2)


# ---------------------------------------------------------------------------------------------- l3k_asm_* without a device
PROTOTYPES = {
    "l3k_asm_element_systems": "int l3k_asm_element_systems(l3k_mf* term, int64_t first, int64_t count, double* d_K, double* d_F);",
    "l3k_asm_side_systems": "int l3k_asm_side_systems(l3k_bnd* term, int64_t first, int64_t count, double* d_K, double* d_F);",
    "l3k_asm_create": "int l3k_asm_create(l3k_mesh* mesh, int n_fields, const int* field_inds, int n_rhs, size_t workspace_bytes, l3k_asm** out);",
    "l3k_asm_begin": "int l3k_asm_begin(l3k_asm* A);",
    "l3k_asm_add_domain": "int l3k_asm_add_domain(l3k_asm* A, l3k_mf* term, int64_t first, int64_t count);",
    "l3k_asm_add_boundary": "int l3k_asm_add_boundary(l3k_asm* A, l3k_bnd* term, int64_t first, int64_t count);",
    "l3k_asm_end": "int l3k_asm_end(l3k_asm* A, const double* d_dirichlet_vals, size_t ldg);",
    "l3k_asm_info_get": "int l3k_asm_info_get(const l3k_asm* A, l3k_asm_info* out);",
    "l3k_asm_destroy": "int l3k_asm_destroy(l3k_asm* A);",
}


def test_symbols_and_prototypes():
    lib = capi.load()
    header = open(os.path.join(ROOT, "include", "l3k.h")).read()
    for name, proto in PROTOTYPES.items():
        assert hasattr(lib, name), name
        assert proto in header, name
        fn = getattr(lib, name)
        assert fn.restype is C.c_int
        n_params = len(re.search(re.escape(name) + r"\((.*?)\);", proto).group(1).split(","))
        assert len(fn.argtypes) == n_params, name
    assert "enum { L3K_ASM_NEW = 0, L3K_ASM_OPEN = 1, L3K_ASM_CLOSED = 2 };" in header


def test_info_layout_matches_the_header():
    names = [n for n, _ in capi.AsmInfo._fields_]
    assert names == ["n", "nnz", "n_missing", "ldr", "n_rhs", "state", "d_row_ptr", "d_col_ind", "d_values", "d_rhs", "csr"]
    assert [t for _, t in capi.AsmInfo._fields_] == [C.c_int64] * 3 + [C.c_size_t] + [C.c_int] * 2 + [C.c_void_p] * 5
    assert C.sizeof(capi.AsmInfo) == 3 * 8 + 8 + 2 * 4 + 5 * 8


def test_refusals_without_a_device():
    """Null handles: -1 and a message naming the call.  Bad field_inds and n_rhs are refused before the mesh is looked at."""
    lib = capi.load()
    out, info = C.c_void_p(), capi.AsmInfo()
    mesh = C.c_void_p(1)  # never dereferenced by the calls below
    one = (C.c_int * 1)(0)
    null_calls = {
        "l3k_asm_element_systems": lambda: lib.l3k_asm_element_systems(None, 0, 0, None, None),
        "l3k_asm_side_systems": lambda: lib.l3k_asm_side_systems(None, 0, 0, None, None),
        "l3k_asm_create": lambda: lib.l3k_asm_create(None, 0, None, 1, 0, C.byref(out)),
        "l3k_asm_begin": lambda: lib.l3k_asm_begin(None),
        "l3k_asm_add_domain": lambda: lib.l3k_asm_add_domain(None, None, 0, 0),
        "l3k_asm_add_boundary": lambda: lib.l3k_asm_add_boundary(None, None, 0, 0),
        "l3k_asm_end": lambda: lib.l3k_asm_end(None, None, 0),
        "l3k_asm_info_get": lambda: lib.l3k_asm_info_get(None, C.byref(info)),
    }
    for name, call in null_calls.items():
        assert call() == -1, name
        assert lib.l3k_last_error().decode() == f"{name}: null argument", name
        with pytest.raises(capi.L3KError, match=name):
            capi.check(call())
    assert lib.l3k_asm_create(mesh, 0, None, 1, 0, None) == -1
    assert lib.l3k_last_error().decode() == "l3k_asm_create: null argument"
    for n_fields, fi in [(-1, None), (2, None), (0, one)]:
        assert lib.l3k_asm_create(mesh, n_fields, fi, 1, 0, C.byref(out)) == -1
        assert "field_inds" in lib.l3k_last_error().decode()
    assert lib.l3k_asm_create(mesh, 0, None, 0, 0, C.byref(out)) == -1
    assert "n_rhs" in lib.l3k_last_error().decode()
    assert out.value is None and lib.l3k_asm_destroy(None) == 0
