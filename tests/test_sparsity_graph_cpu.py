"""The device sparsity-graph builder without a device: the four l3k_graph_* symbols of libl3k.so with the prototypes of include/l3k.h,
the layout of l3k_graph_info, and the refusals that need no handle."""
import ctypes as C
import os
import re

import pytest
import torch

from l3ster_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("l3k_graph_create", "l3k_graph_info_get", "l3k_graph_fill", "l3k_graph_destroy")


def test_symbols_and_prototypes():
    lib = capi.load()
    header = open(os.path.join(ROOT, "include", "l3k.h")).read()
    want = {
        "l3k_graph_create": "int l3k_graph_create(l3k_mesh* mesh, int n_fields, const int* field_inds, int kind, l3k_graph** out);",
        "l3k_graph_info_get": "int l3k_graph_info_get(const l3k_graph* g, l3k_graph_info* out);",
        "l3k_graph_fill": "int l3k_graph_fill(l3k_graph* g, int64_t* d_row_ptr, int32_t* d_col_ind);",
        "l3k_graph_destroy": "int l3k_graph_destroy(l3k_graph* g);",
    }
    for name in NAMES:
        assert hasattr(lib, name), name
        assert want[name] in header, name
        argtypes = getattr(lib, name).argtypes
        assert getattr(lib, name).restype is C.c_int
        # one ctypes argument per parameter of the C prototype
        n_params = len(re.search(re.escape(name) + r"\((.*?)\);", want[name]).group(1).split(","))
        assert len(argtypes) == n_params, name
    assert "enum { L3K_GRAPH_FULL = 0, L3K_GRAPH_CONDENSED = 1 };" in header


def test_info_layout_matches_the_header():
    """int64 n, nnz, n_empty_rows, max_row_len, n_rows_scratch, workspace_bytes; int max_elems_per_node, lds_key_capacity"""
    names = [n for n, _ in capi.GraphInfo._fields_]
    assert names == ["n", "nnz", "n_empty_rows", "max_row_len", "n_rows_scratch", "workspace_bytes", "max_elems_per_node",
                     "lds_key_capacity"]
    assert [t for _, t in capi.GraphInfo._fields_] == [C.c_int64] * 6 + [C.c_int] * 2
    assert C.sizeof(capi.GraphInfo) == 6 * 8 + 2 * 4


def test_entry_points_fail_loudly_without_a_device():
    """No handle can exist without a device; the entry points refuse null handles with -1 and a message naming the call, and
    destroying nothing is a no-op."""
    lib = capi.load()
    out, info = C.c_void_p(), capi.GraphInfo()
    mesh = C.c_void_p(1)  # never dereferenced: `out` is checked with it
    calls = {
        "l3k_graph_create": lambda: lib.l3k_graph_create(None, 0, None, 0, C.byref(out)),
        "l3k_graph_info_get": lambda: lib.l3k_graph_info_get(None, C.byref(info)),
        "l3k_graph_fill": lambda: lib.l3k_graph_fill(None, None, None),
    }
    for name, call in calls.items():
        assert call() == -1, name
        assert lib.l3k_last_error().decode() == f"{name}: null argument", name
        with pytest.raises(capi.L3KError, match=name):
            capi.check(call())
    assert lib.l3k_graph_create(mesh, 0, None, 0, None) == -1
    assert lib.l3k_last_error().decode() == "l3k_graph_create: null argument"
    assert out.value is None and lib.l3k_graph_destroy(None) == 0
    if not torch.cuda.is_available():
        from l3ster_amd import system
        with pytest.raises(system.L3KError, match="no HIP device|no CPU fallback"):
            system.Context(0)
