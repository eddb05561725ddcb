"""Boundary equation kernels in the assembled path without a device: the three new symbols of libl3k.so with the prototypes of
include/l3k.h, and the refusals that need no handle."""
import ctypes as C
import os
import re

import pytest

from l3ster_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WANT = {
    "l3k_bnd_local_assemble": "int l3k_bnd_local_assemble(l3k_bnd* bnd, int64_t first, int64_t count, double* d_K, double* d_F);",
    "l3k_bnd_assemble_global": "int l3k_bnd_assemble_global(l3k_bnd* bnd, int64_t first, int64_t count, const int64_t* d_row_ptr, "
                               "const int32_t* d_col_ind, double* d_values, double* d_rhs, size_t ldr, int skip_dirichlet, "
                               "size_t workspace_bytes, int64_t* n_missing);",
    "l3k_mf_assemble_boundary": "int l3k_mf_assemble_boundary(l3k_mf* mf, int on);",
}


def test_symbols_and_prototypes():
    lib = capi.load()
    header = " ".join(open(os.path.join(ROOT, "include", "l3k.h")).read().split())
    for name, proto in WANT.items():
        assert hasattr(lib, name), name
        assert proto in header, name
        assert getattr(lib, name).restype is C.c_int
        n_params = len(re.search(re.escape(name) + r"\((.*?)\);", proto).group(1).split(","))
        assert len(getattr(lib, name).argtypes) == n_params, name
    assert lib.l3k_version() == 101


def test_null_handles_are_refused_with_the_name_of_the_call():
    lib = capi.load()
    missing = C.c_int64(7)
    calls = {
        "l3k_bnd_local_assemble": lambda: lib.l3k_bnd_local_assemble(None, 0, 0, None, None),
        "l3k_bnd_assemble_global": lambda: lib.l3k_bnd_assemble_global(None, 0, 0, None, None, None, None, 0, 0, 0, C.byref(missing)),
        "l3k_mf_assemble_boundary": lambda: lib.l3k_mf_assemble_boundary(None, 1),
    }
    for name, call in calls.items():
        assert call() == -1, name
        msg = lib.l3k_last_error().decode()
        assert msg.startswith(name + ": null"), msg
        with pytest.raises(capi.L3KError, match=name):
            capi.check(call())
    assert missing.value == 7  # nothing was written through a refused call


def test_python_mirrors_exist():
    from l3ster_amd import system
    for cls, name in ((system.BoundaryTerm, "local_assemble"), (system.BoundaryTerm, "assemble_global"),
                      (system.MatrixFreeSystem, "assemble_boundary")):
        assert callable(getattr(cls, name))
