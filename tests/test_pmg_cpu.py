"""The p-multigrid preconditioner on the CPU: the 1-D transfer table of the library (l3k_interp_1d) against numpy, the restated
V-cycle of tests/pmg_ref.py as a matrix (symmetric, positive definite), the restated p-MG PCG against the restated Jacobi PCG, the
element pairing helper, the new entry points without a device, and the table's generator under ASan + UBSan in a stand-alone
driver (tests/sanitize/interp_driver.cpp)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import pmg_ref as R
from l3ster_amd import capi, solve, system

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = [(pf, pc) for pf in range(2, 9) for pc in range(1, pf)]
_H = {}


@pytest.mark.parametrize("pf,pc", PAIRS)
def test_interp_1d_equals_the_numpy_table(pf, pc):
    T = system.interp_1d(pc, pf)
    want = R.interp_1d(pc, pf)
    assert T.shape == (pf + 1, pc + 1)
    err = np.abs(T - want).max()
    print(f"orders {pc} -> {pf}: max |T - numpy| = {err:.2e}")
    assert err <= 1e-14
    assert np.abs(T.sum(axis=1) - 1.0).max() <= 1e-14  # rows sum to 1
    unit = np.zeros(pc + 1)
    unit[0] = 1.0
    assert np.array_equal(T[0], unit) and np.array_equal(T[-1], unit[::-1])  # the end rows: exactly unit vectors
    xc, xf = system.gll_nodes(pc + 1), system.gll_nodes(pf + 1)
    for k in range(pc + 1):  # monomials up to degree p_c are reproduced
        assert np.abs(T @ xc ** k - xf ** k).max() <= 1e-14, k
    # ... and the transposed direction (a restriction of node values) is served as well
    assert np.abs(system.interp_1d(pf, pc) - R.interp_1d(pf, pc)).max() <= 1e-13


@pytest.mark.parametrize("p", range(1, 9))
def test_interp_1d_of_equal_orders_is_the_identity(p):
    assert np.array_equal(system.interp_1d(p, p), np.eye(p + 1))


def test_interp_1d_refuses_orders_outside_1_to_8():
    lib, out = capi.load(), np.zeros(100)
    ptr = out.ctypes.data_as(capi.c_double_p)
    for pf, pt in ((0, 2), (2, 0), (9, 2), (2, 9)):
        assert lib.l3k_interp_1d(pf, pt, ptr) == -1 and b"l3k_interp_1d" in lib.l3k_last_error()
    assert lib.l3k_interp_1d(2, 1, None) == -1


def hierarchy():
    """2^3 elements, orders 4 -> 2 -> 1, Diffusion3D with U = 4 and T fixed on all sides; dense level operators"""
    if not _H:
        levels, Ps, data, maps = R.hierarchy(2, (4, 2, 1), dense=True)
        _H.update(levels=levels, Ps=Ps, data=data, maps=maps)
    return _H


def test_prolongation_reproduces_trilinear_functions_and_has_one_owner_per_row():
    H = hierarchy()
    for (f, c), P in zip(zip(H["data"][:-1], H["data"][1:]), H["Ps"]):
        Pu = R.prolongation(f["part"], c["part"], 4, None)  # unmasked
        assert np.abs(Pu.sum(axis=1) - 1.0).max() <= 1e-13
        xc, xf = c["part"].node_coords(), f["part"].node_coords()
        # (the geometry is trilinear in the reference coordinates: the constant and the coordinates are reproduced on any mesh)
        for k in range(3):
            assert np.abs(Pu @ np.repeat(xc[:, k], 4) - np.repeat(xf[:, k], 4)).max() <= 1e-13
        assert np.abs(P.numpy()[np.asarray(f["mask"], bool)]).max() == 0.0 and np.abs(P.numpy()[:, np.asarray(c["mask"], bool)]).max() == 0.0


def test_restated_vcycle_is_symmetric_positive_definite():
    H = hierarchy()
    n = H["data"][0]["diag"].size
    assert n == 2916
    I = torch.eye(n, dtype=torch.float64)
    M = np.stack([R.vcycle(H["levels"], H["Ps"], I[i]).numpy() for i in range(n)], axis=1)
    norm = np.linalg.norm(M, 2)
    asym = np.abs(M - M.T).max() / norm
    lam = np.linalg.eigvalsh(0.5 * (M + M.T))
    print(f"restated M^-1: |M - M^T|_max / |M|_2 = {asym:.2e}, eigenvalues in [{lam[0]:.3e}, {lam[-1]:.3e}]")
    assert asym <= 1e-12
    assert lam[0] > 0.0


def test_restated_pmg_pcg_takes_fewer_iterations_than_jacobi():
    H = hierarchy()
    d = H["data"][0]
    b, n = torch.as_tensor(d["rhs"]), d["diag"].size
    xj, xm = torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    rj = solve.cg(d["apply"], b, xj, d["minv"], tol=1e-10, residual_scaling="rhs")
    rm = R.pcg(H["levels"], H["Ps"], b, xm, tol=1e-10, residual_scaling="rhs")
    print(f"outer iterations to 1e-10 on 2^3, order 4: Jacobi {rj.num_iters}, p-multigrid 4 -> 2 -> 1 {rm.num_iters}")
    print(f"|x_pmg - x_jacobi| / |x_jacobi| = {(xm - xj).norm().item() / xj.norm().item():.2e}")
    assert rj.converged and rm.converged
    assert rm.num_iters < rj.num_iters


def test_match_elements_pairs_by_vertices():
    fine, coarse = system.CubePartition(3, 4, perturb=0.1), system.CubePartition(3, 2, perturb=0.1)
    m = system.match_elements(fine, coarse)
    m = np.arange(fine.n_elems) if m is None else m
    assert np.array_equal(np.sort(m), np.arange(fine.n_elems)) and np.array_equal(fine.elem_verts, coarse.elem_verts[m])
    assert system.match_elements(fine, fine) is None
    perm = np.random.default_rng(3).permutation(coarse.n_elems)
    coarse.elem_verts, coarse.elem_nodes = coarse.elem_verts[perm], coarse.elem_nodes[perm]
    m2 = system.match_elements(fine, coarse)
    assert np.array_equal(fine.elem_verts, coarse.elem_verts[m2])
    with pytest.raises(system.L3KError, match="no coarse element"):
        system.match_elements(fine, system.CubePartition(3, 2, perturb=0.05))


def test_new_entry_points_fail_loudly_without_a_device():
    lib = capi.load()
    out, info, res = C.c_void_p(), capi.PmgInfo(), capi.CgResult()
    calls = {
        "l3k_pmg_create": lambda: lib.l3k_pmg_create(None, 2, None, C.byref(out)),
        "l3k_pmg_info_get": lambda: lib.l3k_pmg_info_get(None, C.byref(info)),
        "l3k_pmg_prolong": lambda: lib.l3k_pmg_prolong(None, 1, None, None, 0),
        "l3k_pmg_restrict": lambda: lib.l3k_pmg_restrict(None, 1, None, None),
        "l3k_pmg_apply": lambda: lib.l3k_pmg_apply(None, None, None),
        "l3k_pcg_solve_pmg": lambda: lib.l3k_pcg_solve_pmg(None, None, None, None, None, C.byref(res)),
    }
    for name, call in calls.items():
        assert call() == -1, name
        assert lib.l3k_last_error().decode().startswith(f"{name}: null argument"), name
    assert out.value is None and lib.l3k_pmg_destroy(None) == 0


def test_interp_table_under_asan_and_ubsan(tmp_path):
    """the generator of the table in a stand-alone program of its own (nothing is loaded into Python under a sanitizer)"""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "interp_driver")
    build = subprocess.run([cxx, "-std=c++20", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-Il3ster_amd/csrc", "tests/sanitize/interp_driver.cpp",
                            "l3ster_amd/csrc/host/tables.cpp", "-o", exe], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout + r.stderr[-4000:]
    assert "interp driver: ok" in r.stdout
    for word in ("ERROR: AddressSanitizer", "runtime error:", "ERROR: LeakSanitizer"):
        assert word not in r.stderr, r.stderr[-4000:]
