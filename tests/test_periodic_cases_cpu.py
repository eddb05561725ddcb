"""The designed inputs of periodic_cases.py without a device: every case satisfies the exactness condition and the property it was
designed for, the all-pairs restatement gives the answer worked out on paper, and the stand-alone host walk of the matcher's
per-item functions (tests/cpp/periodic_walk.cpp over device/periodic.hpp and host/periodic.cpp) gives the same answer -- built
with plain flags, with the math flags of the library's device units, and with the host sanitizers.  The inputs from which no grid
can be made end with the library's refusal, not at a time limit."""
import concurrent.futures as cf
import os
import shutil
import subprocess

import numpy as np
import pytest

import periodic_cases as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "l3ster_amd", "csrc")
MATH = ["-ffp-contract=fast", "-fno-signed-zeros", "-ffinite-math-only", "-fno-math-errno"]  # l3ster_amd/build.py: DEVICE
SANITIZE = ["-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
BUILDS = {"plain": ([], []), "math": (MATH, []), "sanitized": (SANITIZE, SANITIZE)}  # flags of the walk, of the host units


def build_walk(out, walk_flags, host_flags):
    """tests/cpp/periodic_walk.cpp with the host units it calls, which keep the flags the library gives them (the finiteness
    checks of host/periodic.cpp must not be folded)"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    common = [hipcc, "-std=c++20", "-O1", "--offload-arch=gfx950", f"-I{ROOT}/include", f"-I{CSRC}"]
    objs = []
    for src, flags in (("tests/cpp/periodic_walk.cpp", walk_flags), ("l3ster_amd/csrc/host/periodic.cpp", host_flags),
                       ("l3ster_amd/csrc/host/tables.cpp", host_flags)):
        objs.append(f"{out}.{os.path.basename(src)}.o")
        r = subprocess.run(common + flags + ["-c", os.path.join(ROOT, src), "-o", objs[-1]], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([hipcc, "--offload-arch=gfx950"] + host_flags + objs + ["-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


@pytest.fixture(scope="module")
def walks(tmp_path_factory):
    where = tmp_path_factory.mktemp("periodic_walk")
    with cf.ThreadPoolExecutor(max_workers=len(BUILDS)) as ex:
        futures = {name: ex.submit(build_walk, str(where / f"periodic_walk_{name}"), *flags) for name, flags in BUILDS.items()}
        return {name: f.result() for name, f in futures.items()}, where


def run_walk(exe, case, where):
    path = str(where / f"{case.name}.case")
    if not os.path.exists(path):
        P.write_case(case, path)
    return subprocess.run([exe, path], capture_output=True, text=True, timeout=5)  # (a hang must fail, not stall the suite)


def walk_result(r):
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    lines = r.stdout.split("\n")
    n_pairs, n_unmatched, n_ambiguous, first = (int(v) for v in lines[0].split())
    pairs = np.array([[int(v) for v in line.split()] for line in lines[1:1 + n_pairs]], dtype=np.uint32).reshape(-1, 2)
    assert pairs.shape[0] == n_pairs
    return pairs[:, 0], pairs[:, 1], n_unmatched, n_ambiguous, first


@pytest.mark.parametrize("case", P.CASES, ids=repr)
def test_case_is_exact_and_as_designed(case):
    exact = P.check_exact(case)  # lattice, bounds, and the match in integers == the brute force
    if case.design is not None:
        case.design(case)
    if case.expect is not None:
        assert P.same_result(P.as_result(*case.expect), exact), (case.expect[1:], exact[2:])
    assert np.all(np.diff(exact[0].astype(np.int64)) > 0)


def test_cases_cover_what_they_are_listed_for():
    names = [c.name for c in P.CASES]
    for dim in (2, 3):
        for prefix, count in (("1-neighbour-cells", 1 + 2 * dim), ("2-out-of-reach", 1), ("2-beyond-int64", 2), ("3-strict-tolerance", 1),
                              ("4-ties", 2), ("5-lowest-slot", 2), ("6a-", 1), ("6b-", 1), ("6c-", 1), ("6d-", 1), ("6e-", dim),
                              ("7-ids", 1), ("8-volume", 3)):
            assert sum(n.startswith(prefix) and (n.endswith(f"-{dim}d") or f"-{dim}d-" in n) for n in names) == count, (prefix, dim)
    assert sum(n.startswith("6f-") for n in names) == 3
    for a, b in P.SAME_ANSWER:  # the third entries are ignored in 2-D
        assert P.by_name(a).z_fill != 0.0 and P.by_name(a).translation[2] == 1e300 and P.by_name(b).z_fill == 0.0
        assert P.same_result(P.reference(P.by_name(a)), P.reference(P.by_name(b)))
    mesh = P.build_mesh(P.by_name("6f-nan-z-2d"))
    assert np.isnan(mesh.elem_verts[:, :, 2]).all() and np.isfinite(mesh.elem_verts[:, :, :2]).all()
    for case in P.CASES:  # every local side is listed where there are sides enough, and the other side's ids are listed nowhere
        mesh = P.build_mesh(case)
        listed = {i for i, _ in case.src + case.dst}
        for elem, side in (mesh.src, mesh.dst):
            assert set(side.tolist()) == set(range(min(2 * case.dim, side.size)))
        assert np.unique(mesh.elem_nodes[~np.isin(mesh.elem_nodes, list(listed))]).size == mesh.elem_nodes.size // 2


@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("case", P.CASES, ids=repr)
def test_walk_equals_brute_force(walks, case, build):
    exes, where = walks
    got = walk_result(run_walk(exes[build], case, where))
    want = P.reference(case)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), case
    assert got[2:] == tuple(int(v) for v in want[2:]), (got[2:], want[2:])


@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("case,word", P.refused_inputs(), ids=repr)
def test_walk_refuses_what_gives_no_grid(walks, case, word, build):
    exes, where = walks
    r = run_walk(exes[build], case, where)  # before the refusal the box from -1e308 to 1e308 ran into the time limit here
    assert r.returncode == 2 and r.stdout == "", (r.returncode, r.stdout[:200], r.stderr[-2000:])
    assert r.stderr.startswith("l3k_periodic_match: ") and word in r.stderr, r.stderr
