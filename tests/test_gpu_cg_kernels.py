"""The vector kernels of the Jacobi-PCG (l3k_cg_init, l3k_cg_dot_pap, l3k_cg_update_z, l3k_cg_update_px, l3k_jacobi_inverse;
api_solver.hip) and the row kernels of the halo exchange and of setValues (l3k_pack_rows, l3k_unpack_add_rows,
l3k_average_values), each alone on raw device vectors against the CPU restatements of tests/cg_ref.py -- at the sizes where
their grid-stride loops and the second reduction stage take a second trip.  A solve corrects a slightly wrong dot product
or beta by itself and still converges; these comparisons do not.

Tolerances (none is taken from what the kernels return):
  element-wise   each output is at most three roundings of one expression of two terms, and the compiler may contract
                 a - b * c into one FMA: |got - ref| <= 4 eps (|term_1| + |term_2|), the terms of that entry's formula.
  sums           the documented algorithm: per thread sequential over its ceil(n / (256 g)) entries, a tree of 256 (depth 8),
                 then the g block sums the same way (ceil(g / 256) sequential, depth 8), g = min(ceil(n / 256), 1024).  Each
                 addition costs one rounding (u = eps / 2) of a partial sum bounded by sum |terms|, each term carries at most
                 4 roundings of its own (r_i, z_i, the product): |got - ref| <= k eps sum |terms| with
                 k = ceil(n / (256 g)) + 8 + ceil(g / 256) + 8 + 2.
  everything else (placement probes, jacobi inverse, pack / unpack / average, frozen rows, slots) bit for bit.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import cg_ref as R
from l3ster_amd import capi, system

pytestmark = pytest.mark.gpu

CG_THREADS = 256  # api_solver.hip: cg_threads, the block of every PCG vector kernel and of the finish kernel
CG_BLOCKS = 1024  # objects.hpp: l3k_cg_blocks, the cap of cgGrid
ROW_BLOCKS = 8192  # objects.hpp: gridFor's cap (blocks of 256 threads)
ONE_GRID = CG_THREADS * CG_BLOCKS  # 262 144 entries: what one trip of the grid-stride loop covers
ROW_GRID = CG_THREADS * ROW_BLOCKS  # 2 097 152

SIZES = {
    "empty": 0,
    "one-entry": 1,
    "block-minus-1": CG_THREADS - 1,
    "one-block": CG_THREADS,
    "block-plus-1": CG_THREADS + 1,
    "finish-256-partials": CG_THREADS * CG_THREADS,  # 65 536: the finish kernel's loop once
    "finish-257-partials": CG_THREADS * CG_THREADS + 1,  # 65 537: its second pass
    "grid-once": ONE_GRID,
    "grid-twice": ONE_GRID + 1,
    "three-trips-ragged": 3 * ONE_GRID + 77,
}
assert max(SIZES.values()) > 256 * 1024  # a cap raised later must not silently empty the several-trips cases
assert [SIZES[k] for k in SIZES] == [0, 1, 255, 256, 257, 65536, 65537, 262144, 262145, 3 * 262144 + 77]
SIZE_PARAMS = [pytest.param(n, id=f"{name}-n{n}") for name, n in SIZES.items()]
ROW_SIZES = [1, CG_THREADS + 1, ROW_GRID, 2 * ROW_GRID + 13]
assert ROW_SIZES == [1, 257, 2097152, 2 * 2097152 + 13]

SENTINELS = np.array([101.5, -102.25, 103.125, -104.5, 105.75, -106.375, 107.625, -108.875])
PAD = np.array([777.25, -778.5, 779.75])  # behind every vector: must survive every call


def probe_positions(n):
    fixed = [0, CG_THREADS - 1, CG_THREADS, n - 1, CG_THREADS * CG_THREADS - 1, CG_THREADS * CG_THREADS, ONE_GRID - 1, ONE_GRID,
             2 * ONE_GRID - 1, 2 * ONE_GRID]
    return sorted({i for i in fixed if 0 <= i < n})


PLACEMENT_PARAMS = [pytest.param(n, i, id=f"{name}-n{n}-i{i}") for name, n in SIZES.items() for i in probe_positions(n)]


def sum_depth(n):
    g = min(max(-(-n // CG_THREADS), 1), CG_BLOCKS)
    return -(-n // (CG_THREADS * g)) + 8 + -(-g // CG_THREADS) + 8 + 2


@pytest.fixture(scope="module")
def ctx():
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return system.Context(0, torch.cuda.current_stream().cuda_stream)


def vp(t):
    return C.c_void_p(t.data_ptr())


def dev(a):
    """the vector on the device, followed by the padding (so that an empty vector still has a valid address)"""
    return torch.as_tensor(np.concatenate([np.asarray(a, dtype=np.float64), PAD]), device="cuda")


def host(t, n):
    a = t.cpu().numpy()
    assert np.array_equal(a[n:].view(np.uint64), PAD.view(np.uint64)), "the entries behind the vector were written"
    return a[:n]


def scalars(values=SENTINELS):
    return torch.as_tensor(np.asarray(values, dtype=np.float64).copy(), device="cuda")


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def same_values(a, b):
    """equal entry by entry, the sign of a zero aside (the library is built with -fno-signed-zeros); no NaN passes"""
    return np.array_equal(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64))


def cg_init(ctx, r, b, p, minv, n, s):
    capi.check(capi.load().l3k_cg_init(ctx._h, vp(r), vp(b), vp(p), C.c_void_p(0) if minv is None else vp(minv), n, vp(s)))


def cg_dot_pap(ctx, p, ap, n, s):
    capi.check(capi.load().l3k_cg_dot_pap(ctx._h, vp(p), vp(ap), n, vp(s)))


def cg_update_z(ctx, z, ap, minv, n, s):
    capi.check(capi.load().l3k_cg_update_z(ctx._h, vp(z), vp(ap), C.c_void_p(0) if minv is None else vp(minv), n, vp(s)))


def cg_update_px(ctx, p, x, z, n, s):
    capi.check(capi.load().l3k_cg_update_px(ctx._h, vp(p), vp(x), vp(z), n, vp(s)))


def close_entries(got, ref, terms):
    got = np.asarray(got, dtype=np.float64).astype(R.LD)
    return bool(np.all(np.abs(got - ref) <= 4 * R.EPS * terms))


def close_sum(got, ref, abs_sum, n):
    return abs(R.LD(got) - R.LD(ref)) <= sum_depth(n) * R.EPS * R.LD(abs_sum)


def nonzero24(rng, n):
    m = R.rand24(rng, n)
    m[m == 0.0] = 1.0
    return m


# ---------------------------------------------------------------------------------------------------- placement
@pytest.mark.parametrize("n,i", PLACEMENT_PARAMS)
def test_every_entry_is_counted_once(ctx, n, i):
    """One-hot probes at the block, finish-kernel and trip boundaries: an entry dropped or counted twice changes the result
    in its leading bits, an entry counted once gives it back bit for bit (the other terms are exact zeros)."""
    rng = np.random.default_rng(1000 + i)
    v = R.rand24(rng, n)
    if v[i] == 0.0:
        v[i] = 1.25
    hot = np.zeros(n)
    hot[i] = 1.0
    # <u, v> = v[i]
    s = scalars()
    cg_dot_pap(ctx, dev(hot), dev(v), n, s)
    assert same_bits(s.cpu().numpy()[1], v[i])
    s = scalars()
    cg_dot_pap(ctx, dev(v), dev(hot), n, s)
    assert same_bits(s.cpu().numpy()[1], v[i])
    # all ones: every entry counts (n < 2^53: the sum of ones is exact in any order)
    s = scalars()
    cg_dot_pap(ctx, dev(np.ones(n)), dev(np.ones(n)), n, s)
    assert s.cpu().numpy()[1] == float(n)
    # init: b one-hot, A x0 = 0, no preconditioner: z = p = b, <r, z> = <r, r> = b[i]^2 (exact: 24-bit b[i])
    b = hot * v[i]
    r, p, s = dev(np.zeros(n)), dev(np.full(n, 5.0)), scalars()
    cg_init(ctx, r, dev(b), p, None, n, s)
    h = s.cpu().numpy()
    assert same_bits(h[2], v[i] * v[i]) and same_bits(h[3], v[i] * v[i]) and same_bits(h[0], h[2])
    assert same_values(host(r, n), b) and same_values(host(p, n), b)
    # update_z: z and Ap one-hot, alpha = 1/2: z[i] = c - d / 2 (exact), both sums its square
    c, d = 3.0 + (i % 7), 0.5 + (i % 5)
    z, s = dev(hot * c), scalars([1.0, 2.0, *SENTINELS[2:]])
    cg_update_z(ctx, z, dev(hot * d), None, n, s)
    h = s.cpu().numpy()
    assert same_values(host(z, n), hot * (c - d / 2))
    assert same_bits(h[2], (c - d / 2) ** 2) and same_bits(h[3], (c - d / 2) ** 2)
    # update_px: p one-hot, alpha = 1/2, beta = 2: x[i] += e / 2, p[i] = z[i] + 2 e; nothing else moves
    e = 1.0 + (i % 3)
    x0, z0 = R.rand24(rng, n), R.rand24(rng, n)
    x0[i], z0[i] = 0.75, -0.5
    p, x, s = dev(hot * e), dev(x0), scalars([1.0, 2.0, 2.0, *SENTINELS[3:]])
    cg_update_px(ctx, p, x, dev(z0), n, s)
    want_x, want_p = x0.copy(), z0.copy()
    want_x[i], want_p[i] = 0.75 + e / 2, -0.5 + 2 * e
    assert same_bits(host(x, n), want_x) and same_bits(host(p, n), want_p)


# ---------------------------------------------------------------------------------------------------- values
@pytest.mark.parametrize("n", SIZE_PARAMS)
def test_dot_pap_values(ctx, n):
    rng = np.random.default_rng(n + 1)
    u, v = R.rand24(rng, n), R.rand24(rng, n, 3.0)
    want, abs_sum = R.dot_exact(u, v)
    du, dv, s = dev(u), dev(v), scalars()
    cg_dot_pap(ctx, du, dv, n, s)
    got = s.cpu().numpy()
    print(f"dot_pap n={n}: got {got[1]!r} exact {want!r} |err| {abs(got[1] - want):.3e} bound {sum_depth(n) * R.EPS * abs_sum:.3e}")
    assert close_sum(got[1], want, abs_sum, n)
    assert same_bits(got[[0, 2, 3, 4, 5, 6, 7]], SENTINELS[[0, 2, 3, 4, 5, 6, 7]])  # slot 1 alone
    assert same_bits(host(du, n), u) and same_bits(host(dv, n), v)
    # the same call again: the same bits (fixed summation order)
    s2 = scalars()
    cg_dot_pap(ctx, du, dv, n, s2)
    assert same_bits(s2.cpu().numpy(), got)
    if n == 0:
        assert got[1] == 0.0


@pytest.mark.parametrize("n", SIZE_PARAMS)
def test_init_values(ctx, n):
    rng = np.random.default_rng(n + 2)
    ax0, b, minv = R.rand24(rng, n), R.rand24(rng, n, 2.0), nonzero24(rng, n)
    ref = R.cg_init_ref(ax0, b, minv)
    r, db, p, dm, s = dev(ax0), dev(b), dev(np.full(n, 9.0)), dev(minv), scalars()
    cg_init(ctx, r, db, p, dm, n, s)
    got, z = s.cpu().numpy(), host(r, n)
    print(f"init n={n}: rz {got[2]!r} ref {float(ref['rz'])!r}; rr {got[3]!r} ref {float(ref['rr'])!r}; bound factor {sum_depth(n)}")
    assert close_entries(z, ref["z"], ref["terms"])
    assert same_bits(host(p, n), z)  # p = z, the same value stored twice
    assert close_sum(got[2], ref["rz"], ref["abs_rz"], n) and close_sum(got[3], ref["rr"], ref["abs_rr"], n)
    # slots: 2 and 3 written, 0 <- 2, the others keep their bits
    assert same_bits(got[0], got[2]) and same_bits(got[[1, 4, 5, 6, 7]], SENTINELS[[1, 4, 5, 6, 7]])
    assert same_bits(host(db, n), b) and same_bits(host(dm, n), minv)
    if n == 0:
        assert got[2] == 0.0 and got[3] == 0.0
    else:
        assert got[3] > 0 and not same_bits(got[2], SENTINELS[2])
    # reproducible
    r2, p2, s2 = dev(ax0), dev(np.full(n, 9.0)), scalars()
    cg_init(ctx, r2, db, p2, dm, n, s2)
    assert same_bits(s2.cpu().numpy(), got) and same_bits(host(r2, n), z)


@pytest.mark.parametrize("n", SIZE_PARAMS)
def test_update_z_values(ctx, n):
    rng = np.random.default_rng(n + 3)
    z0, ap, minv = R.rand24(rng, n), R.rand24(rng, n, 2.0), nonzero24(rng, n)
    s_in = SENTINELS.copy()
    s_in[0], s_in[1] = 0.8125, 2.71875  # <r, z> and <p, A p> of a step: alpha = s[0] / s[1] is not a dyadic number
    ref = R.cg_update_z_ref(z0, ap, minv, s_in[0], s_in[1])
    z, dap, dm, s = dev(z0), dev(ap), dev(minv), scalars(s_in)
    cg_update_z(ctx, z, dap, dm, n, s)
    got, zh = s.cpu().numpy(), host(z, n)
    assert close_entries(zh, ref["z"], ref["terms"])
    # the sums of the z the device wrote (checked entry by entry above): the sum check stands alone
    rz, rr, abs_rz, abs_rr = R.residual_sums_ref(zh, minv)
    print(f"update_z n={n}: rz {got[2]!r} ref {float(rz)!r}; rr {got[3]!r} ref {float(rr)!r}; bound factor {sum_depth(n)}")
    assert close_sum(got[2], rz, abs_rz, n) and close_sum(got[3], rr, abs_rr, n)
    assert same_bits(got[[0, 1, 4, 5, 6, 7]], s_in[[0, 1, 4, 5, 6, 7]])  # slots 2 and 3 alone
    assert same_bits(host(dap, n), ap) and same_bits(host(dm, n), minv)
    if n == 0:
        assert got[2] == 0.0 and got[3] == 0.0
    else:
        assert got[3] > 0 and not same_bits(got[2], SENTINELS[2])
    z2, s2 = dev(z0), scalars(s_in)
    cg_update_z(ctx, z2, dap, dm, n, s2)
    assert same_bits(s2.cpu().numpy(), got) and same_bits(host(z2, n), zh)


@pytest.mark.parametrize("n", SIZE_PARAMS)
def test_update_px_values(ctx, n):
    rng = np.random.default_rng(n + 4)
    p0, x0, z0 = R.rand24(rng, n), R.rand24(rng, n, 4.0), R.rand24(rng, n, 0.5)
    s_in = SENTINELS.copy()
    s_in[0], s_in[1], s_in[2] = 0.8125, 2.71875, 0.3046875  # alpha = s[0] / s[1] = 0.2988..., beta = s[2] / s[0] = 0.375
    ref = R.cg_update_px_ref(p0, x0, z0, s_in[0], s_in[1], s_in[2])
    assert ref["alpha"] != ref["beta"] and ref["beta"] != s_in[2] / s_in[1]
    p, x, z, s = dev(p0), dev(x0), dev(z0), scalars(s_in)
    cg_update_px(ctx, p, x, z, n, s)
    got = s.cpu().numpy()
    assert close_entries(host(x, n), ref["x"], ref["terms_x"])
    assert close_entries(host(p, n), ref["p"], ref["terms_p"])
    assert same_bits(host(z, n), z0)
    # s[0] <- old s[2]; every other slot keeps its bits (slot 4 included: no scratch slot)
    assert same_bits(got[0], s_in[2]) and same_bits(got[1:], s_in[1:])


# ---------------------------------------------------------------------------------------------------- frozen rows, no preconditioner
@pytest.mark.parametrize("frozen", ["a-tenth", "all"])
@pytest.mark.parametrize("n", SIZE_PARAMS)
def test_frozen_rows(ctx, n, frozen):
    """minv == 0 on a tenth of the rows (every tenth entry: in every block of every trip) or on all of them: z = p = 0 there, x
    keeps its bits, the rows are left out of both sums, nothing is NaN or Inf."""
    rng = np.random.default_rng(n + 5)
    ax0, b, minv, ap, x0 = R.rand24(rng, n), R.rand24(rng, n, 2.0), nonzero24(rng, n), R.rand24(rng, n), R.rand24(rng, n, 4.0)
    fr = np.arange(n) % 10 == 3 if frozen == "a-tenth" else np.ones(n, dtype=bool)
    minv[fr] = 0.0
    ref = R.cg_init_ref(ax0, b, minv)
    z, p, dm, s = dev(ax0), dev(np.full(n, 9.0)), dev(minv), scalars()
    cg_init(ctx, z, dev(b), p, dm, n, s)
    h, zh = s.cpu().numpy(), host(z, n)
    assert np.all(np.isfinite(h))
    assert np.all(zh[fr] == 0.0) and np.all(host(p, n)[fr] == 0.0)
    assert close_entries(zh, ref["z"], ref["terms"])
    assert close_sum(h[2], ref["rz"], ref["abs_rz"], n) and close_sum(h[3], ref["rr"], ref["abs_rr"], n)
    # the sums with the frozen rows in would be far away: the check above can tell
    if frozen == "a-tenth" and n >= 255:
        full = float(np.sum((b - ax0) ** 2))
        assert abs(full - float(ref["rr"])) > 1e3 * sum_depth(n) * R.EPS * full
    if frozen == "all":
        assert h[2] == 0.0 and h[3] == 0.0
    # the z pass on these vectors, with the scalars of a step
    s_in = SENTINELS.copy()
    s_in[0], s_in[1], s_in[2] = 0.8125, 2.71875, 0.3046875
    uref = R.cg_update_z_ref(zh, ap, minv, s_in[0], s_in[1])
    s = scalars(s_in)
    cg_update_z(ctx, z, dev(ap), dm, n, s)
    h, z1 = s.cpu().numpy(), host(z, n)
    assert np.all(np.isfinite(h)) and np.all(z1[fr] == 0.0)
    assert close_entries(z1, uref["z"], uref["terms"])
    rz, rr, abs_rz, abs_rr = R.residual_sums_ref(z1, minv)
    assert close_sum(h[2], rz, abs_rz, n) and close_sum(h[3], rr, abs_rr, n)
    if frozen == "all":
        assert h[2] == 0.0 and h[3] == 0.0
    # the p pass: p is 0 on the frozen rows (from init), so x does not move there
    x, s = dev(x0), scalars(s_in)
    p0 = host(p, n).copy()
    cg_update_px(ctx, p, x, z, n, s)
    xh, ph = host(x, n), host(p, n)
    assert same_bits(xh[fr], x0[fr]) and np.all(ph[fr] == 0.0)
    pref = R.cg_update_px_ref(p0, x0, z1, s_in[0], s_in[1], s_in[2])
    assert close_entries(xh, pref["x"], pref["terms_x"]) and close_entries(ph, pref["p"], pref["terms_p"])
    if n > 10 and frozen == "a-tenth":
        assert not same_bits(xh[~fr], x0[~fr])


@pytest.mark.parametrize("n", SIZE_PARAMS)
def test_null_preconditioner_is_the_identity(ctx, n):
    rng = np.random.default_rng(n + 6)
    ax0, b, ap = R.rand24(rng, n), R.rand24(rng, n, 2.0), R.rand24(rng, n)
    ones = dev(np.ones(n))
    out = []
    for minv in (None, ones):
        z, p, s = dev(ax0), dev(np.full(n, 9.0)), scalars()
        cg_init(ctx, z, dev(b), p, minv, n, s)
        first = (host(z, n).copy(), host(p, n).copy(), s.cpu().numpy())
        s = scalars([0.8125, 2.71875, *SENTINELS[2:]])
        cg_update_z(ctx, z, dev(ap), minv, n, s)
        out.append(first + (host(z, n).copy(), s.cpu().numpy()))
    for a, o in zip(*out):
        assert same_bits(a, o)
    # and it is b - A x0 itself, one subtraction
    assert same_bits(out[0][0], b - ax0)


# ---------------------------------------------------------------------------------------------------- jacobi inverse
@pytest.mark.parametrize("n", SIZE_PARAMS + [pytest.param(2 * ROW_GRID + 13, id=f"rows-two-trips-n{2 * ROW_GRID + 13}")])
@pytest.mark.parametrize("damping,threshold", [(1.0, 0.0), (0.7, 1e-3), (0.0, 0.0)])
def test_jacobi_inverse_bit_for_bit(ctx, n, damping, threshold):
    """One division per entry: the float64 quotient, bit for bit -- negative entries, |d| below the threshold, d = 0 under a
    positive threshold, damping 0."""
    rng = np.random.default_rng(n + 7)
    d = rng.standard_normal(n) * np.exp(rng.uniform(-12, 6, n))  # full 53-bit mantissas, magnitudes 1e-6 .. 1e3 and a tail below
    if n:
        d[::5] = -np.abs(d[::5])
        d[::11] = 1e-4 * rng.standard_normal(d[::11].size)  # below the threshold of the second case
    if threshold > 0 and n:
        d[::13] = 0.0  # (with threshold 0 this would be 1 / 0: the library is built with finite-math-only)
    else:
        d[d == 0.0] = 1.0
    dd, out = dev(d), dev(np.full(n, 5.0))
    capi.check(capi.load().l3k_jacobi_inverse(ctx._h, vp(dd), n, damping, threshold, vp(out)))
    got, want = host(out, n), R.jacobi_inverse_ref(d, damping, threshold)
    if damping == 0.0:  # sign(d) * 0: the sign of a zero is not promised (no-signed-zeros build)
        assert np.all(got == 0.0)
    else:
        assert np.all(np.isfinite(want)) and same_bits(got, want)
        assert n < 20 or (want < 0).any()
        assert n < 20 or threshold == 0 or (np.abs(want) == damping / threshold).any()
    assert same_bits(host(dd, n), d)


# ---------------------------------------------------------------------------------------------------- row kernels
@pytest.mark.parametrize("ncols", [1, 3])
@pytest.mark.parametrize("n", ROW_SIZES)
def test_pack_and_unpack_add_rows(ctx, n, ncols):
    """dst[i + n c] = src[idx[i] + ld c] and dst[idx[i] + ld c] += src[i + n c], bit for bit against numpy indexing; idx a
    random choice of n distinct rows out of ld = n + 5, in random order."""
    rng = np.random.default_rng(n + ncols)
    ld = n + 5
    idx = rng.permutation(ld)[:n].astype(np.int32)
    didx = torch.as_tensor(np.concatenate([idx, np.zeros(1, np.int32)]), device="cuda")
    owned = rng.standard_normal((ncols, ld))
    d_owned, buf = dev(owned.reshape(-1)), dev(np.full(ncols * n, 5.0))
    lib = capi.load()
    capi.check(lib.l3k_pack_rows(ctx._h, vp(d_owned), ld, ncols, vp(didx), n, vp(buf)))
    packed = host(buf, ncols * n).reshape(ncols, n)
    assert same_bits(packed, owned[:, idx])
    assert same_bits(host(d_owned, ncols * ld), owned.reshape(-1))
    # unpack-add of other values into a matrix of the same shape
    recv = rng.standard_normal((ncols, n))
    d_recv = dev(recv.reshape(-1))
    capi.check(lib.l3k_unpack_add_rows(ctx._h, vp(d_recv), n, vp(didx), vp(d_owned), ld, ncols))
    want = owned.copy()
    want[:, idx] += recv
    got = host(d_owned, ncols * ld).reshape(ncols, ld)
    assert same_bits(got, want)
    rest = np.setdiff1d(np.arange(ld), idx)
    assert rest.size == 5 and same_bits(got[:, rest], owned[:, rest])  # rows that are not listed keep their bits
    assert same_bits(host(d_recv, ncols * n), recv.reshape(-1))


@pytest.mark.parametrize("n", ROW_SIZES)
def test_average_values(ctx, n):
    rng = np.random.default_rng(n + 9)
    total, count = rng.standard_normal(n), rng.integers(0, 4, n).astype(np.float64)
    if n > 1:
        count[0], count[-1] = 0.0, 3.0
    before = rng.standard_normal(n)
    ds, dc, dv = dev(total), dev(count), dev(before)
    capi.check(capi.load().l3k_average_values(ctx._h, vp(ds), vp(dc), n, vp(dv)))
    got = host(dv, n)
    want = before.copy()
    want[count > 0] = total[count > 0] / count[count > 0]
    assert same_bits(got, want)
    assert n < 20 or ((count == 0).any() and same_bits(got[count == 0], before[count == 0]))
    assert same_bits(host(ds, n), total) and same_bits(host(dc, n), count)


# ---------------------------------------------------------------------------------------------------- the protocol as a whole
@pytest.mark.parametrize("n", SIZE_PARAMS)
def test_one_iteration_through_the_pieces_against_the_dense_recurrence(ctx, n):
    """init, dot_pap, update_z, update_px chained as a host does (A = a diagonal matrix, so that A p is one product per entry
    on the CPU): the scalars each call leaves and x after the step equal those of cg_ref.pcg_ref's formulas."""
    if n == 0:
        s = scalars()
        one = dev(np.zeros(0))
        cg_init(ctx, one, one, one, None, 0, s)
        cg_dot_pap(ctx, one, one, 0, s)
        h = s.cpu().numpy()
        assert np.all(h[:4] == 0.0) and same_bits(h[4:], SENTINELS[4:])
        return
    rng = np.random.default_rng(n + 10)
    a = np.abs(R.rand24(rng, n)) + 0.5  # the diagonal of A
    b, x0 = R.rand24(rng, n), R.rand24(rng, n)
    minv = R.jacobi_inverse_ref(a).astype(np.float32).astype(np.float64)
    z, p, x, dm, s = dev(a * x0), dev(np.zeros(n)), dev(x0), dev(minv), scalars()
    cg_init(ctx, z, dev(b), p, dm, n, s)
    ph = host(p, n)
    ap = a * ph  # (one rounding per entry: the operator's own arithmetic is not under test here)
    dap = dev(ap)
    cg_dot_pap(ctx, p, dap, n, s)
    h1 = s.cpu().numpy()
    cg_update_z(ctx, z, dap, dm, n, s)
    h2 = s.cpu().numpy()
    cg_update_px(ctx, p, x, z, n, s)
    h3 = s.cpu().numpy()
    LD = R.LD
    r0 = b.astype(LD) - (a * x0).astype(LD)
    rz0, pap = R._sum(r0 * minv * r0), R._sum(ph.astype(LD) * ap.astype(LD))
    k = sum_depth(n)
    assert abs(LD(h1[0]) - rz0) <= k * R.EPS * rz0 and abs(LD(h1[1]) - pap) <= k * R.EPS * pap
    alpha = np.float64(h1[0]) / np.float64(h1[1])
    x_ref = x0.astype(LD) + LD(alpha) * ph.astype(LD)
    assert close_entries(host(x, n), x_ref, np.abs(x0) + np.abs(alpha * ph))
    assert same_bits(h2[[0, 1]], h1[[0, 1]]) and same_bits(h3[0], h2[2]) and same_bits(h3[1:], h2[1:])
    assert same_bits(h3[4:], SENTINELS[4:])
    # a step of CG on an SPD system lowers the energy norm of the error: <r, r> may go either way, <r, z> > 0 stays
    assert h2[2] > 0 and h2[3] > 0
