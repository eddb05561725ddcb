"""The orthogonalisation kernels of GMRES one by one (l3k_gmres_multi_dot, l3k_gmres_project, l3k_gmres_combine; device/gmres.hpp)
against numpy in longdouble.

Sizes: n in {1, 255, 257, 4099, 262144 + 3} -- below, at and above one workgroup of 256 rows, a ragged last workgroup, and one past
the grid of 1024 x 256 threads, where threads stride; k in {1, 2, 7, 8, 9, 31, 33} around the chunk of 8 columns and its ragged
last chunk.  ld = n rounded up to 4, plus 4, with NaN in the padding: a read past n poisons the result.

Bounds (derived, not tuned; u = EPS = 2^-52 bounds the unit roundoff 2^-53 with a factor 2 to spare):
  a dot product of n terms summed in ANY order, products rounded or fused: |h - h^| <= (n + 2) EPS sum_i |v_i w_i|
  a row of w - V h, k subtractions of rounded or fused products:           |w_i - w^_i| <= (k + 2) EPS (|w_i| + sum_j |v_ij h_j|)
k in {100, 200, 255} takes the LDS row tile at 64, 32 and 16 rows (9 takes 256, 31 and 33 take 128; below 8 the registers), k in
{256, 259} the chunked sweeps above what the tile takes.
The second dot product of l3k_gmres_project is held against the longdouble dot products of the w the DEVICE stored."""
import ctypes as C

import numpy as np
import pytest
import torch

from l3ster_amd import capi, system

pytestmark = pytest.mark.gpu
LD, EPS = np.longdouble, float(np.finfo(np.float64).eps)
NS, KS = [1, 255, 257, 4099, 262144 + 3], [1, 2, 7, 8, 9, 31, 33]
_CTX, _DATA = [], {}


def ctx():
    if not _CTX:
        torch.cuda.set_device(0)
        _CTX.append(system.Context(0, torch.cuda.current_stream().cuda_stream))
    return _CTX[0]


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")


def vp(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def data(n, k):
    """V (k, ld) with NaN padding, w, h_in, y, x, a mask with every third row frozen -- and the longdouble sums on them; once"""
    if (n, k) in _DATA:
        return _DATA[n, k]
    rng = np.random.default_rng(1000 * k + n % 997)
    ld = (n + 3) // 4 * 4 + 4
    V = np.full((k, ld), np.nan)
    V[:, :n] = rng.standard_normal((k, n))
    w, h_in, y, x = rng.standard_normal(n), rng.standard_normal(k + 1), rng.standard_normal(k), rng.standard_normal(n)
    mask = np.where(np.arange(n) % 3 == 1, 0.0, rng.uniform(0.5, 2.0, n))
    d = dict(n=n, k=k, ld=ld, V=V, w=w, h_in=h_in, y=y, x=x, mask=mask, dV=dev(V), VL=V[:, :n].astype(LD))
    _DATA[n, k] = d
    return d


def dots(d, w):
    """(h, sum of |terms|) of multiDot in longdouble"""
    wl = np.asarray(w, dtype=LD)
    h = np.concatenate([d["VL"] @ wl, [wl @ wl]])
    a = np.concatenate([np.abs(d["VL"]) @ np.abs(wl), [wl @ wl]])
    return h, a


def multi_dot(d, w, mask=None):
    h = torch.full((d["k"] + 1,), float("nan"), dtype=torch.float64, device="cuda")
    capi.check(capi.load().l3k_gmres_multi_dot(ctx()._h, vp(d["dV"]), d["ld"], d["k"], vp(w), vp(mask), d["n"], vp(h)))
    return h


def project(d, w, h_in, mask=None):
    h = torch.full((d["k"] + 1,), float("nan"), dtype=torch.float64, device="cuda")
    capi.check(capi.load().l3k_gmres_project(ctx()._h, vp(d["dV"]), d["ld"], d["k"], vp(w), vp(mask), d["n"], vp(h_in), vp(h)))
    return h


def check_dots(d, h_dev, w_host, label):
    h, a = dots(d, w_host)
    err = np.abs(h_dev.cpu().numpy().astype(LD) - h)
    bound = (d["n"] + 2) * EPS * a
    worst = float(np.max(err / np.maximum(bound, LD(1e-300))))
    print(f"{label} n {d['n']} k {d['k']}: worst |h - h^| / bound = {worst:.3e}")
    assert np.isfinite(h_dev.cpu().numpy()).all() and (err <= bound).all()


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n", NS)
def test_multi_dot(n, k):
    d = data(n, k)
    w = dev(d["w"])
    h1, h2 = multi_dot(d, w), multi_dot(d, w)
    check_dots(d, h1, d["w"], "multi_dot")
    assert torch.equal(h1, h2)  # two runs: equal bits
    assert torch.equal(w, dev(d["w"]))  # (w is an input)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n", NS)
def test_project(n, k):
    d = data(n, k)
    outs, h_in = [], dev(d["h_in"])
    for _ in range(2):
        w = dev(d["w"])
        outs.append((project(d, w, h_in), w))
    (h, w), (h_b, w_b) = outs
    assert torch.equal(h, h_b) and torch.equal(w, w_b)  # two runs: equal bits
    wl, hl = d["w"].astype(LD), d["h_in"][:k].astype(LD)
    want = wl - hl @ d["VL"]
    bound = (k + 2) * EPS * (np.abs(wl) + np.abs(hl) @ np.abs(d["VL"]))
    err = np.abs(w.cpu().numpy().astype(LD) - want)
    print(f"project n {n} k {k}: worst row |w - w^| / bound = {float(np.max(err / bound)):.3e}")
    assert (err <= bound).all()
    check_dots(d, h, w.cpu().numpy(), "project")


@pytest.mark.parametrize("n,k", [(4099, 100), (300, 200), (4099, 255), (257, 256), (4099, 259)])
def test_every_tile_height_and_the_sweeps_above_the_tile(n, k):
    test_multi_dot(n, k)
    test_project(n, k)


@pytest.mark.parametrize("n,k", [(1, 1), (257, 9), (4099, 8), (262144 + 3, 33), (4099, 200), (4099, 259)])
def test_frozen_rows_and_planted_nan(n, k):
    """With a mask, w counts as 0 on the frozen rows: NaN planted there reaches no output, and the stored w is 0 there"""
    d = data(n, k)
    frozen = d["mask"] == 0
    if n == 1:  # (the one row frozen: everything is zero)
        frozen = np.array([True])
    mask = dev(np.where(frozen, 0.0, d["mask"]))
    w_host = np.where(frozen, np.nan, d["w"])
    w_zero = np.where(frozen, 0.0, d["w"])
    w_nan = dev(w_host)
    h = multi_dot(d, w_nan, mask)
    check_dots(d, h, w_zero, "multi_dot, masked")
    w = dev(w_host)
    h_in = dev(d["h_in"])
    h2 = project(d, w, h_in, mask)
    w_out = w.cpu().numpy()
    assert np.isfinite(w_out).all() and not w_out[frozen].any()
    wl, hl = w_zero.astype(LD), d["h_in"][:k].astype(LD)
    want = np.where(frozen, LD(0), wl - hl @ d["VL"])
    bound = (k + 2) * EPS * (np.abs(wl) + np.abs(hl) @ np.abs(d["VL"]))
    assert (np.abs(w_out.astype(LD) - want) <= bound).all()
    check_dots(d, h2, w_out, "project, masked")
    # -0.0 in the mask is a frozen row too (the test is on the bits)
    if n > 1:
        m2 = np.where(frozen, -0.0, d["mask"])
        m2 = dev(m2)
        assert torch.equal(multi_dot(d, w_nan, m2), h)


@pytest.mark.parametrize("n,k", [(1, 1), (255, 7), (4099, 9), (262144 + 3, 31)])
@pytest.mark.parametrize("with_minv", [False, True])
def test_combine(n, k, with_minv):
    """x += [minv (.)] sum_j y_j v_j; a row with minv == 0 keeps the bits of x, -0.0 included"""
    d = data(n, k)
    x0 = d["x"].copy()
    x0[::5] = -0.0
    minv = d["mask"] if with_minv else None
    xs, y, mv = [], dev(d["y"]), None if minv is None else dev(minv)
    for _ in range(2):
        x = dev(x0)
        capi.check(capi.load().l3k_gmres_combine(ctx()._h, vp(d["dV"]), d["ld"], k, vp(y), vp(mv), n, vp(x)))
        xs.append(x)
    assert torch.equal(xs[0], xs[1])
    got = xs[0].cpu().numpy()
    yl, ml = d["y"].astype(LD), (np.ones(n) if minv is None else minv).astype(LD)
    want = x0.astype(LD) + ml * (yl @ d["VL"])
    bound = (k + 3) * EPS * (np.abs(x0) + np.abs(ml) * (np.abs(yl) @ np.abs(d["VL"])))
    assert (np.abs(got.astype(LD) - want) <= bound).all()
    if with_minv:
        frozen = minv == 0
        assert np.array_equal(got[frozen].view(np.int64), x0[frozen].view(np.int64))


def test_refusals_of_the_pieces():
    d, lib = data(255, 7), capi.load()
    w, h = dev(d["w"]), torch.zeros(8, dtype=torch.float64, device="cuda")

    def refused(rc, text):
        assert rc == -1 and text in lib.l3k_last_error().decode(), lib.l3k_last_error().decode()

    refused(lib.l3k_gmres_multi_dot(ctx()._h, vp(d["dV"]), d["ld"], 0, vp(w), None, 255, vp(h)), "l3k_gmres_multi_dot: k = 0")
    refused(lib.l3k_gmres_multi_dot(ctx()._h, vp(d["dV"]), d["ld"] + 2, 7, vp(w), None, 255, vp(h)), "must be a multiple of 4")
    refused(lib.l3k_gmres_multi_dot(ctx()._h, vp(d["dV"]), 252, 7, vp(w), None, 255, vp(h)), "at least n = 255")
    refused(lib.l3k_gmres_multi_dot(ctx()._h, vp(d["dV"]), d["ld"], 7, None, None, 255, vp(h)), "l3k_gmres_multi_dot: null argument")
    refused(lib.l3k_gmres_project(ctx()._h, vp(d["dV"]), d["ld"], 0, vp(w), None, 255, vp(h), vp(h)), "l3k_gmres_project: k = 0")
    refused(lib.l3k_gmres_project(ctx()._h, vp(d["dV"]), d["ld"] + 1, 7, vp(w), None, 255, vp(h), vp(h)), "must be a multiple of 4")
    refused(lib.l3k_gmres_project(ctx()._h, vp(d["dV"]), d["ld"], 7, vp(w), None, 255, None, vp(h)), "l3k_gmres_project: null argument")
    refused(lib.l3k_gmres_combine(ctx()._h, vp(d["dV"]), d["ld"], 0, vp(h), None, 255, vp(w)), "l3k_gmres_combine: k = 0")
    refused(lib.l3k_gmres_combine(ctx()._h, vp(d["dV"]), d["ld"] + 3, 7, vp(h), None, 255, vp(w)), "must be a multiple of 4")
    assert torch.equal(w, dev(d["w"])) and not h.any()
