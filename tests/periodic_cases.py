"""Designed inputs for the periodic node matcher (l3k_periodic_match): point sets on a lattice, packed into order-1 meshes of
flat elements, each built so that one branch of the matcher decides the answer.  numpy only.

A case is two lists of (node id, point), source and destination, a translation and a tolerance.  `build_mesh` packs the points
2^(dim-1) at a time onto one side of an element of their own (the side number cycles over all 2 dim sides, the last element is
padded with its last entry), gives the opposite side the same coordinates and ids that are listed nowhere, and returns what
system.periodic_match and periodic_ref.brute_force_match take.  The matcher reads vertices and ids only; with flat elements the
box of the destination vertices is exactly the box of the designed destination points, and at order 1 the GLL weights are 0 and
1, so a node's location is its vertex bit for bit.

Exactness.  Every coordinate, translation and tolerance is an integer multiple of 2^-12 (a lattice unit), coordinates are below
2^42 units, tolerances at most 2^19 units.  Then for every (source image, destination node) either all coordinate differences
are below 2^20 units -- the image, the differences, their squares and the sum of the squares are exact in double, in any order,
with or without FMA, two different sums differ by more than 2^-43 relative and so do their square roots: `d < tolerance`,
`d < best_d` and `d == best_d` come out the same on the device, in numpy and in integers -- or one difference is 2^20 units or
more, twice the largest tolerance, and the pair does not qualify in any arithmetic.  `check_exact` checks all of that and redoes
the match in integers.  The figures of the cases are therefore stated in lattice units below (`tol`, `h` and the points are ints).

`grid` restates the grid of the library (host/periodic.cpp: periodicMakeGrid; device/periodic.hpp: cellKey, matchNode): the box,
h, lo = box_lo - h, m and the cell of a point.  Cases that assert cell membership choose the tolerance and the box so that h is a
power of two and every cell border a lattice number: the restated cells are then exact, and each such case asserts the cell
relation it was built for in its `design`, so that it cannot silently stop exercising it.

Two figures are not the ones first proposed for these cases, because those contradict the bound of 2^42 units (2^30) on the
coordinates: the far image of "out of reach" lies at +-2^40 units (2^28), the far box of "grid regimes" at (2^29, -2^29, 2^20).
And "every neighbour cell" needs one destination node per offset vector: a partner in the cell above its image lies in the lower
half of its cell, one in the cell below in the upper half, so no single node has images in all 3^dim cells around it."""
import itertools
import math

import numpy as np

import periodic_ref as R

UNIT = 2.0 ** -12
COORD_LIMIT = 1 << 42  # lattice units
TOL_LIMIT = 1 << 19
NEAR = 1 << 20


class Case:
    """src, dst: [(node id, (x, y, z))] in listing order (a node may be listed several times, z = 0 in 2-D); expect: None or
    (pairs {src id: dst id}, n_unmatched, n_ambiguous, first_unmatched) as designed on paper; design: None or a function of the
    case that asserts what the case was built to exercise; z_fill: the z entry of every vertex in 2-D (ignored by the matcher)."""

    def __init__(self, name, dim, src, dst, t, tol, expect=None, design=None, z_fill=0.0, t_z=None):
        def points(listing):
            return [(int(i), tuple(float(v) * UNIT for v in (tuple(p) + (0,))[:3])) for i, p in listing]

        self.name, self.dim = name, dim
        self.src, self.dst = points(src), points(dst)
        self.translation = tuple(float(v) * UNIT for v in (tuple(t) + (0,))[:3])
        if t_z is not None:
            self.translation = self.translation[:2] + (t_z,)
        self.tolerance = float(tol) * UNIT
        self.expect, self.design, self.z_fill = expect, design, z_fill

    def __repr__(self):
        return self.name


class PointMesh:
    """dim, order = 1, elem_nodes uint32 [n][2^dim], elem_verts [n][2^dim][3], src / dst = (face_elem int64, face_side uint8)"""
    order = 1


_MESHES, _REFERENCES = {}, {}


def build_mesh(case):
    if case.name in _MESHES:
        return _MESHES[case.name]
    dim = case.dim
    k, nv = 2 ** (dim - 1), 2 ** dim
    sn = R.side_nodes(dim, 1)  # the slot order of a side
    used = np.array([i for i, _ in case.src + case.dst], dtype=np.int64)
    sets = []
    for listing in (case.src, case.dst):
        ids = np.array([i for i, _ in listing], dtype=np.int64)
        pts = np.array([p for _, p in listing], dtype=np.float64).reshape(-1, 3)
        pad = (-ids.size) % k
        if pad:
            ids, pts = np.concatenate([ids, np.repeat(ids[-1:], pad)]), np.concatenate([pts, np.repeat(pts[-1:], pad, axis=0)])
        sets.append((ids.reshape(-1, k), pts.reshape(-1, k, 3)))
    n_each = [s[0].shape[0] for s in sets]
    n_fresh = sum(n_each) * k
    candidates = np.arange(1 << 30, (1 << 30) + n_fresh + used.size, dtype=np.int64)
    fresh = candidates[~np.isin(candidates, used)][:n_fresh].reshape(-1, k)
    mesh = PointMesh()
    mesh.dim = dim
    mesh.elem_nodes = np.zeros((sum(n_each), nv), dtype=np.uint32)
    mesh.elem_verts = np.zeros((sum(n_each), nv, 3), dtype=np.float64)
    faces, first = [], 0
    for (ids, pts), n in zip(sets, n_each):
        elem = first + np.arange(n, dtype=np.int64)
        side = (np.arange(n) % (2 * dim)).astype(np.uint8)
        rows = elem[:, None]
        mesh.elem_nodes[rows, sn[side]] = ids
        mesh.elem_nodes[rows, sn[side ^ 1]] = fresh[first:first + n]
        mesh.elem_verts[rows, sn[side]] = pts
        mesh.elem_verts[rows, sn[side ^ 1]] = pts
        faces.append((elem, side))
        first += n
    if dim == 2:
        mesh.elem_verts[:, :, 2] = case.z_fill
    mesh.src, mesh.dst = faces
    _MESHES[case.name] = mesh
    return mesh


def reference(case):
    """periodic_ref.brute_force_match of the case, computed once"""
    if case.name not in _REFERENCES:
        mesh = build_mesh(case)
        _REFERENCES[case.name] = R.brute_force_match(mesh, mesh.src, mesh.dst, case.translation, case.tolerance)
    return _REFERENCES[case.name]


def as_result(pairs, n_unmatched, n_ambiguous, first):
    """a designed expectation in the form of brute_force_match"""
    src = sorted(pairs)
    return np.array(src, dtype=np.uint32), np.array([pairs[s] for s in src], dtype=np.uint32), n_unmatched, n_ambiguous, first


def same_result(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and tuple(int(v) for v in a[2:]) == tuple(int(v) for v in b[2:])


def write_case(case, path):
    """the binary form tests/cpp/periodic_walk.cpp reads"""
    mesh = build_mesh(case)
    with open(path, "wb") as f:
        f.write(np.array([mesh.dim, 1, mesh.elem_nodes.shape[0], mesh.src[0].size, mesh.dst[0].size], dtype=np.int64).tobytes())
        f.write(np.array(case.translation + (case.tolerance,), dtype=np.float64).tobytes())
        f.write(np.ascontiguousarray(mesh.elem_nodes, dtype=np.uint32).tobytes())
        f.write(np.ascontiguousarray(mesh.elem_verts, dtype=np.float64).tobytes())
        for elem, side in (mesh.src, mesh.dst):
            f.write(elem.astype(np.int64).tobytes())
            f.write(side.astype(np.uint8).tobytes())


# ------------------------------------------------------------------------------------------------------------------- exactness
def to_units(x):
    k = x * 4096.0
    assert math.isfinite(k) and k == math.floor(k), f"{x!r} is not on the lattice"
    return int(k)


def first_listing(listing, dim):
    """{node id: the point of its lowest slot, in lattice units}; every listed coordinate is checked"""
    out = {}
    for i, p in listing:
        u = tuple(to_units(v) for v in p[:dim])
        assert all(abs(v) < COORD_LIMIT for v in u), (i, p)
        out.setdefault(i, u)
    return out


def check_exact(case):
    """The exactness condition of the module's docstring, checked, and the match redone in integers: squared lattice distances
    against the squared tolerance.  Asserts that the result equals brute_force_match and returns it."""
    dim = case.dim
    S, D = first_listing(case.src, dim), first_listing(case.dst, dim)
    t = [to_units(v) for v in case.translation[:dim]]
    tol = to_units(case.tolerance)
    assert 0 < tol <= TOL_LIMIT
    d_ids = np.array(sorted(D), dtype=np.int64)
    d_pts = np.array([D[i] for i in d_ids.tolist()], dtype=np.int64).reshape(-1, dim)
    pairs, n_unmatched, n_ambiguous, first = {}, 0, 0, -1
    for s in sorted(S):
        img = [S[s][a] + t[a] for a in range(dim)]
        best = None
        if all(abs(v) < 2 * COORD_LIMIT for v in img) and d_ids.size:  # else 2^42 units or more from every destination node
            # below 2^43 units: the image is exact in double
            diff = np.abs(np.array(img, dtype=np.int64)[None, :] - d_pts)
            near = np.nonzero((diff < NEAR).all(axis=1))[0]  # the others are 2^20 units >= 2 tolerance away along an axis
            d2 = (diff[near] ** 2).sum(axis=1)  # < 3 * 2^40: exact in double as well
            ok = near[d2 < tol * tol]
            if ok.size:
                order = np.lexsort((d_ids[ok], d2[d2 < tol * tol]))
                best = int(d_ids[ok[order[0]]])
                n_ambiguous += ok.size > 1
        if best is None:
            first = s if n_unmatched == 0 else first
            n_unmatched += 1
        elif best != s:
            pairs[s] = best
    exact = as_result(pairs, n_unmatched, int(n_ambiguous), first)
    assert same_result(exact, reference(case)), (case, exact[2:], reference(case)[2:])
    return exact


# ------------------------------------------------------------------------------------------------------------------- the grid
class Grid:
    """periodicMakeGrid and the cell arithmetic of cellKey / matchNode, restated in numpy doubles"""

    def __init__(self, dim, box_lo, box_hi, tolerance):
        self.dim, self.box_lo, self.box_hi = dim, box_lo, box_hi
        extent = np.float64(max(0.0, float((box_hi - box_lo).max())))
        h = max(np.float64(2.0) * np.float64(tolerance), extent / np.float64(1 << 20))
        while not np.ceil(extent / h) + 3.0 < float(1 << 21):
            h *= 2.0
        self.extent, self.h, self.lo, self.inv_h, self.m = extent, h, box_lo - h, np.float64(1.0) / h, int(np.ceil(extent / h)) + 3

    def floor(self, p):
        """floor((p - lo) inv_h) per axis as a double: what matchNode tests against -1 and m"""
        return np.floor((np.asarray(p, dtype=np.float64)[:self.dim] - self.lo) * self.inv_h)

    def cell(self, p):
        return tuple(int(v) for v in self.floor(p))

    def near(self, p):
        f = self.floor(p)
        return bool(np.all((f >= -1.0) & (f <= float(self.m))))

    def keys(self, pts):
        """key of every row of pts"""
        c = np.clip(np.floor((np.asarray(pts, dtype=np.float64)[:, :self.dim] - self.lo) * self.inv_h), 0, self.m - 1).astype(np.int64)
        return sum(c[:, a] << (21 * a) for a in range(self.dim))

    def key(self, p):
        """cellKey: clamped, x in the low bits"""
        k = 0
        for a in reversed(range(self.dim)):
            k = k << 21 | min(max(self.cell(p)[a], 0), self.m - 1)
        return k


def grid(case):
    mesh = build_mesh(case)
    v = mesh.elem_verts[mesh.dst[0]][:, :, :case.dim].reshape(-1, case.dim)
    lo, hi = (v.min(axis=0), v.max(axis=0)) if v.size else (np.zeros(case.dim), np.zeros(case.dim))
    return Grid(case.dim, lo, hi, case.tolerance)


def image(case, p):
    """the translated source point, as the matcher forms it"""
    return tuple(np.float64(p[a]) + np.float64(case.translation[a]) if a < case.dim else 0.0 for a in range(3))


def src_point(case, node):
    return next(p for i, p in case.src if i == node)


def dst_point(case, node):
    return next(p for i, p in case.dst if i == node)


def add(p, q):
    return tuple(a + b for a, b in zip(p, q))


def sub(p, q):
    return tuple(a - b for a, b in zip(p, q))


# ----------------------------------------------------------------------------------------------------- 1. every neighbour cell
def neighbour_cells(dim, variant, axis=None):
    """tol 2^-3, h 2^-2 = 1024 units, box of n cells from O: cell border c lies at O + (c - 1) h.  One destination node per offset
    vector o, on the lower border of its cell where o = -1 (the first of them on a cell corner, where it belongs to the upper cell
    on every axis), a quarter into it where o = 0, one unit below its upper border where o = +1; its image 100 units below, above,
    above it: in the cell o away.  The nodes are 4 cells apart along the axis `spread`.  variant "low": along `axis` the nodes lie
    in cell 1, the lowest a destination node can lie in, so the images of o = -1 lie in cell 0; "high": the node of o = -1 lies on
    the upper face of the box, alone in cell m - 2, the others in cell m - 3, so the blocks searched touch cell m - 1.  Strays in
    cells -1, m - 1 and m of `axis` are near, search clamped blocks and find nothing.  Both corners of the box are matched as
    well: the upper one is the last entry of the sorted cell keys."""
    tol, h = 512, 1024
    offsets = list(itertools.product((-1, 0, 1), repeat=dim))
    n = 8 + 4 * len(offsets) + 4
    m = n + 3
    O = (-7000, 3000, 11000)[:dim]
    t = (-3 * 4096, 5 * 4096 + 7, -11)[:dim]
    spread = 0 if variant == "interior" else (axis + 1) % dim
    top = tuple(o + n * h for o in O)
    dst, src, images, pairs = [(90, O), (91, top)], [(290, sub(O, t)), (291, sub(top, t))], {}, {290: 90, 291: 91}
    for k, o in enumerate(offsets):
        node, img = [], []
        for b in range(dim):
            if b == spread:
                c = 5 + 4 * k
            elif b == axis:
                c = 1 if variant == "low" else (m - 2 if o[b] == -1 else m - 3)
            else:
                c = 5
            x = O[b] + (c - 1) * h + {-1: 0, 0: h // 4, 1: h - 1}[o[b]]
            node.append(x), img.append(x + (-100 if o[b] == -1 else 100))
        dst.append((100 + k, tuple(node))), src.append((200 + k, sub(img, t)))
        pairs[200 + k] = 100 + k
    strays = {}
    if variant != "interior":
        first_image = add(src[2][1], t)
        for j, c in enumerate((-1, m - 1, m)):
            p = list(first_image)
            p[axis] = O[axis] + (c - 1) * h + h // 2
            src.append((300 + j, sub(p, t)))
            strays[300 + j] = c

    def design(case):
        g = grid(case)
        assert g.h == h * UNIT and g.m == m and np.array_equal(g.lo, (np.array(O) - h) * UNIT)
        assert np.array_equal(g.floor(dst_point(case, 100)), (np.array(dst_point(case, 100)[:dim]) - g.lo) * g.inv_h)  # on a corner
        seen = set()
        for k in range(len(offsets)):
            ci, cd = g.cell(image(case, src_point(case, 200 + k))), g.cell(dst_point(case, 100 + k))
            seen.add(tuple(a - b for a, b in zip(ci, cd)))
            assert tuple(a - b for a, b in zip(ci, cd)) == offsets[k]
            if variant == "low":
                assert cd[axis] == 1 and ci[axis] == 1 + offsets[k][axis]
            if variant == "high":
                assert cd[axis] == (m - 2 if offsets[k][axis] == -1 else m - 3) and max(ci[axis], cd[axis]) + 1 <= m - 1
        assert seen == set(offsets)
        if variant == "low":
            assert min(g.cell(image(case, src_point(case, 200 + k)))[axis] for k in range(len(offsets))) == 0
        if variant == "high":
            assert max(g.cell(image(case, src_point(case, 200 + k)))[axis] for k in range(len(offsets))) == m - 2  # block: to m - 1
        for node, c in strays.items():
            p = image(case, src_point(case, node))
            assert g.cell(p)[axis] == c and g.near(p)
        keys = sorted(g.key(p) for _, p in case.dst)
        assert keys[-1] == g.key(dst_point(case, 91)) and keys[-2] < keys[-1] and keys[0] == g.key(dst_point(case, 90))

    name = f"1-neighbour-cells-{dim}d-{variant}" + ("" if axis is None else f"-axis{axis}")
    return Case(name, dim, src, dst, t, tol, expect=(pairs, len(strays), 0, 300 if strays else -1), design=design)


# -------------------------------------------------------------------------------------------------------------- 2. out of reach
def out_of_reach(dim):
    """tol 2^-3, h 1024 units, a box of 8 cells (m = 11).  Per axis and sign one image exactly 2 cells from the box (floor = -1:
    near, nothing found), one a unit further out (floor = -2: not near), one a unit inside 3 cells above it (floor = m: near) and one
    exactly 3 cells above (floor = m + 1: not near); one image at +-2^40 units.  Three matched nodes with ids below and above
    those of the strays are not affected."""
    tol, h, n = 512, 1024, 8
    m = n + 3
    O = (2048, -4096, 1024)[:dim]
    t = (9 * 4096, -2 * 4096, 77)[:dim]
    top = tuple(o + n * h for o in O)
    mid = tuple(o + 3 * h + 17 for o in O)
    dst = [(10, O), (11, top), (12, mid)]
    src = [(20, sub(O, t)), (45, sub(top, t)), (90, sub(add(mid, (30, 40, 0)[:dim]), t))]
    inside = tuple(o + 4 * h + 5 for o in O)
    floors, node = {}, 30
    for a in range(dim):
        for x, f in ((O[a] - 2 * h, -1), (O[a] - 2 * h - 1, -2), (top[a] + 3 * h - 1, m), (top[a] + 3 * h, m + 1)):
            p = list(inside)
            p[a] = x
            src.append((node, sub(p, t)))
            floors[node] = (a, f)
            node += 1
    for x in (1 << 40, -(1 << 40)):
        p = list(inside)
        p[0] = x
        src.append((node, sub(p, t)))
        floors[node] = (0, None)
        node += 1

    def design(case):
        g = grid(case)
        assert g.h == h * UNIT and g.m == m
        for s, (a, f) in floors.items():
            p = image(case, src_point(case, s))
            if f is None:
                assert abs(p[0]) == 2.0 ** 28 and not g.near(p)
            else:
                assert g.floor(p)[a] == f and g.near(p) == (f in (-1, m))
        assert any(not g.near(image(case, src_point(case, s))) for s in floors)

    return Case(f"2-out-of-reach-{dim}d", dim, src, dst, t, tol, expect=({20: 10, 45: 11, 90: 12}, len(floors), 0, 30), design=design)


def beyond_int64(dim, sign):
    """tol 2^-12 on a box of 2^8: tolerance-driven h = 2^-11, and a translation of +-2^53 along x: (p - lo) inv_h is +-2^64,
    finite, and must be refused before it is converted to an integer.  Nothing matches."""
    tol = 1
    O = (-(1 << 19), 1 << 18, 0)[:dim]
    top = tuple(o + (1 << 20) for o in O)
    t = (sign * (1 << 65), 0, 0)[:dim]
    dst = [(1, O), (2, top), (3, tuple(o + 4096 for o in O))]
    src = [(7, O), (5, top), (9, tuple(o + 4096 for o in O)), (6, tuple(o - 5 for o in O))]

    def design(case):
        g = grid(case)
        assert g.h == 2 * UNIT and g.h == 2.0 * case.tolerance > g.extent / 2.0 ** 20
        for _, p in case.src:
            f = g.floor(image(case, p))[0]
            assert np.isfinite(f) and abs(f) > 2.0 ** 63 and not g.near(image(case, p))

    return Case(f"2-beyond-int64-{dim}d-{'plus' if sign > 0 else 'minus'}", dim, src, dst, t, tol, expect=({}, 4, 0, 5), design=design)


# ---------------------------------------------------------------------------------------------------------- 3. strict tolerance
def strict_tolerance(dim):
    """tol = 26 units.  Offsets of length exactly 26 = |(10, 24)| = |(6, 8, 24)| do not match, of length 25 = tol - 2^-12 =
    |(7, 24)| = |(15, 20)| = |(9, 12, 20)| match: along each axis and diagonally, with every sign."""
    tol = 26
    shapes = [(26, 0, 0), (25, 0, 0), (10, 24, 0), (7, 24, 0), (15, 20, 0)] + ([(6, 8, 24), (9, 12, 20), (24, 10, 0)] if dim == 3 else [])
    offsets = []
    for shape in shapes:
        for perm in sorted(set(itertools.permutations(shape[:dim]))):
            nz = [a for a in range(dim) if perm[a]]
            for signs in itertools.product((1, -1), repeat=len(nz)):
                o = list(perm)
                for a, sg in zip(nz, signs):
                    o[a] *= sg
                offsets.append(tuple(o))
    offsets = sorted(set(offsets))
    base, t = (-20000, -8000, 5000)[:dim], (3 * 4096 + 1, -4096, 2)[:dim]
    src, dst, pairs, unmatched = [], [], {}, []
    for j, o in enumerate(offsets):
        d = add(base, (j * 4096, (j % 3) * 2048, (j % 5) * 1024)[:dim])
        dst.append((1000 + j, d)), src.append((2000 + j, sub(add(d, o), t)))
        if sum(v * v for v in o) < tol * tol:
            pairs[2000 + j] = 1000 + j
        else:
            assert sum(v * v for v in o) == tol * tol
            unmatched.append(2000 + j)

    def design(case):
        assert len(unmatched) >= 4 * dim and len(pairs) >= 4 * dim
        lengths = {sum(v * v for v in o) for o in offsets}
        assert lengths == {tol * tol, (tol - 1) ** 2}
        for a in range(dim):  # along each axis, both lengths; and diagonal ones
            assert {abs(o[a]) for o in offsets if sum(map(abs, o)) == abs(o[a])} == {tol, tol - 1}
        assert any(all(o) for o in offsets)

    return Case(f"3-strict-tolerance-{dim}d", dim, src, dst, t, tol, expect=(pairs, len(unmatched), 0, min(unmatched)), design=design)


# ------------------------------------------------------------------------------------------------------- 4. ties and saturation
def ties(dim, swap):
    """tol 2^-3, h 1024 units.  Regions 8 cells apart along x, each around a point P on a cell corner.  0 / 1 / 2: two nodes at
    300 units either side of P along x / y / z, in different cells; 3: two nodes at 300 units, |(-180, -240)| and |(300, 0)|, in
    diagonal cells.  The lowest id wins; with `swap` the two ids change places, so that the winner is the node the search meets
    second.  4: two ids at one point.  5: three qualifiers.  6: five qualifiers, the nearest has the highest id but one.  7: a nearer
    node with a higher id against a farther one with a lower id.  Every source node is ambiguous, and counted once."""
    tol, h, n = 512, 1024, 80
    O = (-4096, 8192, -2048)[:dim]
    t = (4096, 4096 * 3, -4096)[:dim]
    top = tuple(o + n * h for o in O)
    dst, src, pairs, tied = [(1, O), (2, top)], [], {}, []

    def P(r):
        return tuple(O[b] + ((8 + 8 * r) if b == 0 else 8) * h for b in range(dim))

    def vec(*v):
        return tuple(v[:dim]) + (0,) * (dim - len(v[:dim]))

    def region(r, nodes, winner):
        for i, off in nodes:
            dst.append((i, add(P(r), vec(*off))))
        src.append((100 + r, sub(P(r), t)))
        pairs[100 + r] = winner

    for r, (a, b) in enumerate([((-300, 0, 0), (300, 0, 0)), ((0, -300, 0), (0, 300, 0)), ((0, 0, -300), (0, 0, 300)),
                                ((-180, -240, 0), (300, 0, 0))]):
        if r == 2 and dim == 2:
            continue
        lo_id, hi_id = 10 + r, 20 + r
        region(r, [(hi_id if swap else lo_id, a), (lo_id if swap else hi_id, b)], lo_id)
        tied.append((100 + r, hi_id if swap else lo_id, lo_id if swap else hi_id))
    region(4, [(24, (50, 50, 0)), (14, (50, 50, 0))], 14)
    region(5, [(15, (100, 0, 0)), (25, (0, 150, 0)), (35, (-200, 0, 0))], 15)
    region(6, [(16, (400, 0, 0)), (26, (0, 300, 0)), (36, (-200, 0, 0)), (46, (0, -100, 0)), (56, (270, 360, 0))], 46)
    region(7, [(17, (240, 320, 0)), (27, (-60, 80, 0))], 27)

    def design(case):
        g = grid(case)
        assert g.h == h * UNIT
        for s, first, second in tied:
            p, a, b = image(case, src_point(case, s)), dst_point(case, first), dst_point(case, second)
            da, db = [sum(to_units(p[c] - q[c]) ** 2 for c in range(dim)) for q in (a, b)]
            assert da == db == 300 * 300 and g.cell(a) != g.cell(b) and g.key(a) < g.key(b)  # `first` is met first
        assert (not swap) == all(first < second for _, first, second in tied)

    return Case(f"4-ties-{dim}d-{'swapped' if swap else 'plain'}", dim, src, dst, t, tol, expect=(pairs, 0, len(pairs), -1), design=design)


# --------------------------------------------------------------------------------------------------------------- 5. lowest slot
def lowest_slot(dim, reverse):
    """Source node 5 is listed by two sides at two places, L1 and L2, 50 and 51 are the destination nodes at their images: the
    place of the lower slot decides.  Destination node 6 is listed at M1 and M2, 60 and 61 are the source nodes whose images they
    are: one matches 6, the other nothing.  `reverse` lists the second place first."""
    tol = 512
    t = (-4096 * 5, 4096 * 2 + 3, 4096)[:dim]
    step = 16384

    def at(j):
        return (j * step, -j * step // 2, 3 * j * step)[:dim]

    L, M = (at(1), at(2)), (at(3), at(4))
    if reverse:
        L, M = L[::-1], M[::-1]
    fill_src = [(70 + j, sub(at(10 + j), t)) for j in range(6)]
    fill_dst = [(80 + j, at(10 + j)) for j in range(6)]
    src = [(5, L[0])] + fill_src[:4] + [(5, L[1])] + fill_src[4:] + [(60, sub(at(3), t)), (61, sub(at(4), t))]
    dst = [(6, M[0])] + fill_dst[:4] + [(6, M[1])] + fill_dst[4:] + [(50, add(at(1), t)), (51, add(at(2), t))]
    pairs = {70 + j: 80 + j for j in range(6)}
    pairs[5] = 51 if reverse else 50
    pairs[61 if reverse else 60] = 6

    def design(case):
        k = 2 ** (dim - 1)
        for listing, node in ((case.src, 5), (case.dst, 6)):
            slots = [j for j, (i, _) in enumerate(listing) if i == node]
            assert len(slots) == 2 and slots[0] // k != slots[1] // k  # two sides
            assert listing[slots[0]][1] != listing[slots[1]][1]
        assert (src_point(case, 5) == tuple(v * UNIT for v in (at(2) if reverse else at(1)) + (0,) * (3 - dim)))

    return Case(f"5-lowest-slot-{dim}d-{'reversed' if reverse else 'forward'}", dim, src, dst, t, tol,
                expect=(pairs, 1, 0, 60 if reverse else 61), design=design)


# -------------------------------------------------------------------------------------------------------------- 6. grid regimes
def regime(name, dim, box_lo, box_hi, tol, h, m, single=False, z_fill=0.0, t_z=None):
    """Destination nodes on both corners of the box and at an inner point; images on the corners, tol - 1 units from the inner
    point (matched), tol units from it (not matched) and 5 tol from it.  The design asserts h and m of the restated grid."""
    box_lo, box_hi = tuple(box_lo[:dim]), tuple(box_hi[:dim])
    t = (4096 * 7 + 1, -4096 * 3, 4096 + 2)[:dim]
    inner = box_lo if single else tuple(lo + (hi - lo) // 4 + (1 if hi > lo + 4 else 0) for lo, hi in zip(box_lo, box_hi))
    dst = [(3, inner)] if single else [(1, box_lo), (2, box_hi), (3, inner)]
    e = (1,) + (0,) * (dim - 1)
    src = [] if single else [(11, sub(box_lo, t)), (12, sub(box_hi, t))]
    src += [(13, sub(add(inner, tuple((tol - 1) * v for v in e)), t)), (14, sub(sub(inner, tuple(tol * v for v in e)), t)),
            (15, sub(add(inner, tuple(5 * tol * v for v in e[::-1])), t))]
    pairs = {13: 3} if single else {11: 1, 12: 2, 13: 3}

    def design(case):
        g = grid(case)
        assert g.h == h * UNIT and g.m == m, (g.h / UNIT, g.m)
        assert np.array_equal(g.box_lo, np.array(box_lo) * UNIT) and np.array_equal(g.box_hi, np.array(box_lo if single else box_hi) * UNIT)

    return Case(f"6{name}-{dim}d", dim, src, dst, t, tol, expect=(pairs, 2, 0, 14), design=design, z_fill=z_fill, t_z=t_z)


def regimes(dim):
    E22, E21 = 1 << 22, 1 << 21  # extents in units: 2^10 and 2^9
    out = [regime("a-tolerance-driven-h", dim, (-E21 + 4096, -E21, -E21 - 8192), (E21 + 4096, E21, E21 - 8192), 64, 128, (1 << 15) + 3),
           regime("b-extent-driven-h", dim, (-(1 << 20), -(1 << 20) + 7, -(1 << 19)), (1 << 20, (1 << 20) + 7, 3 * (1 << 19)), 1, 2, (1 << 20) + 3),
           regime("c-single-point", dim, (-12345, 777, 4096), (-12345, 777, 4096), 64, 128, 3, single=True),
           regime("d-far-origin", dim, (1 << 41, -(1 << 41), 1 << 32), ((1 << 41) + 65536, -(1 << 41) + 65536, (1 << 32) + 65536), 64, 128, 512 + 3)]
    for long_axis in range(dim):
        lo = (-(1 << 21), 4096, -8192)
        hi = tuple(lo[a] + (E22 if a == long_axis else 64) for a in range(3))
        out.append(regime(f"e-thin-along-{'xyz'[long_axis]}", dim, lo, hi, 1, 4, (1 << 20) + 3))
    return out


def ignored_z():
    """2-D: the third entry of every vertex and of the translation is ignored (include/l3k.h); the answer is that of z = 0"""
    args = (2, (-4096, 8192), (4096 * 3, 4096 * 5), 64, 128, 128 + 3)
    return [regime("f-plain-z", *args), regime("f-huge-z", *args, z_fill=1e300, t_z=1e300), regime("f-nan-z", *args, z_fill=np.nan, t_z=1e300)]


# ---------------------------------------------------------------------------------------------------------- 7. ids and identity
def ids_and_identity(dim):
    """Ids 2^31 - 1, 2^31 and 0xfffffffe on both sides, the first unmatched node 2^31; node 40 is in both sets and its own nearest
    partner (dropped); node 41 is in both sets but 42 is nearer (kept, ambiguous); 50, 51, 52 all map onto 53."""
    tol = 512
    t = (4096 * 2, -4096 * 6 - 5, 4096 * 9)[:dim]
    B31, TOP = 1 << 31, 0xfffffffe

    def at(j):
        return (-j * 8192, j * 8192 + 3, 40960 - j * 4096)[:dim]

    e = (1,) + (0,) * (dim - 1)
    dst = [(B31, at(1)), (B31 - 1, at(3)), (TOP, at(4)), (40, at(5)), (41, add(at(6), tuple(30 * v for v in e))),
           (42, sub(at(6), tuple(10 * v for v in e))), (53, at(7)), (7, at(12))]
    src = [(B31 - 1, sub(at(1), t)), (B31, sub(at(2), t)), (TOP, sub(at(3), t)), (TOP - 1, sub(at(9), t)), (40, sub(at(5), t)),
           (41, sub(at(6), t)), (50, sub(add(at(7), tuple(100 * v for v in e)), t)), (51, sub(sub(at(7), tuple(200 * v for v in e)), t)),
           (52, sub(add(at(7), tuple(300 * v for v in e[::-1])), t)), (3, sub(at(4), t))]
    pairs = {B31 - 1: B31, TOP: B31 - 1, 3: TOP, 41: 42, 50: 53, 51: 53, 52: 53}

    def design(case):
        assert {i for i, _ in case.src} & {i for i, _ in case.dst} >= {B31 - 1, B31, TOP, 40, 41}

    return Case(f"7-ids-and-identity-{dim}d", dim, src, dst, t, tol, expect=(pairs, 2, 1, B31), design=design)


# -------------------------------------------------------------------------------------------------------------------- 8. volume
def volume(dim, seed):
    """tol 2^-3, h 1024 units, a box of about 64 cells.  4096 destination nodes: 600 in the cell at the upper end of the box on
    every axis (the last run of the sorted keys, which ends at n_dst), 600 in the cell at its lower end, the rest uniform.  4096
    source nodes: copies of destination nodes a few units off, copies tol - 5 .. tol + 5 units off, and strays in and around the
    box.  Every node is listed 1 to 8 times, in shuffled order.  What matches is decided by check_exact and the brute force."""
    rng = np.random.default_rng(1000 * dim + seed)
    tol, h, n, n_nodes, n_cluster = 512, 1024, 64, 4096, 600
    O = np.array((-30000, 12000, 4000)[:dim], dtype=np.int64)
    t = np.array((4096 * 11 + 3, -4096 * 4, 4096 * 2 + 1)[:dim], dtype=np.int64)
    low = O + rng.integers(0, h, (n_cluster, dim))  # cell 1
    low[0] = O
    high = O + (n - 1) * h + rng.integers(0, h, (n_cluster, dim))  # cell n
    high[0] = O + n * h - 1
    rest = O + h + rng.integers(0, (n - 2) * h, (n_nodes - 2 * n_cluster, dim))
    d_pts = np.concatenate([low, rest, high])
    d_ids = rng.permutation(3 * n_nodes)[:n_nodes].astype(np.int64)
    d_ids[np.argmax(d_ids)], d_ids[-1] = d_ids[-1], d_ids.max()  # the highest id in the last cell: the very last sorted entry
    kind = rng.choice(3, n_nodes, p=(0.7, 0.15, 0.15))
    kind[-1] = 0
    s_pts = d_pts.copy()
    jitter = kind == 0
    s_pts[jitter] += rng.integers(-3, 4, (int(jitter.sum()), dim))
    s_pts[-1] = d_pts[-1]  # the last sorted entry has an image of its own, on the spot
    edge = kind == 1
    direction = rng.normal(size=(int(edge.sum()), dim))
    direction /= np.linalg.norm(direction, axis=1, keepdims=True)
    s_pts[edge] += np.rint(direction * rng.uniform(tol - 5, tol + 5, (int(edge.sum()), 1))).astype(np.int64)
    stray = kind == 2
    s_pts[stray] = O - 4 * h + rng.integers(0, (n + 8) * h, (int(stray.sum()), dim))
    s_pts -= t
    s_ids = rng.permutation(3 * n_nodes)[:n_nodes].astype(np.int64)

    def listing(ids, pts):
        times = rng.integers(1, 9, ids.size)
        where = rng.permutation(np.repeat(np.arange(ids.size), times))
        return [(int(ids[j]), tuple(int(v) for v in pts[j])) for j in where.tolist()]

    def design(case):
        g = grid(case)
        assert g.h == h * UNIT and g.m == n + 3
        nodes = dict((i, p) for i, p in reversed(case.dst))  # (every listing of a node has the same point here)
        ids, keys = np.array(list(nodes)), g.keys(np.array(list(nodes.values())))
        assert keys.size == n_nodes and (keys == keys.max()).sum() == n_cluster and (keys == keys.min()).sum() == n_cluster
        assert ids[keys == keys.max()].max() == int(d_ids[-1]) == ids.max()  # the last entry of the sorted keys
        ref = reference(case)
        assert ref[2] > 100 and ref[3] > 500 and ref[0].size > 2500  # unmatched, ambiguous, pairs: all kinds occur
        assert int(s_ids[-1]) in ref[0].tolist()
        k = 2 ** (dim - 1)
        assert len(case.src) // k > 4 * 256 and len(case.dst) // k > 4 * 256  # several workgroups in every kernel
        counts = np.bincount(np.unique([i for i, _ in case.dst], return_inverse=True)[1])
        assert counts.min() == 1 and counts.max() == 8

    return Case(f"8-volume-{dim}d-seed{seed}", dim, listing(s_ids, s_pts), listing(d_ids, d_pts), tuple(int(v) for v in t), tol, design=design)


# ---------------------------------------------------------------------------------------------------------------- the case list
def _all_cases():
    out = []
    for dim in (2, 3):
        out.append(neighbour_cells(dim, "interior"))
        for axis in range(dim):
            out += [neighbour_cells(dim, "low", axis), neighbour_cells(dim, "high", axis)]
        out += [out_of_reach(dim), beyond_int64(dim, 1), beyond_int64(dim, -1), strict_tolerance(dim)]
        out += [ties(dim, False), ties(dim, True), lowest_slot(dim, False), lowest_slot(dim, True)]
        out += regimes(dim)
        out.append(ids_and_identity(dim))
    out += ignored_z()
    out += [volume(dim, seed) for dim in (2, 3) for seed in range(3)]
    assert len({c.name for c in out}) == len(out)
    return out


CASES = _all_cases()
SAME_ANSWER = [("6f-huge-z-2d", "6f-plain-z-2d"), ("6f-nan-z-2d", "6f-plain-z-2d")]  # (case, the case it must agree with)


def by_name(name):
    return next(c for c in CASES if c.name == name)


# ------------------------------------------------------------------------------------------------------------ refused inputs
class RawCase(Case):
    """points, translation and tolerance as given, not on the lattice"""

    def __init__(self, name, dim, src, dst, translation, tolerance):
        self.name, self.dim, self.src, self.dst = name, dim, src, dst
        self.translation, self.tolerance, self.z_fill, self.expect, self.design = translation, tolerance, 0.0, None, None


def refused_inputs():
    """[(case, the word its refusal must contain)]: finite inputs from which no grid can be made.  A box from -1e308 to 1e308
    (its extent overflows), a tolerance of 1e308 (twice the tolerance overflows), the smallest subnormal tolerance on a single
    destination point (the inverse of the cell edge overflows)."""
    one = [(1, (0.25, 0.5, 0.0))]
    return [(RawCase("refused-box-overflow", 2, [(5, (0.0, 0.0, 0.0))], [(1, (-1e308, 0.0, 0.0)), (2, (1e308, 1.0, 0.0))],
                     (1.0, 0.0, 0.0), 1e-12), "box"),
            (RawCase("refused-tolerance-overflow", 3, [(5, (0.0, 0.0, 0.0))], [(1, (0.0, 0.0, 0.0)), (2, (1.0, 1.0, 1.0))],
                     (1.0, 0.0, 0.0), 1e308), "tolerance"),
            (RawCase("refused-subnormal-tolerance", 2, [(5, (0.25, 0.5, 0.0))], one, (0.0, 0.0, 0.0), 5e-324), "tolerance")]
