"""Quad (2-D) support on the host: the kernel registry, the square mesh generator and the dimension-aware partition.  No GPU."""
import numpy as np
import pytest

import oracle_lib as O
from l3ster_amd import system
from l3ster_amd.partition import PartitionedMesh, rcb_partition
from test_oracle_boundary import _square_mesh


@pytest.mark.parametrize("kid", [system.KERNEL_DIFFUSION2D, system.KERNEL_DIFFUSION2D_VAR])
def test_kernel_info_matches_oracle(kid):
    info, ref = system.kernel_info(kid), O.kernel_params(kid)
    assert (info["dimension"], info["n_equations"], info["n_unknowns"], info["n_fields"]) == (ref["dim"], ref["E"], ref["U"], ref["F"])
    assert info["dimension"] == 2 and info["param_bytes"] == 0


def test_quad_instances_registered():
    inst = set(system.instances())
    for p in range(1, 7):
        for R in (1, 2):
            assert (system.KERNEL_DIFFUSION2D, p, p + 1, R) in inst
    assert (system.KERNEL_DIFFUSION2D, 4, 9, 2) in inst
    for shape in [(2, 3, 1), (4, 5, 1), (4, 9, 2)]:
        assert (system.KERNEL_DIFFUSION2D_VAR,) + shape in inst


@pytest.mark.parametrize("ne,p", [(3, 1), (4, 2), ((5, 3), 3), ((2, 4), 4), (3, 6)])
def test_square_mesh_conventions(ne, p):
    m = system.SquarePartition(ne, p, perturb=0.1)
    ne2 = (ne,) * 2 if np.isscalar(ne) else ne
    n = p + 1
    assert m.dim == 2 and m.elem_verts.shape == (m.n_elems, 4, 3) and m.elem_nodes.shape == (m.n_elems, n * n)
    assert m.n_elems == np.prod(ne2) == m.n_interior_elems and m.n_ghost_nodes == 0
    assert m.n_owned_nodes == np.prod([p * e + 1 for e in ne2]) == m.n_global_nodes
    assert np.array_equal(np.unique(m.elem_nodes), np.arange(m.n_owned_nodes))  # a numbering of all nodes
    assert np.all(m.elem_verts[:, :, 2] == 0.0)
    # element-internal nodes after every non-internal node, contiguous per element, lexicographic
    idx = np.arange(n * n)
    ix, iy = idx % n, idx // n
    internal = (ix > 0) & (ix < p) & (iy > 0) & (iy < p)
    n_int = (p - 1) ** 2
    if n_int:
        first_internal = m.n_owned_nodes - m.n_elems * n_int
        ids = m.elem_nodes[:, internal].astype(np.int64)
        assert ids.min() == first_internal
        assert np.all(np.diff(ids, axis=1) == 1)
        assert np.all(np.diff(ids[:, 0]) == n_int)
        assert m.elem_nodes[:, ~internal].max() < first_internal
    # boundary bits follow the grid position (sides 0 y=0, 1 y=1, 2 x=0, 3 x=1)
    Nx, Ny = p * ne2[0] + 1, p * ne2[1] + 1
    gx, gy = m.node_grid_id % Nx, m.node_grid_id // Nx
    assert np.array_equal(np.sort(m.node_grid_id), np.arange(Nx * Ny))
    b = m.node_boundary
    assert np.array_equal((b & 1) != 0, gy == 0) and np.array_equal((b & 2) != 0, gy == Ny - 1)
    assert np.array_equal((b & 4) != 0, gx == 0) and np.array_equal((b & 8) != 0, gx == Nx - 1)
    fe, fs = m.boundary_sides()
    assert fe.size == 2 * (ne2[0] + ne2[1])
    # nodes shared by neighbouring elements map to the same point; unperturbed positions sit on the GLL grid
    gll = system.gll_nodes(n)
    pos = {}
    for e in range(m.n_elems):
        for i in range(n * n):
            xyz = O.map_to_physical(2, m.elem_verts[e], [gll[i % n], gll[i // n]])
            node = int(m.elem_nodes[e, i])
            if node in pos:
                np.testing.assert_allclose(xyz, pos[node], atol=1e-14)
            pos[node] = xyz
    coords = m.node_coords()
    np.testing.assert_allclose(coords[[k for k in pos]], np.array(list(pos.values())), atol=1e-14)
    # unperturbed: grid node gx = ex*p + i sits at x = (ex + (gll_i + 1) / 2) / ne
    xy = system.SquarePartition(ne, p).node_coords()
    np.testing.assert_allclose(xy[:, 0], (gx // p + (gll[gx % p] + 1) / 2) / ne2[0], atol=1e-14)
    np.testing.assert_allclose(xy[:, 1], (gy // p + (gll[gy % p] + 1) / 2) / ne2[1], atol=1e-14)


def test_square_mesh_positive_jacobian():
    m = system.SquarePartition((7, 5), 3, perturb=0.2)
    x, w = O.gl_rule(4)
    v = m.elem_verts
    for xi in x:
        for eta in x:
            dxdxi = .25 * ((1 - eta) * (v[:, 1, :2] - v[:, 0, :2]) + (1 + eta) * (v[:, 3, :2] - v[:, 2, :2]))
            dxdeta = .25 * ((1 - xi) * (v[:, 2, :2] - v[:, 0, :2]) + (1 + xi) * (v[:, 3, :2] - v[:, 1, :2]))
            assert np.all(dxdxi[:, 0] * dxdeta[:, 1] - dxdxi[:, 1] * dxdeta[:, 0] > 0)


def test_square_mesh_rejects_bad_arguments():
    with pytest.raises(system.L3KError):
        system.SquarePartition(0, 2)
    with pytest.raises(system.L3KError):
        system.SquarePartition(3, 0)


@pytest.mark.parametrize("world", [3, 4])
def test_partitioned_square_mesh(world):
    p = 3
    m = system.SquarePartition((6, 5), p, perturb=0.1)
    parts = rcb_partition(m.elem_verts, world)
    ranks = [PartitionedMesh(m.elem_nodes, m.elem_verts, None, parts, r, world, p, device="cpu") for r in range(world)]
    assert sum(r.n_owned_nodes for r in ranks) == m.n_owned_nodes
    assert sum(r.n_elems for r in ranks) == m.n_elems
    owned_grid = np.concatenate([r.node_grid_id[:r.n_owned_nodes] for r in ranks])
    assert np.array_equal(np.sort(owned_grid), np.arange(m.n_owned_nodes))
    coords_global = m.node_coords()
    for r in ranks:
        assert r.dim == 2 and r.elem_verts.shape[1:] == (4, 3) and r.elem_nodes.shape[1] == (p + 1) ** 2
        # interior elements first: they touch owned nodes only
        assert np.all(r.elem_nodes[:r.n_interior_elems] < r.n_owned_nodes)
        # local node positions agree with the global mesh through node_grid_id
        np.testing.assert_allclose(r.node_coords(), coords_global[r.node_grid_id], atol=1e-14)
        # exchange plan: my ghosts are owned by the neighbours that list them as send nodes
        for q, (g0, g1) in zip(r.nbr_rank, r.ghost_ranges):
            other = ranks[q]
            gids = r.node_grid_id[r.n_owned_nodes + g0:r.n_owned_nodes + g1]
            k = other.nbr_rank.index(r.rank)
            sent = other.node_grid_id[other.send_nodes[k]]
            assert np.array_equal(np.sort(gids), np.sort(sent))


@pytest.mark.parametrize("p", [1, 2, 4])
def test_oracle_apply_on_square_partition_matches_reference_numbering(p):
    """The oracle's apply on SquarePartition's numbering equals the one on _square_mesh's lexicographic numbering after
    permuting the nodes: the two meshes are the same mesh."""
    ne, U = 4, 3
    nq = p + 1
    m = system.SquarePartition(ne, p)
    ref_nodes, ref_verts, ref_coords, _ = _square_mesh(ne, p)
    np.testing.assert_allclose(m.elem_verts, ref_verts, atol=1e-15)
    # node k of SquarePartition == lexicographic grid node node_grid_id[k] of _square_mesh
    perm = m.node_grid_id.astype(np.int64)
    assert np.array_equal(perm[m.elem_nodes.astype(np.int64)], ref_nodes.astype(np.int64))
    rng = np.random.default_rng(p)
    x_ref = rng.uniform(-1, 1, (ref_coords.shape[0] * U, 1))
    x_mine = x_ref.reshape(-1, U)[perm].reshape(-1, 1)
    mv_ref = O.MeshView(2, p, nq, ref_nodes, ref_verts, ref_coords.shape[0], U, np.arange(U))
    mv_mine = O.MeshView(2, p, nq, m.elem_nodes, m.elem_verts, m.n_owned_nodes, U, np.arange(U))
    y_ref = O.mf_apply(mv_ref, O.KERNEL_DIFFUSION2D, x_ref)
    y_mine = O.mf_apply(mv_mine, O.KERNEL_DIFFUSION2D, x_mine)
    np.testing.assert_allclose(y_mine.reshape(-1, U), y_ref.reshape(-1, U)[perm], rtol=0, atol=1e-13 * np.abs(y_ref).max())
