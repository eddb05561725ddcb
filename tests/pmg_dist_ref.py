"""CPU restatement of the p-multigrid transfer on a PARTITIONED mesh (include/l3k.h: l3k_transfer_*) in numpy, dense, on top of
tests/pmg_ref.py: per rank the matrix P_r with one row per OWNED fine node and one column per LOCAL coarse node (owned, then
ghost), under the partitioned ownership rule -- a fine node is handled by the rank that owns it, there by the lowest local fine
element that contains it; ghost fine nodes have no handler -- and the assembly of the ranks' matrices into one global matrix
through node_grid_id, the partition-independent node id."""
import numpy as np

import pmg_ref as R

SENTINEL = np.iinfo(np.int64).max


def owners(fine_part):
    """owner[local node] = the lowest local element that contains the node, for OWNED nodes; SENTINEL for ghost nodes"""
    own = np.full(fine_part.n_local_nodes, SENTINEL, dtype=np.int64)
    for e in range(fine_part.n_elems - 1, -1, -1):
        nodes = fine_part.elem_nodes[e].astype(np.int64)
        own[nodes[nodes < fine_part.n_owned_nodes]] = e
    return own


def rank_node_prolongation(fine_part, coarse_part, elem_map=None):
    """P_r (owned fine nodes x local coarse nodes, dense) of one rank.  Every component of a node moves alike."""
    T = R.interp_1d(coarse_part.order, fine_part.order)
    Pe = T
    for _ in range(fine_part.dim - 1):
        Pe = np.kron(T, Pe)
    own = owners(fine_part)
    P = np.zeros((fine_part.n_owned_nodes, coarse_part.n_local_nodes))
    for e in range(fine_part.n_elems):
        ec = e if elem_map is None else int(elem_map[e])
        fn, cn = fine_part.elem_nodes[e].astype(np.int64), coarse_part.elem_nodes[ec].astype(np.int64)
        mine = own[fn] == e  # (never true for a ghost node: its owner is the sentinel)
        P[np.ix_(fn[mine], cn)] = Pe[mine]
    return P


def grid_index(whole):
    """index[grid id] = local node of the single-rank partition `whole`"""
    idx = np.full(int(whole.node_grid_id.max()) + 1, -1, dtype=np.int64)
    idx[whole.node_grid_id] = np.arange(whole.n_local_nodes)
    return idx


def assemble(fine_parts, coarse_parts, Ps, whole_fine, whole_coarse):
    """(P, rows): the ranks' P_r summed into one matrix in the node numbering of the single-rank partitions `whole_*`, and the
    number of rows each global fine node received (the rule asks for exactly one)"""
    fi, ci = grid_index(whole_fine), grid_index(whole_coarse)
    P = np.zeros((whole_fine.n_local_nodes, whole_coarse.n_local_nodes))
    rows = np.zeros(whole_fine.n_local_nodes, dtype=np.int64)
    for f, c, Pr in zip(fine_parts, coarse_parts, Ps):
        r = fi[f.node_grid_id[:f.n_owned_nodes]]
        P[np.ix_(r, ci[c.node_grid_id[:c.n_local_nodes]])] += Pr
        np.add.at(rows, r, 1)
    return P, rows


def restrict_export_add(fine_parts, coarse_parts, Ps, whole_fine, whole_coarse, rf):
    """r_c of the whole mesh the way the ranks compute it: each rank applies P_r^T to its owned rows of rf (whole numbering,
    [nodes][U]) into its local coarse rows -- owned and ghost -- and the export-add sums every ghost row into its owner's"""
    fi, ci = grid_index(whole_fine), grid_index(whole_coarse)
    rc = np.zeros((whole_coarse.n_local_nodes,) + rf.shape[1:])
    for f, c, Pr in zip(fine_parts, coarse_parts, Ps):
        local = Pr.T @ rf[fi[f.node_grid_id[:f.n_owned_nodes]]]
        np.add.at(rc, ci[c.node_grid_id[:c.n_local_nodes]], local)
    return rc
