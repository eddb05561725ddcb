// periodic.cpp -- periodic boundary conditions, step 2: the matched node pairs become an ordinary mesh (host only, no context).
//
// The reference forms the connected components of the match graph (getComponents, bcs/PeriodicBC.hpp) and lets every dof of a
// component stand for one unknown.  Here the identification is carried out on the connectivity itself: every component keeps its
// lowest node id, the kept nodes are ranked in ascending old id, and elem_nodes is rewritten through that map.  Only non-internal
// nodes can be paired, a representative is never above the nodes it stands for, and ranks ascend with the old ids, so the
// [non-internal | internal, contiguous per element] numbering l3k_mesh_create, the condensation and the partitioner rely on
// survives.  Also the finiteness checks of l3k_periodic_match and the construction of its box and grid (host/periodic.hpp): this
// unit is not built with -ffinite-math-only, so a box or a tolerance the grid cannot be made from is refused here.
#include "host/periodic.hpp"
#include "l3k.h"

#include <cmath>
#include <cstdint>
#include <new>
#include <string>
#include <vector>

namespace l3k::dev
{
void setError(const char* fmt, ...);
}

namespace l3k::host
{
bool allFinite(const double* v, size_t n)
{
    for (size_t i = 0; i < n; ++i)
        if (!std::isfinite(v[i]))
            return false;
    return true;
}
const char* periodicCheckReals(int dim, const double* translation, const double* tolerance)
{
    if (!allFinite(translation, size_t(dim)))
        return "the translation is not finite";
    if (!(std::isfinite(*tolerance) && *tolerance > 0.))
        return "the tolerance must be finite and positive";
    return nullptr;
}

std::string periodicMakeGrid(int dim, const double* box_lo, const double* box_hi, double tolerance, l3k::periodic::Grid* grid)
{
    using l3k::periodic::cell_bits;
    double extent = 0.;
    for (int a = 0; a < dim; ++a)
    {
        const double e = box_hi[a] - box_lo[a];
        if (!std::isfinite(e)) // finite vertices, e.g. -1e308 and 1e308, whose difference overflows
            return "the box of the destination vertices has an extent that is not finite";
        extent = e > extent ? e : extent;
    }
    const double two_tol = 2. * tolerance;
    if (!std::isfinite(two_tol))
        return "the tolerance is too large: twice the tolerance is not finite";
    double h = two_tol > extent / double(1 << 20) ? two_tol : extent / double(1 << 20);
    // h >= extent / 2^20 leaves at most 2^20 + 3 cells: the doubling guards the rounding of the quotient, a few turns at the most
    const double cell_limit = double(int64_t(1) << cell_bits);
    for (int turn = 0; !(std::ceil(extent / h) + 3. < cell_limit); ++turn)
    {
        if (turn == 64 || !std::isfinite(h))
            return "the box of the destination vertices and the tolerance give no finite cell edge";
        h *= 2.;
    }
    const double inv_h = 1. / h;
    if (!std::isfinite(h) || !(h > 0.))
        return "the box of the destination vertices and the tolerance give no finite cell edge";
    if (!std::isfinite(inv_h))
        return "the tolerance is too small: the inverse of the cell edge is not finite";
    if (inv_h == 0.)
        return "the tolerance or the box of the destination vertices is too large: the inverse of the cell edge is zero";
    for (int a = 0; a < 3; ++a)
    {
        grid->lo[a] = a < dim ? box_lo[a] - h : 0.;
        if (!std::isfinite(grid->lo[a]))
            return "the box of the destination vertices has no finite cell below it";
    }
    grid->inv_h = inv_h;
    grid->m     = int64_t(std::ceil(extent / h)) + 3;
    return {};
}

std::string periodicBoxAndGrid(int dim, const double* elem_verts, int64_t n_src, const int64_t* src_elem, int64_t n_dst,
                               const int64_t* dst_elem, double tolerance, l3k::periodic::Grid* grid)
{
    const int nv = 1 << dim;
    double    lo[3] = {0., 0., 0.}, hi[3] = {0., 0., 0.};
    for (int64_t f = 0; f < n_src + n_dst; ++f)
    {
        const bool    is_dst = f >= n_src;
        const int64_t e      = is_dst ? dst_elem[f - n_src] : src_elem[f];
        const double* v      = elem_verts + e * nv * 3;
        for (int c = 0; c < nv; ++c)
            if (!allFinite(v + c * 3, size_t(dim)))
                return "element " + std::to_string(e) + " has a vertex that is not finite";
        if (!is_dst)
            continue;
        for (int c = 0; c < nv; ++c)
            for (int a = 0; a < dim; ++a)
            {
                const double x     = v[c * 3 + a];
                const bool   first = f == n_src && c == 0;
                lo[a]              = first || x < lo[a] ? x : lo[a];
                hi[a]              = first || x > hi[a] ? x : hi[a];
            }
    }
    return periodicMakeGrid(dim, lo, hi, tolerance, grid);
}
} // namespace l3k::host

extern "C" int l3k_periodic_merge(int64_t n_nodes, int64_t n_noninternal, int64_t n_pairs, const uint32_t* pair_a,
                                  const uint32_t* pair_b, int64_t n_entries, uint32_t* elem_nodes, uint32_t* node_map,
                                  int64_t* n_nodes_out, int64_t* n_noninternal_out, int64_t* n_components)
{
    using l3k::dev::setError;
    if (n_nodes < 0 || n_noninternal < 0 || n_noninternal > n_nodes || n_nodes >= (int64_t(1) << 32) || n_pairs < 0 || n_entries < 0)
    {
        setError("l3k_periodic_merge: need 0 <= n_noninternal <= n_nodes < 2^32 and non-negative counts");
        return -1;
    }
    if ((n_pairs > 0 && (!pair_a || !pair_b)) || (n_entries > 0 && !elem_nodes) || (n_nodes > 0 && !node_map) || !n_nodes_out ||
        !n_noninternal_out || !n_components)
    {
        setError("l3k_periodic_merge: null arrays with non-zero counts, or null counters");
        return -1;
    }
    for (int64_t i = 0; i < n_pairs; ++i)
        if (pair_a[i] >= uint64_t(n_noninternal) || pair_b[i] >= uint64_t(n_noninternal))
        {
            setError("l3k_periodic_merge: pair %lld = (%u, %u) names an element-internal node or one outside [0,%lld)", (long long)i,
                     pair_a[i], pair_b[i], (long long)n_noninternal);
            return -1;
        }
    for (int64_t i = 0; i < n_entries; ++i)
        if (elem_nodes[i] >= uint64_t(n_nodes))
        {
            setError("l3k_periodic_merge: elem_nodes[%lld] = %u is outside [0,%lld)", (long long)i, elem_nodes[i], (long long)n_nodes);
            return -1;
        }
    std::vector< uint32_t > parent;
    std::vector< bool >     has_member; // roots something else points at
    try
    {
        parent.resize(size_t(n_noninternal));
        has_member.assign(size_t(n_noninternal), false);
    }
    catch (const std::bad_alloc&)
    {
        setError("l3k_periodic_merge: out of memory");
        return -3;
    }
    for (size_t i = 0; i < parent.size(); ++i)
        parent[i] = uint32_t(i);
    const auto find = [&](uint32_t x) {
        uint32_t r = x;
        while (parent[r] != r)
            r = parent[r];
        while (parent[x] != r) // path compression
        {
            const uint32_t next = parent[x];
            parent[x]           = r;
            x                   = next;
        }
        return r;
    };
    for (int64_t i = 0; i < n_pairs; ++i)
    {
        const uint32_t ra = find(pair_a[i]), rb = find(pair_b[i]);
        if (ra != rb) // the lower id stays the root: the root of a component is its lowest node
            parent[ra < rb ? rb : ra] = ra < rb ? ra : rb;
    }
    // a root precedes the nodes it stands for, so one ascending pass ranks the kept nodes and maps the others
    uint32_t rank = 0;
    for (int64_t i = 0; i < n_nodes; ++i)
    {
        const uint32_t r = i < n_noninternal ? find(uint32_t(i)) : uint32_t(i);
        node_map[i]      = r == uint32_t(i) ? rank++ : node_map[r];
    }
    // components with more than one node
    for (size_t i = 0; i < parent.size(); ++i)
        if (parent[i] != uint32_t(i))
            has_member[find(uint32_t(i))] = true;
    int64_t n_comp = 0;
    for (size_t i = 0; i < parent.size(); ++i)
        n_comp += has_member[i];
    for (int64_t i = 0; i < n_entries; ++i)
        elem_nodes[i] = node_map[elem_nodes[i]];
    *n_nodes_out       = int64_t(rank);
    *n_noninternal_out = n_noninternal - (n_nodes - int64_t(rank));
    *n_components      = n_comp;
    return 0;
}
