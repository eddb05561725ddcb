// periodic.cpp -- periodic boundary conditions, step 2: the matched node pairs become an ordinary mesh (host only, no context).
//
// The reference forms the connected components of the match graph (getComponents, bcs/PeriodicBC.hpp) and lets every dof of a
// component stand for one unknown.  Here the identification is carried out on the connectivity itself: every component keeps its
// lowest node id, the kept nodes are ranked in ascending old id, and elem_nodes is rewritten through that map.  Only non-internal
// nodes can be paired, a representative is never above the nodes it stands for, and ranks ascend with the old ids, so the
// [non-internal | internal, contiguous per element] numbering l3k_mesh_create, the condensation and the partitioner rely on
// survives.  Also the finiteness checks of l3k_periodic_match (host/periodic.hpp).
#include "host/periodic.hpp"
#include "l3k.h"

#include <cmath>
#include <cstdint>
#include <new>
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
