// api_periodic.hip -- periodic boundary conditions, step 1: which node of the source sides is the image of which node of the
// destination sides (BCDefinition::definePeriodic, bcs/BCDefinition.hpp:92-104; bcs/PeriodicBC.hpp: getNodeLocationData, NodeMatcher).
//
// The reference gathers the physical location of every boundary node, translates the source side and looks every translated node
// up among the destination nodes within a tolerance.  Here only the listed sides travel to the device (their vertices and side
// node ids, gathered on the host); one lane per (side, side node) evaluates the bi-/tri-linear location; the nodes of either set
// are made unique by a sort on (node id, slot) -- a node listed through several sides keeps the location of its lowest slot --;
// the destination nodes are binned on a uniform grid of edge h >= 2 tolerance (at most 2^20 + 3 cells per axis, so that the cell
// coordinates pack into one 64-bit key with x in the low bits) and sorted by cell key; every source node then scans the 3^(dim-1)
// runs of three x-adjacent cells around its translated location, each found by one lower bound.  The winner is the nearest
// qualifying destination node, ties to the lowest id: decided by comparing (distance, id) of every candidate, so the order of the
// nodes inside a cell -- and with it the stability of the sorts -- does not enter the result.  Memory grows with the number of
// listed side nodes.  Work per source node grows with the number of destination nodes in the 3^dim cells around it: a handful as
// long as the tolerance is below the node spacing; a tolerance above the node spacing is legal and merely slow (every source node
// then walks all the destination nodes within 3 h of it).  Integer and fp64 work with no reuse: plain one-thread-per-item kernels, no LDS.
// The box of the destination vertices and the grid over it are made on the host (host/periodic.hpp), which refuses a box or a
// tolerance that gives no grid before anything is launched.
#include "objects.hpp"

#include "device/periodic.hpp"
#include "host/periodic.hpp"
#include "host/tables.hpp"

#include <cmath>
#include <rocprim/rocprim.hpp>

namespace
{
using l3k::dev::setError;
using namespace l3k::periodic; // the per-item work: device/periodic.hpp

__global__ void sideNodeLocations(int dim, int n1, int ns, int64_t n_sides, const double* __restrict__ verts,
                                  const uint8_t* __restrict__ side, const uint32_t* __restrict__ ids, const double* __restrict__ gll,
                                  double* __restrict__ loc, uint64_t* __restrict__ keys)
{
    const int64_t t = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
    if (t < n_sides * ns)
        sideNodeLocation(t, dim, n1, ns, verts, side, ids, gll, loc, keys);
}

__global__ void markNewIds(const uint64_t* __restrict__ sorted, int64_t n, uint32_t* __restrict__ head)
{
    const int64_t t = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
    if (t < n)
        head[t] = startsNewId(t, sorted);
}

__global__ void compactNodes(const uint64_t* __restrict__ sorted, const uint32_t* __restrict__ incl, int64_t n,
                             const double* __restrict__ loc, uint32_t* __restrict__ uid, double* __restrict__ uloc)
{
    const int64_t t = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
    if (t < n)
        compactNode(t, sorted, incl, loc, uid, uloc);
}

__global__ void cellKeys(int dim, Grid g, const double* __restrict__ uloc, int64_t n, uint64_t* __restrict__ keys,
                         uint32_t* __restrict__ vals)
{
    const int64_t t = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
    if (t >= n)
        return;
    keys[t] = cellKey(t, dim, g, uloc);
    vals[t] = uint32_t(t);
}

// one lane per unique source node; one writer per output
__global__ void matchNodes(int dim, Grid g, double t0, double t1, double t2, double tolerance, const double* __restrict__ sloc,
                           int64_t n_src, const uint64_t* __restrict__ dkeys, const uint32_t* __restrict__ dvals,
                           const uint32_t* __restrict__ did, const double* __restrict__ dloc, int64_t n_dst,
                           uint32_t* __restrict__ partner, uint8_t* __restrict__ n_qualify)
{
    const int64_t t = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
    if (t >= n_src)
        return;
    const double translation[3] = {t0, t1, t2};
    matchNode(t, dim, g, translation, tolerance, sloc, dkeys, dvals, did, dloc, n_dst, partner, n_qualify);
}

inline unsigned blocksFor(int64_t n)
{
    return unsigned((n + 255) / 256);
}

template < typename... Args >
int sortOnDevice(size_t n, hipStream_t s, Args... args)
{
    size_t tmp_bytes = 0;
    L3K_HIP(rocprim::merge_sort(nullptr, tmp_bytes, args..., n, rocprim::less< uint64_t >(), s));
    DevBuf< char > tmp;
    if (int rc = tmp.alloc(tmp_bytes ? tmp_bytes : 1))
        return rc;
    L3K_HIP(rocprim::merge_sort(tmp.ptr, tmp_bytes, args..., n, rocprim::less< uint64_t >(), s));
    L3K_HIP(hipStreamSynchronize(s)); // (tmp is a local)
    return 0;
}

// The unique nodes of the listed sides, ascending in the node id, with their locations
struct NodeSet
{
    DevBuf< uint32_t > id;
    DevBuf< double >   loc;
    int64_t            n = 0;
};

int uniqueSideNodes(hipStream_t s, int dim, int order, const uint32_t* elem_nodes, const double* elem_verts, int64_t n_sides,
                    const int64_t* elem, const uint8_t* side, const double* d_gll, NodeSet& out)
{
    const int     n1 = order + 1, ns = dim == 3 ? n1 * n1 : n1, nv = 1 << dim;
    const int64_t N = dim == 3 ? int64_t(n1) * n1 * n1 : int64_t(n1) * n1, n = n_sides * ns;
    if (n == 0)
        return 0;
    // what the listed sides need, gathered on the host: the whole connectivity stays where it is
    std::vector< double >   verts(size_t(n_sides) * nv * 3);
    std::vector< uint32_t > ids(size_t(n), 0u);
    for (int64_t f = 0; f < n_sides; ++f)
    {
        std::copy_n(elem_verts + elem[f] * nv * 3, nv * 3, verts.begin() + f * nv * 3);
        for (int q = 0; q < ns; ++q)
        {
            int ijk[3];
            sideNodeIndex(dim, n1, side[f], q, ijk);
            ids[size_t(f * ns + q)] = elem_nodes[elem[f] * N + ijk[0] + n1 * (ijk[1] + n1 * ijk[2])];
        }
    }
    DevBuf< double >   d_verts, loc;
    DevBuf< uint8_t >  d_side;
    DevBuf< uint32_t > d_ids, head;
    DevBuf< uint64_t > keys, sorted;
    if (int rc = d_verts.upload(verts.data(), verts.size(), s))
        return rc;
    if (int rc = d_side.upload(side, size_t(n_sides), s))
        return rc;
    if (int rc = d_ids.upload(ids.data(), ids.size(), s))
        return rc;
    if (loc.alloc(size_t(n) * 3) || keys.alloc(size_t(n)) || sorted.alloc(size_t(n)) || head.alloc(size_t(n)))
        return -3;
    hipLaunchKernelGGL(sideNodeLocations, dim3(blocksFor(n)), dim3(256), 0, s, dim, n1, ns, n_sides, d_verts.ptr, d_side.ptr, d_ids.ptr,
                       d_gll, loc.ptr, keys.ptr);
    L3K_HIP(hipGetLastError());
    if (int rc = sortOnDevice(size_t(n), s, keys.ptr, sorted.ptr)) // (synchronises: the host vectors may go after it)
        return rc;
    hipLaunchKernelGGL(markNewIds, dim3(blocksFor(n)), dim3(256), 0, s, sorted.ptr, n, head.ptr);
    size_t scan_bytes = 0;
    L3K_HIP(rocprim::inclusive_scan(nullptr, scan_bytes, head.ptr, head.ptr, size_t(n), rocprim::plus< uint32_t >(), s));
    DevBuf< char > tmp;
    if (int rc = tmp.alloc(scan_bytes ? scan_bytes : 1))
        return rc;
    L3K_HIP(rocprim::inclusive_scan(tmp.ptr, scan_bytes, head.ptr, head.ptr, size_t(n), rocprim::plus< uint32_t >(), s));
    uint32_t n_unique = 0;
    L3K_HIP(hipMemcpyAsync(&n_unique, head.ptr + (n - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    L3K_HIP(hipStreamSynchronize(s));
    out.n = n_unique;
    if (out.id.alloc(n_unique) || out.loc.alloc(size_t(n_unique) * 3))
        return -3;
    hipLaunchKernelGGL(compactNodes, dim3(blocksFor(n)), dim3(256), 0, s, sorted.ptr, head.ptr, n, loc.ptr, out.id.ptr, out.loc.ptr);
    L3K_HIP(hipGetLastError());
    L3K_HIP(hipStreamSynchronize(s)); // (the inputs of the kernel are locals)
    return 0;
}

bool sidesInsideMesh(const char* what, int dim, int64_t n_elems, int64_t n, const int64_t* elem, const uint8_t* side)
{
    for (int64_t i = 0; i < n; ++i)
        if (elem[i] < 0 || elem[i] >= n_elems || side[i] >= 2 * dim)
        {
            setError("l3k_periodic_match: %s side %lld = (element %lld, side %d) is outside the mesh", what, (long long)i,
                     (long long)elem[i], int(side[i]));
            return false;
        }
    return true;
}
} // namespace

extern "C" int l3k_periodic_match(l3k_ctx* ctx, int dim, int order, int64_t n_elems, const uint32_t* elem_nodes,
                                  const double* elem_verts, int64_t n_src, const int64_t* src_elem, const uint8_t* src_side,
                                  int64_t n_dst, const int64_t* dst_elem, const uint8_t* dst_side, const double translation[3],
                                  double tolerance, uint32_t* pair_src, uint32_t* pair_dst, int64_t* n_pairs, int64_t* n_unmatched,
                                  int64_t* n_ambiguous, int64_t* first_unmatched)
{
    if (!ctx || !n_pairs || !n_unmatched || !n_ambiguous || !first_unmatched || !translation)
    {
        setError("l3k_periodic_match: null context, translation or counters");
        return -1;
    }
    if (dim != 2 && dim != 3)
    {
        setError("l3k_periodic_match: dim = %d, only quads (2) and hexes (3) have sides to match", dim);
        return -1;
    }
    if (order < 1 || order > 8)
    {
        setError("l3k_periodic_match: order = %d is outside 1 .. 8", order);
        return -1;
    }
    if (n_elems < 0 || n_src < 0 || n_dst < 0 || (n_elems > 0 && (!elem_nodes || !elem_verts)) ||
        (n_src > 0 && (!src_elem || !src_side || !pair_src || !pair_dst)) || (n_dst > 0 && (!dst_elem || !dst_side)))
    {
        setError("l3k_periodic_match: negative counts or null arrays with non-zero counts");
        return -1;
    }
    const int     n1 = order + 1, ns = dim == 3 ? n1 * n1 : n1;
    const int64_t slot_limit = int64_t(1) << 32; // the sort keys carry (node id, slot) in 32 bits each
    if (n_src >= slot_limit / ns || n_dst >= slot_limit / ns)
    {
        setError("l3k_periodic_match: %lld + %lld listed sides have 2^32 side nodes or more", (long long)n_src, (long long)n_dst);
        return -1;
    }
    if (!sidesInsideMesh("source", dim, n_elems, n_src, src_elem, src_side) ||
        !sidesInsideMesh("destination", dim, n_elems, n_dst, dst_elem, dst_side))
        return -1;
    if (const char* wrong = l3k::host::periodicCheckReals(dim, translation, &tolerance)) // (not here: this unit is finite-math)
    {
        setError("l3k_periodic_match: %s", wrong);
        return -1;
    }
    // the vertices of the listed sides, the box of the destination vertices and the grid over it: on the host, in a unit that is not
    // finite-math, which refuses what gives no grid before anything is launched or written
    Grid grid;
    if (const std::string wrong = l3k::host::periodicBoxAndGrid(dim, elem_verts, n_src, src_elem, n_dst, dst_elem, tolerance, &grid);
        !wrong.empty())
    {
        setError("l3k_periodic_match: %s", wrong.c_str());
        return -1;
    }
    *n_pairs = *n_unmatched = *n_ambiguous = 0;
    *first_unmatched                       = -1;
    if (n_src == 0)
        return 0;

    L3K_HIP(hipSetDevice(ctx->device));
    hipStream_t       s   = ctx->stream;
    const auto        gll = l3k::host::gllNodes(n1);
    DevBuf< double >  d_gll;
    if (int rc = d_gll.upload(gll.data(), gll.size(), s))
        return rc;
    NodeSet src, dst;
    if (int rc = uniqueSideNodes(s, dim, order, elem_nodes, elem_verts, n_src, src_elem, src_side, d_gll.ptr, src))
        return rc;
    if (int rc = uniqueSideNodes(s, dim, order, elem_nodes, elem_verts, n_dst, dst_elem, dst_side, d_gll.ptr, dst))
        return rc;
    DevBuf< uint64_t > keys, keys_sorted;
    DevBuf< uint32_t > vals, vals_sorted, partner;
    DevBuf< uint8_t >  n_qualify;
    if (dst.n > 0)
    {
        if (keys.alloc(size_t(dst.n)) || keys_sorted.alloc(size_t(dst.n)) || vals.alloc(size_t(dst.n)) || vals_sorted.alloc(size_t(dst.n)))
            return -3;
        hipLaunchKernelGGL(cellKeys, dim3(blocksFor(dst.n)), dim3(256), 0, s, dim, grid, dst.loc.ptr, dst.n, keys.ptr, vals.ptr);
        L3K_HIP(hipGetLastError());
        if (int rc = sortOnDevice(size_t(dst.n), s, keys.ptr, keys_sorted.ptr, vals.ptr, vals_sorted.ptr))
            return rc;
    }
    if (partner.alloc(size_t(src.n)) || n_qualify.alloc(size_t(src.n)))
        return -3;
    hipLaunchKernelGGL(matchNodes, dim3(blocksFor(src.n)), dim3(256), 0, s, dim, grid, translation[0], translation[1],
                       dim == 3 ? translation[2] : 0., tolerance, src.loc.ptr, src.n, keys_sorted.ptr, vals_sorted.ptr, dst.id.ptr,
                       dst.loc.ptr, dst.n, partner.ptr, n_qualify.ptr);
    L3K_HIP(hipGetLastError());
    std::vector< uint32_t > h_id(size_t(src.n)), h_partner(size_t(src.n));
    std::vector< uint8_t >  h_qualify(size_t(src.n));
    L3K_HIP(hipMemcpyAsync(h_id.data(), src.id.ptr, sizeof(uint32_t) * size_t(src.n), hipMemcpyDeviceToHost, s));
    L3K_HIP(hipMemcpyAsync(h_partner.data(), partner.ptr, sizeof(uint32_t) * size_t(src.n), hipMemcpyDeviceToHost, s));
    L3K_HIP(hipMemcpyAsync(h_qualify.data(), n_qualify.ptr, size_t(src.n), hipMemcpyDeviceToHost, s));
    L3K_HIP(hipStreamSynchronize(s));
    for (int64_t u = 0; u < src.n; ++u) // ascending in the source node id already
    {
        if (h_qualify[size_t(u)] == 0)
        {
            if (*n_unmatched == 0)
                *first_unmatched = int64_t(h_id[size_t(u)]);
            ++*n_unmatched;
            continue;
        }
        *n_ambiguous += h_qualify[size_t(u)] > 1;
        if (h_id[size_t(u)] != h_partner[size_t(u)])
        {
            pair_src[*n_pairs] = h_id[size_t(u)];
            pair_dst[*n_pairs] = h_partner[size_t(u)];
            ++*n_pairs;
        }
    }
    return 0;
}
