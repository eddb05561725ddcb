// The steps of l3k_periodic_match (csrc/api_periodic.hip) walked on the host: the per-item functions of device/periodic.hpp called
// in plain loops, std::sort where the library sorts on the device, and the box and the grid from the host function the library
// calls (host/periodic.hpp).  Needs no device and no library: it is compiled together with host/periodic.cpp and host/tables.cpp.
//
//     periodic_walk CASE        CASE: int64 dim, order, n_elems, n_src, n_dst; double translation[3], tolerance;
//                                     uint32 elem_nodes[n_elems][(order+1)^dim]; double elem_verts[n_elems][2^dim][3];
//                                     int64 src_elem[n_src]; uint8 src_side[n_src]; int64 dst_elem[n_dst]; uint8 dst_side[n_dst]
//
// Prints "n_pairs n_unmatched n_ambiguous first_unmatched" and one "src dst" line per pair; exit status 0.  A refusal of the
// library's (the reals, the vertices, the box, the grid) goes to stderr as the library words it, exit status 2; an unreadable
// case, exit status 3.
#include "device/periodic.hpp"
#include "host/periodic.hpp"
#include "host/tables.hpp"

#include <algorithm>
#include <cstdio>
#include <string>
#include <utility>
#include <vector>

namespace l3k::dev
{
void setError(const char*, ...) {} // (host/periodic.cpp reports the refusals of l3k_periodic_merge through it: not called here)
} // namespace l3k::dev

namespace
{
using namespace l3k::periodic;

template < typename T >
bool readInto(std::FILE* f, std::vector< T >& v, size_t n)
{
    v.resize(n);
    return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}

// The unique nodes of the listed sides, ascending in the node id, with their locations (uniqueSideNodes of the library)
struct NodeSet
{
    std::vector< uint32_t > id;
    std::vector< double >   loc;
    int64_t                 n = 0;
};

NodeSet uniqueSideNodes(int dim, int order, const uint32_t* elem_nodes, const double* elem_verts, int64_t n_sides, const int64_t* elem,
                        const uint8_t* side, const double* gll)
{
    NodeSet       out;
    const int     n1 = order + 1, ns = dim == 3 ? n1 * n1 : n1, nv = 1 << dim;
    const int64_t N = dim == 3 ? int64_t(n1) * n1 * n1 : int64_t(n1) * n1, n = n_sides * ns;
    if (n == 0)
        return out;
    std::vector< double >   verts(size_t(n_sides) * nv * 3);
    std::vector< uint32_t > ids(static_cast< size_t >(n), 0u);
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
    std::vector< double >   loc(size_t(n) * 3);
    std::vector< uint64_t > keys(static_cast< size_t >(n));
    for (int64_t t = 0; t < n; ++t)
        sideNodeLocation(t, dim, n1, ns, verts.data(), side, ids.data(), gll, loc.data(), keys.data());
    std::vector< uint64_t > sorted(keys);
    std::sort(sorted.begin(), sorted.end());
    std::vector< uint32_t > head(static_cast< size_t >(n));
    for (int64_t t = 0; t < n; ++t)
        head[size_t(t)] = startsNewId(t, sorted.data());
    for (int64_t t = 1; t < n; ++t) // the inclusive scan
        head[size_t(t)] += head[size_t(t - 1)];
    out.n = head[size_t(n - 1)];
    out.id.resize(size_t(out.n));
    out.loc.resize(size_t(out.n) * 3);
    for (int64_t t = 0; t < n; ++t)
        compactNode(t, sorted.data(), head.data(), loc.data(), out.id.data(), out.loc.data());
    return out;
}
} // namespace

int main(int argc, char** argv)
{
    std::FILE* f = argc == 2 ? std::fopen(argv[1], "rb") : nullptr;
    if (!f)
    {
        std::fputs("usage: periodic_walk CASE\n", stderr);
        return 3;
    }
    int64_t head[5];
    double  reals[4];
    if (std::fread(head, sizeof(int64_t), 5, f) != 5 || std::fread(reals, sizeof(double), 4, f) != 4)
        return 3;
    const int     dim = int(head[0]), order = int(head[1]);
    const int64_t n_elems = head[2], n_src = head[3], n_dst = head[4];
    if ((dim != 2 && dim != 3) || order < 1 || order > 8 || n_elems < 0 || n_src < 0 || n_dst < 0)
        return 3;
    const int               n1 = order + 1, nv = 1 << dim;
    const int64_t           N  = dim == 3 ? int64_t(n1) * n1 * n1 : int64_t(n1) * n1;
    std::vector< uint32_t > elem_nodes;
    std::vector< double >   elem_verts;
    std::vector< int64_t >  src_elem, dst_elem;
    std::vector< uint8_t >  src_side, dst_side;
    if (!readInto(f, elem_nodes, size_t(n_elems * N)) || !readInto(f, elem_verts, size_t(n_elems) * nv * 3) ||
        !readInto(f, src_elem, size_t(n_src)) || !readInto(f, src_side, size_t(n_src)) || !readInto(f, dst_elem, size_t(n_dst)) ||
        !readInto(f, dst_side, size_t(n_dst)))
        return 3;
    std::fclose(f);
    for (int64_t i = 0; i < n_src + n_dst; ++i)
    {
        const int64_t e = i < n_src ? src_elem[size_t(i)] : dst_elem[size_t(i - n_src)];
        const int     s = i < n_src ? src_side[size_t(i)] : dst_side[size_t(i - n_src)];
        if (e < 0 || e >= n_elems || s >= 2 * dim)
            return 3;
    }
    const double* translation = reals;
    const double  tolerance   = reals[3];
    if (const char* wrong = l3k::host::periodicCheckReals(dim, translation, &tolerance))
    {
        std::fprintf(stderr, "l3k_periodic_match: %s\n", wrong);
        return 2;
    }
    Grid grid;
    if (const std::string wrong = l3k::host::periodicBoxAndGrid(dim, elem_verts.data(), n_src, src_elem.data(), n_dst, dst_elem.data(),
                                                               tolerance, &grid);
        !wrong.empty())
    {
        std::fprintf(stderr, "l3k_periodic_match: %s\n", wrong.c_str());
        return 2;
    }
    int64_t n_pairs = 0, n_unmatched = 0, n_ambiguous = 0, first_unmatched = -1;
    std::vector< std::pair< uint32_t, uint32_t > > pairs;
    if (n_src > 0)
    {
        const auto    gll = l3k::host::gllNodes(n1);
        const NodeSet src = uniqueSideNodes(dim, order, elem_nodes.data(), elem_verts.data(), n_src, src_elem.data(), src_side.data(),
                                            gll.data());
        const NodeSet dst = uniqueSideNodes(dim, order, elem_nodes.data(), elem_verts.data(), n_dst, dst_elem.data(), dst_side.data(),
                                            gll.data());
        std::vector< std::pair< uint64_t, uint32_t > > cells(static_cast< size_t >(dst.n)); // (cell key, destination node)
        for (int64_t t = 0; t < dst.n; ++t)
            cells[size_t(t)] = {cellKey(t, dim, grid, dst.loc.data()), uint32_t(t)};
        std::sort(cells.begin(), cells.end());
        std::vector< uint64_t > dkeys(static_cast< size_t >(dst.n));
        std::vector< uint32_t > dvals(static_cast< size_t >(dst.n));
        for (int64_t t = 0; t < dst.n; ++t)
            dkeys[size_t(t)] = cells[size_t(t)].first, dvals[size_t(t)] = cells[size_t(t)].second;
        const double            t3[3] = {translation[0], translation[1], dim == 3 ? translation[2] : 0.};
        std::vector< uint32_t > partner(static_cast< size_t >(src.n));
        std::vector< uint8_t >  n_qualify(static_cast< size_t >(src.n));
        for (int64_t t = 0; t < src.n; ++t)
            matchNode(t, dim, grid, t3, tolerance, src.loc.data(), dkeys.data(), dvals.data(), dst.id.data(), dst.loc.data(), dst.n,
                      partner.data(), n_qualify.data());
        for (int64_t u = 0; u < src.n; ++u) // the tally of the library: ascending in the source node id already
        {
            if (n_qualify[size_t(u)] == 0)
            {
                if (n_unmatched == 0)
                    first_unmatched = int64_t(src.id[size_t(u)]);
                ++n_unmatched;
                continue;
            }
            n_ambiguous += n_qualify[size_t(u)] > 1;
            if (src.id[size_t(u)] != partner[size_t(u)])
            {
                pairs.emplace_back(src.id[size_t(u)], partner[size_t(u)]);
                ++n_pairs;
            }
        }
    }
    std::printf("%lld %lld %lld %lld\n", (long long)n_pairs, (long long)n_unmatched, (long long)n_ambiguous, (long long)first_unmatched);
    for (const auto& [s, d] : pairs)
        std::printf("%u %u\n", s, d);
    return 0;
}
