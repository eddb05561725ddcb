// l3k::periodicMerge and l3k::periodicMatch of include/l3k/operator.hpp.  Without arguments: the host-only merge on two quads side
// by side, periodic left -> right (needs no device).  With the argument "match": also the match on the device, on the same mesh.
#include "l3k/operator.hpp"

#include <cstdio>
#include <cstring>

int main(int argc, char** argv)
{
    // nodes 0 1 2 / 3 4 5: two order-1 quads (v = i + 2j) of [0,2] x [0,1]
    std::vector< uint32_t >     elem_nodes{0, 1, 3, 4, 1, 2, 4, 5};
    const std::vector< double > elem_verts{0, 0, 0, 1, 0, 0, 0, 1, 0, 1, 1, 0, 1, 0, 0, 2, 0, 0, 1, 1, 0, 2, 1, 0};
    std::vector< uint32_t >     a{0, 3}, b{2, 5};
    if (argc > 1 && !std::strcmp(argv[1], "match"))
    {
        l3k::Context               ctx{0};
        const std::vector< int64_t > se{0}, de{1};
        const std::vector< uint8_t > ss{2}, ds{3}; // x- of the left quad onto x+ of the right one
        const auto pairs = l3k::periodicMatch(ctx, 2, 1, elem_nodes, elem_verts, se, ss, de, ds, {2., 0., 0.});
        if (pairs.src != a || pairs.dst != b || pairs.n_unmatched || pairs.n_ambiguous || pairs.first_unmatched != -1)
        {
            std::puts("periodicMatch: wrong pairs");
            return 1;
        }
        a = pairs.src, b = pairs.dst;
    }
    int64_t    n_nodes = 6, n_noninternal = 6, n_components = 0;
    const auto node_map = l3k::periodicMerge(elem_nodes, n_nodes, n_noninternal, a, b, &n_components);
    const bool ok = node_map == std::vector< uint32_t >{0, 1, 0, 2, 3, 2} && elem_nodes == std::vector< uint32_t >{0, 1, 2, 3, 1, 0, 3, 2} &&
                    n_nodes == 4 && n_noninternal == 4 && n_components == 2;
    bool threw = false;
    try
    {
        const std::vector< uint32_t > outside{9};
        l3k::periodicMerge(elem_nodes, n_nodes, n_noninternal, outside, outside);
    }
    catch (const std::runtime_error& e)
    {
        threw = std::strstr(e.what(), "l3k_periodic_merge") != nullptr;
    }
    std::puts(ok && threw ? "OK" : "FAILED");
    return ok && threw ? 0 : 1;
}
