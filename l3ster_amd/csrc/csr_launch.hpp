// csr_launch.hpp -- what the launches of the CSR operator (api_csr.hip) and of its distributed twin (api_csr_dist.hip) share: the
// grid of a launch in which groups of lanes walk rows, the dispatch on the operator's lanes per row and the automatic choice of them.
#ifndef L3K_CSR_LAUNCH_HPP
#define L3K_CSR_LAUNCH_HPP

#include "device/csr.hpp"

#include <type_traits>

namespace l3k::csr
{
// blocks of a launch in which groups of `lanes` lanes walk n rows: at most cg_blocks, so that the partials of a reducing kernel
// fit the context's workspace
inline int csrGrid(int64_t n, int lanes)
{
    const int64_t g = (n * lanes + cg_threads - 1) / cg_threads;
    return int(g < 1 ? 1 : (g > red::cg_blocks ? red::cg_blocks : g));
}
// f(std::integral_constant< int, L >) for the operator's lanes per row
template < typename F >
int withLanes(int lanes, F&& f)
{
    switch (lanes)
    {
    case 4: return f(std::integral_constant< int, 4 >{});
    case 16: return f(std::integral_constant< int, 16 >{});
    default: return f(std::integral_constant< int, 64 >{});
    }
}
// The automatic choice from the mean length of the non-empty rows.  The cut points 8 and 64 are the starting values, NOT measured:
// DESIGN.md 4.12 says what tools/bench_csr.py has to show before they move
inline int chooseLanes(double mean_row_len)
{
    return mean_row_len <= 8. ? 4 : mean_row_len <= 64. ? 16 : 64;
}
// do the vectors [p, p + span) and [q, q + span2) share memory?
inline bool overlap(const double* p, size_t span, const double* q, size_t span2)
{
    return p < q + span2 && q < p + span;
}
} // namespace l3k::csr
#endif
