// chol_symbolic.cpp -- the symbolic phase of the band Cholesky solver and its host-only entry point l3k_chol_order (the reference
// hands this phase to Amesos2: preOrdering + symbolicFactorization on the first call, solve/Amesos2Solvers.hpp:18-32).
//
// 1. Active rows: the rows that store an entry.  Empty rows (internal dofs of a condensed graph, dofs outside field_inds) stay out.
// 2. Structural symmetry: every stored (i, j) needs a stored (j, i); the first pair without one, in row-major order, is refused.
// 3. Reverse Cuthill-McKee, component by component in ascending order of each component's lowest row.  A component starts from a
//    pseudo-peripheral node: from its lowest row r, repeat { c = the node of the last BFS level of r with the lowest (degree,
//    index); if the BFS from c is deeper than the one from r, r = c and again } and keep r.  The Cuthill-McKee pass appends the
//    unnumbered neighbours of each numbered node in ascending (degree, index).  The concatenated order is reversed as a whole.
//    degree = stored off-diagonal entries of the row.  Nothing depends on addresses or hashing: same input, same permutation.
// 4. Blocks of nb x nb.  H(K) = E(K) - K with E(K) = max(E(K - 1), K + the lowest block row below which block column K of the
//    permuted lower triangle stores nothing): the monotone envelope, closed under Cholesky fill.
#include "host/chol_symbolic.hpp"
#include "l3k.h"

#include <algorithm>
#include <new>
#include <utility>

namespace l3k::dev
{
void setError(const char* fmt, ...);
}

namespace l3k::host
{
namespace
{
using l3k::dev::setError;

int checkGraph(int64_t n, const int64_t* row_ptr, const int32_t* col_ind, const char* who)
{
    if (n < 0 || n > INT32_MAX || !row_ptr)
    {
        setError("%s: need 0 <= n < 2^31 and a row_ptr", who);
        return -1;
    }
    if (row_ptr[0] != 0)
    {
        setError("%s: row_ptr[0] is not 0", who);
        return -1;
    }
    for (int64_t i = 0; i < n; ++i)
    {
        if (row_ptr[i + 1] < row_ptr[i])
        {
            setError("%s: row_ptr decreases at row %lld", who, (long long)i);
            return -1;
        }
        if (row_ptr[i + 1] > row_ptr[i] && !col_ind)
        {
            setError("%s: null col_ind for a graph with entries", who);
            return -1;
        }
        for (int64_t e = row_ptr[i]; e < row_ptr[i + 1]; ++e)
            if (col_ind[e] < 0 || col_ind[e] >= n || (e > row_ptr[i] && col_ind[e] <= col_ind[e - 1]))
            {
                setError("%s: the columns of row %lld are not strictly ascending inside [0, n)", who, (long long)i);
                return -1;
            }
    }
    return 0;
}

struct Graph
{
    int64_t                 n;
    const int64_t*          row_ptr;
    const int32_t*          col_ind;
    std::vector< int32_t >  degree;
    std::vector< uint32_t > mark; // BFS stamps
    uint32_t                stamp = 0;

    // BFS from root over nodes not yet numbered: `nodes` in visiting order, level l = nodes[starts[l] .. starts[l + 1])
    void levels(int32_t root, const std::vector< uint8_t >& numbered, std::vector< int32_t >& nodes, std::vector< int64_t >& starts)
    {
        ++stamp;
        nodes.clear();
        starts.clear();
        nodes.push_back(root);
        mark[size_t(root)] = stamp;
        starts.push_back(0);
        size_t begin = 0;
        while (begin < nodes.size())
        {
            const size_t end = nodes.size();
            for (size_t q = begin; q < end; ++q)
            {
                const int32_t v = nodes[q];
                for (int64_t e = row_ptr[v]; e < row_ptr[v + 1]; ++e)
                {
                    const int32_t w = col_ind[e];
                    if (w != v && mark[size_t(w)] != stamp && !numbered[size_t(w)])
                    {
                        mark[size_t(w)] = stamp;
                        nodes.push_back(w);
                    }
                }
            }
            starts.push_back(int64_t(end));
            begin = end;
        }
        // the loop pushed one boundary per level; the last is the end of the list
    }
    bool before(int32_t a, int32_t b) const // ascending (degree, index)
    {
        return degree[size_t(a)] != degree[size_t(b)] ? degree[size_t(a)] < degree[size_t(b)] : a < b;
    }
};
} // namespace

int cholSymbolic(int64_t n, const int64_t* row_ptr, const int32_t* col_ind, int block, CholSymbolic& out, const char* who)
{
    if (block != 0 && block != 32 && block != 64)
    {
        setError("%s: block = %d; it is 0 (choose), 32 or 64", who, block);
        return -1;
    }
    if (int rc = checkGraph(n, row_ptr, col_ind, who))
        return rc;
    try
    {
        out   = CholSymbolic{};
        out.n = n;
        // ---- structural symmetry
        for (int64_t i = 0; i < n; ++i)
            for (int64_t e = row_ptr[i]; e < row_ptr[i + 1]; ++e)
            {
                const int32_t  j  = col_ind[e];
                const int32_t *lo = col_ind + row_ptr[j], *hi = col_ind + row_ptr[j + 1];
                if (j != i && !std::binary_search(lo, hi, int32_t(i)))
                {
                    setError("%s: the graph is not structurally symmetric: (%lld, %d) is stored and (%d, %lld) is not", who, (long long)i, j,
                             j, (long long)i);
                    return -1;
                }
            }
        // ---- reverse Cuthill-McKee over the active rows
        Graph g{n, row_ptr, col_ind, {}, {}, 0};
        g.degree.assign(size_t(n), 0);
        g.mark.assign(size_t(n), 0);
        for (int64_t i = 0; i < n; ++i)
        {
            int32_t d = 0;
            for (int64_t e = row_ptr[i]; e < row_ptr[i + 1]; ++e)
                d += col_ind[e] != i;
            g.degree[size_t(i)] = d;
        }
        std::vector< uint8_t >  numbered(size_t(n), 0);
        std::vector< int32_t >  order, nodes, nodes2, nbrs;
        std::vector< int64_t >  starts, starts2;
        for (int64_t s = 0; s < n; ++s)
        {
            if (numbered[size_t(s)] || row_ptr[s + 1] == row_ptr[s])
                continue;
            int32_t r = int32_t(s);
            g.levels(r, numbered, nodes, starts);
            for (;;)
            {
                const size_t nl = starts.size() - 1; // levels of the BFS from r
                int32_t      c  = nodes[size_t(starts[nl - 1])];
                for (int64_t q = starts[nl - 1]; q < starts[nl]; ++q)
                    if (g.before(nodes[size_t(q)], c))
                        c = nodes[size_t(q)];
                if (c == r)
                    break;
                g.levels(c, numbered, nodes2, starts2);
                if (starts2.size() <= starts.size())
                    break;
                r = c;
                nodes.swap(nodes2);
                starts.swap(starts2);
            }
            size_t head = order.size();
            order.push_back(r);
            numbered[size_t(r)] = 1;
            while (head < order.size())
            {
                const int32_t v = order[head++];
                nbrs.clear();
                for (int64_t e = row_ptr[v]; e < row_ptr[v + 1]; ++e)
                    if (!numbered[size_t(col_ind[e])])
                        nbrs.push_back(col_ind[e]);
                std::sort(nbrs.begin(), nbrs.end(), [&](int32_t a, int32_t b) { return g.before(a, b); });
                for (int32_t w : nbrs)
                {
                    numbered[size_t(w)] = 1;
                    order.push_back(w);
                }
            }
        }
        std::reverse(order.begin(), order.end());
        out.n_active = int64_t(order.size());
        out.inv.assign(size_t(n), -1);
        for (size_t k = 0; k < order.size(); ++k)
            out.inv[size_t(order[k])] = int32_t(k);
        out.perm = std::move(order);
        // ---- block size and the monotone envelope
        int64_t reach = 0; // the largest distance of a stored entry from the diagonal after the ordering
        for (int64_t i = 0; i < n; ++i)
            for (int64_t e = row_ptr[i]; e < row_ptr[i + 1]; ++e)
                reach = std::max(reach, int64_t(out.inv[size_t(i)]) - int64_t(out.inv[size_t(col_ind[e])]));
        const int nb = block ? block : (reach >= 64 ? 64 : 32);
        out.nb       = nb;
        out.n_blocks = (out.n_active + nb - 1) / nb;
        out.heights.assign(size_t(out.n_blocks), 0);
        for (int64_t i = 0; i < n; ++i)
            for (int64_t e = row_ptr[i]; e < row_ptr[i + 1]; ++e)
            {
                const int64_t bi = out.inv[size_t(i)] / nb, bj = out.inv[size_t(col_ind[e])] / nb;
                if (bi > bj && bi - bj > out.heights[size_t(bj)])
                    out.heights[size_t(bj)] = int32_t(bi - bj);
            }
        out.col_off.assign(size_t(out.n_blocks) + 1, 0);
        int64_t     end  = 0; // E(K - 1)
        const double nb3 = double(nb) * nb * nb;
        for (int64_t k = 0; k < out.n_blocks; ++k)
        {
            end                     = std::max(end, k + out.heights[size_t(k)]);
            const int64_t h         = end - k;
            out.heights[size_t(k)]  = int32_t(h);
            out.max_height          = std::max(out.max_height, h);
            out.col_off[size_t(k) + 1] = out.col_off[size_t(k)] + 1 + h;
            const double upd        = double(h) * double(h + 1) * nb3; // h (h + 1) / 2 block products of 2 nb^3
            out.update_flops += upd;
            out.factor_flops += nb3 / 3. + double(h) * nb3 + upd;
        }
        out.total_blocks = out.col_off[size_t(out.n_blocks)];
        out.factor_bytes = size_t(out.total_blocks) * size_t(nb) * size_t(nb) * sizeof(double);
    }
    catch (const std::bad_alloc&)
    {
        setError("%s: out of host memory in the symbolic phase", who);
        return -3;
    }
    return 0;
}

int cholCheckBytes(const CholSymbolic& s, size_t max_bytes, const char* who)
{
    if (max_bytes == 0 || s.factor_bytes <= max_bytes)
        return 0;
    setError("%s: the factor needs %zu bytes (%lld blocks of %d x %d, largest H = %lld), more than max_bytes = %zu; nothing was allocated",
             who, s.factor_bytes, (long long)s.total_blocks, s.nb, s.nb, (long long)s.max_height, max_bytes);
    return -1;
}
} // namespace l3k::host

extern "C" int l3k_chol_order(int64_t n, const int64_t* row_ptr, const int32_t* col_ind, int32_t* perm_out, int32_t* heights_out, int* nb,
                              int64_t* n_active, size_t* bytes)
{
    using l3k::dev::setError;
    if (!nb || !n_active || !bytes || (n > 0 && (!perm_out || !heights_out)))
    {
        setError("l3k_chol_order: null argument");
        return -1;
    }
    l3k::host::CholSymbolic s;
    if (int rc = l3k::host::cholSymbolic(n, row_ptr, col_ind, *nb, s, "l3k_chol_order"))
        return rc;
    const size_t limit = *bytes;
    *nb                = s.nb;
    *n_active          = s.n_active;
    *bytes             = s.factor_bytes;
    if (int rc = l3k::host::cholCheckBytes(s, limit, "l3k_chol_order"))
        return rc;
    for (int64_t i = 0; i < n; ++i)
        perm_out[i] = i < s.n_active ? s.perm[size_t(i)] : -1;
    std::copy(s.heights.begin(), s.heights.end(), heights_out);
    return 0;
}
