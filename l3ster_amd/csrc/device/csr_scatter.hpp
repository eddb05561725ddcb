// csr_scatter.hpp -- the device pieces every kernel shares that sums local systems into the caller's CSR arrays
// (assembledScatter*Kernel in api_assembled.hip, condensedScatterKernel in api_condense.hip, quadSplitKernel and schurProduct in
// quad_condense.hpp).  No kernels here.
//
// THE SEARCH RULE.  A wave takes one node of a local system: the U rows (node, u) of K_e, the lanes over the entries of a row.  The
// position of an entry's column in the CSR row of u = 0 is found by ONE binary search; relative to the start of the row it is the
// guess for the rows u > 0 (the rows of one node carry the same columns in a finite-element graph).  A guess is checked against
// col_ind before it is used, and a row without that structure falls back to its own search: same results on any graph.  An entry
// whose column the row does not hold is not added but counted (Tpetra's sumIntoLocalValues skips entries outside the graph and
// reports how many it took), a skipped column is neither added nor counted, and the wave's count goes to the sink's counter with
// one atomic add at the end.
#ifndef L3K_DEVICE_CSR_SCATTER_HPP
#define L3K_DEVICE_CSR_SCATTER_HPP

#include "common.hpp"

namespace l3k::dev
{
// first position in [lo, hi) with col_ind >= col
__device__ __forceinline__ int64_t csrLowerBound(const int32_t* __restrict__ col_ind, int64_t lo, int64_t hi, int64_t col)
{
    while (lo < hi)
    {
        const int64_t mid = (lo + hi) >> 1;
        if (col_ind[mid] < col)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}
// does position pos (not below the row's start) of a row that ends at re hold col?
__device__ __forceinline__ bool csrHolds(const int32_t* __restrict__ col_ind, int64_t re, int64_t pos, int64_t col)
{
    return pos < re && col_ind[pos] == col;
}
// position of col in the row [rb, re), or -1: `guess` (in [rb, ...)) is checked first, the row is searched only if it misses
__device__ __forceinline__ int64_t csrFind(const int32_t* __restrict__ col_ind, int64_t rb, int64_t re, int64_t guess, int64_t col)
{
    if (csrHolds(col_ind, re, guess, col))
        return guess;
    const int64_t pos = csrLowerBound(col_ind, rb, re, col);
    return csrHolds(col_ind, re, pos, col) ? pos : -1;
}

// where the sums go: the caller's graph, its values, its right-hand sides (column r at + r * ldr) and the counter of the entries
// outside the graph (or null)
struct CsrSink
{
    const int64_t*      row_ptr;
    const int32_t*      col_ind;
    double *            values, *rhs;
    size_t              ldr;
    unsigned long long* n_missing;
};
// the wave's count of entries outside the graph -> the sink's counter
__device__ __forceinline__ void csrCountMissing(const CsrSink& s, unsigned missing)
{
    if (missing && s.n_missing)
        atomicAdd(s.n_missing, static_cast< unsigned long long >(missing));
}

// The U global rows of one node: row[u] = node_dofs + field_inds[u]; live[u] unless the row is skipped as a Dirichlet row
// (dirichlet == nullptr: every row is live); their ranges in the graph once loadRanges has run -- after the kernel's early return
// where it has no matrix to add, so that a launch for the right-hand sides alone never reads row_ptr
template < int U >
struct NodeRows
{
    int64_t row[U], rb[U], re[U];
    bool    live[U];

    __device__ __forceinline__ NodeRows(int64_t node_dofs, const int* field_inds, const uint8_t* dirichlet, int skip)
    {
#pragma unroll
        for (int u = 0; u < U; ++u)
        {
            row[u]  = node_dofs + field_inds[u];
            live[u] = !(skip && dirichlet && dirichlet[row[u]]);
        }
    }
    __device__ __forceinline__ void loadRanges(const int64_t* __restrict__ row_ptr)
    {
#pragma unroll
        for (int u = 0; u < U; ++u)
        {
            rb[u] = row_ptr[row[u]];
            re[u] = row_ptr[row[u] + 1];
        }
    }
    // rhs[r][row[u]] += Fb[r * ldf + u] for the n_rhs right-hand sides, the lanes over (r, u), u fastest
    __device__ __forceinline__ void addRhs(const CsrSink& s, int lane, int n_rhs, const double* __restrict__ Fb, int64_t ldf) const
    {
        for (int t = lane; t < n_rhs * U; t += 64) // (n_rhs * U may exceed the wave: e.g. 17 right-hand sides of 4 unknowns)
        {
            const int r = t / U, u = t - r * U;
            bool      lv = false;
            int64_t   rw = 0;
#pragma unroll
            for (int uu = 0; uu < U; ++uu) // (compile-time indexing of the per-unknown registers)
                if (uu == u)
                {
                    lv = live[uu];
                    rw = row[uu];
                }
            if (lv)
                unsafeAtomicAdd(s.rhs + size_t(r) * s.ldr + rw, Fb[r * ldf + u]);
        }
    }
    // values[(row[u], col)] += k(u) for the live rows, by the search rule above; returns the number of entries it could not place
    template < typename ValueOfRow >
    __device__ __forceinline__ unsigned addEntry(const CsrSink& s, int64_t col, ValueOfRow&& k) const
    {
        const int64_t first = csrLowerBound(s.col_ind, rb[0], re[0], col); // the entry's one search
        unsigned      missing = 0;
#pragma unroll
        for (int u = 0; u < U; ++u)
        {
            if (!live[u])
                continue;
            const int64_t pos = u == 0 ? (csrHolds(s.col_ind, re[0], first, col) ? first : -1)
                                       : csrFind(s.col_ind, rb[u], re[u], rb[u] + (first - rb[0]), col);
            if (pos >= 0)
                unsafeAtomicAdd(s.values + pos, k(u));
            else
                ++missing;
        }
        return missing;
    }
};
} // namespace l3k::dev
#endif
