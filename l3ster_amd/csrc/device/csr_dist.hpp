// csr_dist.hpp -- kernels of the distributed CSR operator (include/l3k.h: l3k_csr_dist_*): the local matrix A_r of one rank over
// its local dofs [owned | ghost] applied as its share of A = sum_r R_r^T A_r R_r (the sub-assembled form).  The
// rows of A_r fall into three classes -- interior (owned, every column owned), border (owned, some ghost column), ghost -- kept
// as ascending row lists; an apply walks a list, or a slice of one, with csrApplyKernel's scheme (csr.hpp) on a vector that is
// split into its owned and its ghost part.
//
// As in csr.hpp nothing accumulates atomically into floating-point data: a row has one writer and the lanes of a row are
// combined by the same fixed butterfly, so a row of a world of one rank gets the bits l3k_csr_apply gives it.  The row lists
// are built by an ordered compaction (block counts, a scan of them, ordered writes): their content does not depend on the
// order in which anything lands.
#ifndef L3K_DEVICE_CSR_DIST_HPP
#define L3K_DEVICE_CSR_DIST_HPP

#include "csr.hpp"

namespace l3k::csr
{
enum RowClass : int
{
    row_interior = 0,
    row_border   = 1,
    row_ghost    = 2,
    n_row_classes
};
// the class of row i: the columns of a row ascend, so its last one decides whether it holds a ghost column; an empty owned row is
// interior
__device__ __forceinline__ int rowClass(const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ col_ind, int64_t i, int64_t n_owned)
{
    if (i >= n_owned)
        return row_ghost;
    const int64_t b = row_ptr[i], e = row_ptr[i + 1];
    return e > b && col_ind[e - 1] >= n_owned ? row_border : row_interior;
}
// rows [block * chunk, (block + 1) * chunk) belong to a block, in both kernels below (chunk: a multiple of cg_threads)
// first kernel: counts[block][class]
static __global__ __launch_bounds__(cg_threads) void csrRowClassCountKernel(const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ col_ind,
                                                                            int64_t n, int64_t n_owned, int64_t chunk, int* __restrict__ counts)
{
    __shared__ int sh[n_row_classes];
    if (threadIdx.x < n_row_classes)
        sh[threadIdx.x] = 0;
    __syncthreads();
    const int64_t begin = int64_t(blockIdx.x) * chunk, end = begin + chunk < n ? begin + chunk : n;
    int           mine[n_row_classes] = {0, 0, 0};
    for (int64_t i = begin + threadIdx.x; i < end; i += cg_threads)
        ++mine[rowClass(row_ptr, col_ind, i, n_owned)];
    for (int c = 0; c < n_row_classes; ++c)
        if (mine[c])
            atomicAdd(sh + c, mine[c]); // (integers: the sum does not depend on the order)
    __syncthreads();
    if (threadIdx.x < n_row_classes)
        counts[blockIdx.x * n_row_classes + threadIdx.x] = sh[threadIdx.x];
}
// second kernel, one thread: counts[block][class] <- the position of the block's first row of the class in its list;
// totals[class] <- the length of the list (at most cg_blocks blocks)
static __global__ void csrRowClassScanKernel(int* __restrict__ counts, int n_blocks, int* __restrict__ totals)
{
    if (blockIdx.x != 0 || threadIdx.x != 0)
        return;
    for (int c = 0; c < n_row_classes; ++c)
    {
        int at = 0;
        for (int b = 0; b < n_blocks; ++b)
        {
            const int k                   = counts[b * n_row_classes + c];
            counts[b * n_row_classes + c] = at;
            at += k;
        }
        totals[c] = at;
    }
}
// exclusive prefix sum of v over the block's threads, `total` their sum (sh: cg_threads ints)
__device__ __forceinline__ int blockExclusiveScan(int v, int* __restrict__ sh, int& total)
{
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int d = 1; d < cg_threads; d <<= 1)
    {
        const int t = threadIdx.x >= d ? sh[threadIdx.x - d] : 0;
        __syncthreads();
        sh[threadIdx.x] += t;
        __syncthreads();
    }
    total           = sh[cg_threads - 1];
    const int before = sh[threadIdx.x] - v;
    __syncthreads();
    return before;
}
// third kernel: the rows of every class written in ascending order behind the offsets of the scan (lists[c]: the list of class c)
static __global__ __launch_bounds__(cg_threads) void csrRowClassFillKernel(const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ col_ind,
                                                                           int64_t n, int64_t n_owned, int64_t chunk,
                                                                           const int* __restrict__ offsets, int32_t* __restrict__ list0,
                                                                           int32_t* __restrict__ list1, int32_t* __restrict__ list2)
{
    __shared__ int sh[cg_threads];
    int32_t* const lists[n_row_classes] = {list0, list1, list2};
    int            at[n_row_classes];
    for (int c = 0; c < n_row_classes; ++c)
        at[c] = offsets[blockIdx.x * n_row_classes + c];
    const int64_t begin = int64_t(blockIdx.x) * chunk, end = begin + chunk < n ? begin + chunk : n;
    for (int64_t tile = begin; tile < end; tile += cg_threads) // (uniform over the block: every thread meets every barrier)
    {
        const int64_t i   = tile + threadIdx.x;
        const int     cls = i < end ? rowClass(row_ptr, col_ind, i, n_owned) : -1;
        for (int c = 0; c < n_row_classes; ++c)
        {
            int       total  = 0;
            const int before = blockExclusiveScan(cls == c ? 1 : 0, sh, total);
            if (cls == c)
                lists[c][at[c] + before] = int32_t(i);
            at[c] += total;
        }
    }
}

// csrApplyKernel (csr.hpp) over the rows rows[0 .. n_rows) of the local matrix, on split vectors: column j reads x[j] where
// j < n_owned, xg[j - n_owned] otherwise; row i writes y[i] <- alpha (A x)_i + beta y[i] where i < n_owned (beta == 0: y is not
// read) and yg[i - n_owned] <- alpha (A x)_i otherwise -- a ghost row is this rank's share of its owner's row: it goes into the
// export buffer, which therefore needs no zeroing, an empty ghost row stores alpha 0.  SPLIT = false: the rows of the interior
// list, whose columns and rows are all owned -- xg and yg are not touched.  Same lanes, loads, accumulators and butterfly as
// csrApplyKernel: the same bits per row.
// WITH_DOT (the interior list, NC = 1, n_rows > 0; l3k_csr_dist_apply_energy): the block sums of x_i y_i over the launch's rows go
// to partial[blockIdx.x], for cgFinishKernel -- csrApplyKernel's WITH_DOT on a row list; y is stored as without it
template < int L, int NC, bool SPLIT, bool WITH_DOT = false >
__global__ __launch_bounds__(cg_threads) void csrDistApplyKernel(const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ col_ind,
                                                                 const double* __restrict__ values, const int32_t* __restrict__ rows,
                                                                 int64_t n_rows, int64_t n_owned, const double* __restrict__ x, size_t ldx,
                                                                 const double* __restrict__ xg, size_t ldxg, double* __restrict__ y,
                                                                 size_t ldy, double* __restrict__ yg, size_t ldyg, double alpha, double beta,
                                                                 double* __restrict__ partial = nullptr)
{
    static_assert(!WITH_DOT || (NC == 1 && !SPLIT));
    const int     lane   = threadIdx.x % L;
    const int64_t groups = int64_t(gridDim.x) * (cg_threads / L);
    int64_t       r      = (int64_t(blockIdx.x) * cg_threads + threadIdx.x) / L;
    double        dot[1] = {0.};
    // The list entry of the group's NEXT row is fetched while the current row is walked, by an unconditional load (the last row
    // names itself again), and is turned into the next row's address BEFORE the current row's store: the top of the loop then
    // issues the row_ptr load at once and one wait covers it and the store, as in csrApplyKernel.  (The wait counter of loads and
    // stores is one in-order counter here: a value consumed behind the store costs the store's round trip on every row.)
    const bool idle = r >= n_rows;
    if constexpr (!WITH_DOT)
        if (idle)
            return;
    int32_t i_first = rows[idle ? 0 : r]; // (WITH_DOT: a group without a row stays for the barriers of the block sum)
    asm volatile("" : "+v"(i_first)); // (awaited ahead of the loop, so that the loop's head waits for nothing)
    const int64_t* rp = row_ptr + i_first;
    for (; r < n_rows; r += groups)
    {
        const int64_t i      = rp - row_ptr;
        int32_t       i_next = rows[r + groups < n_rows ? r + groups : r];
        const int64_t e      = rp[1];
        double        xi     = 0.; // (WITH_DOT: x_i is fetched with the row, ahead of the store -- a load behind it would wait for it)
        if constexpr (WITH_DOT)
            xi = x[i];
        double acc[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c)
            acc[c] = 0.;
        for (int64_t k = rp[0] + lane; k < e; k += L)
        {
            const int64_t j = __builtin_nontemporal_load(col_ind + k);
            const double  a = __builtin_nontemporal_load(values + k);
            if (!SPLIT || j < n_owned)
            {
#pragma unroll
                for (int c = 0; c < NC; ++c)
                    acc[c] += a * x[c * ldx + j];
            }
            else
            {
#pragma unroll
                for (int c = 0; c < NC; ++c)
                    acc[c] += a * xg[c * ldxg + (j - n_owned)];
            }
        }
#pragma unroll
        for (int c = 0; c < NC; ++c)
            acc[c] = groupSum< L >(acc[c]);
        asm volatile("" : "+v"(i_next)); // (no instruction: the value is awaited HERE, ahead of the store)
        rp = row_ptr + i_next;
        if (lane == 0)
        {
            if constexpr (WITH_DOT)
                dot[0] += xi * (alpha * acc[0]); // (alpha = 1, beta = 0: x_i times the value stored below)
            if (SPLIT && i >= n_owned)
            {
#pragma unroll
                for (int c = 0; c < NC; ++c)
                    yg[c * ldyg + (i - n_owned)] = alpha * acc[c];
            }
            else if (beta == 0.)
            {
#pragma unroll
                for (int c = 0; c < NC; ++c)
                    y[c * ldy + i] = alpha * acc[c];
            }
            else
            {
#pragma unroll
                for (int c = 0; c < NC; ++c)
                    y[c * ldy + i] = alpha * acc[c] + beta * y[c * ldy + i];
            }
        }
    }
    if constexpr (WITH_DOT)
    {
        __shared__ double sh[cg_threads];
        red::storePartials(dot, sh, partial);
    }
}
// An INTERIOR row that a neighbour holds as a ghost row is completed by the unpack-add as well -- after its x_i y_i went into the
// row kernel's sum.  What it still lacks is x_i times what one neighbour's message added: block sums over that message (rows: the
// neighbour's send list, vals: the received values, n of each) into partial[blockIdx.x].  A border row of the list is left out:
// the border pass reads its final y
static __global__ __launch_bounds__(cg_threads) void csrDistReceivedDotKernel(const int64_t* __restrict__ row_ptr,
                                                                              const int32_t* __restrict__ col_ind, int64_t n_owned,
                                                                              const int32_t* __restrict__ rows, const double* __restrict__ vals,
                                                                              int64_t n, const double* __restrict__ x,
                                                                              double* __restrict__ partial)
{
    __shared__ double sh[cg_threads];
    double            dot[1] = {0.};
    for (int64_t k = int64_t(blockIdx.x) * cg_threads + threadIdx.x; k < n; k += int64_t(gridDim.x) * cg_threads)
    {
        const int64_t i = rows[k];
        if (rowClass(row_ptr, col_ind, i, n_owned) == row_interior)
            dot[0] += x[i] * vals[k];
    }
    red::storePartials(dot, sh, partial);
}
// the border rows' share of <x, y> once y is complete there (behind the unpack-add): block sums of x_i y_i over the border list
// into partial[blockIdx.x].  Reads x and y at border rows only
static __global__ __launch_bounds__(cg_threads) void csrDistBorderDotKernel(const int32_t* __restrict__ rows, int64_t n_rows,
                                                                            const double* __restrict__ x, const double* __restrict__ y,
                                                                            double* __restrict__ partial)
{
    __shared__ double sh[cg_threads];
    double            dot[1] = {0.};
    for (int64_t r = int64_t(blockIdx.x) * cg_threads + threadIdx.x; r < n_rows; r += int64_t(gridDim.x) * cg_threads)
    {
        const int64_t i = rows[r];
        dot[0] += x[i] * y[i];
    }
    red::storePartials(dot, sh, partial);
}

// the local diagonal over [owned | ghost]: csrDiagKernel's a_ii (0 where none is stored), the owned rows into diag, the ghost rows
// into diag_ghost (this rank's share of its owners' diagonal, for the export)
static __global__ __launch_bounds__(cg_threads) void csrDistDiagKernel(const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ col_ind,
                                                                       const double* __restrict__ values, int64_t n, int64_t n_owned,
                                                                       double* __restrict__ diag, double* __restrict__ diag_ghost)
{
    for (int64_t i = int64_t(blockIdx.x) * cg_threads + threadIdx.x; i < n; i += int64_t(gridDim.x) * cg_threads)
    {
        const int64_t k = findColumn(col_ind, row_ptr[i], row_ptr[i + 1], i);
        const double  v = k >= 0 ? values[k] : 0.;
        if (i < n_owned)
            diag[i] = v;
        else
            diag_ghost[i - n_owned] = v;
    }
}
// ... and, behind the export, csrDiagKernel's formula on the summed diagonal of the owned rows: minv = 0 on an empty owned row
static __global__ __launch_bounds__(cg_threads) void csrDistMinvKernel(const int64_t* __restrict__ row_ptr, int64_t n_owned,
                                                                       const double* __restrict__ diag, double damping, double threshold,
                                                                       double* __restrict__ minv)
{
    for (int64_t i = int64_t(blockIdx.x) * cg_threads + threadIdx.x; i < n_owned; i += int64_t(gridDim.x) * cg_threads)
    {
        const double v = diag[i], a = fabs(v);
        minv[i]        = row_ptr[i + 1] > row_ptr[i] ? (v < 0. ? -damping : damping) / (a > threshold ? a : threshold) : 0.;
    }
}

// l3k_csr_dirichlet_dist, first kernel: the smallest flagged OWNED row without a stored diagonal (a flagged ghost row needs none:
// it becomes a zero row)
static __global__ __launch_bounds__(cg_threads) void csrDistDirichletCheckKernel(const int64_t* __restrict__ row_ptr,
                                                                                 const int32_t* __restrict__ col_ind, int64_t n_owned,
                                                                                 const uint8_t* __restrict__ mask,
                                                                                 unsigned long long* __restrict__ flag)
{
    for (int64_t i = int64_t(blockIdx.x) * cg_threads + threadIdx.x; i < n_owned; i += int64_t(gridDim.x) * cg_threads)
        if (mask[i] && findColumn(col_ind, row_ptr[i], row_ptr[i + 1], i) < 0)
            atomicMin(flag, static_cast< unsigned long long >(i));
}
// ... second kernel: csrDirichletKernel with the owner rule.  A flagged owned row becomes the identity row and its rhs the
// prescribed value; a flagged ghost row becomes an all-zero row with rhs 0 -- the owner holds the 1 and the value; an unflagged
// row, owned or ghost, gives rhs -= a_ij g_j over its flagged columns j (owned or ghost: g is over the local dofs) in
// csrDirichletKernel's fixed order and zeroes those entries.  Summed over the ranks this is DirichletBCAlgebraic::apply
// (bcs/DirichletBC.hpp:82-150) on the global matrix
template < int L >
__global__ __launch_bounds__(cg_threads) void csrDistDirichletKernel(const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ col_ind,
                                                                     double* __restrict__ values, int64_t n, int64_t n_owned,
                                                                     const uint8_t* __restrict__ mask, const double* __restrict__ g,
                                                                     size_t ldg, double* __restrict__ rhs, size_t ldr, int ncols)
{
    const int     lane   = threadIdx.x % L;
    const int64_t groups = int64_t(gridDim.x) * (cg_threads / L);
    for (int64_t i = (int64_t(blockIdx.x) * cg_threads + threadIdx.x) / L; i < n; i += groups)
    {
        const int64_t b = row_ptr[i], e = row_ptr[i + 1];
        if (mask[i])
        {
            const bool owned = i < n_owned;
            for (int64_t k = b + lane; k < e; k += L)
                values[k] = owned && col_ind[k] == i ? 1. : 0.;
            for (int c = lane; c < ncols; c += L)
                rhs[c * ldr + i] = owned ? g[c * ldg + i] : 0.;
            continue;
        }
        for (int c = 0; c < ncols; ++c)
        {
            double acc = 0.;
            for (int64_t k = b + lane; k < e; k += L)
            {
                const int64_t j = col_ind[k];
                if (mask[j])
                    acc += values[k] * g[c * ldg + j];
            }
            acc = groupSum< L >(acc);
            if (lane == 0)
                rhs[c * ldr + i] -= acc;
        }
        for (int64_t k = b + lane; k < e; k += L)
            if (mask[col_ind[k]])
                values[k] = 0.;
    }
}
} // namespace l3k::csr
#endif
