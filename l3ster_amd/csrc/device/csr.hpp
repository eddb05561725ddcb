// csr.hpp -- kernels of the device CSR operator (include/l3k.h: l3k_csr_*): validation, y <- alpha A x + beta y, diagonal,
// algebraic Dirichlet conditions.  row_ptr int64 [n + 1], col_ind int32 ascending within a row, values double: the format of
// l3k_assembled_scatter.
//
// Nothing in here accumulates atomically into floating-point data: a row has one writer, the lanes of a row are combined by a
// fixed butterfly and <x, A x> goes through the two-stage reduction of the PCG.  Applies, and with them the solves on a CSR
// operator, are therefore bitwise reproducible on ANY context -- the deterministic mode of l3k_ctx concerns element launches only.
#ifndef L3K_DEVICE_CSR_HPP
#define L3K_DEVICE_CSR_HPP

#include "reduce.hpp"

namespace l3k::csr
{
using red::cg_threads;

// the word a checking kernel reports through: the smallest key wins, so the offence named is the first one in (row, kind) order
constexpr unsigned long long no_offence = ~0ull;
enum Offence : unsigned
{
    first_row_ptr_not_zero = 1,
    row_ptr_decreasing     = 2,
    column_out_of_range    = 3,
    columns_not_ascending  = 4,
};
__device__ __forceinline__ void report(unsigned long long* flag, int64_t row, unsigned what)
{
    atomicMin(flag, static_cast< unsigned long long >(row) * 8ull + what);
}
// flag[0] offence key, flag[1] empty rows, flag[2] longest row, flag[3] nnz = row_ptr[n]
constexpr int flag_words = 4;

// first pass of the validation: row_ptr alone (nothing is read through it), and the row statistics of l3k_csr_info
static __global__ __launch_bounds__(cg_threads) void csrCheckRowsKernel(const int64_t* __restrict__ row_ptr, int64_t n,
                                                                        unsigned long long* __restrict__ flag)
{
    const int64_t t = int64_t(blockIdx.x) * cg_threads + threadIdx.x;
    if (t == 0)
    {
        if (row_ptr[0] != 0)
            report(flag, 0, first_row_ptr_not_zero);
        flag[3] = static_cast< unsigned long long >(row_ptr[n]);
    }
    unsigned long long empty = 0, longest = 0;
    for (int64_t i = t; i < n; i += int64_t(gridDim.x) * cg_threads)
    {
        const int64_t b = row_ptr[i], e = row_ptr[i + 1];
        if (e < b)
        {
            report(flag, i, row_ptr_decreasing);
            continue;
        }
        empty += e == b;
        longest = static_cast< unsigned long long >(e - b) > longest ? static_cast< unsigned long long >(e - b) : longest;
    }
    if (empty)
        atomicAdd(flag + 1, empty);
    if (longest)
        atomicMax(flag + 2, longest);
}
// second pass, on the same stream: does nothing unless row_ptr passed -- only then is every k in [row_ptr[i], row_ptr[i + 1]) an
// index into col_ind.  16 lanes walk a row
static __global__ __launch_bounds__(cg_threads) void csrCheckColsKernel(const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ col_ind,
                                                                        int64_t n, unsigned long long* __restrict__ flag)
{
    constexpr int L = 16;
    if (*static_cast< volatile unsigned long long* >(flag) != no_offence)
        return;
    const int     lane   = threadIdx.x % L;
    const int64_t groups = int64_t(gridDim.x) * (cg_threads / L);
    for (int64_t i = (int64_t(blockIdx.x) * cg_threads + threadIdx.x) / L; i < n; i += groups)
    {
        const int64_t b = row_ptr[i], e = row_ptr[i + 1];
        for (int64_t k = b + lane; k < e; k += L)
        {
            const int32_t c = col_ind[k];
            if (c < 0 || c >= n)
                report(flag, i, column_out_of_range);
            else if (k > b && col_ind[k - 1] >= c)
                report(flag, i, columns_not_ascending);
        }
    }
}

// sum over the L lanes of a row's group, the same value in all of them: a fixed butterfly, no LDS
template < int L >
__device__ __forceinline__ double groupSum(double v)
{
#pragma unroll
    for (int w = L / 2; w > 0; w >>= 1)
        v += __shfl_xor(v, w);
    return v;
}

// y[c] <- alpha A x[c] + beta y[c] for NC columns (c at + c * ldx / ldy).  A group of L lanes of a wave64 owns a row, the groups
// walk the rows with a grid stride; lane l reads the entries row_ptr[i] + l, + L, ... (col_ind and values are streamed once:
// non-temporal loads; x is reused across rows: ordinary loads), one accumulator per column, so the NC columns share each load of
// col_ind and values.  The group's first lane stores; beta == 0: y is not read.  An empty row gives beta y.
// WITH_DOT (NC = 1, alpha = 1, beta = 0): the partials of <x, A x> over the group's rows, for cgFinishKernel.
// x and y must not overlap.
template < int L, int NC, bool WITH_DOT >
__global__ __launch_bounds__(cg_threads) void csrApplyKernel(const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ col_ind,
                                                             const double* __restrict__ values, int64_t n, const double* __restrict__ x,
                                                             size_t ldx, double* __restrict__ y, size_t ldy, double alpha, double beta,
                                                             double* __restrict__ partial)
{
    static_assert(!WITH_DOT || NC == 1);
    const int     lane   = threadIdx.x % L;
    const int64_t groups = int64_t(gridDim.x) * (cg_threads / L);
    double        dot[1] = {0.};
    for (int64_t i = (int64_t(blockIdx.x) * cg_threads + threadIdx.x) / L; i < n; i += groups)
    {
        const int64_t e = row_ptr[i + 1];
        double        acc[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c)
            acc[c] = 0.;
        for (int64_t k = row_ptr[i] + lane; k < e; k += L)
        {
            const int64_t j = __builtin_nontemporal_load(col_ind + k);
            const double  a = __builtin_nontemporal_load(values + k);
#pragma unroll
            for (int c = 0; c < NC; ++c)
                acc[c] += a * x[c * ldx + j];
        }
#pragma unroll
        for (int c = 0; c < NC; ++c)
            acc[c] = groupSum< L >(acc[c]);
        if (lane == 0)
        {
            if constexpr (WITH_DOT)
            {
                y[i] = acc[0];
                dot[0] += x[i] * acc[0];
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

// position of column `col` in the (ascending) row [b, e), or -1
__device__ __forceinline__ int64_t findColumn(const int32_t* __restrict__ col_ind, int64_t b, int64_t e, int64_t col)
{
    while (b < e)
    {
        const int64_t m = b + (e - b) / 2;
        const int64_t c = col_ind[m];
        if (c == col)
            return m;
        if (c < col)
            b = m + 1;
        else
            e = m;
    }
    return -1;
}
// diag[i] = a_ii (0 where none is stored); minv[i] = sign(a_ii) damping / max(|a_ii|, threshold) as jacobiInverseKernel has it on
// every non-empty row and 0 on an empty one: the PCG freezes such a row.  Either output may be nullptr
static __global__ __launch_bounds__(cg_threads) void csrDiagKernel(const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ col_ind,
                                                                   const double* __restrict__ values, int64_t n, double damping,
                                                                   double threshold, double* __restrict__ diag, double* __restrict__ minv)
{
    for (int64_t i = int64_t(blockIdx.x) * cg_threads + threadIdx.x; i < n; i += int64_t(gridDim.x) * cg_threads)
    {
        const int64_t b = row_ptr[i], e = row_ptr[i + 1];
        const int64_t k = findColumn(col_ind, b, e, i);
        const double  v = k >= 0 ? values[k] : 0., a = fabs(v);
        if (diag)
            diag[i] = v;
        if (minv)
            minv[i] = e > b ? (v < 0. ? -damping : damping) / (a > threshold ? a : threshold) : 0.;
    }
}

// l3k_csr_dirichlet, first kernel: the smallest masked row without a stored diagonal, if any (nothing is written before the
// host has seen the answer)
static __global__ __launch_bounds__(cg_threads) void csrDirichletCheckKernel(const int64_t* __restrict__ row_ptr,
                                                                             const int32_t* __restrict__ col_ind, int64_t n,
                                                                             const uint8_t* __restrict__ mask,
                                                                             unsigned long long* __restrict__ flag)
{
    for (int64_t i = int64_t(blockIdx.x) * cg_threads + threadIdx.x; i < n; i += int64_t(gridDim.x) * cg_threads)
        if (mask[i] && findColumn(col_ind, row_ptr[i], row_ptr[i + 1], i) < 0)
            atomicMin(flag, static_cast< unsigned long long >(i));
}
// ... second kernel, DirichletBCAlgebraic::apply in place (bcs/DirichletBC.hpp:82-150).  A group of L lanes per row.  A masked row
// becomes the identity row and its rhs the prescribed value; in an unmasked row every entry in a masked column j gives
// rhs -= a_ij g_j (lane partial sums in entry order, then the butterfly: a fixed order; the group's first lane is the row's
// only writer) and is then zeroed.  A row reads and writes entries of its own only
template < int L >
__global__ __launch_bounds__(cg_threads) void csrDirichletKernel(const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ col_ind,
                                                                 double* __restrict__ values, int64_t n, const uint8_t* __restrict__ mask,
                                                                 const double* __restrict__ g, size_t ldg, double* __restrict__ rhs,
                                                                 size_t ldr, int ncols)
{
    const int     lane   = threadIdx.x % L;
    const int64_t groups = int64_t(gridDim.x) * (cg_threads / L);
    for (int64_t i = (int64_t(blockIdx.x) * cg_threads + threadIdx.x) / L; i < n; i += groups)
    {
        const int64_t b = row_ptr[i], e = row_ptr[i + 1];
        if (mask[i])
        {
            for (int64_t k = b + lane; k < e; k += L)
                values[k] = col_ind[k] == i ? 1. : 0.;
            for (int c = lane; c < ncols; c += L)
                rhs[c * ldr + i] = g[c * ldg + i];
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
