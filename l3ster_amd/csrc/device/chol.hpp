// chol.hpp -- kernels of the band Cholesky solver on a device CSR operator (include/l3k.h: l3k_chol_*; launched from api_chol.hip).
//
// Storage (host/chol_symbolic.hpp): blocks of NB x NB doubles, column-major inside a block (entry (r, c) at c * NB + r); block
// column K holds its diagonal block and the H(K) blocks below it contiguously, first block col_off[K]; block (I, J) of the lower
// triangle is at col_off[J] + (I - J).  K + H(K) never decreases, so the factor fills no block outside the storage.
//
// Factorisation, right-looking, three launches per block column: cholDiagKernel (one workgroup, L_KK in LDS), cholPanelKernel (one
// workgroup per block below: A_IK L_KK^-T) and cholUpdateKernel (one workgroup per block pair K < J <= I <= K + H(K):
// A_IJ -= L_IK L_JK^T on the FP64 matrix cores).  Solve: gather, per block column a diagonal solve and an update launch forwards
// and backwards, scatter.  No kernel waits for another workgroup, every block and every vector segment has one writer per launch,
// sums run in a fixed order and nothing accumulates atomically: factor and solve are bitwise reproducible.
#ifndef L3K_DEVICE_CHOL_HPP
#define L3K_DEVICE_CHOL_HPP

#include "reduce.hpp"

namespace l3k::chol
{
constexpr int threads = 256;
using mfma_d4         = __attribute__((ext_vector_type(4))) double;

// status[0]: non-positive or non-finite pivots met, status[1]: the row (in the permuted numbering) of the first
constexpr int status_words = 2;

// Is the pivot with these bits positive and finite?  The device translation units are built with -ffinite-math-only, which folds
// the usual tests -- and folds a test of the exponent bits as well once it sits behind a parameter of type double (the compiler
// marks such a parameter as never NaN or Inf: the pivot test came out as !(0 < d), which takes +Inf for a good pivot).  So the
// decision is made on an integer that never was a double parameter: good are the bits of +denorm_min .. +DBL_MAX, that is
// 1 .. 0x7fefffffffffffff; 0, the sign bit, and an exponent of all ones (Inf, NaN) fall outside
__device__ __forceinline__ bool goodPivotBits(unsigned long long bits)
{
    return bits - 1ull < 0x7fefffffffffffffull;
}

// ---- fill: storage <- lower triangle of P A P^T (the storage was zeroed); the padding of the last block <- identity
template < int NB >
static __global__ __launch_bounds__(threads) void cholFillKernel(const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ col_ind,
                                                                 const double* __restrict__ values, int64_t n,
                                                                 const int32_t* __restrict__ inv, const int64_t* __restrict__ col_off,
                                                                 double* __restrict__ L, int64_t n_active, int64_t n_blocks)
{
    const int64_t t = int64_t(blockIdx.x) * threads + threadIdx.x, stride = int64_t(gridDim.x) * threads;
    for (int64_t i = t; i < n; i += stride)
    {
        const int64_t pi = inv[i];
        if (pi < 0)
            continue;
        for (int64_t e = row_ptr[i]; e < row_ptr[i + 1]; ++e)
        {
            const int64_t pj = inv[col_ind[e]];
            if (pj < 0 || pj > pi)
                continue;
            const int64_t bi = pi / NB, bj = pj / NB;
            L[(col_off[bj] + (bi - bj)) * (NB * NB) + (pj % NB) * NB + pi % NB] = values[e];
        }
    }
    for (int64_t p = n_active + t; p < n_blocks * NB; p += stride)
        L[col_off[n_blocks - 1] * (NB * NB) + (p % NB) * NB + p % NB] = 1.;
}

// ---- diagonal block: A_KK = L L^T in LDS, right-looking, by one workgroup; the strict upper triangle comes back as 0.  A pivot
// that is not positive and finite is replaced by 1, counted, and the first one's row noted (one thread, launches are in order)
template < int NB >
static __global__ __launch_bounds__(threads) void cholDiagKernel(double* __restrict__ D, int64_t row0, unsigned long long* __restrict__ status)
{
    __shared__ double s[NB * NB];
    const int         tid = threadIdx.x;
    for (int i = tid; i < NB * NB; i += threads)
        s[i] = D[i];
    for (int c = 0; c < NB; ++c)
    {
        __syncthreads();
        double     d   = s[c * NB + c];
        const bool bad = !goodPivotBits(__builtin_bit_cast(unsigned long long, d));
        if (bad)
        {
            d = 1.;
            if (tid == 0)
            {
                if (status[0] == 0)
                    status[1] = static_cast< unsigned long long >(row0 + c);
                ++status[0];
            }
        }
        const double piv = sqrt(d);
        __syncthreads();
        if (tid == c)
            s[c * NB + c] = piv;
        else if (tid > c && tid < NB)
            s[c * NB + tid] /= piv;
        __syncthreads();
        for (int i = (c + 1) * NB + tid; i < NB * NB; i += threads)
        {
            const int r = i % NB, c2 = i / NB;
            if (r >= c2)
                s[i] -= s[c * NB + r] * s[c * NB + c2];
        }
    }
    __syncthreads();
    for (int i = tid; i < NB * NB; i += threads)
        D[i] = i % NB >= i / NB ? s[i] : 0.;
}

// ---- panel: block b of the H(K) blocks below the diagonal one, X L_KK^T = A_IK row by row, right-looking in LDS
template < int NB >
static __global__ __launch_bounds__(threads) void cholPanelKernel(double* __restrict__ colK)
{
    __shared__ double a[NB * NB];
    const int         tid = threadIdx.x;
    const double*     Ld  = colK;
    double*           X   = colK + (int64_t(blockIdx.x) + 1) * (NB * NB);
    for (int i = tid; i < NB * NB; i += threads)
        a[i] = X[i];
    for (int c = 0; c < NB; ++c)
    {
        __syncthreads();
        if (tid < NB)
            a[c * NB + tid] /= Ld[c * NB + c];
        __syncthreads();
        for (int i = (c + 1) * NB + tid; i < NB * NB; i += threads)
            a[i] -= a[c * NB + i % NB] * Ld[c * NB + i / NB];
    }
    __syncthreads();
    for (int i = tid; i < NB * NB; i += threads)
        X[i] = a[i];
}

// ---- trailing update: workgroup p = the pair (i, j), 1 <= j <= i <= H, p = i (i - 1) / 2 + j - 1, of block column K:
// A(K + i, K + j) -= L(K + i, K) L(K + j, K)^T with v_mfma_f64_16x16x4_f64.  The product is formed transposed -- first operand
// from L(K + j, K), second from L(K + i, K) -- so that the 16 lanes of a result row run along a column of the column-major
// target: D[m][n] = C[row 16 ti + n][col 16 tj + m], m = (lane >> 4) + 4 reg, n = lane & 15.  Four waves share the (NB / 16)^2
// tiles; fragments come straight from global memory (a block is read by at most four waves of this workgroup, from L2).  On a
// diagonal pair the tiles above the diagonal are skipped (nothing reads them).
template < int NB >
static __global__ __launch_bounds__(threads) void cholUpdateKernel(double* __restrict__ L, const int64_t* __restrict__ col_off, int64_t K)
{
    constexpr int T = NB / 16, TPW = T * T / 4;
    const int64_t p = blockIdx.x;
    int64_t       i = int64_t((1. + sqrt(1. + 8. * double(p))) / 2.);
    while (i * (i - 1) / 2 > p)
        --i;
    while ((i + 1) * i / 2 <= p)
        ++i;
    const int64_t j = p - i * (i - 1) / 2 + 1;
    const double* A = L + (col_off[K] + i) * (NB * NB);
    const double* B = L + (col_off[K] + j) * (NB * NB);
    double*       Cb = L + (col_off[K + j] + (i - j)) * (NB * NB);

    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int ti = (wave * TPW) / T, tj0 = (wave * TPW) % T;
    mfma_d4   acc[TPW];
#pragma unroll
    for (int q = 0; q < TPW; ++q)
        acc[q] = mfma_d4{0., 0., 0., 0.};
    for (int k0 = 0; k0 < NB; k0 += 4)
    {
        const int    k  = k0 + (lane >> 4);
        const double af = A[k * NB + ti * 16 + (lane & 15)];
#pragma unroll
        for (int q = 0; q < TPW; ++q)
        {
            const double bf = B[k * NB + (tj0 + q) * 16 + (lane & 15)];
            acc[q]          = __builtin_amdgcn_mfma_f64_16x16x4f64(bf, af, acc[q], 0, 0, 0);
        }
    }
#pragma unroll
    for (int q = 0; q < TPW; ++q)
    {
        const int tj = tj0 + q;
        if (i == j && ti < tj)
            continue;
#pragma unroll
        for (int reg = 0; reg < 4; ++reg)
        {
            const int c = tj * 16 + (lane >> 4) + 4 * reg, r = ti * 16 + (lane & 15);
            Cb[c * NB + r] -= acc[q][reg];
        }
    }
}

// ---- solve: w [ncols][ldw] is the permuted workspace over the n_blocks * NB padded rows
static __global__ __launch_bounds__(threads) void cholGatherKernel(const double* __restrict__ b, size_t ldb, double* __restrict__ w, size_t ldw,
                                                                   const int32_t* __restrict__ perm, int64_t n_active, int64_t n_padded)
{
    const size_t col = blockIdx.y;
    for (int64_t p = int64_t(blockIdx.x) * threads + threadIdx.x; p < n_padded; p += int64_t(gridDim.x) * threads)
        w[col * ldw + p] = p < n_active ? b[col * ldb + perm[p]] : 0.;
}
static __global__ __launch_bounds__(threads) void cholScatterKernel(const double* __restrict__ w, size_t ldw, double* __restrict__ x, size_t ldx,
                                                                    const int32_t* __restrict__ perm, int64_t n_active)
{
    const size_t col = blockIdx.y;
    for (int64_t p = int64_t(blockIdx.x) * threads + threadIdx.x; p < n_active; p += int64_t(gridDim.x) * threads)
        x[col * ldx + perm[p]] = w[col * ldw + p];
}

// L_KK into LDS with a leading dimension of NB + 1: its columns and its rows are both read without bank conflicts
template < int NB >
__device__ __forceinline__ void stageDiag(const double* __restrict__ Lkk, double* s)
{
    for (int i = threadIdx.x; i < NB * NB; i += threads)
        s[(i / NB) * (NB + 1) + i % NB] = i % NB >= i / NB ? Lkk[i] : 0.;
    __syncthreads();
}

// forward, diagonal block: w_K <- L_KK^-1 w_K, one workgroup per column; the substitution runs in one wave, lane r holds row r
template < int NB >
static __global__ __launch_bounds__(threads) void cholFwdDiagKernel(const double* __restrict__ Lkk, double* __restrict__ wK, size_t ldw)
{
    __shared__ double s[NB * (NB + 1)];
    stageDiag< NB >(Lkk, s);
    if (threadIdx.x >= 64)
        return;
    const int lane = threadIdx.x;
    double*   w    = wK + size_t(blockIdx.x) * ldw;
    double    x    = lane < NB ? w[lane] : 0.;
    for (int c = 0; c < NB; ++c)
    {
        if (lane == c)
            x /= s[c * (NB + 1) + c];
        const double xc = __shfl(x, c);
        if (lane > c && lane < NB)
            x -= s[c * (NB + 1) + lane] * xc;
    }
    if (lane < NB)
        w[lane] = x;
}
// forward, update: w_I -= L_IK w_K for block b = I - K - 1 of the H(K) blocks below, one workgroup per (block, column); the
// 256 / NB thread groups of a row take a quarter (an eighth) of the k range each and are summed in a fixed order
template < int NB >
static __global__ __launch_bounds__(threads) void cholFwdUpdateKernel(const double* __restrict__ colK, double* __restrict__ wK, size_t ldw)
{
    constexpr int     parts = threads / NB, span = NB / parts;
    __shared__ double xk[NB], red[threads];
    const double*     Blk = colK + (int64_t(blockIdx.x) + 1) * (NB * NB);
    double*           w   = wK + size_t(blockIdx.y) * ldw;
    const int         tid = threadIdx.x, r = tid % NB, part = tid / NB;
    if (tid < NB)
        xk[tid] = w[tid];
    __syncthreads();
    double sum = 0.;
    for (int k = part * span; k < (part + 1) * span; ++k)
        sum += Blk[k * NB + r] * xk[k];
    red[tid] = sum;
    __syncthreads();
    if (tid < NB)
    {
        double t = red[tid];
        for (int q = 1; q < parts; ++q)
            t += red[q * NB + tid];
        w[(int64_t(blockIdx.x) + 1) * NB + tid] -= t;
    }
}
// backward, update: t_b = L_IK^T w_I for block b = I - K - 1, one workgroup per (block, column), into scratch [ncols][H][NB]: a
// wave per column of the block, a fixed butterfly over its lanes.  cholBwdDiagKernel sums the t_b in ascending b
template < int NB >
static __global__ __launch_bounds__(threads) void cholBwdPartialKernel(const double* __restrict__ colK, const double* __restrict__ wK, size_t ldw,
                                                                      double* __restrict__ scratch, size_t lds)
{
    const double* Blk  = colK + (int64_t(blockIdx.x) + 1) * (NB * NB);
    const double* wi   = wK + size_t(blockIdx.y) * ldw + (int64_t(blockIdx.x) + 1) * NB;
    double*       t    = scratch + size_t(blockIdx.y) * lds + size_t(blockIdx.x) * NB;
    const int     wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const double  xi   = lane < NB ? wi[lane] : 0.;
    for (int c = wave; c < NB; c += threads / 64)
    {
        double v = lane < NB ? Blk[c * NB + lane] * xi : 0.;
        for (int m = 32; m > 0; m >>= 1)
            v += __shfl_xor(v, m);
        if (lane == 0)
            t[c] = v;
    }
}
// backward, diagonal block: w_K <- L_KK^-T (w_K - sum_b t_b), one workgroup per column
template < int NB >
static __global__ __launch_bounds__(threads) void cholBwdDiagKernel(const double* __restrict__ Lkk, double* __restrict__ wK, size_t ldw, int H,
                                                                   const double* __restrict__ scratch, size_t lds)
{
    __shared__ double s[NB * (NB + 1)];
    stageDiag< NB >(Lkk, s);
    if (threadIdx.x >= 64)
        return;
    const int     lane = threadIdx.x;
    double*       w    = wK + size_t(blockIdx.x) * ldw;
    const double* t    = scratch + size_t(blockIdx.x) * lds;
    double        x    = 0.;
    if (lane < NB)
    {
        double sum = 0.;
        for (int b = 0; b < H; ++b)
            sum += t[size_t(b) * NB + lane];
        x = w[lane] - sum;
    }
    for (int c = NB - 1; c >= 0; --c)
    {
        if (lane == c)
            x /= s[c * (NB + 1) + c];
        const double xc = __shfl(x, c);
        if (lane < c)
            x -= s[lane * (NB + 1) + c] * xc;
    }
    if (lane < NB)
        w[lane] = x;
}
} // namespace l3k::chol
#endif
