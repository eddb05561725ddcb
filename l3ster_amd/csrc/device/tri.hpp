// tri.hpp -- kernels of the triangular preconditioners on a device CSR operator (include/l3k.h: l3k_tri_*): symmetric Gauss-Seidel
// and ILU(0), what the reference reaches through Ifpack2 (solve/Ifpack2Preconditioners.hpp:97-101,134-157).  Both are sparse
// triangular solves over LEVELS (host/tri_levels.cpp): the rows of a level depend on rows of earlier levels only, so a level is
// one data-parallel pass.  A level wider than the plan's fuse_rows is one launch of a level kernel (groups of L lanes walk a slice
// of the level-ordered row list with a grid stride); a run of consecutive narrower levels is one launch of a fused kernel, in which
// ONE workgroup walks the levels with a workgroup barrier between them.  The ILU(0) factorisation runs on the same row lists.
//
// The rules of device/csr.hpp hold: a row has one writer, the lanes of a row are combined by csr::groupSum, nothing accumulates
// atomically in floating point (the pivot counters are integers), no kernel waits for another workgroup.  A row's arithmetic is
// rowSolve / iluRow whichever kernel calls it: the result does not depend on the launch plan, on the grid or on the context.
#ifndef L3K_DEVICE_TRI_HPP
#define L3K_DEVICE_TRI_HPP

#include "csr.hpp"

namespace l3k::tri
{
using csr::cg_threads;

// status[0]: pivots (SGS: diagonal entries) that were zero or not finite, status[1]: the lowest such row (~0: none)
constexpr int status_words = 2;

// Is the number with these bits zero, Inf or NaN?  Decided on the integer, loaded as one: the device translation units are built
// with -ffinite-math-only, which folds the floating-point tests (device/chol.hpp: goodPivotBits)
__device__ __forceinline__ bool badPivotBits(unsigned long long bits)
{
    const unsigned long long mag = bits & 0x7fffffffffffffffull;
    return mag == 0ull || mag >= 0x7ff0000000000000ull;
}
__device__ __forceinline__ void reportPivot(unsigned long long* status, int64_t row)
{
    atomicAdd(status, 1ull);
    atomicMin(status + 1, static_cast< unsigned long long >(row));
}
// Stores of this wave become visible to its later loads: the lanes of a row hand entries of the row to each other through global
// memory (iluRow), and so do the waves of a workgroup across a barrier (levelBarrier).  The waves of a workgroup share one L1, so
// workgroup scope needs no cache action; the explicit wait stands behind the fence because the fence's own may be dropped
__device__ __forceinline__ void storesVisible()
{
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}
// between two levels of a fused kernel: every store of the level before is ordered before every load of the level after
__device__ __forceinline__ void levelBarrier()
{
    storesVisible();
    __syncthreads();
}

// diag_pos[i] = position of a_ii in values, -1 on an empty row (l3k_tri_create has refused an active row without one);
// mask[i] = 1 on an active row, 0 on an empty one
static __global__ __launch_bounds__(cg_threads) void triDiagPosKernel(const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ col_ind,
                                                                      int64_t n, int64_t* __restrict__ diag_pos, double* __restrict__ mask)
{
    for (int64_t i = int64_t(blockIdx.x) * cg_threads + threadIdx.x; i < n; i += int64_t(gridDim.x) * cg_threads)
    {
        const int64_t b = row_ptr[i], e = row_ptr[i + 1];
        diag_pos[i]     = e > b ? csr::findColumn(col_ind, b, e, i) : -1;
        mask[i]         = e > b ? 1. : 0.;
    }
}
// SGS: dinv[i] = omega / a_ii from A's current values (0 on an empty row); a diagonal entry that is zero or not finite counts as 1
static __global__ __launch_bounds__(cg_threads) void triRecipDiagKernel(const int64_t* __restrict__ diag_pos, const double* __restrict__ values,
                                                                        int64_t n, double omega, double* __restrict__ dinv,
                                                                        unsigned long long* __restrict__ status)
{
    for (int64_t i = int64_t(blockIdx.x) * cg_threads + threadIdx.x; i < n; i += int64_t(gridDim.x) * cg_threads)
    {
        const int64_t d = diag_pos[i];
        if (d < 0)
        {
            dinv[i] = 0.;
            continue;
        }
        if (badPivotBits(reinterpret_cast< const unsigned long long* >(values)[d]))
        {
            reportPivot(status, i);
            dinv[i] = omega;
        }
        else
            dinv[i] = omega / values[d];
    }
}
// ILU(0), after the copy of A's values: a_ii <- sign(a_ii) * absolute + relative * a_ii (Ifpack2's "fact: absolute threshold" and
// "fact: relative threshold"; the defaults 0 and 1 leave the bits of a_ii)
static __global__ __launch_bounds__(cg_threads) void triThresholdKernel(const int64_t* __restrict__ diag_pos, int64_t n, double absolute,
                                                                        double relative, double* __restrict__ f)
{
    for (int64_t i = int64_t(blockIdx.x) * cg_threads + threadIdx.x; i < n; i += int64_t(gridDim.x) * cg_threads)
    {
        const int64_t d = diag_pos[i];
        if (d >= 0)
        {
            const double v = f[d];
            f[d]           = fma(relative, v, v < 0. ? -absolute : absolute);
        }
    }
}

// ---- the solves.  What a row computes from the sum s of its entries on the wanted side of the diagonal times the final z there:
enum Solve : int
{
    sgs_lower  = 0, // (D / omega + L) y = r:              y_i = (r_i - s) * dinv_i,   entries of A
    sgs_upper  = 1, // (D / omega + U) z = c D y:          z_i = (c a_ii y_i - s) * dinv_i,  c = (2 - omega) / omega, entries of A
    ilu0_lower = 2, // L y = r, unit diagonal:             y_i = r_i - s,              entries of the factor
    ilu0_upper = 3, // U z = y:                            z_i = (y_i - s) / u_ii,     entries of the factor
};
struct SolveArgs
{
    const int64_t* row_ptr;
    const int32_t* col_ind;
    const int64_t* diag_pos;
    const double*  values; // A's (SGS) or the factor's (ILU0); not written while a solve runs
    const double*  dinv;   // SGS
    const double*  r;
    double*        z; // written and read by different threads of one kernel: no __restrict__, no non-temporal load
    double         c;
};
// Lane `lane` of the L that own row i: the entries kb + lane, + L, ... in entry order, then the fixed butterfly; the first lane
// writes.  Columns of empty rows carry z = 0 (the caller zeroed them), so their entries add nothing
template < int L, int MODE >
__device__ __forceinline__ void rowSolve(const SolveArgs& a, int64_t i, int lane)
{
    constexpr bool lower = MODE == sgs_lower || MODE == ilu0_lower;
    const int64_t  d     = a.diag_pos[i];
    const int64_t  kb = lower ? a.row_ptr[i] : d + 1, ke = lower ? d : a.row_ptr[i + 1];
    double         s = 0.;
    for (int64_t k = kb + lane; k < ke; k += L)
        s = fma(a.values[k], a.z[a.col_ind[k]], s);
    s = csr::groupSum< L >(s);
    if (lane == 0)
    {
        if constexpr (MODE == sgs_lower)
            a.z[i] = (a.r[i] - s) * a.dinv[i];
        else if constexpr (MODE == sgs_upper)
            a.z[i] = (a.c * a.values[d] * a.r[i] - s) * a.dinv[i];
        else if constexpr (MODE == ilu0_lower)
            a.z[i] = a.r[i] - s;
        else
            a.z[i] = (a.r[i] - s) / a.values[d];
    }
}
// one level (or a slice of one): rows[0 .. count) are independent of each other
template < int L, int MODE >
__global__ __launch_bounds__(cg_threads) void triLevelSolveKernel(SolveArgs a, const int32_t* __restrict__ rows, int64_t count)
{
    const int     lane   = threadIdx.x % L;
    const int64_t groups = int64_t(gridDim.x) * (cg_threads / L);
    for (int64_t q = (int64_t(blockIdx.x) * cg_threads + threadIdx.x) / L; q < count; q += groups)
        rowSolve< L, MODE >(a, rows[q], lane);
}
// the levels [l0, l1) by ONE workgroup: level l is rows[level_ptr[l] .. level_ptr[l + 1])
template < int L, int MODE >
__global__ __launch_bounds__(cg_threads) void triFusedSolveKernel(SolveArgs a, const int32_t* __restrict__ rows,
                                                                  const int64_t* __restrict__ level_ptr, int64_t l0, int64_t l1)
{
    const int lane = threadIdx.x % L, group = threadIdx.x / L;
    for (int64_t l = l0; l < l1; ++l)
    {
        const int64_t e = level_ptr[l + 1];
        for (int64_t q = level_ptr[l] + group; q < e; q += cg_threads / L)
            rowSolve< L, MODE >(a, rows[q], lane);
        if (l + 1 < l1)
            levelBarrier();
    }
}

// ---- ILU(0), row-wise IKJ in A's pattern, in place in f (the copy of A's values).  The L lanes of row i take its stored active
// k < i one after the other, ascending: l_ik = a_ik / u_kk, then the lanes share the entries j > k of row k (final: an earlier
// level) and each finds j in row i by a search in its sorted columns: a_ij -= l_ik u_kj.  Within a step every entry of row i has
// at most one writer.  Across steps an entry written by one lane is read by another (as a_ij, and as a_ik' once j = k'): row i stays
// in global memory and EVERY step starts behind storesVisible().  Rows and columns that are empty are outside the factorisation.
// At the end the pivot u_ii is tested: zero or not finite -> 1, counted
struct FactorArgs
{
    const int64_t*      row_ptr;
    const int32_t*      col_ind;
    const int64_t*      diag_pos;
    double*             f;
    unsigned long long* status;
};
template < int L >
__device__ __forceinline__ void iluRow(const FactorArgs& a, int64_t i, int lane)
{
    const int64_t b = a.row_ptr[i], e = a.row_ptr[i + 1], d = a.diag_pos[i];
    for (int64_t kk = b; kk < d; ++kk)
    {
        const int64_t k  = a.col_ind[kk];
        const int64_t dk = a.diag_pos[k];
        if (dk < 0)
            continue;
        storesVisible();
        const double  lik = a.f[kk] / a.f[dk];
        const int64_t ek  = a.row_ptr[k + 1];
        for (int64_t m = dk + 1 + lane; m < ek; m += L)
        {
            const int64_t j = a.col_ind[m];
            if (a.diag_pos[j] < 0)
                continue;
            const int64_t p = csr::findColumn(a.col_ind, kk + 1, e, j);
            if (p >= 0)
                a.f[p] = fma(-lik, a.f[m], a.f[p]);
        }
        if (lane == 0)
            a.f[kk] = lik; // (every lane has read a_ik: lik depends on that load)
    }
    storesVisible();
    if (lane == 0 && badPivotBits(reinterpret_cast< const unsigned long long* >(a.f)[d]))
    {
        reportPivot(a.status, i);
        a.f[d] = 1.;
    }
}
template < int L >
__global__ __launch_bounds__(cg_threads) void triLevelFactorKernel(FactorArgs a, const int32_t* __restrict__ rows, int64_t count)
{
    const int     lane   = threadIdx.x % L;
    const int64_t groups = int64_t(gridDim.x) * (cg_threads / L);
    for (int64_t q = (int64_t(blockIdx.x) * cg_threads + threadIdx.x) / L; q < count; q += groups)
        iluRow< L >(a, rows[q], lane);
}
template < int L >
__global__ __launch_bounds__(cg_threads) void triFusedFactorKernel(FactorArgs a, const int32_t* __restrict__ rows,
                                                                   const int64_t* __restrict__ level_ptr, int64_t l0, int64_t l1)
{
    const int lane = threadIdx.x % L, group = threadIdx.x / L;
    for (int64_t l = l0; l < l1; ++l)
    {
        const int64_t e = level_ptr[l + 1];
        for (int64_t q = level_ptr[l] + group; q < e; q += cg_threads / L)
            iluRow< L >(a, rows[q], lane);
        if (l + 1 < l1)
            levelBarrier();
    }
}
} // namespace l3k::tri
#endif
