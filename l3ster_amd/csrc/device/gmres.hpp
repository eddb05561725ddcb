// gmres.hpp -- the kernels of restarted GMRES (api_gmres.hip; include/l3k.h: l3k_gmres_*), for gfx950.  The basis V is column
// major: column j at V + j * ld, rows across lanes, so every load is coalesced.  Every dot product is a two-stage reduction in a
// fixed order (blockSum, then one finishing workgroup per column that sums the partials in index order): no floating-point
// atomics, equal bits for a given n and k on any context.  No kernel waits for another workgroup.
//
// Two routes, by the number nb of basis vectors (counted from the loops below, vectors of n doubles per pass):
//   nb < gm_chunk             registers: one chunk of gm_chunk accumulators holds every column and <w, w>; a row's V values stay in
//                             registers between the update and the second dot product.  multiDot reads nb + 1, projectRedot reads
//                             nb + 1 and writes 1.  One reduction tree for the chunk
//   gm_chunk <= nb < 256      tileKernel: a tile of T rows by nb columns in LDS between the two sweeps, one accumulator per column
//                             and thread across the tiles.  The same counts: V and w once per pass
//   nb >= 256, or no tile fits: the chunked sweeps (dotColumns): multiDot reads nb + ceil((nb + 1) / gm_chunk), projectRedot reads V
//                             twice.  Only restart lengths above 255 get here
#ifndef L3K_DEVICE_GMRES_HPP
#define L3K_DEVICE_GMRES_HPP

#include "../reduce.hpp"

namespace l3k::gmres
{
using l3k::red::blockSum;
using l3k::red::cg_blocks;
using l3k::red::cg_threads;
using l3k::red::liveRow;
constexpr int gm_chunk = 8;
// the device scalar block of a solve (doubles; the host reads all of it in one copy)
enum Slot : int
{
    s_rr        = 0, // <r, r> of the explicit residual over the live rows
    s_bb        = 1, // <b, b>
    s_est       = 2, // |g_{k+1}|: the residual estimate of the cycle, not scaled
    s_orth      = 3, // max over the steps of max_j |t_j| / nu
    s_nu        = 4, // nu of the last step
    s_kvalid    = 5, // columns of H that are valid in this cycle
    s_breakdown = 6, // != 0: the cycle has ended in a breakdown, later launches of the cycle do nothing
    s_beta      = 7, // the norm of the residual the cycle started from
    n_slots     = 8
};
__device__ __forceinline__ int64_t firstRow()
{
    return int64_t(blockIdx.x) * cg_threads + threadIdx.x;
}
__device__ __forceinline__ int64_t rowStep()
{
    return int64_t(gridDim.x) * cg_threads;
}
__device__ __forceinline__ bool stopped(const double* sc)
{
    return sc && sc[s_breakdown] != 0.;
}
// the block sums of a chunk of accumulators, columns j0 .. min(j0 + gm_chunk - 1, nb), into partial[j * gridDim.x + blockIdx.x]: ONE
// tree for the whole chunk (sh holds gm_chunk * cg_threads doubles), every column summed in the order of blockSum
__device__ __forceinline__ void storeChunk(const double (&acc)[gm_chunk], int j0, int nb, double* __restrict__ sh, double* __restrict__ partial)
{
    __syncthreads(); // (sh is read at the end of the chunk before)
#pragma unroll
    for (int c = 0; c < gm_chunk; ++c)
        sh[c * cg_threads + threadIdx.x] = acc[c];
    __syncthreads();
    for (int w = cg_threads / 2; w > 0; w >>= 1)
    {
        if (threadIdx.x < w)
#pragma unroll
            for (int c = 0; c < gm_chunk; ++c)
                sh[c * cg_threads + threadIdx.x] += sh[c * cg_threads + threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x < gm_chunk && j0 + int(threadIdx.x) <= nb)
        partial[size_t(j0 + threadIdx.x) * gridDim.x + blockIdx.x] = sh[threadIdx.x * cg_threads];
}
// partial[j * gridDim.x + blockIdx.x] = this block's share of <v_j, w> for j < nb and of <w, w> for j = nb; w counts as 0 on the
// frozen rows (mask != nullptr and mask == 0 on the bits), whatever it holds there
__device__ __forceinline__ void dotColumns(const double* __restrict__ V, size_t ld, int nb, const double* w, const double* __restrict__ mask,
                                           int64_t n, double* __restrict__ sh, double* __restrict__ partial)
{
    for (int j0 = 0; j0 <= nb; j0 += gm_chunk)
    {
        double acc[gm_chunk];
#pragma unroll
        for (int c = 0; c < gm_chunk; ++c)
            acc[c] = 0.;
        for (int64_t i = firstRow(); i < n; i += rowStep())
        {
            const bool   live = mask ? liveRow(mask[i]) : true;
            const double wv   = w[i];
            const double wi   = live ? wv : 0.;
#pragma unroll
            for (int c = 0; c < gm_chunk; ++c)
            {
                const int j = j0 + c; // (uniform: scalar branches)
                if (j < nb)
                    acc[c] += __builtin_nontemporal_load(V + size_t(j) * ld + i) * wi;
                else if (j == nb)
                    acc[c] += wi * wi;
            }
        }
        storeChunk(acc, j0, nb, sh, partial);
    }
}
// multiDot, first stage
static __global__ __launch_bounds__(cg_threads) void multiDotKernel(const double* __restrict__ V, size_t ld, int nb, const double* w,
                                                                    const double* __restrict__ mask, int64_t n, double* __restrict__ partial,
                                                                    const double* __restrict__ sc)
{
    __shared__ double sh[gm_chunk * cg_threads];
    if (stopped(sc))
        return;
    dotColumns(V, ld, nb, w, mask, n, sh, partial);
}
// projectRedot, first stage: w <- w - V h_in (0 stored on the frozen rows), then the partials of multiDot on the new w.  A thread
// reads in the second sweep the rows of w it has stored in the first
static __global__ __launch_bounds__(cg_threads) void projectRedotKernel(const double* __restrict__ V, size_t ld, int nb, double* w,
                                                                        const double* __restrict__ mask, int64_t n,
                                                                        const double* __restrict__ h_in, double* __restrict__ partial,
                                                                        const double* __restrict__ sc)
{
    __shared__ double sh[gm_chunk * cg_threads];
    if (stopped(sc))
        return;
    if (nb < gm_chunk) // one chunk holds every column and <w, w>: a row's V values stay in registers, V and w are read once
    {
        double acc[gm_chunk];
#pragma unroll
        for (int c = 0; c < gm_chunk; ++c)
            acc[c] = 0.;
        for (int64_t i = firstRow(); i < n; i += rowStep())
        {
            const bool   live = mask ? liveRow(mask[i]) : true;
            const double wv   = w[i];
            double       wi   = live ? wv : 0.;
            double       v[gm_chunk];
#pragma unroll
            for (int c = 0; c < gm_chunk; ++c)
                v[c] = c < nb ? __builtin_nontemporal_load(V + size_t(c) * ld + i) : 0.;
#pragma unroll
            for (int c = 0; c < gm_chunk; ++c)
                if (c < nb)
                    wi -= v[c] * h_in[c];
            wi   = live ? wi : 0.;
            w[i] = wi;
#pragma unroll
            for (int c = 0; c < gm_chunk; ++c)
                acc[c] += c < nb ? v[c] * wi : (c == nb ? wi * wi : 0.);
        }
        storeChunk(acc, 0, nb, sh, partial);
        return;
    }
    for (int64_t i = firstRow(); i < n; i += rowStep())
    {
        const bool   live = mask ? liveRow(mask[i]) : true;
        const double wv   = w[i];
        double       wi   = live ? wv : 0.;
        for (int j0 = 0; j0 < nb; j0 += gm_chunk)
        {
            double v[gm_chunk]; // (the loads of a chunk are in flight together)
#pragma unroll
            for (int c = 0; c < gm_chunk; ++c)
                v[c] = j0 + c < nb ? __builtin_nontemporal_load(V + size_t(j0 + c) * ld + i) : 0.;
#pragma unroll
            for (int c = 0; c < gm_chunk; ++c)
                if (j0 + c < nb)
                    wi -= v[c] * h_in[j0 + c];
        }
        w[i] = live ? wi : 0.;
    }
    dotColumns(V, ld, nb, w, nullptr, n, sh, partial); // (the frozen rows of w hold 0 now)
}
// The row-tile kernel of both passes for gm_chunk <= nb < cg_threads: V and w come from HBM ONCE.  A workgroup walks tiles of T rows
// (T a power of two, 16 .. 256, the largest whose nb columns fit the LDS budget, tilePlan in api_gmres.hip).  Load: thread (r, g) =
// (tid % T, tid / T) brings the columns g, g + G, ... of row r into the tile (column stride T + 1: the dot products below read it
// across columns without bank conflicts) and, with `project`, its share of sum_j v_j h_j; the shares are summed in the order of g,
// the new w of the row goes to HBM and to LDS.  Dot products: thread (c, q) = (tid % (nb + 1), tid / (nb + 1)) owns column c for the
// rows q, q + S, ... of every tile, in ONE accumulator that lives across the tiles (c = nb: <w, w>); at the end the S shares of a
// column are summed in the order of q.  No block sum, a fixed order, no atomics
template < bool project >
static __global__ __launch_bounds__(cg_threads) void tileKernel(const double* __restrict__ V, size_t ld, int nb, double* w,
                                                                const double* __restrict__ mask, int64_t n, const double* __restrict__ h_in,
                                                                double* __restrict__ partial, const double* __restrict__ sc, int T)
{
    extern __shared__ double tile_lds[];
    if (stopped(sc))
        return;
    const int TP = T + 1, G = cg_threads / T, C = nb + 1, S = cg_threads / C;
    double *  tile = tile_lds, *psum = tile + size_t(nb) * TP, *wt = psum + cg_threads, *red = wt + T; // nb TP | 256 | T | 256
    const int r = threadIdx.x % T, g = threadIdx.x / T, c = threadIdx.x % C, q = threadIdx.x / C;
    double    acc = 0.;
    const int64_t n_tiles = (n + T - 1) / T;
    for (int64_t t = blockIdx.x; t < n_tiles; t += gridDim.x)
    {
        const int64_t row = t * T + r;
        const bool    in  = row < n;
        double        ps  = 0.;
#pragma unroll 4
        for (int j = g; j < nb; j += G)
        {
            const double v   = in ? __builtin_nontemporal_load(V + size_t(j) * ld + row) : 0.;
            tile[j * TP + r] = v;
            if constexpr (project)
                ps += v * h_in[j];
        }
        if constexpr (project)
        {
            psum[threadIdx.x] = ps; // (= psum[g * T + r])
            __syncthreads();
        }
        if (g == 0)
        {
            const bool live = in && (mask ? liveRow(mask[row]) : true);
            double     wi   = 0.;
            if (in)
            {
                const double wv = w[row];
                wi              = live ? wv : 0.;
            }
            if constexpr (project)
            {
                for (int k = 0; k < G; ++k)
                    wi -= psum[k * T + r];
                wi = live ? wi : 0.;
                if (in)
                    w[row] = wi;
            }
            wt[r] = wi;
        }
        __syncthreads();
        if (q < S)
        {
            if (c < nb)
                for (int i = q; i < T; i += S)
                    acc += tile[c * TP + i] * wt[i];
            else
                for (int i = q; i < T; i += S)
                    acc += wt[i] * wt[i];
        }
        __syncthreads(); // (the next tile overwrites the LDS)
    }
    red[threadIdx.x] = acc; // (= red[q * C + c] for q < S)
    __syncthreads();
    if (threadIdx.x < C)
    {
        double sum = 0.;
        for (int k = 0; k < S; ++k)
            sum += red[k * C + threadIdx.x];
        partial[size_t(threadIdx.x) * gridDim.x + blockIdx.x] = sum;
    }
}
// second stage: out[j] = sum of partial[j][0 .. n_blocks) in index order; one workgroup per column
static __global__ __launch_bounds__(cg_threads) void finishKernel(const double* __restrict__ partial, int n_blocks, double* __restrict__ out,
                                                                  const double* __restrict__ sc)
{
    __shared__ double sh[cg_threads];
    if (stopped(sc))
        return;
    double acc = 0.;
    for (int i = threadIdx.x; i < n_blocks; i += cg_threads)
        acc += partial[size_t(blockIdx.x) * n_blocks + i];
    const double t = blockSum(acc, sh);
    if (threadIdx.x == 0)
        out[blockIdx.x] = t;
}
// r <- b - r on the live rows (r holds A x on entry), 0 on the frozen ones; partials of <r, r> (column 0)
static __global__ __launch_bounds__(cg_threads) void residualKernel(double* __restrict__ r, const double* __restrict__ b,
                                                                    const double* __restrict__ mask, int64_t n, double* __restrict__ partial)
{
    __shared__ double sh[cg_threads];
    double            acc = 0.;
    for (int64_t i = firstRow(); i < n; i += rowStep())
    {
        const bool   live = mask ? liveRow(mask[i]) : true;
        const double d    = __builtin_nontemporal_load(b + i) - __builtin_nontemporal_load(r + i);
        const double ri   = live ? d : 0.;
        __builtin_nontemporal_store(ri, r + i);
        acc += ri * ri;
    }
    const double t = blockSum(acc, sh);
    if (threadIdx.x == 0)
        partial[blockIdx.x] = t;
}
// the head of a cycle behind the host's look at <r, r>: g = beta e_0, no valid column, no breakdown
static __global__ void startCycleKernel(double* __restrict__ sc, double* __restrict__ g)
{
    const double beta = sqrt(sc[s_rr]);
    g[0]              = beta;
    sc[s_beta]        = beta;
    sc[s_est]         = beta;
    sc[s_nu]          = beta;
    sc[s_kvalid]      = 0.;
    sc[s_breakdown]   = 0.;
}
// scaleInto: dst = src / sc[slot] (v_0 = r / beta, v_{k+1} = w / nu); nothing after a breakdown.  src == dst is allowed
static __global__ __launch_bounds__(cg_threads) void scaleIntoKernel(const double* src, double* dst, int64_t n, const double* __restrict__ sc,
                                                                     int slot)
{
    if (stopped(sc))
        return;
    const double f = 1. / sc[slot];
    for (int64_t i = firstRow(); i < n; i += rowStep())
        dst[i] = src[i] * f;
}
// z = minv (.) v: the Jacobi step of the right preconditioner (a frozen row has minv = 0 and v = 0)
static __global__ __launch_bounds__(cg_threads) void jacobiKernel(const double* __restrict__ v, const double* __restrict__ minv,
                                                                  double* __restrict__ z, int64_t n)
{
    for (int64_t i = firstRow(); i < n; i += rowStep())
    {
        const double m = minv[i];
        z[i]           = liveRow(m) ? m * v[i] : 0.;
    }
}
// combine.  mode 0: x += [minv (.)] sum_j y_j v_j on the live rows (the frozen rows of x are not written);  mode 1: x = sum_j y_j v_j
// on every row (u of the Precond-based solves);  mode 2: x += V[0] on the live rows of minv (the axpy behind the apply)
template < int mode >
static __global__ __launch_bounds__(cg_threads) void combineKernel(const double* __restrict__ V, size_t ld, int nb, const double* __restrict__ y,
                                                                   const double* __restrict__ minv, int64_t n, double* __restrict__ x)
{
    for (int64_t i = firstRow(); i < n; i += rowStep())
    {
        const double m = minv ? minv[i] : 1.;
        if (mode != 1 && !liveRow(m))
            continue;
        double u = 0.;
        if constexpr (mode == 2)
            u = V[i];
        else
            for (int j0 = 0; j0 < nb; j0 += gm_chunk)
            {
                double v[gm_chunk];
#pragma unroll
                for (int c = 0; c < gm_chunk; ++c)
                    v[c] = j0 + c < nb ? __builtin_nontemporal_load(V + size_t(j0 + c) * ld + i) : 0.;
#pragma unroll
                for (int c = 0; c < gm_chunk; ++c)
                    if (j0 + c < nb)
                        u += v[c] * y[j0 + c];
            }
        if constexpr (mode == 0)
            x[i] += m * u;
        else if constexpr (mode == 1)
            x[i] = u;
        else
            x[i] += u;
    }
}
// hessenberg: step k of a cycle (nb = k + 1 basis vectors), one workgroup.  Column k of H becomes h1 + h2 with nu = sqrt(t[nb])
// below it; the stored rotations go over it, a new one annihilates nu, g and the estimate follow.  H is column major with ldh rows
// and holds R afterwards.  Breakdown (nu = 0 or nu <= 2^-52 ||H[0..k, k]||): the column is valid, the cycle ends, the flag stops
// every later launch of the cycle
constexpr int hess_lds = 2048;
// the larger of two values, or NaN if either is one: fmax would drop it, and the library is built with -ffinite-math-only, so the
// test is on the bits
__device__ __forceinline__ double maxOrNan(double a, double b)
{
    const auto nan = [](double x) { return (__double_as_longlong(x) & 0x7fffffffffffffffLL) > 0x7ff0000000000000LL; };
    return nan(a) ? a : (nan(b) || b > a ? b : a);
}
static __global__ __launch_bounds__(cg_threads) void hessenbergKernel(const double* __restrict__ h1, const double* __restrict__ h2,
                                                                      const double* __restrict__ t, int k, double* __restrict__ H, int ldh,
                                                                      double* __restrict__ cs, double* __restrict__ sn, double* __restrict__ g,
                                                                      double* __restrict__ sc)
{
    __shared__ double sh[cg_threads];
    __shared__ double col_lds[hess_lds];
    if (stopped(sc))
        return;
    const int nb  = k + 1;
    double*   col = col_lds; // (nb + 1 <= hess_lds: l3k_gmres_create refuses a longer restart)
    double    sq = 0., tmax = 0.;
    for (int j = threadIdx.x; j < nb; j += cg_threads)
    {
        const double h = h1[j] + h2[j];
        col[j]         = h;
        sq += h * h;
        tmax = maxOrNan(tmax, fabs(t[j]));
    }
    const double norm2 = blockSum(sq, sh);
    __syncthreads();
    // (the maximum through the same tree)
    sh[threadIdx.x] = tmax;
    __syncthreads();
    for (int w = cg_threads / 2; w > 0; w >>= 1)
    {
        if (threadIdx.x < w)
            sh[threadIdx.x] = maxOrNan(sh[threadIdx.x], sh[threadIdx.x + w]);
        __syncthreads();
    }
    if (threadIdx.x == 0)
    {
        const double nu2 = t[nb];
        const double nu  = nu2 > 0. ? sqrt(nu2) : 0.;
        const bool   bd  = !(nu > 0x1p-52 * sqrt(norm2));
        for (int j = 0; j < k; ++j)
        {
            const double a = col[j], b = col[j + 1];
            col[j]         = cs[j] * a + sn[j] * b;
            col[j + 1]     = cs[j] * b - sn[j] * a;
        }
        const double a = col[k], r = hypot(a, nu);
        const double c = r > 0. ? a / r : 1., s = r > 0. ? nu / r : 0.;
        cs[k] = c, sn[k] = s;
        col[k]           = r;
        col[k + 1]       = 0.;
        const double gk  = g[k];
        g[k]             = c * gk;
        g[k + 1]         = -s * gk;
        sc[s_est]        = fabs(s * gk);
        sc[s_nu]         = nu;
        sc[s_kvalid]     = double(k + 1);
        if (bd)
            sc[s_breakdown] = 1.;
        else
            sc[s_orth] = maxOrNan(sc[s_orth], sh[0] / nu);
    }
    __syncthreads();
    for (int j = threadIdx.x; j <= nb; j += cg_threads)
        H[size_t(k) * ldh + j] = col_lds[j];
}
// y = R^-1 g for the kv valid columns, one workgroup, column oriented: y_j = g_j / R_jj, then g_i -= R_ij y_j for i < j.  y starts
// as a copy of g; a zero on the diagonal (a singular block) gives y_j = 0
static __global__ __launch_bounds__(cg_threads) void triSolveKernel(const double* __restrict__ H, int ldh, const double* __restrict__ g, int kv,
                                                                    double* y)
{
    for (int i = threadIdx.x; i < kv; i += cg_threads)
        y[i] = g[i];
    __syncthreads();
    for (int j = kv - 1; j >= 0; --j)
    {
        const double d  = H[size_t(j) * ldh + j];
        const double yj = d != 0. ? y[j] / d : 0.;
        __syncthreads(); // (everyone has read y[j])
        if (threadIdx.x == 0)
            y[j] = yj;
        for (int i = threadIdx.x; i < j; i += cg_threads)
            y[i] -= H[size_t(j) * ldh + i] * yj;
        __syncthreads();
    }
}
} // namespace l3k::gmres
#endif
