// reduce.hpp -- the two-stage reduction that api_solver.hip (the PCG's dot products) and api_csr.hip (<x, A x> of the CSR apply)
// share: block sums in a fixed order into the context's workspace, one finishing block into the scalar block s.
#ifndef L3K_REDUCE_HPP
#define L3K_REDUCE_HPP

#include "objects.hpp"

namespace l3k::red
{
constexpr int cg_threads = 256, cg_blocks = l3k_cg_blocks;
__device__ __forceinline__ double blockSum(double v, double* sh)
{
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int w = cg_threads / 2; w > 0; w >>= 1)
    {
        if (threadIdx.x < w)
            sh[threadIdx.x] += sh[threadIdx.x + w];
        __syncthreads();
    }
    return sh[0];
}
// A row is live where minv != 0, frozen otherwise.  For every double -- NaN and both zeros included -- liveRow(m) and m != 0.
// agree; the test is on the BITS of minv because the library is built with -ffinite-math-only and without signed zeros, under
// which m != 0. ? m * e : 0. may be folded to m * e -- and a non-finite e (A z on a frozen row) would get through.
__device__ __forceinline__ bool liveRow(double m)
{
    return (__double_as_longlong(m) & 0x7fffffffffffffffLL) != 0;
}
// block sums of acc[0 .. n_rows) in a fixed order: partial[k * gridDim.x + blockIdx.x]
template < int n_rows >
__device__ __forceinline__ void storePartials(const double (&acc)[n_rows], double* __restrict__ sh, double* __restrict__ partial)
{
    for (int k = 0; k < n_rows; ++k)
    {
        if (k)
            __syncthreads();
        const double t = blockSum(acc[k], sh);
        if (threadIdx.x == 0)
            partial[k * gridDim.x + blockIdx.x] = t;
    }
}
// the finish stage of a reduction: s[dst0] = sum partial[0][:], s[dst1] = sum partial[1][:] (dst1 < 0: one row; no other slot is
// written)
static __global__ __launch_bounds__(cg_threads) void cgFinishKernel(const double* __restrict__ partial, int n_blocks,
                                                                    double* __restrict__ s, int dst0, int dst1)
{
    __shared__ double sh[cg_threads];
    for (int row = 0; row < (dst1 >= 0 ? 2 : 1); ++row)
    {
        double acc = 0.;
        for (int i = threadIdx.x; i < n_blocks; i += cg_threads)
            acc += partial[row * n_blocks + i];
        __syncthreads();
        const double t = blockSum(acc, sh);
        if (threadIdx.x == 0)
            s[row == 0 ? dst0 : dst1] = t;
    }
}
inline int cgWorkspace(l3k_ctx* ctx)
{
    if (!ctx->red_ws) // (allocated by l3k_ctx_create on the context's device)
    {
        setError("context without reduction workspace");
        return -3;
    }
    return 0;
}
// the slots of s that the finish stage of a reduction writes (cgFinishKernel)
struct Slots
{
    int dst0, dst1 = -1;
};
// the finish stage behind a kernel of n_blocks blocks that left its partials in the context's workspace
inline void launchFinish(l3k_ctx* ctx, int n_blocks, double* d_s, Slots to)
{
    hipLaunchKernelGGL(cgFinishKernel, dim3(1), dim3(cg_threads), 0, ctx->stream, ctx->red_ws, n_blocks, d_s, to.dst0, to.dst1);
}
} // namespace l3k::red
#endif
