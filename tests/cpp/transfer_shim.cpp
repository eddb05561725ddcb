// l3k::Transfer of include/l3k/operator.hpp on a single-rank cube at orders 2 and 1: the prolongation of the constant 1 is 1 at every
// fine node (the rows of P sum to 1) and the restriction of 1 sums to the number of fine dofs (every fine node is read once); a pair
// in the wrong sequence throws.  Prints OK.
#include "l3k/operator.hpp"

#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <vector>

#define HIP_OK(call)                                                                                                   \
    do                                                                                                                 \
    {                                                                                                                  \
        if ((call) != hipSuccess)                                                                                      \
        {                                                                                                              \
            std::fprintf(stderr, "%s failed\n", #call);                                                                \
            return 1;                                                                                                  \
        }                                                                                                              \
    } while (0)

int main()
{
    constexpr int U = 2;
    l3k::Context    ctx;
    l3k::CubeMesh   fine_h({2, 2, 2}, 2), coarse_h({2, 2, 2}, 1);
    l3k::DeviceMesh fine(ctx, fine_h, U), coarse(ctx, coarse_h, U);
    l3k::Transfer   transfer(ctx, fine, coarse);
    const auto      info = transfer.info();
    if (info.order_fine != 2 || info.order_coarse != 1 || info.n_owned_dofs_fine != fine.nOwnedDofs() || info.n_ghost_dofs_coarse != 0)
        return 1;
    const size_t          nf = size_t(info.n_owned_dofs_fine), nc = size_t(info.n_owned_dofs_coarse);
    std::vector< double > ones(nf, 1.), xf(nf, 7.), rc(nc, 7.);
    double *              d_one, *d_xf, *d_rc;
    HIP_OK(hipMalloc(reinterpret_cast< void** >(&d_one), nf * sizeof(double)));
    HIP_OK(hipMalloc(reinterpret_cast< void** >(&d_xf), nf * sizeof(double)));
    HIP_OK(hipMalloc(reinterpret_cast< void** >(&d_rc), nc * sizeof(double)));
    HIP_OK(hipMemcpy(d_one, ones.data(), nf * sizeof(double), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_xf, xf.data(), nf * sizeof(double), hipMemcpyHostToDevice));
    transfer.prolong(d_one, nullptr, d_xf); // (nc <= nf: the first nc ones are the coarse vector)
    transfer.restrict(d_one, d_rc, nullptr);
    l3k::pmgResidual(ctx, d_xf, d_xf, d_one, d_one, int64_t(nf)); // x_f - 1 on every row (minv = 1: all live)
    ctx.synchronize();
    HIP_OK(hipMemcpy(xf.data(), d_xf, nf * sizeof(double), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(rc.data(), d_rc, nc * sizeof(double), hipMemcpyDeviceToHost));
    double worst = 0.;
    for (double v : xf)
        worst = std::max(worst, std::abs(v));
    const double sum = std::accumulate(rc.begin(), rc.end(), 0.);
    bool         threw = false;
    try
    {
        l3k::Transfer wrong(ctx, coarse, fine);
    }
    catch (const std::runtime_error&)
    {
        threw = true;
    }
    (void)hipFree(d_one), (void)hipFree(d_xf), (void)hipFree(d_rc);
    if (worst > 1e-13 || std::abs(sum - double(nf)) > 1e-10 * double(nf) || !threw)
    {
        std::printf("FAILED: |P 1 - 1| = %g, sum P^T 1 = %g of %zu, threw %d\n", worst, sum, nf, int(threw));
        return 1;
    }
    std::printf("OK\n");
    return 0;
}
