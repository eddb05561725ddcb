// chol_shim.cpp -- l3k::Cholesky (include/l3k/operator.hpp) used the way the reference uses alg_sys.solve(Klu2{}): the Diffusion2D
// problem of tests/Diffusion2D.hpp on 2 x 1 quads of order 4 with static condensation, Dirichlet values of the temperature on all
// four sides read from argv[1] (raw doubles [n], written by the Python test so that both routes start from the same bits);
// beginAssembly / assembleProblem / endAssembly, factor, solve, recover.  The solution [n] is written to argv[2] for the Python test,
// which runs the same steps through solve.direct_solve.  No entry of this system has more than two addends, so the assembled
// values, and with them the solution, are the same bits on every run.
// Build: hipcc -std=c++20 -Iinclude tests/cpp/chol_shim.cpp -Ll3ster_amd/lib -ll3k -o /tmp/chol_shim
#include "l3k/operator.hpp"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

int main(int argc, char** argv)
{
    constexpr int   p = 4, U = 3;
    l3k::Context    ctx{0};
    l3k::SquareMesh mesh{{2, 1}, p};
    const int64_t   n = mesh.nLocalNodes() * U;
    const int       temperature[] = {0};
    const auto      mask = mesh.dirichletMask(U, temperature, 0xf);
    l3k::DeviceMesh dmesh{ctx, mesh, U, mask.data()};
    int             failures = 0;

    std::vector< double > g(static_cast< size_t >(n), 0.);
    if (argc > 1)
    {
        std::FILE* f = std::fopen(argv[1], "rb");
        if (!f || std::fread(g.data(), sizeof(double), g.size(), f) != g.size())
            ++failures;
        if (f)
            std::fclose(f);
    }
    else
        for (int64_t i = 0; i < n; i += U)
            g[size_t(i)] = mask[size_t(i)] ? 1. : 0.;
    double *d_g = nullptr, *d_x = nullptr;
    if (hipMalloc(reinterpret_cast< void** >(&d_g), n * sizeof(double)) != hipSuccess ||
        hipMalloc(reinterpret_cast< void** >(&d_x), n * sizeof(double)) != hipSuccess ||
        hipMemcpy(d_g, g.data(), n * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemset(d_x, 0, n * sizeof(double)) != hipSuccess)
    {
        std::fprintf(stderr, "HIP allocation failed\n");
        return 2;
    }

    l3k::MatrixFreeSystem diffusion{dmesh, L3K_KERNEL_DIFFUSION2D};
    l3k::AssembledSystem  sys{dmesh, {}, 1, 0, l3k::Condensation::ElementBoundary};
    sys.beginAssembly();
    sys.assembleProblem(diffusion, 0, mesh.view().n_elems);
    sys.endAssembly(d_g, size_t(n));
    const auto info = sys.info();

    // a factor above the limit is refused before anything is allocated, with the bytes in the message
    bool threw = false;
    try
    {
        l3k::Cholesky too_small{info.csr, 1};
    }
    catch (const std::runtime_error& e)
    {
        threw = std::string{e.what()}.find("bytes") != std::string::npos;
    }
    failures += !threw;

    l3k::Cholesky chol{info.csr};
    // solving before factoring is refused
    threw = false;
    try
    {
        chol.solve(info.d_rhs, d_x);
    }
    catch (const std::runtime_error&)
    {
        threw = true;
    }
    failures += !threw;
    chol.factor();
    chol.solve(info.d_rhs, d_x);
    sys.recover(d_x, size_t(n));
    const auto ci = chol.info();
    failures += ci.n != n || ci.n_active <= 0 || ci.n_active >= n || ci.factored != 1 || ci.n_bad_pivots != 0 || ci.first_bad_row != -1 ||
                (ci.block != 32 && ci.block != 64) || ci.n_blocks != (ci.n_active + ci.block - 1) / ci.block;
    l3k::Cholesky moved{std::move(chol)};
    failures += moved.info().factored != 1;

    std::vector< double > sol(static_cast< size_t >(n));
    if (hipMemcpy(sol.data(), d_x, n * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
        ++failures;
    double largest = 0.;
    for (double v : sol)
    {
        failures += !std::isfinite(v);
        largest = std::fmax(largest, std::fabs(v));
    }
    failures += !(largest > 0.);
    std::printf("condensed Diffusion2D through l3k::Cholesky: n = %lld, active %lld, %lld blocks of %d, largest H %lld, %zu bytes\n",
                (long long)ci.n, (long long)ci.n_active, (long long)ci.n_blocks, ci.block, (long long)ci.max_height, ci.factor_bytes);
    if (argc > 2)
    {
        std::FILE* f = std::fopen(argv[2], "wb");
        if (!f || std::fwrite(sol.data(), sizeof(double), sol.size(), f) != sol.size())
            ++failures;
        if (f)
            std::fclose(f);
    }
    (void)hipFree(d_g);
    (void)hipFree(d_x);
    std::printf(failures ? "FAILED\n" : "OK\n");
    return failures;
}
