// quad_condense_shim.cpp -- l3k::AssembledSystem with Condensation::ElementBoundary (include/l3k/operator.hpp), used the way the
// reference uses CondensationPolicy::ElementBoundary: the Diffusion2D problem of tests/Diffusion2D.hpp on 2 x 2 quads of order 3,
// Dirichlet T = x on the left and right sides, Adiabatic2D on the bottom and top; beginAssembly / assembleProblem / endAssembly on the
// condensed system, Jacobi PCG on the primary dofs, recover for the element-internal ones.  The solution [n] is written to argv[1]
// (raw doubles) for the Python test, which runs the same steps through system.AssembledSystem.
// Build: hipcc -std=c++20 -Iinclude tests/cpp/quad_condense_shim.cpp -Ll3ster_amd/lib -ll3k -o /tmp/quad_condense_shim
#include "l3k/operator.hpp"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <vector>

int main(int argc, char** argv)
{
    constexpr int    p = 3, U = 3, N1 = p + 1;
    l3k::Context     ctx{0};
    l3k::SquareMesh  mesh{{2, 2}, p};
    const auto&      v = mesh.view();
    const int64_t    n_nodes = mesh.nLocalNodes(), n = n_nodes * U;
    const int        temperature[] = {0};
    const auto       mask = mesh.dirichletMask(U, temperature, 0xc); // sides 2 (x = 0) and 3 (x = 1)
    l3k::DeviceMesh  dmesh{ctx, mesh, U, mask.data()};
    double gll[N1];
    l3k::check(l3k_gll_nodes(N1, gll));
    std::vector< double > x(size_t(n_nodes), 0.);
    for (int64_t e = 0; e < v.n_elems; ++e)
        for (int a = 0; a < N1 * N1; ++a)
        {
            const double  xi = gll[a % N1], eta = gll[a / N1];
            const double* c  = v.elem_verts + e * 12;
            x[v.elem_nodes[e * N1 * N1 + a]] = .25 * ((1. - xi) * (1. - eta) * c[0] + (1. + xi) * (1. - eta) * c[3] +
                                                      (1. - xi) * (1. + eta) * c[6] + (1. + xi) * (1. + eta) * c[9]);
        }
    std::vector< double > g(size_t(n), 0.);
    for (int64_t i = 0; i < n_nodes; ++i)
        g[size_t(i * U)] = mask[size_t(i * U)] ? x[size_t(i)] : 0.;
    double *d_g = nullptr, *d_x = nullptr, *d_minv = nullptr;
    if (hipMalloc(reinterpret_cast< void** >(&d_g), n * sizeof(double)) != hipSuccess ||
        hipMalloc(reinterpret_cast< void** >(&d_x), n * sizeof(double)) != hipSuccess ||
        hipMalloc(reinterpret_cast< void** >(&d_minv), n * sizeof(double)) != hipSuccess ||
        hipMemcpy(d_g, g.data(), n * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemset(d_x, 0, n * sizeof(double)) != hipSuccess)
    {
        std::fprintf(stderr, "HIP allocation failed\n");
        return 2;
    }

    l3k::MatrixFreeSystem diffusion{dmesh, L3K_KERNEL_DIFFUSION2D};
    const auto            walls = mesh.boundarySides(0x3); // sides 0 (y = 0) and 1 (y = 1)
    l3k::BoundaryTerm     adiabatic{dmesh, L3K_KERNEL_ADIABATIC2D, walls};
    l3k::AssembledSystem  sys{dmesh, {}, 1, 0, l3k::Condensation::ElementBoundary};
    int                   failures = 0;
    // recover on an open system is refused
    sys.beginAssembly();
    bool threw = false;
    try
    {
        sys.recover(d_x, size_t(n));
    }
    catch (const std::runtime_error& e)
    {
        threw = std::string{e.what()}.find("not closed") != std::string::npos;
    }
    failures += !threw;
    sys.assembleProblem(diffusion, 0, v.n_elems);
    sys.assembleProblem(adiabatic, 0, int64_t(walls.elems.size()));
    sys.endAssembly(d_g, size_t(n));
    const auto ci = sys.condInfo();
    failures += ci.condensed != 1 || ci.n_primary_nodes != 4 * p || ci.n_internal_nodes != (p - 1) * (p - 1) || ci.n_elems != v.n_elems ||
                ci.n_failed != 0;
    const auto res = sys.solve(d_x, d_minv, {1e-13, 20000, 2, 1});
    sys.recover(d_x, size_t(n));
    std::vector< double > sol(static_cast< size_t >(n));
    (void)hipMemcpy(sol.data(), d_x, n * sizeof(double), hipMemcpyDeviceToHost);
    double err = 0.;
    for (int64_t i = 0; i < n_nodes; ++i)
    {
        err = std::fmax(err, std::fabs(sol[size_t(i * U)] - x[size_t(i)]));
        err = std::fmax(err, std::fabs(sol[size_t(i * U + 1)] - 1.));
        err = std::fmax(err, std::fabs(sol[size_t(i * U + 2)]));
    }
    const auto info = sys.info();
    std::printf("condensed Diffusion2D: n = %lld, nnz = %lld, store %lld bytes, %d iterations, max nodal error against T = x, q = (1, 0): %.3e\n",
                (long long)info.n, (long long)info.nnz, (long long)ci.store_bytes, res.iterations, err);
    failures += !(err < 1e-7) || info.n_missing != 0 || info.state != L3K_ASM_CLOSED;
    // the element-level observable: W_e of the first element is symmetric
    const int             Nb = 4 * p * U;
    double*               d_W = nullptr;
    std::vector< double > W(size_t(Nb) * Nb);
    if (hipMalloc(reinterpret_cast< void** >(&d_W), W.size() * sizeof(double)) != hipSuccess)
        return 2;
    sys.schurUpdates(0, 1, d_W, nullptr);
    (void)hipMemcpy(W.data(), d_W, W.size() * sizeof(double), hipMemcpyDeviceToHost);
    double wmax = 0.;
    for (int i = 0; i < Nb; ++i)
        for (int j = 0; j < Nb; ++j)
        {
            failures += W[size_t(i) * Nb + j] != W[size_t(j) * Nb + i];
            wmax = std::fmax(wmax, std::fabs(W[size_t(i) * Nb + j]));
        }
    failures += !(wmax > 0.);
    if (argc > 1)
    {
        std::FILE* f = std::fopen(argv[1], "wb");
        if (!f || std::fwrite(sol.data(), sizeof(double), sol.size(), f) != sol.size())
            ++failures;
        if (f)
            std::fclose(f);
    }
    (void)hipFree(d_W);
    (void)hipFree(d_g);
    (void)hipFree(d_x);
    (void)hipFree(d_minv);
    std::printf(failures ? "FAILED\n" : "OK\n");
    return failures;
}
