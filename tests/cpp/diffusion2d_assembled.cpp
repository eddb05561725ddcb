// diffusion2d_assembled.cpp -- l3k::AssembledSystem (include/l3k/operator.hpp) used the way the reference's 2-D regression test
// uses algsys::AssembledSystem (tests/Diffusion2D.hpp, Diffusion2DAssembledTest): 4 x 4 quads on [0,1]^2 at order 2, Dirichlet
// T = x on the left and right sides, Adiabatic2D on the bottom and top, beginAssembly / assembleProblem(domain kernel) /
// assembleProblem(boundary kernel) / endAssembly, Jacobi PCG at 1e-10 on the assembled matrix; T = x, q = (1, 0) lies in the
// discrete space.  Then the states: a closed system refuses assembleProblem, beginAssembly reopens it, and a second assembly gives
// the same solution.
// Build: hipcc -std=c++20 -Iinclude tests/cpp/diffusion2d_assembled.cpp -Ll3ster_amd/lib -ll3k -o /tmp/diffusion2d_assembled
#include "l3k/operator.hpp"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <vector>

int main()
{
    constexpr int    p = 2, U = 3, N1 = p + 1;
    l3k::Context     ctx{0};
    l3k::SquareMesh  mesh{{4, 4}, p};
    const auto&      v = mesh.view();
    const int64_t    n_nodes = mesh.nLocalNodes(), n = n_nodes * U;
    const int        temperature[] = {0};
    const auto       mask = mesh.dirichletMask(U, temperature, 0xc); // sides 2 (x = 0) and 3 (x = 1)
    l3k::DeviceMesh  dmesh{ctx, mesh, U, mask.data()};
    // x of every node from the vertices of its elements and the GLL points
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
        hipMemcpy(d_g, g.data(), n * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)
    {
        std::fprintf(stderr, "HIP allocation failed\n");
        return 2;
    }

    l3k::MatrixFreeSystem diffusion{dmesh, L3K_KERNEL_DIFFUSION2D};
    const auto            walls = mesh.boundarySides(0x3); // sides 0 (y = 0) and 1 (y = 1)
    l3k::BoundaryTerm     adiabatic{dmesh, L3K_KERNEL_ADIABATIC2D, walls};
    l3k::AssembledSystem  sys{dmesh};
    int                   failures = 0;
    const auto assemble_and_solve = [&](std::vector< double >& sol) {
        sys.beginAssembly();
        sys.assembleProblem(diffusion, 0, v.n_elems);
        sys.assembleProblem(adiabatic, 0, int64_t(walls.elems.size()));
        sys.endAssembly(d_g, size_t(n));
        (void)hipMemset(d_x, 0, n * sizeof(double));
        const auto res = sys.solve(d_x, d_minv, {1e-10, 20000, 2, 1});
        sol.resize(size_t(n));
        (void)hipMemcpy(sol.data(), d_x, n * sizeof(double), hipMemcpyDeviceToHost);
        return res;
    };
    std::vector< double > sol, again;
    const auto            res  = assemble_and_solve(sol);
    const auto            info = sys.info();
    double                err  = 0.;
    for (int64_t i = 0; i < n_nodes; ++i)
    {
        err = std::fmax(err, std::fabs(sol[size_t(i * U)] - x[size_t(i)]));
        err = std::fmax(err, std::fabs(sol[size_t(i * U + 1)] - 1.));
        err = std::fmax(err, std::fabs(sol[size_t(i * U + 2)]));
    }
    std::printf("assembled Diffusion2D: n = %lld, nnz = %lld, %d iterations, max nodal error against T = x, q = (1, 0): %.3e\n",
                (long long)info.n, (long long)info.nnz, res.iterations, err);
    failures += !(err < 1e-7) || info.n_missing != 0 || info.state != L3K_ASM_CLOSED || info.n != n || !info.csr;

    // a closed system refuses assembleProblem; beginAssembly reopens it
    bool threw = false;
    try
    {
        sys.assembleProblem(diffusion, 0, v.n_elems);
    }
    catch (const std::runtime_error& e)
    {
        threw = std::string{e.what()}.find("not open") != std::string::npos;
    }
    failures += !threw;
    l3k::AssembledSystem moved = std::move(sys); // move-only: the handle travels
    sys                        = std::move(moved);
    assemble_and_solve(again);
    double diff = 0.;
    for (size_t i = 0; i < sol.size(); ++i)
        diff = std::fmax(diff, std::fabs(sol[i] - again[i]));
    std::printf("second assembly: max difference of the solutions %.3e\n", diff);
    failures += !(diff < 1e-9);

    (void)hipFree(d_g);
    (void)hipFree(d_x);
    (void)hipFree(d_minv);
    std::printf(failures ? "FAILED\n" : "OK\n");
    return failures;
}
