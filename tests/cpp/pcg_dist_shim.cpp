// pcg_dist_shim.cpp -- l3k::DistributedCsr::pcgSolve and ::chebyshev (include/l3k/operator.hpp) in a WORLD OF ONE rank over the
// in-process transport: the Diffusion2D problem of tests/Diffusion2D.hpp on 3 x 2 quads of order 3 (tests/cpp/asm_dist_shim.cpp),
// assembled as a partitioned system and solved by the collective solve -- what alg_sys.solve(CG{...}) is on every rank of an MPI run
// of the reference -- with the Jacobi and with the Chebyshev-Jacobi preconditioner, against the single-rank solve on the local
// l3k_csr (the same iteration count) and against T = x, q = (1, 0).
// Build: hipcc -std=c++20 -Iinclude tests/cpp/pcg_dist_shim.cpp -Ll3ster_amd/lib -ll3k -o /tmp/pcg_dist_shim
#include "l3k/operator.hpp"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

int main()
{
    constexpr int    p = 3, U = 3, N1 = p + 1;
    l3k::Context     ctx{0};
    l3k::SquareMesh  mesh{{3, 2}, p, 0.1};
    const auto&      v = mesh.view();
    const int64_t    n_nodes = mesh.nLocalNodes(), n = n_nodes * U;
    const int        temperature[] = {0};
    const auto       mask = mesh.dirichletMask(U, temperature, 0xc); // sides 2 (x = 0) and 3 (x = 1)
    l3k::DeviceMesh  dmesh{ctx, mesh, U, mask.data()};
    l3k::InprocGroup group{1};
    l3k::Halo        halo{ctx, mesh, U, group.transport(0), 0, 1};
    double           gll[N1];
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
    double* d = nullptr; // g | x of the collective Jacobi solve | of the Chebyshev solve | of the single-rank solve | minv | s[8]
    if (hipMalloc(reinterpret_cast< void** >(&d), (5 * n + 8) * sizeof(double)) != hipSuccess ||
        hipMemset(d, 0, (5 * n + 8) * sizeof(double)) != hipSuccess ||
        hipMemcpy(d, g.data(), n * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)
    {
        std::fprintf(stderr, "HIP allocation failed\n");
        return 2;
    }
    double *d_g = d, *d_x = d + n, *d_xc = d + 2 * n, *d_x1 = d + 3 * n, *d_minv = d + 4 * n, *d_s = d + 5 * n;

    l3k::MatrixFreeSystem diffusion{dmesh, L3K_KERNEL_DIFFUSION2D};
    const auto            walls = mesh.boundarySides(0x3); // sides 0 (y = 0) and 1 (y = 1)
    l3k::BoundaryTerm     adiabatic{dmesh, L3K_KERNEL_ADIABATIC2D, walls};
    l3k::AssembledSystem  sys{dmesh, halo};
    int                   failures = 0;
    sys.beginAssembly();
    sys.assembleProblem(diffusion, 0, v.n_elems);
    sys.assembleProblem(adiabatic, 0, int64_t(walls.elems.size()));
    sys.endAssembly(d_g, size_t(n));
    const auto                info = sys.info();
    const l3k::DistributedCsr op   = sys.distributed();
    op.diag(nullptr, d_minv);
    // a reduction in a world of one leaves the values alone
    const double two = 2.;
    (void)hipMemcpy(d_s, &two, sizeof two, hipMemcpyHostToDevice);
    halo.allreduceSum(d_s, 1);
    double back = 0.;
    (void)hipMemcpy(&back, d_s, sizeof back, hipMemcpyDeviceToHost);
    failures += back != 2.;
    // the collective solves against the single-rank one
    const l3k_cg_opts   opts{1e-13, 20000, 2, 1};
    const l3k_cg_result jac = op.pcgSolve(info.d_rhs, d_x, d_minv, opts);
    const auto          ch  = op.chebyshev(d_minv, {2, 30., 10, 1.1, 0.});
    const auto          ci  = ch.info();
    const l3k_cg_result cheb = op.pcgSolve(info.d_rhs, d_xc, nullptr, opts, &ch);
    l3k_cg_result       one{};
    l3k::check(l3k_csr_pcg_solve(info.csr, info.d_rhs, d_x1, d_minv, &opts, &one));
    failures += jac.iterations != one.iterations || !(ci.lambda_est > 0.) || ci.power_iters != 10 || ci.degree != 2;
    failures += !(cheb.iterations < jac.iterations);
    // a preconditioner of another operator is refused
    {
        const l3k::CsrOperator   local2{ctx, info.n, info.d_row_ptr, info.d_col_ind, info.d_values};
        const l3k::DistributedCsr op2{local2, halo, n};
        bool                      threw = false;
        try
        {
            (void)op2.pcgSolve(info.d_rhs, d_x1, nullptr, opts, &ch);
        }
        catch (const std::runtime_error& e)
        {
            threw = std::string{e.what()}.find("another system") != std::string::npos;
        }
        failures += !threw;
    }
    double err = 0.;
    for (double* d_sol : {d_x, d_xc})
    {
        std::vector< double > sol(static_cast< size_t >(n));
        (void)hipMemcpy(sol.data(), d_sol, n * sizeof(double), hipMemcpyDeviceToHost);
        for (int64_t i = 0; i < n_nodes; ++i)
        {
            err = std::fmax(err, std::fabs(sol[size_t(i * U)] - x[size_t(i)]));
            err = std::fmax(err, std::fabs(sol[size_t(i * U + 1)] - 1.));
            err = std::fmax(err, std::fabs(sol[size_t(i * U + 2)]));
        }
    }
    std::printf("collective solve in a world of one: n = %lld, Jacobi %d iterations (single rank %d), Chebyshev degree 2 %d iterations, "
                "lambda_est %.6f, max nodal error against T = x, q = (1, 0): %.3e\n",
                (long long)info.n, jac.iterations, one.iterations, cheb.iterations, ci.lambda_est, err);
    failures += !(err < 1e-7);
    (void)hipFree(d);
    std::printf(failures ? "FAILED\n" : "OK\n");
    return failures;
}
