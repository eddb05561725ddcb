// tri_shim.cpp -- l3k::TriangularPreconditioner (include/l3k/operator.hpp) used the way the reference uses
// alg_sys.solve(CG{opts, Ifpack2SGSOpts{}}) and alg_sys.solve(Gmres{opts, Ifpack2IluKOpts{}}) in tests/SolverTests.cpp:221-232: its
// makeSPDMatrix(100) -- tridiagonal [.5 2 .5], identity end rows, the zeroed couplings stored -- as a CsrOperator, b = A x*.  ILU(0)
// of a tridiagonal matrix is its LU: CG and GMRES stop after one iteration; SGS takes a few; the solutions are compared with x*.
// Build: hipcc -std=c++20 -Iinclude tests/cpp/tri_shim.cpp -Ll3ster_amd/lib -ll3k -o /tmp/tri_shim
#include "l3k/operator.hpp"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

template < typename T >
T* upload(const std::vector< T >& v)
{
    T* d = nullptr;
    if (hipMalloc(reinterpret_cast< void** >(&d), v.size() * sizeof(T)) != hipSuccess ||
        hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess)
    {
        std::fprintf(stderr, "HIP allocation failed\n");
        std::exit(2);
    }
    return d;
}

int main()
{
    constexpr int64_t n = 100;
    l3k::Context      ctx{0};
    int               failures = 0;

    std::vector< int64_t > row_ptr{0};
    std::vector< int32_t > col_ind;
    std::vector< double >  values, xs(n), b(n, 0.);
    for (int64_t i = 0; i < n; ++i)
    {
        const bool end = i == 0 || i == n - 1;
        xs[size_t(i)]  = std::cos(0.3 * double(i));
        if (i > 0)
            col_ind.push_back(int32_t(i - 1)), values.push_back(end || i == 1 ? 0. : .5);
        col_ind.push_back(int32_t(i)), values.push_back(end ? 1. : 2.);
        if (i + 1 < n)
            col_ind.push_back(int32_t(i + 1)), values.push_back(end || i == n - 2 ? 0. : .5);
        row_ptr.push_back(int64_t(col_ind.size()));
    }
    for (int64_t i = 0; i < n; ++i)
        for (int64_t e = row_ptr[size_t(i)]; e < row_ptr[size_t(i) + 1]; ++e)
            b[size_t(i)] += values[size_t(e)] * xs[size_t(col_ind[size_t(e)])];
    int64_t* d_rp = upload(row_ptr);
    int32_t* d_ci = upload(col_ind);
    double * d_v = upload(values), *d_b = upload(b), *d_x = upload(std::vector< double >(n, 0.));

    l3k::CsrOperator A{ctx, n, d_rp, d_ci, d_v};
    const auto       error_of = [&](const char* what, int iterations, double achieved) {
        std::vector< double > x(n);
        if (hipMemcpy(x.data(), d_x, n * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
            std::exit(2);
        double err = 0.;
        for (int64_t i = 0; i < n; ++i)
            err = std::fmax(err, std::fabs(x[size_t(i)] - xs[size_t(i)]));
        std::printf("%s: %d iterations, achieved %.3e, |x - x*|_inf %.3e\n", what, iterations, achieved, err);
        if (hipMemset(d_x, 0, n * sizeof(double)) != hipSuccess)
            std::exit(2);
        return err;
    };

    // an object that was not factored is refused by name
    l3k::TriangularPreconditioner ilu{A, l3k::TriangularPreconditioner::ilu0};
    bool                          threw = false;
    try
    {
        A.solve(d_b, d_x, ilu);
    }
    catch (const std::runtime_error& e)
    {
        threw = std::string{e.what()}.find("l3k_csr_pcg_solve_tri") != std::string::npos;
    }
    failures += !threw;

    ilu.factor();
    const auto info = ilu.info();
    failures += !(info.n == n && info.n_active == n && info.kind == L3K_TRI_ILU0 && info.n_levels_lower == n && info.n_levels_upper == n &&
                  info.n_launches_lower == 1 && info.n_launches_upper == 1 && info.factored == 1 && info.n_bad_pivots == 0 && info.bytes > 0);

    l3k_cg_opts cg_opts{1e-6, 10000, 2, 1};
    const auto  cg_ilu = A.solve(d_b, d_x, ilu, cg_opts);
    failures += !(cg_ilu.converged && cg_ilu.iterations == 1 && error_of("CG + ILU(0)", cg_ilu.iterations, cg_ilu.achieved_tol) <= 1e-12);

    l3k::Gmres     gmres{ctx, n, 30};
    l3k_gmres_opts gm_opts = l3k::Gmres::default_opts;
    gm_opts.tol = 1e-6, gm_opts.residual_scaling = 2;
    const auto gm_ilu = gmres.solve(A, d_b, d_x, ilu, gm_opts);
    failures += !(gm_ilu.converged && gm_ilu.iterations == 1 && gm_ilu.restarts == 0 &&
                  error_of("GMRES(30) + ILU(0)", gm_ilu.iterations, gm_ilu.achieved_tol) <= 1e-12);

    l3k::TriangularPreconditioner sgs{A, l3k::TriangularPreconditioner::sgs};
    sgs.factor();
    const auto cg_sgs = A.solve(d_b, d_x, sgs, cg_opts);
    failures += !(cg_sgs.converged && cg_sgs.iterations > 1 && cg_sgs.iterations <= 8 && error_of("CG + SGS", cg_sgs.iterations, cg_sgs.achieved_tol) <= 1e-5);
    const auto gm_sgs = gmres.solve(A, d_b, d_x, sgs, gm_opts);
    failures += !(gm_sgs.converged && gm_sgs.iterations > 1 && gm_sgs.iterations <= 8 &&
                  error_of("GMRES(30) + SGS", gm_sgs.iterations, gm_sgs.achieved_tol) <= 1e-5);

    // apply = solveUpper(solveLower), and SGS has no factor values
    double *d_y = upload(std::vector< double >(n, 0.)), *d_z = upload(std::vector< double >(n, 0.)), *d_z2 = upload(std::vector< double >(n, 0.));
    ilu.solveLower(d_b, d_y);
    ilu.solveUpper(d_y, d_z);
    ilu.apply(d_b, d_z2);
    std::vector< double > z(n), z2(n);
    if (hipMemcpy(z.data(), d_z, n * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(z2.data(), d_z2, n * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
        return 2;
    failures += !(z == z2);
    threw = false;
    try
    {
        sgs.values(d_y);
    }
    catch (const std::runtime_error& e)
    {
        threw = std::string{e.what()}.find("l3k_tri_values") != std::string::npos;
    }
    failures += !threw;

    // a damping outside (0, 2) is refused by the constructor
    threw = false;
    try
    {
        l3k_tri_opts bad = l3k::TriangularPreconditioner::sgs;
        bad.damping      = 2.;
        l3k::TriangularPreconditioner refused{A, bad};
    }
    catch (const std::runtime_error& e)
    {
        threw = std::string{e.what()}.find("outside (0, 2)") != std::string::npos;
    }
    failures += !threw;

    std::printf(failures ? "FAILED (%d)\n" : "OK\n", failures);
    return failures ? 1 : 0;
}
