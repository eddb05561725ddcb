// gmres_shim.cpp -- l3k::Gmres (include/l3k/operator.hpp) used the way the reference uses alg_sys.solve(Gmres{...}): a non-symmetric
// tridiagonal matrix (-1 - c, 2.5 + 0.5 sin i, -1 + c), c = 0.5, on 1000 rows as a CsrOperator, b = A x* with x*_i = cos(0.1 i),
// Jacobi on the right, GMRES(30) to 1e-10 of |b|; the solution is compared with x*.  Conjugate gradients cannot serve this matrix.
// Build: hipcc -std=c++20 -Iinclude tests/cpp/gmres_shim.cpp -Ll3ster_amd/lib -ll3k -o /tmp/gmres_shim
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
    constexpr int64_t n = 1000;
    constexpr double  c = 0.5;
    l3k::Context      ctx{0};
    int               failures = 0;

    std::vector< int64_t > row_ptr{0};
    std::vector< int32_t > col_ind;
    std::vector< double >  values, xs(n), b(n, 0.), minv(n);
    for (int64_t i = 0; i < n; ++i)
    {
        xs[size_t(i)] = std::cos(0.1 * double(i));
        if (i > 0)
            col_ind.push_back(int32_t(i - 1)), values.push_back(-1. - c);
        col_ind.push_back(int32_t(i)), values.push_back(2.5 + 0.5 * std::sin(double(i)));
        if (i + 1 < n)
            col_ind.push_back(int32_t(i + 1)), values.push_back(-1. + c);
        row_ptr.push_back(int64_t(col_ind.size()));
        minv[size_t(i)] = 1. / (2.5 + 0.5 * std::sin(double(i)));
    }
    for (int64_t i = 0; i < n; ++i)
        for (int64_t e = row_ptr[size_t(i)]; e < row_ptr[size_t(i) + 1]; ++e)
            b[size_t(i)] += values[size_t(e)] * xs[size_t(col_ind[size_t(e)])];
    int64_t* d_rp = upload(row_ptr);
    int32_t* d_ci = upload(col_ind);
    double * d_v = upload(values), *d_b = upload(b), *d_minv = upload(minv), *d_x = upload(std::vector< double >(n, 0.));

    l3k::CsrOperator A{ctx, n, d_rp, d_ci, d_v};

    // a workspace above the limit is refused before anything is allocated, with the bytes in the message
    bool threw = false;
    try
    {
        l3k::Gmres too_small{ctx, n, 30, 1};
    }
    catch (const std::runtime_error& e)
    {
        threw = std::string{e.what()}.find("bytes") != std::string::npos;
    }
    failures += !threw;

    l3k::Gmres gmres{ctx, n, 30};
    const auto info = gmres.info();
    failures += !(info.n == n && info.ld % 4 == 0 && info.ld >= n && info.restart_length == 30 && info.bytes > 0);

    // a workspace of another size is refused
    threw = false;
    try
    {
        l3k::Gmres other{ctx, n + 1, 30};
        other.solve(A, d_b, d_x, d_minv);
    }
    catch (const std::runtime_error& e)
    {
        threw = std::string{e.what()}.find("l3k_csr_gmres_solve") != std::string::npos;
    }
    failures += !threw;

    l3k_gmres_opts opts = l3k::Gmres::default_opts;
    opts.tol = 1e-10, opts.residual_scaling = 2;
    const auto res = gmres.solve(A, d_b, d_x, d_minv, opts);
    std::vector< double > x(n);
    if (hipMemcpy(x.data(), d_x, n * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
        return 2;
    double err = 0.;
    for (int64_t i = 0; i < n; ++i)
        err = std::fmax(err, std::fabs(x[size_t(i)] - xs[size_t(i)]));
    std::printf("GMRES(30): %d iterations, %d restarts, achieved %.3e, estimate %.3e, orth_loss %.3e, |x - x*|_inf %.3e\n", res.iterations,
                res.restarts, res.achieved_tol, res.estimate, res.orth_loss, err);
    failures += !(res.converged && res.restarts >= 1 && res.achieved_tol <= 1e-10 && err <= 1e-8);

    // too few iterations: the wrapper throws like the reference
    threw = false;
    try
    {
        opts.max_iters = 3;
        if (hipMemset(d_x, 0, n * sizeof(double)) != hipSuccess)
            return 2;
        gmres.solve(A, d_b, d_x, d_minv, opts);
    }
    catch (const std::runtime_error& e)
    {
        threw = std::string{e.what()} == "Solver failed to converge";
    }
    failures += !threw;

    std::printf(failures ? "FAILED (%d)\n" : "OK\n", failures);
    return failures ? 1 : 0;
}
