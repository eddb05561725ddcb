// multiterm_shim.cpp -- l3k::MultiTermSystem and l3k::ElementSubset (include/l3k/operator.hpp), used the way the reference sums
// assembleProblem calls over domains (tests/MultiDomainTest.cpp): 3 x 3 x 3 perturbed hexes of order 2, Diffusion3D with one set of
// coefficients on the elements [0, 10) and with another on [10, 27), each term on a mesh of its own over the same nodes, Dirichlet
// T on the sides z = 0 and z = 1.  On a deterministic context: y <- 0.7 A x - 0.3 y, then diag / rhs, the masked Jacobi inverse and
// a PCG solve.  y and the solution [n each] are written to argv[1] (raw doubles) for the Python test, which runs the same steps
// through system.MultiTermSystem and expects the same bits.
// Build: hipcc -std=c++20 -Iinclude tests/cpp/multiterm_shim.cpp -Ll3ster_amd/lib -ll3k -o /tmp/multiterm_shim
#include "l3k/operator.hpp"

#include <hip/hip_runtime.h>

#include <cstdio>
#include <numeric>
#include <vector>

namespace
{
struct Coefficients
{
    double k, s;
};
double* toDevice(const std::vector< double >& h)
{
    double* d = nullptr;
    if (hipMalloc(reinterpret_cast< void** >(&d), h.size() * sizeof(double)) != hipSuccess ||
        hipMemcpy(d, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)
        throw std::runtime_error{"HIP allocation failed"};
    return d;
}
} // namespace

int main(int argc, char** argv)
{
    constexpr int p = 2, U = 4, k_split = 10;
    l3k::Context  ctx{0};
    ctx.setDeterministic();
    l3k::CubeMesh mesh{{3, 3, 3}, p, {1, 1, 1}, 0, 0.1};
    const auto&   v = mesh.view();
    const int64_t n = mesh.nLocalNodes() * U;
    const int     temperature[] = {0};
    const auto    mask = mesh.dirichletMask(U, temperature, 0x3);
    std::vector< int64_t > all(static_cast< size_t >(v.n_elems));
    std::iota(all.begin(), all.end(), int64_t{0});
    const std::span< const int64_t > elems{all};
    l3k::ElementSubset    low{mesh, elems.first(k_split)}, high{mesh, elems.subspan(k_split)};
    l3k::DeviceMesh       rows{ctx, mesh, U, mask.data()}, mesh_low{ctx, low, U, mask.data()}, mesh_high{ctx, high, U, mask.data()};
    l3k::MatrixFreeSystem a{mesh_low, L3K_KERNEL_DIFFUSION3D, Coefficients{0.7, 1.3}}, b{mesh_high, L3K_KERNEL_DIFFUSION3D, Coefficients{2., 0.5}};
    l3k::MultiTermSystem  sys{rows};
    int                   failures = 0;
    sys.assembleProblem(a);
    sys.assembleProblem(b);
    bool threw = false;
    try
    {
        sys.apply(nullptr, size_t(n), nullptr, size_t(n));
    }
    catch (const std::runtime_error&)
    {
        threw = true; // (not finalized, and null vectors)
    }
    failures += !threw;
    sys.endAssembly();
    const auto info = sys.info();
    failures += info.n_terms != 2 || info.n_rows != n || info.n_active_rows != n || info.finalized != 1;

    // x_i, y_i in [-1/2, 1/2): exact binary fractions, the same on any host
    std::vector< double > x(static_cast< size_t >(n)), y(static_cast< size_t >(n));
    for (int64_t i = 0; i < n; ++i)
    {
        x[size_t(i)] = double(uint32_t(uint64_t(i) * 2654435761u)) * 0x1p-32 - .5;
        y[size_t(i)] = double(uint32_t(uint64_t(i) * 2246822519u)) * 0x1p-32 - .5;
    }
    double *d_x = toDevice(x), *d_y = toDevice(y);
    sys.apply(d_x, size_t(n), d_y, size_t(n), 1, .7, -.3);
    std::vector< double > zeros(static_cast< size_t >(n), 0.), out(static_cast< size_t >(2 * n));
    double *d_diag = toDevice(zeros), *d_rhs = toDevice(zeros), *d_minv = toDevice(zeros), *d_sol = toDevice(zeros);
    sys.diagAndRhs(nullptr, 0, d_diag, d_rhs, size_t(n));
    sys.jacobiInverse(d_diag, d_minv);
    const auto res = sys.solve(d_rhs, d_sol, d_minv, {1e-10, 5000, 1, 1});
    ctx.synchronize();
    (void)hipMemcpy(out.data(), d_y, n * sizeof(double), hipMemcpyDeviceToHost);
    (void)hipMemcpy(out.data() + n, d_sol, n * sizeof(double), hipMemcpyDeviceToHost);
    std::printf("two Diffusion3D terms on %d + %lld elements: n = %lld, %d iterations, residual %.3e\n", k_split, (long long)(v.n_elems - k_split),
                (long long)n, res.iterations, res.achieved_tol);
    if (argc > 1)
    {
        std::FILE* f = std::fopen(argv[1], "wb");
        if (!f || std::fwrite(out.data(), sizeof(double), out.size(), f) != out.size())
            ++failures;
        if (f)
            std::fclose(f);
    }
    for (double* d : {d_x, d_y, d_diag, d_rhs, d_minv, d_sol})
        (void)hipFree(d);
    std::printf(failures ? "FAILED\n" : "OK\n");
    return failures;
}
