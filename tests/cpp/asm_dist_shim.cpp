// asm_dist_shim.cpp -- l3k::AssembledSystem(mesh, halo, ...) and l3k::DistributedCsr (include/l3k/operator.hpp) in a WORLD OF ONE rank
// over the in-process transport: the Diffusion2D problem of tests/Diffusion2D.hpp on 3 x 2 quads of order 3, Dirichlet T = x on the
// left and right sides, Adiabatic2D on the bottom and top; beginAssembly / assembleProblem / endAssembly on the partitioned system
// (prescribed values over the owned dofs), then the distributed operator against the local l3k_csr, which in a world of one is the
// same matrix: the apply and the Jacobi diagonal bit for bit, and the solve against T = x, q = (1, 0).
// Build: hipcc -std=c++20 -Iinclude tests/cpp/asm_dist_shim.cpp -Ll3ster_amd/lib -ll3k -o /tmp/asm_dist_shim
#include "l3k/operator.hpp"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

int main()
{
    constexpr int     p = 3, U = 3, N1 = p + 1;
    l3k::Context      ctx{0};
    l3k::SquareMesh   mesh{{3, 2}, p, 0.1};
    const auto&       v = mesh.view();
    const int64_t     n_nodes = mesh.nLocalNodes(), n = n_nodes * U;
    const int         temperature[] = {0};
    const auto        mask = mesh.dirichletMask(U, temperature, 0xc); // sides 2 (x = 0) and 3 (x = 1)
    l3k::DeviceMesh   dmesh{ctx, mesh, U, mask.data()};
    l3k::InprocGroup  group{1};
    l3k::Halo         halo{ctx, mesh, U, group.transport(0), 0, 1};
    double            gll[N1];
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
    std::vector< double > g(size_t(n), 0.), probe(static_cast< size_t >(n));
    for (int64_t i = 0; i < n_nodes; ++i)
        g[size_t(i * U)] = mask[size_t(i * U)] ? x[size_t(i)] : 0.;
    for (int64_t i = 0; i < n; ++i)
        probe[size_t(i)] = std::sin(0.37 * double(i));
    double* d = nullptr; // g | x | minv | minv of the local operator | probe | y | y of the local operator
    if (hipMalloc(reinterpret_cast< void** >(&d), 7 * n * sizeof(double)) != hipSuccess ||
        hipMemset(d, 0, 7 * n * sizeof(double)) != hipSuccess ||
        hipMemcpy(d, g.data(), n * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d + 4 * n, probe.data(), n * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)
    {
        std::fprintf(stderr, "HIP allocation failed\n");
        return 2;
    }
    double *d_g = d, *d_x = d + n, *d_minv = d + 2 * n, *d_minv1 = d + 3 * n, *d_probe = d + 4 * n, *d_y = d + 5 * n, *d_y1 = d + 6 * n;

    l3k::MatrixFreeSystem diffusion{dmesh, L3K_KERNEL_DIFFUSION2D};
    const auto            walls = mesh.boundarySides(0x3); // sides 0 (y = 0) and 1 (y = 1)
    l3k::BoundaryTerm     adiabatic{dmesh, L3K_KERNEL_ADIABATIC2D, walls};
    l3k::AssembledSystem  sys{dmesh, halo};
    int                   failures = 0;
    sys.beginAssembly();
    failures += sys.distInfo().dist != nullptr; // not handed out while the system is open
    bool threw = false;
    try
    {
        (void)sys.distributed();
    }
    catch (const std::runtime_error& e)
    {
        threw = std::string{e.what()}.find("not closed") != std::string::npos;
    }
    failures += !threw;
    sys.assembleProblem(diffusion, 0, v.n_elems);
    sys.assembleProblem(adiabatic, 0, int64_t(walls.elems.size()));
    sys.endAssembly(d_g, size_t(n));
    const auto info = sys.info();
    const auto di   = sys.distInfo();
    failures += info.state != L3K_ASM_CLOSED || info.n_missing != 0 || di.n_owned != n || di.n_ghost != 0 || !di.dist || !info.csr;
    const l3k::DistributedCsr op = sys.distributed();
    const auto                oi = op.info();
    failures += oi.n_owned != n || oi.n_ghost != 0 || oi.n_interior_rows != n || oi.n_border_rows != 0 || oi.n_ghost_rows != 0 ||
                oi.local != info.csr;
    // the apply and the diagonal of the distributed operator are those of the local one, bit for bit
    op.apply(d_probe, size_t(n), d_y, size_t(n), 1, -0.5, 0.);
    l3k::check(l3k_csr_apply(info.csr, d_probe, size_t(n), d_y1, size_t(n), 1, -0.5, 0.));
    op.diag(nullptr, d_minv);
    l3k::check(l3k_csr_diag(info.csr, nullptr, 1., 0., d_minv1));
    std::vector< double > a(static_cast< size_t >(2 * n)), b(static_cast< size_t >(2 * n));
    (void)hipMemcpy(a.data(), d_y, n * sizeof(double), hipMemcpyDeviceToHost);
    (void)hipMemcpy(a.data() + n, d_minv, n * sizeof(double), hipMemcpyDeviceToHost);
    (void)hipMemcpy(b.data(), d_y1, n * sizeof(double), hipMemcpyDeviceToHost);
    (void)hipMemcpy(b.data() + n, d_minv1, n * sizeof(double), hipMemcpyDeviceToHost);
    const bool same = std::memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0;
    double     ymax = 0.;
    for (int64_t i = 0; i < n; ++i)
        ymax = std::fmax(ymax, std::fabs(a[size_t(i)]));
    failures += !same || !(ymax > 0.);
    // the solve: in a world of one the local matrix is the global one
    l3k_cg_opts   opts{1e-13, 20000, 2, 1};
    l3k_cg_result res{};
    l3k::check(l3k_csr_pcg_solve(info.csr, info.d_rhs, d_x, d_minv, &opts, &res));
    std::vector< double > sol(static_cast< size_t >(n));
    (void)hipMemcpy(sol.data(), d_x, n * sizeof(double), hipMemcpyDeviceToHost);
    double err = 0.;
    for (int64_t i = 0; i < n_nodes; ++i)
    {
        err = std::fmax(err, std::fabs(sol[size_t(i * U)] - x[size_t(i)]));
        err = std::fmax(err, std::fabs(sol[size_t(i * U + 1)] - 1.));
        err = std::fmax(err, std::fabs(sol[size_t(i * U + 2)]));
    }
    std::printf("partitioned Diffusion2D in a world of one: n = %lld, nnz = %lld, apply and diagonal %s the local operator's, %d "
                "iterations, max nodal error against T = x, q = (1, 0): %.3e\n",
                (long long)info.n, (long long)info.nnz, same ? "equal" : "DIFFER FROM", res.iterations, err);
    failures += !res.converged || !(err < 1e-7);
    (void)hipFree(d);
    std::printf(failures ? "FAILED\n" : "OK\n");
    return failures;
}
