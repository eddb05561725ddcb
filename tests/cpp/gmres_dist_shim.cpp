// gmres_dist_shim.cpp -- l3k::DistributedCsr::gmresSolve (include/l3k/operator.hpp) on TWO ranks, threads of this process over the
// in-process transport: the non-symmetric chain of tests/gmres_dist_ref.py -- the tridiagonal (-1 - c, 2.5 + 0.5 sin i, -1 + c),
// c = 0.9, 3 000 rows in sub-assembled form, link i with the owner of row i, a row's diagonal halved between its two links -- solved
// by the collective GMRES(30) with the Jacobi preconditioner, what alg_sys.solve(Gmres{...}) is on every rank of an MPI run of the
// reference, against x*_i = cos 0.1 i.  A rank thread only computes and stores; main compares.
// Build: hipcc -std=c++20 -Iinclude tests/cpp/gmres_dist_shim.cpp -Ll3ster_amd/lib -ll3k -o /tmp/gmres_dist_shim
#include "l3k/operator.hpp"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <exception>
#include <functional>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

namespace
{
constexpr int64_t N = 3000, HALF = N / 2;
constexpr double  C = 0.9;
double diagonal(int64_t i)
{
    return 2.5 + 0.5 * std::sin(double(i));
}
// the exchange lists of one rank of the chain, in the form Halo reads from a mesh's view(): rank 0 holds a ghost copy of rank 1's
// first row
struct ChainLists
{
    struct View
    {
        int            n_nbrs;
        const int*     nbr_rank;
        const int64_t *send_offsets, *ghost_offsets;
        const int32_t* send_nodes;
    };
    int     nbr;
    int64_t send_offsets[2], ghost_offsets[2];
    int32_t first = 0;
    explicit ChainLists(int rank) : nbr{1 - rank}, send_offsets{0, rank == 1 ? 1 : 0}, ghost_offsets{0, rank == 0 ? 1 : 0} {}
    View view() const { return {1, &nbr, send_offsets, ghost_offsets, &first}; }
};
struct Left
{
    std::vector< double > x;
    l3k_gmres_result      res{};
    std::string           error;
};
template < typename T >
T* upload(const std::vector< T >& h)
{
    T* d = nullptr;
    if (hipMalloc(reinterpret_cast< void** >(&d), (h.size() + 1) * sizeof(T)) != hipSuccess ||
        hipMemcpy(d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess)
        throw std::runtime_error{"HIP allocation failed"};
    return d;
}
void rankBody(int rank, const l3k::InprocGroup& group, Left& out)
try
{
    if (hipSetDevice(0) != hipSuccess)
        throw std::runtime_error{"hipSetDevice failed"};
    hipStream_t stream = nullptr;
    if (hipStreamCreate(&stream) != hipSuccess)
        throw std::runtime_error{"hipStreamCreate failed"};
    const int64_t s = rank * HALF, no = HALF, ng = rank == 0 ? 1 : 0, nl = no + ng;
    // the local matrix over [owned | ghost]: the links s .. s + no - 1 that exist (link i joins the rows i and i + 1)
    std::vector< int64_t > row_ptr{0};
    std::vector< int32_t > col;
    std::vector< double >  val;
    for (int64_t a = 0; a < nl; ++a)
    {
        const int64_t i = s + a; // global row
        const bool    from_left = a > 0 && i - 1 >= s, from_right = a < no && i + 1 < N; // links i - 1 and i of this rank
        if (from_left)
            col.push_back(int32_t(a - 1)), val.push_back(-1. - C);
        double d = 0.;
        if (from_left) // (an end row has one link, which takes the whole diagonal)
            d += (i == N - 1 ? 1. : 0.5) * diagonal(i);
        if (from_right)
            d += (i == 0 ? 1. : 0.5) * diagonal(i);
        if (from_left || from_right)
            col.push_back(int32_t(a)), val.push_back(d);
        if (from_right)
            col.push_back(int32_t(a + 1)), val.push_back(-1. + C);
        row_ptr.push_back(int64_t(col.size()));
    }
    const size_t          n_rows = static_cast< size_t >(no);
    std::vector< double > b(n_rows), minv(n_rows);
    const auto            xs = [](int64_t i) { return std::cos(0.1 * double(i)); };
    for (int64_t a = 0; a < no; ++a)
    {
        const int64_t i = s + a;
        b[size_t(a)]    = diagonal(i) * xs(i) + (i > 0 ? (-1. - C) * xs(i - 1) : 0.) + (i + 1 < N ? (-1. + C) * xs(i + 1) : 0.);
        minv[size_t(a)] = 1. / diagonal(i);
    }
    {
        l3k::Context              ctx{0, stream};
        const ChainLists          lists{rank};
        const l3k::Halo           halo{ctx, lists, 1, group.transport(rank), rank, 2};
        int64_t*                  d_row_ptr = upload(row_ptr);
        int32_t*                  d_col     = upload(col);
        const std::vector< double > zeros(n_rows, 0.);
        double *                  d_val = upload(val), *d_b = upload(b), *d_minv = upload(minv), *d_x = upload(zeros);
        const l3k::CsrOperator    local{ctx, nl, d_row_ptr, d_col, d_val};
        const l3k::DistributedCsr op{local, halo, no};
        const l3k::Gmres          ws = l3k::Gmres::collective(ctx, no, 30);
        out.res                      = op.gmresSolve(ws, d_b, d_x, d_minv, {1e-10, 10000, 2, 1, 39});
        ctx.synchronize();
        out.x.resize(size_t(no));
        if (hipMemcpy(out.x.data(), d_x, size_t(no) * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
            throw std::runtime_error{"hipMemcpy failed"};
        for (void* p : {static_cast< void* >(d_row_ptr), static_cast< void* >(d_col), static_cast< void* >(d_val), static_cast< void* >(d_b),
                        static_cast< void* >(d_minv), static_cast< void* >(d_x)})
            (void)hipFree(p);
    }
    (void)hipStreamDestroy(stream);
}
catch (const std::exception& e)
{
    out.error = e.what();
}
} // namespace

int main()
{
    l3k::InprocGroup group{2};
    Left             left[2];
    {
        std::thread t0{rankBody, 0, std::cref(group), std::ref(left[0])}, t1{rankBody, 1, std::cref(group), std::ref(left[1])};
        t0.join();
        t1.join();
    }
    int failures = 0;
    for (int r = 0; r < 2; ++r)
        if (!left[r].error.empty())
        {
            std::fprintf(stderr, "rank %d: %s\n", r, left[r].error.c_str());
            ++failures;
        }
    if (failures)
    {
        std::printf("FAILED\n");
        return failures;
    }
    double err = 0.;
    for (int r = 0; r < 2; ++r)
        for (int64_t a = 0; a < HALF; ++a)
            err = std::fmax(err, std::fabs(left[r].x[size_t(a)] - std::cos(0.1 * double(r * HALF + a))));
    const l3k_gmres_result &a = left[0].res, &b = left[1].res;
    std::printf("collective GMRES(30) on two ranks: %d iterations, %d restarts, achieved %.3e, max error against x* %.3e\n", a.iterations,
                a.restarts, a.achieved_tol, err);
    failures += !(a.converged && b.converged) || a.iterations != b.iterations || a.restarts != b.restarts || a.restarts < 1;
    failures += std::memcmp(&a.achieved_tol, &b.achieved_tol, sizeof(double)) != 0 || std::memcmp(&a.estimate, &b.estimate, sizeof(double)) != 0;
    failures += !(err <= 1e-7);
    std::printf(failures ? "FAILED\n" : "OK\n");
    return failures;
}
