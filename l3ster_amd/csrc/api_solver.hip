// api_solver.hip -- Jacobi-preconditioned conjugate gradients of libl3k.so: fused vector kernels and the drivers, written once over
// the matrix-free operator and the device CSR operator, of one rank or of a partitioned system (LinOp, solver.hpp: the partitioned
// makers bring the all-reduce of the scalar block as a hook, and the same loops are then the collective solves at the end of the file).
#include "reduce.hpp"
#include "solver.hpp"

namespace
{
// ---- fused vector kernels of the Jacobi-PCG iteration (solve/BelosSolvers.hpp:116-122 "Block CG" with one column +
// solve/NativePreconditioners.hpp:36-96).  Scalars live in a device array s: 0 <r,z>, 1 <p,Ap>, 2 <r,z> new, 3 <r,r>.
// Every dot product is a two-stage reduction in a fixed order (bitwise reproducible for a given grid).
using namespace l3k::red; // cg_threads, cg_blocks, liveRow, storePartials and the finish stage (reduce.hpp, shared with api_csr.hip)
// the rows of a thread: firstRow(), firstRow() + rowStep(), ... < n
__device__ __forceinline__ int64_t firstRow()
{
    return int64_t(blockIdx.x) * cg_threads + threadIdx.x;
}
__device__ __forceinline__ int64_t rowStep()
{
    return int64_t(gridDim.x) * cg_threads;
}
__global__ __launch_bounds__(cg_threads) void cgDotKernel(const double* __restrict__ u, const double* __restrict__ v, int64_t n,
                                                          double* __restrict__ partial)
{
    __shared__ double sh[cg_threads];
    double            acc[1] = {0.};
    for (int64_t i = firstRow(); i < n; i += rowStep())
        acc[0] += __builtin_nontemporal_load(u + i) * __builtin_nontemporal_load(v + i);
    storePartials(acc, sh, partial);
}
// the shift: <r,z> of this iteration becomes the old one.  A launch of its own AFTER the vector kernel that divides by s[0]:
// every block of that kernel must have read alpha and beta first
__global__ void cgShiftKernel(double* __restrict__ s)
{
    s[0] = s[2];
}
// The iteration keeps the PRECONDITIONED residual z = M^-1 r instead of r (Jacobi: r = z / minv element-wise), and x moves in the
// p pass: 9 vector passes per iteration instead of 11 (the vector kernels run at the HBM rate, so passes are what counts):
//   z pass:  alpha = s[0]/s[1]; z -= alpha minv Ap; partial <r, z>, <r, r> with r = z / minv     reads z, Ap, minv; writes z
//   p pass:  x += alpha p; beta = s[2]/s[0]; p = z + beta p                                       reads z, p, x;   writes p, x
// The same iterates in exact arithmetic; in floating point z is updated where r was (one rounding of minv * Ap more, one of
// minv * r less).  Rows with minv == 0 (a preconditioner zeroed on constrained dofs, l3k_jacobi_inverse with damping 0) are FROZEN:
// z = p = 0 there, x keeps its initial value, and -- since r cannot be recovered from z = 0 -- they are left out of <r, r>, i.e.
// the convergence test runs over the rows the iteration can change (include/l3k.h: l3k_pcg_solve).
__global__ __launch_bounds__(cg_threads) void cgUpdateZKernel(double* __restrict__ z, const double* __restrict__ ap,
                                                              const double* __restrict__ minv, const double* __restrict__ s,
                                                              int64_t n, double* __restrict__ partial)
{
    __shared__ double sh[cg_threads];
    const double      alpha  = s[0] / s[1];
    double            acc[2] = {0., 0.}; // <r, z>, <r, r>
    for (int64_t i = firstRow(); i < n; i += rowStep())
    {
        // (every array is streamed once and is far larger than the caches: non-temporal loads and stores, +3-6 % of HBM rate)
        const double m  = minv ? __builtin_nontemporal_load(minv + i) : 1.;
        const double zi = __builtin_nontemporal_load(z + i) - alpha * (m * __builtin_nontemporal_load(ap + i));
        const double ri = minv ? (liveRow(m) ? zi / m : 0.) : zi; // (0 / 0 on a frozen row would poison both sums)
        __builtin_nontemporal_store(zi, z + i);
        acc[0] += ri * zi;
        acc[1] += ri * ri;
    }
    storePartials(acc, sh, partial);
}
__global__ __launch_bounds__(cg_threads) void cgUpdatePXKernel(double* __restrict__ p, double* __restrict__ x, const double* __restrict__ z,
                                                               int64_t n, const double* __restrict__ s)
{
    const double alpha = s[0] / s[1], beta = s[2] / s[0];
    for (int64_t i = firstRow(); i < n; i += rowStep())
    {
        const double pi = __builtin_nontemporal_load(p + i);
        __builtin_nontemporal_store(__builtin_nontemporal_load(x + i) + alpha * pi, x + i);
        __builtin_nontemporal_store(__builtin_nontemporal_load(z + i) + beta * pi, p + i);
    }
}
// z = minv (b - r) (r holds A x0 on entry and z on return); p = z; partial <r, z>, <r, r>
__global__ __launch_bounds__(cg_threads) void cgInitKernel(double* __restrict__ r, const double* __restrict__ b,
                                                           double* __restrict__ p, const double* __restrict__ minv, int64_t n,
                                                           double* __restrict__ partial)
{
    __shared__ double sh[cg_threads];
    double            acc[2] = {0., 0.}; // <r, z>, <r, r>
    for (int64_t i = firstRow(); i < n; i += rowStep())
    {
        const double m  = minv ? __builtin_nontemporal_load(minv + i) : 1.;
        const double ri = liveRow(m) ? __builtin_nontemporal_load(b + i) - __builtin_nontemporal_load(r + i) : 0.; // (frozen rows: out of the residual norm from the start, as in the z pass)
        const double zi = m * ri;
        __builtin_nontemporal_store(zi, r + i);
        __builtin_nontemporal_store(zi, p + i);
        acc[0] += ri * zi;
        acc[1] += ri * ri;
    }
    storePartials(acc, sh, partial);
}
// NativeJacobiImpl::init (solve/NativePreconditioners.hpp:75-96): sign(d) * damping / max(|d|, threshold)
__global__ void jacobiInverseKernel(const double* __restrict__ d, int64_t n, double damping, double threshold, double* __restrict__ out)
{
    for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x)
    {
        const double v = d[i], a = fabs(v);
        out[i]         = (v < 0. ? -damping : damping) / (a > threshold ? a : threshold);
    }
}
inline int cgGrid(int64_t n)
{
    const int64_t g = (n + cg_threads - 1) / cg_threads;
    return int(g < 1 ? 1 : (g > cg_blocks ? cg_blocks : g));
}
// ---- Chebyshev-Jacobi preconditioner (solve/Ifpack2Preconditioners.hpp:26-36,107-131; include/l3k.h: l3k_cheb_create) and the
// vector kernels of the PCG that keeps r itself.  Frozen rows (liveRow) are stored as 0.
// w = z = c0 minv r (2 reads, 2 writes); with_dot: partial <r, z> (a polynomial of degree 1 ends here)
template < bool with_dot >
__global__ __launch_bounds__(cg_threads) void chebFirstKernel(const double* __restrict__ r, const double* __restrict__ minv, double c0,
                                                              double* __restrict__ w, double* __restrict__ z, int64_t n,
                                                              double* __restrict__ partial)
{
    __shared__ double sh[cg_threads];
    double            acc[1] = {0.};
    for (int64_t i = firstRow(); i < n; i += rowStep())
    {
        const double m  = minv ? __builtin_nontemporal_load(minv + i) : 1.;
        const double ri = __builtin_nontemporal_load(r + i);
        const double wi = liveRow(m) ? c0 * (m * ri) : 0.;
        __builtin_nontemporal_store(wi, w + i);
        __builtin_nontemporal_store(wi, z + i);
        if constexpr (with_dot)
            acc[0] += liveRow(m) ? ri * wi : 0.;
    }
    if constexpr (with_dot)
        storePartials(acc, sh, partial);
}
// w = a w + b minv (r - Az); z += w (5 reads, 2 writes: the 7 vector passes of an inner apply); with_dot: the last step of an
// application also leaves the partials of <r, z>, so the outer iteration has no pass of its own for that dot product
template < bool with_dot >
__global__ __launch_bounds__(cg_threads) void chebStepKernel(const double* __restrict__ r, const double* __restrict__ az,
                                                             const double* __restrict__ minv, double a, double b, double* __restrict__ w,
                                                             double* __restrict__ z, int64_t n, double* __restrict__ partial)
{
    __shared__ double sh[cg_threads];
    double            acc[1] = {0.};
    for (int64_t i = firstRow(); i < n; i += rowStep())
    {
        const double m    = minv ? __builtin_nontemporal_load(minv + i) : 1.;
        const double ri   = __builtin_nontemporal_load(r + i);
        const double wn   = a * __builtin_nontemporal_load(w + i) + b * (m * (ri - __builtin_nontemporal_load(az + i)));
        const double zn   = __builtin_nontemporal_load(z + i) + wn;
        const bool   live = liveRow(m);
        __builtin_nontemporal_store(live ? wn : 0., w + i);
        __builtin_nontemporal_store(live ? zn : 0., z + i);
        if constexpr (with_dot)
            acc[0] += live ? ri * zn : 0.;
    }
    if constexpr (with_dot)
        storePartials(acc, sh, partial);
}
// r = b - A x0 on the live rows (r holds A x0 on entry), 0 on the frozen ones; partial <r, r>
__global__ __launch_bounds__(cg_threads) void cgInitRKernel(double* __restrict__ r, const double* __restrict__ b,
                                                            const double* __restrict__ minv, int64_t n, double* __restrict__ partial)
{
    __shared__ double sh[cg_threads];
    double            acc[1] = {0.};
    for (int64_t i = firstRow(); i < n; i += rowStep())
    {
        const double m  = minv ? __builtin_nontemporal_load(minv + i) : 1.;
        const double d  = __builtin_nontemporal_load(b + i) - __builtin_nontemporal_load(r + i);
        const double ri = liveRow(m) ? d : 0.;
        __builtin_nontemporal_store(ri, r + i);
        acc[0] += ri * ri;
    }
    storePartials(acc, sh, partial);
}
// alpha = s[0]/s[1]; x += alpha p; r -= alpha Ap; partial <r, r> over the live rows (frozen rows: r = 0, x is not written).
// Reads x, r, p, Ap and the mask minv, writes x, r
__global__ __launch_bounds__(cg_threads) void cgUpdateRXKernel(double* __restrict__ x, double* __restrict__ r, const double* __restrict__ p,
                                                               const double* __restrict__ ap, const double* __restrict__ minv,
                                                               const double* __restrict__ s, int64_t n, double* __restrict__ partial)
{
    __shared__ double sh[cg_threads];
    const double      alpha  = s[0] / s[1];
    double            acc[1] = {0.};
    for (int64_t i = firstRow(); i < n; i += rowStep())
    {
        const double m  = minv ? __builtin_nontemporal_load(minv + i) : 1.;
        const double xn = __builtin_nontemporal_load(x + i) + alpha * __builtin_nontemporal_load(p + i);
        const double rn = __builtin_nontemporal_load(r + i) - alpha * __builtin_nontemporal_load(ap + i);
        const double ri = liveRow(m) ? rn : 0.;
        if (liveRow(m))
            __builtin_nontemporal_store(xn, x + i);
        __builtin_nontemporal_store(ri, r + i);
        acc[0] += ri * ri;
    }
    storePartials(acc, sh, partial);
}
// beta = s[2]/s[0]; p = z + beta p (the shift s[0] <- s[2] follows in cgShiftKernel, after every block has read beta)
__global__ __launch_bounds__(cg_threads) void cgUpdatePKernel(double* __restrict__ p, const double* __restrict__ z, int64_t n,
                                                              const double* __restrict__ s)
{
    const double beta = s[2] / s[0];
    for (int64_t i = firstRow(); i < n; i += rowStep())
        __builtin_nontemporal_store(__builtin_nontemporal_load(z + i) + beta * __builtin_nontemporal_load(p + i), p + i);
}
// power method on D^-1 A.  Start vector (include/l3k.h): y_i = h(i) * 2^-31 - 1 on the live rows; partial <y, y>
__global__ __launch_bounds__(cg_threads) void powerStartKernel(double* __restrict__ y, const double* __restrict__ minv, int64_t n,
                                                               double* __restrict__ partial)
{
    __shared__ double sh[cg_threads];
    double            acc[1] = {0.};
    for (int64_t i = firstRow(); i < n; i += rowStep())
    {
        uint32_t h = uint32_t(uint64_t(i));
        h ^= h >> 16;
        h *= 0x7feb352du;
        h ^= h >> 15;
        h *= 0x846ca68bu;
        h ^= h >> 16;
        const double yi = liveRow(__builtin_nontemporal_load(minv + i)) ? double(h) * 0x1p-31 - 1. : 0.;
        __builtin_nontemporal_store(yi, y + i);
        acc[0] += yi * yi;
    }
    storePartials(acc, sh, partial);
}
// y = minv (A x) in place (y holds A x on entry); partials <x, y>, <y, y>
__global__ __launch_bounds__(cg_threads) void powerStepKernel(double* __restrict__ y, const double* __restrict__ minv,
                                                              const double* __restrict__ x, int64_t n, double* __restrict__ partial)
{
    __shared__ double sh[cg_threads];
    double            acc[2] = {0., 0.};
    for (int64_t i = firstRow(); i < n; i += rowStep())
    {
        const double m  = __builtin_nontemporal_load(minv + i);
        const double yn = m * __builtin_nontemporal_load(y + i);
        const double yi = liveRow(m) ? yn : 0.;
        __builtin_nontemporal_store(yi, y + i);
        acc[0] += __builtin_nontemporal_load(x + i) * yi;
        acc[1] += yi * yi;
    }
    storePartials(acc, sh, partial);
}
// ... followed by the rescale x = y * s^-1/2 with s = <y, y> read from the device block
__global__ __launch_bounds__(cg_threads) void powerScaleKernel(double* __restrict__ x, const double* __restrict__ y, int64_t n,
                                                               const double* __restrict__ s)
{
    const double f = 1. / sqrt(s[1]);
    for (int64_t i = firstRow(); i < n; i += rowStep())
        __builtin_nontemporal_store(__builtin_nontemporal_load(y + i) * f, x + i);
}
// ------------------------------------------------------------------------------------------------ launches
// One reducing pass over n rows: kernel(args..., n, partials), then the finish stage into s[to.dst0] (and s[to.dst1]).  d_s == nullptr:
// the kernel alone (an instance that leaves no partials)
template < typename... Params, typename... Args >
int launchReduce(l3k_ctx* ctx, void (*kernel)(Params...), int64_t n, double* d_s, Slots to, Args... args)
{
    if (int rc = cgWorkspace(ctx))
        return rc;
    const int g = cgGrid(n);
    hipLaunchKernelGGL(kernel, dim3(g), dim3(cg_threads), 0, ctx->stream, args..., n, ctx->red_ws);
    if (d_s)
        launchFinish(ctx, g, d_s, to);
    L3K_HIP(hipGetLastError());
    return 0;
}
// s[0] <- s[2], enqueued behind the vector kernel that read s[0] (cgShiftKernel)
int launchShift(l3k_ctx* ctx, double* d_s)
{
    hipLaunchKernelGGL(cgShiftKernel, dim3(1), dim3(1), 0, ctx->stream, d_s);
    L3K_HIP(hipGetLastError());
    return 0;
}
// ------------------------------------------------------------------------------------------------ single-rank drivers
// What l3k_pcg_solve and l3k_pcg_solve_cheb share around their loop bodies
constexpr l3k_cg_opts cg_default_opts{1e-6, 10000, 0, 1}; // (opts == NULL, include/l3k.h)
const char* const     pcg_single_rank =
    "%s is the single-rank solver; partitioned systems call l3k_pcg_solve_dist, or iterate with the l3k_cg_* pieces and an "
    "all-reduce of the scalar block between them (l3ster_amd/solve.py)";
const char* const cheb_single_rank =
    "%s serves single-rank systems; this mesh has ghost nodes: partitioned systems iterate with l3k_cheb_first / l3k_cheb_step / "
    "l3k_cg_update_rx / l3k_cg_update_p and their own applies and all-reduces (pcg_distributed in l3ster_amd/solve.py), or call "
    "l3k_cheb_create_dist and l3k_pcg_solve_dist";
int singleRankOnly(const l3k_mf* mf, const char* message, const char* who)
{
    if (mf->mesh->n_ghost_nodes != 0)
    {
        setError(message, who);
        return -1;
    }
    return 0;
}
struct CgDriver
{
    l3k_cg_opts o;
    l3k_ctx*    ctx;
    double*     s; // the device block
    double      h[4] = {}, scale = 1., res = 0.;
    int         it = 0;

    int readScalars() // (the 32 bytes of a convergence check)
    {
        L3K_HIP(hipMemcpyAsync(h, s, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
        L3K_HIP(hipStreamSynchronize(ctx->stream));
        return 0;
    }
    // with s[3] = <r, r> of the initial residual (reduced) on the stream: the residual scale and the first scaled residual
    int start(const l3k::solver::LinOp& A, const double* d_b, int64_t n)
    {
        if (o.residual_scaling == 2)
        {
            if (int rc = l3k_cg_dot_pap(ctx, d_b, d_b, n, s)) // s[1] = <b, b> (scratch use of the slot)
                return rc;
            if (int rc = A.reduce(s, 1, 1))
                return rc;
        }
        if (int rc = readScalars())
            return rc;
        const double rr0 = std::sqrt(h[3]);
        if (o.residual_scaling == 1)
            scale = rr0 > 0. ? rr0 : 1.;
        else if (o.residual_scaling == 2)
            scale = std::sqrt(h[1]) > 1e-300 ? std::sqrt(h[1]) : 1e-300;
        res = rr0 / scale;
        return 0;
    }
    bool running() const { return res > o.tol && it < o.max_iters; }
    // one more iteration is on the stream: <r, r> is read every check_every iterations and after the last one
    int afterIteration()
    {
        ++it;
        if (it % (o.check_every > 0 ? o.check_every : 1) == 0 || it == o.max_iters)
        {
            if (int rc = readScalars())
                return rc;
            res = std::sqrt(h[3]) / scale;
        }
        return 0;
    }
    void report(l3k_cg_result* result) const
    {
        result->achieved_tol = res;
        result->iterations   = it;
        result->converged    = res <= o.tol;
    }
};
using l3k::solver::LinOp;
using l3k::solver::Precond;
int haloReduce(void* halo, double* d_vals, int count)
{
    return l3k_halo_allreduce_sum(static_cast< l3k_halo* >(halo), d_vals, count);
}
// <x, A x> of the partitioned matrix-free operator (LinOp::energy_route): the element kernels accumulate their elements' shares,
// l3k_cg_dot_pap the owned rows' -- the two do not add up across ranks, so all ranks take one route, agreed at the first call by
// all-reducing "my launches did not fuse" (it depends on the launch sizes only) in s[4], a slot the iteration does not use
int mfDistEnergy(const LinOp& op, const double* x, double* y, double* s)
{
    l3k_mf* const mf = static_cast< l3k_mf* >(op.object);
    const size_t  ld = size_t(op.n > 0 ? op.n : 1);
    if (op.energy_route == 2)
    {
        if (int rc = l3k_mf_apply_dist(mf, op.halo, x, ld, y, ld, 1, 1., 0.))
            return rc;
        return l3k_cg_dot_pap(op.ctx, x, y, op.n, s);
    }
    if (int rc = l3k_mf_energy_begin(mf, s))
        return rc;
    const int rc    = l3k_mf_apply_dist(mf, op.halo, x, ld, y, ld, 1, 1., 0.);
    int       fused = 0;
    if (int rc2 = l3k_mf_energy_end(mf, x, &fused))
        return rc2;
    if (rc)
        return rc;
    if (op.energy_route == 0)
    {
        double not_fused = fused ? 0. : 1.;
        L3K_HIP(hipMemcpyAsync(s + 4, &not_fused, sizeof not_fused, hipMemcpyHostToDevice, op.ctx->stream));
        L3K_HIP(hipStreamSynchronize(op.ctx->stream)); // (not_fused is a local)
        if (int rc3 = op.reduce(s, 4, 1))
            return rc3;
        L3K_HIP(hipMemcpyAsync(&not_fused, s + 4, sizeof not_fused, hipMemcpyDeviceToHost, op.ctx->stream));
        L3K_HIP(hipStreamSynchronize(op.ctx->stream));
        op.energy_route = not_fused == 0. ? 1 : 2;
    }
    else if (!fused)
    {
        setError("l3k_pcg_solve_dist: the element kernels stopped accumulating <p, A p>");
        return -3;
    }
    return op.energy_route == 1 ? 0 : l3k_cg_dot_pap(op.ctx, x, y, op.n, s); // (the dot product overwrites s[1])
}
} // namespace
LinOp l3k::solver::mfOp(l3k_mf* mf)
{
    return {mf->ctx, mf->mesh->nOwnedDofs(), mf,
            [](const LinOp& op, const double* x, double* y) {
                return l3k_mf_apply(static_cast< l3k_mf* >(op.object), x, size_t(op.n), y, size_t(op.n), 1, 1., 0.);
            },
            [](const LinOp& op, const double* x, double* y, double* s) {
                return l3k_mf_apply_energy(static_cast< l3k_mf* >(op.object), x, y, s);
            }};
}
LinOp l3k::solver::csrOp(l3k_csr* A)
{
    return {A->ctx, A->n, A,
            [](const LinOp& op, const double* x, double* y) {
                return l3k_csr_apply(static_cast< l3k_csr* >(op.object), x, size_t(op.n), y, size_t(op.n), 1, 1., 0.);
            },
            [](const LinOp& op, const double* x, double* y, double* s) {
                return l3k_csr_apply_energy(static_cast< l3k_csr* >(op.object), x, y, s);
            }};
}
LinOp l3k::solver::mfDistOp(l3k_mf* mf, l3k_halo* halo)
{
    return {mf->ctx,
            mf->mesh->nOwnedDofs(),
            mf,
            [](const LinOp& op, const double* x, double* y) {
                const size_t ld = size_t(op.n > 0 ? op.n : 1);
                return l3k_mf_apply_dist(static_cast< l3k_mf* >(op.object), op.halo, x, ld, y, ld, 1, 1., 0.);
            },
            &mfDistEnergy,
            &haloReduce,
            halo};
}
LinOp l3k::solver::csrDistOp(l3k_csr_dist* D)
{
    return {l3k::csr::contextOf(D),
            l3k::csr::ownedRows(D),
            D,
            [](const LinOp& op, const double* x, double* y) {
                const size_t ld = size_t(op.n > 0 ? op.n : 1);
                return l3k_csr_dist_apply(static_cast< l3k_csr_dist* >(op.object), x, ld, y, ld, 1, 1., 0.);
            },
            [](const LinOp& op, const double* x, double* y, double* s) {
                return l3k_csr_dist_apply_energy(static_cast< l3k_csr_dist* >(op.object), x, y, s);
            },
            &haloReduce,
            l3k::csr::haloOf(D)};
}
using l3k::solver::csrOp;
using l3k::solver::mfOp;
int l3k::solver::dotInto(l3k_ctx* ctx, const double* d_u, const double* d_v, int64_t n, double* d_s, int slot)
{
    return launchReduce(ctx, cgDotKernel, n, d_s, {slot}, d_u, d_v);
}

extern "C" {

// ------------------------------------------------------------------------------------------------ Jacobi-PCG
int l3k_jacobi_inverse(l3k_ctx* ctx, const double* d_diag, int64_t n, double damping, double threshold, double* d_minv)
{
    if (!ctx || (n > 0 && (!d_diag || !d_minv)))
    {
        setError("l3k_jacobi_inverse: null argument");
        return -1;
    }
    if (n > 0)
        hipLaunchKernelGGL(jacobiInverseKernel, dim3(gridFor(n)), dim3(256), 0, ctx->stream, d_diag, n, damping, threshold, d_minv);
    L3K_HIP(hipGetLastError());
    return 0;
}
int l3k_cg_init(l3k_ctx* ctx, double* d_r, const double* d_b, double* d_p, const double* d_minv, int64_t n, double* d_s)
{
    if (!ctx || !d_r || !d_b || !d_p || !d_s)
    {
        setError("l3k_cg_init: null argument");
        return -1;
    }
    if (int rc = launchReduce(ctx, cgInitKernel, n, d_s, {2, 3}, d_r, d_b, d_p, d_minv))
        return rc;
    return launchShift(ctx, d_s); // (this rank's <r,z> is the old one of the first iteration)
}
int l3k_cg_dot_pap(l3k_ctx* ctx, const double* d_p, const double* d_ap, int64_t n, double* d_s)
{
    if (!ctx || !d_p || !d_ap || !d_s)
    {
        setError("l3k_cg_dot_pap: null argument");
        return -1;
    }
    return launchReduce(ctx, cgDotKernel, n, d_s, {1}, d_p, d_ap);
}
int l3k_cg_update_z(l3k_ctx* ctx, double* d_z, const double* d_ap, const double* d_minv, int64_t n, double* d_s)
{
    if (!ctx || !d_z || !d_ap || !d_s)
    {
        setError("l3k_cg_update_z: null argument");
        return -1;
    }
    return launchReduce(ctx, cgUpdateZKernel, n, d_s, {2, 3}, d_z, d_ap, d_minv, d_s);
}
int l3k_cg_update_px(l3k_ctx* ctx, double* d_p, double* d_x, const double* d_z, int64_t n, double* d_s)
{
    if (!ctx || !d_p || !d_x || !d_z || !d_s)
    {
        setError("l3k_cg_update_px: null argument");
        return -1;
    }
    hipLaunchKernelGGL(cgUpdatePXKernel, dim3(cgGrid(n)), dim3(cg_threads), 0, ctx->stream, d_p, d_x, d_z, n, d_s);
    return launchShift(ctx, d_s);
}
} // extern "C"
namespace
{
// the iteration of l3k_pcg_solve / l3k_csr_pcg_solve (include/l3k.h)
int pcgSolve(const LinOp& A, const double* d_b, double* d_x, const double* d_minv, const l3k_cg_opts* opts, l3k_cg_result* result)
{
    l3k_ctx*         ctx = A.ctx;
    const int64_t    n   = A.n;
    DevBuf< double > work; // z (the preconditioned residual, in the array named r) | p | ap | s[8]
    if (int rc = work.alloc(size_t(3 * n + 8)))
        return rc;
    double *r = work.ptr, *p = r + n, *ap = p + n, *s = ap + n;
    if (n == 0) // (a rank of a partitioned system that owns no row may bring null vectors: the kernels touch none of them)
        d_b = d_x = work.ptr;
    CgDriver cg{opts ? *opts : cg_default_opts, ctx, s};
    // z = M^-1 (b - A x0), p = z
    if (int rc = A.apply(d_x, r))
        return rc;
    if (int rc = l3k_cg_init(ctx, r, d_b, p, d_minv, n, s))
        return rc;
    if (A.reduce_fn) // (l3k_cg_init shifted this rank's <r, z>: the reduced one is shifted again)
    {
        if (int rc = A.reduce(s, 2, 2))
            return rc;
        if (int rc = launchShift(ctx, s))
            return rc;
    }
    if (int rc = cg.start(A, d_b, n))
        return rc;
    while (cg.running())
    {
        if (int rc = A.applyEnergy(p, ap, s)) // ap = A p, s[1] = <p, A p>
            return rc;
        if (int rc = A.reduce(s, 1, 1))
            return rc;
        if (int rc = l3k_cg_update_z(ctx, r, ap, d_minv, n, s)) // (r holds z = M^-1 r)
            return rc;
        if (int rc = A.reduce(s, 2, 2))
            return rc;
        if (int rc = l3k_cg_update_px(ctx, p, d_x, r, n, s))
            return rc;
        if (int rc = cg.afterIteration())
            return rc;
    }
    cg.report(result);
    return 0;
}
// the same for a multivector of right-hand sides (the reference's systems carry n_rhs columns: Belos "Block CG" with block size 1
// iterates them one after the other, solve/BelosSolvers.hpp:116-122): column c of d_b / d_x at + c * ld; results[ncols]
int pcgCheckCols(const char* who, const void* object, size_t n, const double* d_b, size_t ldb, double* d_x, size_t ldx, int ncols,
                 const l3k_cg_result* results)
{
    if (!object || !d_b || !d_x || !results || ncols < 1)
    {
        setError("%s: bad argument", who);
        return -1;
    }
    if (ncols > 1 && (ldb < n || ldx < n))
    {
        setError("%s: leading dimension smaller than the number of owned dofs", who);
        return -1;
    }
    return 0;
}
int pcgSolveCols(const LinOp& A, const double* d_b, size_t ldb, double* d_x, size_t ldx, int ncols, const double* d_minv,
                 const l3k_cg_opts* opts, l3k_cg_result* results)
{
    for (int c = 0; c < ncols; ++c)
        if (int rc = pcgSolve(A, d_b + ldb * c, d_x + ldx * c, d_minv, opts, results + c))
            return rc;
    return 0;
}
} // namespace
extern "C" {
int l3k_pcg_solve(l3k_mf* mf, const double* d_b, double* d_x, const double* d_minv, const l3k_cg_opts* opts,
                  l3k_cg_result* result)
{
    if (!mf || !d_b || !d_x || !result)
    {
        setError("l3k_pcg_solve: null argument");
        return -1;
    }
    if (int rc = singleRankOnly(mf, pcg_single_rank, "l3k_pcg_solve"))
        return rc;
    return pcgSolve(mfOp(mf), d_b, d_x, d_minv, opts, result);
}
int l3k_csr_pcg_solve(l3k_csr* A, const double* d_b, double* d_x, const double* d_minv, const l3k_cg_opts* opts,
                      l3k_cg_result* result)
{
    if (!A || !d_b || !d_x || !result)
    {
        setError("l3k_csr_pcg_solve: null argument");
        return -1;
    }
    return pcgSolve(csrOp(A), d_b, d_x, d_minv, opts, result);
}
int l3k_pcg_solve_cols(l3k_mf* mf, const double* d_b, size_t ldb, double* d_x, size_t ldx, int ncols, const double* d_minv,
                       const l3k_cg_opts* opts, l3k_cg_result* results)
{
    if (int rc = pcgCheckCols("l3k_pcg_solve_cols", mf, mf ? size_t(mf->mesh->nOwnedDofs()) : 0, d_b, ldb, d_x, ldx, ncols, results))
        return rc;
    if (int rc = singleRankOnly(mf, pcg_single_rank, "l3k_pcg_solve")) // (each column is an l3k_pcg_solve)
        return rc;
    return pcgSolveCols(mfOp(mf), d_b, ldb, d_x, ldx, ncols, d_minv, opts, results);
}
int l3k_csr_pcg_solve_cols(l3k_csr* A, const double* d_b, size_t ldb, double* d_x, size_t ldx, int ncols, const double* d_minv,
                           const l3k_cg_opts* opts, l3k_cg_result* results)
{
    if (int rc = pcgCheckCols("l3k_csr_pcg_solve_cols", A, A ? size_t(A->n) : 0, d_b, ldb, d_x, ldx, ncols, results))
        return rc;
    return pcgSolveCols(csrOp(A), d_b, ldb, d_x, ldx, ncols, d_minv, opts, results);
}
// ------------------------------------------------------------------------------------------------ Chebyshev-Jacobi
} // extern "C"
int l3k::solver::chebApply(l3k_cheb* c, const double* r, double* z, double* w, double* az, double* d_s)
{
    l3k_ctx*  ctx = c->op.ctx;
    const int d   = c->info.degree;
    if (int rc = l3k_cheb_first(ctx, r, c->minv, c->coef.c0, w, z, c->n, d == 1 ? d_s : nullptr))
        return rc;
    for (int k = 1; k < d; ++k)
    {
        if (int rc = c->op.apply(z, az))
            return rc;
        if (int rc = l3k_cheb_step(ctx, r, az, c->minv, c->coef.a[k - 1], c->coef.b[k - 1], w, z, c->n, k == d - 1 ? d_s : nullptr))
            return rc;
    }
    return d_s ? c->op.reduce(d_s, 2, 1) : 0; // (the inner applies need no reduction; <r, z> is summed over the ranks)
}
using l3k::solver::chebApply;
extern "C" {
int l3k_cheb_first(l3k_ctx* ctx, const double* d_r, const double* d_minv, double c0, double* d_w, double* d_z, int64_t n, double* d_s)
{
    if (!ctx || !d_r || !d_w || !d_z)
    {
        setError("l3k_cheb_first: null argument");
        return -1;
    }
    return launchReduce(ctx, d_s ? chebFirstKernel< true > : chebFirstKernel< false >, n, d_s, {2}, d_r, d_minv, c0, d_w, d_z);
}
int l3k_cheb_step(l3k_ctx* ctx, const double* d_r, const double* d_az, const double* d_minv, double a, double b, double* d_w,
                  double* d_z, int64_t n, double* d_s)
{
    if (!ctx || !d_r || !d_az || !d_w || !d_z)
    {
        setError("l3k_cheb_step: null argument");
        return -1;
    }
    return launchReduce(ctx, d_s ? chebStepKernel< true > : chebStepKernel< false >, n, d_s, {2}, d_r, d_az, d_minv, a, b, d_w,
                        d_z);
}
int l3k_cg_update_rx(l3k_ctx* ctx, double* d_x, double* d_r, const double* d_p, const double* d_ap, const double* d_minv, int64_t n,
                     double* d_s)
{
    if (!ctx || !d_x || !d_r || !d_p || !d_ap || !d_s)
    {
        setError("l3k_cg_update_rx: null argument");
        return -1;
    }
    return launchReduce(ctx, cgUpdateRXKernel, n, d_s, {3}, d_x, d_r, d_p, d_ap, d_minv, d_s);
}
int l3k_cg_update_p(l3k_ctx* ctx, double* d_p, const double* d_z, int64_t n, double* d_s)
{
    if (!ctx || !d_p || !d_z || !d_s)
    {
        setError("l3k_cg_update_p: null argument");
        return -1;
    }
    hipLaunchKernelGGL(cgUpdatePKernel, dim3(cgGrid(n)), dim3(cg_threads), 0, ctx->stream, d_p, d_z, n, d_s);
    return launchShift(ctx, d_s); // (as in l3k_cg_update_px)
}
} // extern "C"
namespace
{
// l3k_cheb_create / l3k_csr_cheb_create (`who` in the messages): options, the power method on D^-1 A, the coefficients
int chebCreate(const LinOp& A, const char* who, const double* d_minv, const l3k_cheb_opts* opts, l3k_cheb** out)
{
    const l3k_cheb_opts o = opts ? *opts : l3k_cheb_opts{1, 30., 10, 1.1, 0.};
    if (const char* why = l3k::host::chebCheckOpts(o.degree, &o.cond_est, o.max_power_iters, &o.boost_factor, &o.lambda_max))
    {
        setError("%s: %s", who, why);
        return -1;
    }
    if (int rc = cgWorkspace(A.ctx))
        return rc;
    auto c  = std::make_unique< l3k_cheb >();
    c->op   = A;
    c->minv = d_minv;
    c->n    = A.n;
    c->ld   = (c->n + 3) / 4 * 4;
    if (int rc = c->work.alloc(size_t(2 * c->ld + 8)))
        return rc;
    l3k_ctx*      ctx = A.ctx;
    hipStream_t   st  = ctx->stream;
    const int64_t n   = c->n;
    double *      x = c->work.ptr, *y = x + c->ld, *s = y + c->ld;
    double        est   = o.lambda_max;
    int           steps = 0;
    if (!(o.lambda_max > 0.))
    {
        if (int rc = launchReduce(ctx, powerStartKernel, n, s, {1}, y, d_minv))
            return rc;
        if (int rc = A.reduce(s, 1, 1))
            return rc;
        for (; steps < o.max_power_iters; ++steps)
        {
            hipLaunchKernelGGL(powerScaleKernel, dim3(cgGrid(n)), dim3(cg_threads), 0, st, x, y, n, s);
            L3K_HIP(hipGetLastError());
            if (int rc = A.apply(x, y))
                return rc;
            if (int rc = launchReduce(ctx, powerStepKernel, n, s, {0, 1}, y, d_minv, x))
                return rc;
            if (int rc = A.reduce(s, 0, 2))
                return rc;
        }
        L3K_HIP(hipMemcpyAsync(&est, s, sizeof est, hipMemcpyDeviceToHost, st)); // (the one readback of the creation)
        L3K_HIP(hipStreamSynchronize(st));
        if (!l3k::host::chebFinite(&est) || !(est > 0.))
        {
            setError("%s: the power method on D^-1 A gave the eigenvalue estimate %g after %d steps; it must be finite and "
                     "positive (is the operator positive definite, and minv its inverse diagonal with at least one non-zero row?)",
                     who, est, steps);
            return -1;
        }
    }
    c->info.lambda_est       = est;
    c->info.lambda_max       = o.lambda_max > 0. ? o.lambda_max : o.boost_factor * est;
    c->info.lambda_min       = c->info.lambda_max / o.cond_est;
    c->info.degree           = o.degree;
    c->info.power_iters      = steps;
    c->info.applies_per_call = o.degree - 1;
    c->coef                  = l3k::host::chebCoeffs(c->info.lambda_max, c->info.lambda_min, o.degree);
    *out                     = c.release();
    return 0;
}
} // namespace
extern "C" {
int l3k_cheb_create(l3k_mf* mf, const double* d_minv, const l3k_cheb_opts* opts, l3k_cheb** out)
{
    if (!mf || !d_minv || !out)
    {
        setError("l3k_cheb_create: null argument");
        return -1;
    }
    if (int rc = singleRankOnly(mf, cheb_single_rank, "l3k_cheb_create"))
        return rc;
    return chebCreate(mfOp(mf), "l3k_cheb_create", d_minv, opts, out);
}
int l3k_csr_cheb_create(l3k_csr* A, const double* d_minv, const l3k_cheb_opts* opts, l3k_cheb** out)
{
    if (!A || !d_minv || !out)
    {
        setError("l3k_csr_cheb_create: null argument");
        return -1;
    }
    return chebCreate(csrOp(A), "l3k_csr_cheb_create", d_minv, opts, out);
}
int l3k_cheb_info_get(const l3k_cheb* c, l3k_cheb_info* out)
{
    if (!c || !out)
    {
        setError("l3k_cheb_info_get: null argument");
        return -1;
    }
    *out = c->info;
    return 0;
}
int l3k_cheb_apply(l3k_cheb* c, const double* d_r, double* d_z)
{
    if (!c || !d_r || !d_z)
    {
        setError("l3k_cheb_apply: null argument");
        return -1;
    }
    if (d_r < d_z + c->n && d_z < d_r + c->n) // (z is written before r is read for the last time)
    {
        setError("l3k_cheb_apply: r and z overlap");
        return -1;
    }
    return chebApply(c, d_r, d_z, c->work.ptr, c->work.ptr + c->ld, nullptr);
}
int l3k_cheb_destroy(l3k_cheb* c)
{
    delete c;
    return 0;
}
} // extern "C"
// the iteration of l3k_pcg_solve_cheb / l3k_csr_pcg_solve_cheb / l3k_pcg_solve_pmg (include/l3k.h)
int l3k::solver::pcgSolvePrecond(const LinOp& A, const char* who, const double* d_b, double* d_x, const Precond& M,
                                 const l3k_cg_opts* opts, l3k_cg_result* result)
{
    if (M.system != A.object)
    {
        setError("%s: the preconditioner was created for another system", who);
        return -1;
    }
    l3k_ctx*         ctx = A.ctx;
    const int64_t    n = M.n, ld = M.ld;
    DevBuf< double > work; // r | z | p | ap (A z inside the preconditioner) | w | s[8]
    if (int rc = work.alloc(size_t(5 * ld + 8)))
        return rc;
    double *r = work.ptr, *z = r + ld, *p = z + ld, *ap = p + ld, *w = ap + ld, *s = w + ld;
    if (n == 0) // (a rank of a partitioned system that owns no row may bring null vectors: the kernels touch none of them)
        d_b = d_x = work.ptr;
    CgDriver cg{opts ? *opts : cg_default_opts, ctx, s};
    // r = b - A x0 (0 on the frozen rows), s[3] = <r, r>
    if (int rc = A.apply(d_x, r))
        return rc;
    if (int rc = launchReduce(ctx, cgInitRKernel, n, s, {3}, r, d_b, M.mask))
        return rc;
    if (int rc = A.reduce(s, 3, 1))
        return rc;
    if (int rc = cg.start(A, d_b, n))
        return rc;
    if (cg.running())
    {
        // z = M^-1 r, s[2] = <r, z>; p = z; s[0] <- s[2]
        if (int rc = M.apply(r, z, w, ap, s))
            return rc;
        L3K_HIP(hipMemcpyAsync(p, z, size_t(n) * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
        if (int rc = launchShift(ctx, s))
            return rc;
    }
    while (cg.running())
    {
        if (int rc = A.applyEnergy(p, ap, s)) // ap = A p, s[1] = <p, A p>
            return rc;
        if (int rc = A.reduce(s, 1, 1))
            return rc;
        if (int rc = l3k_cg_update_rx(ctx, d_x, r, p, ap, M.mask, n, s))
            return rc;
        if (int rc = A.reduce(s, 3, 1))
            return rc;
        if (int rc = cg.afterIteration())
            return rc;
        if (cg.res <= cg.o.tol || cg.it >= cg.o.max_iters) // (x is final: no preconditioner application for a direction nobody takes)
            break;
        if (int rc = M.apply(r, z, w, ap, s)) // (ap is free until the next apply: it holds A z in here)
            return rc;
        if (int rc = l3k_cg_update_p(ctx, p, z, n, s))
            return rc;
    }
    cg.report(result);
    return 0;
}
// the Chebyshev object as the preconditioner of that loop
Precond l3k::solver::chebPrecond(l3k_cheb* c)
{
    return {c, c->op.object, c->minv, c->n, c->ld,
            [](void* o, const double* r, double* z, double* w, double* az, double* s) { return chebApply(static_cast< l3k_cheb* >(o), r, z, w, az, s); }};
}
using l3k::solver::chebPrecond;
extern "C" {
int l3k_pcg_solve_cheb(l3k_mf* mf, const double* d_b, double* d_x, l3k_cheb* c, const l3k_cg_opts* opts, l3k_cg_result* result)
{
    if (!mf || !d_b || !d_x || !c || !result)
    {
        setError("l3k_pcg_solve_cheb: null argument");
        return -1;
    }
    if (int rc = singleRankOnly(mf, cheb_single_rank, "l3k_pcg_solve_cheb"))
        return rc;
    return l3k::solver::pcgSolvePrecond(mfOp(mf), "l3k_pcg_solve_cheb", d_b, d_x, chebPrecond(c), opts, result);
}
int l3k_csr_pcg_solve_cheb(l3k_csr* A, const double* d_b, double* d_x, l3k_cheb* c, const l3k_cg_opts* opts, l3k_cg_result* result)
{
    if (!A || !d_b || !d_x || !c || !result)
    {
        setError("l3k_csr_pcg_solve_cheb: null argument");
        return -1;
    }
    return l3k::solver::pcgSolvePrecond(csrOp(A), "l3k_csr_pcg_solve_cheb", d_b, d_x, chebPrecond(c), opts, result);
}
} // extern "C"
// ------------------------------------------------------------------------------------------------ sums of matrix-free terms
// The same loops on l3k_mfs (include/l3k.h), single rank
using l3k::solver::mfsOp;
int l3k::solver::mfsSolvable(const l3k_mfs* S, const char* message, const char* who)
{
    if (!S->finalized)
    {
        setError("%s: call l3k_mfs_finalize first", who);
        return -1;
    }
    if (S->rows->n_ghost_nodes != 0)
    {
        setError(message, who);
        return -1;
    }
    return 0;
}
using l3k::solver::mfsSolvable;
extern "C" {
int l3k_mfs_pcg_solve(l3k_mfs* S, const double* d_b, double* d_x, const double* d_minv, const l3k_cg_opts* opts, l3k_cg_result* result)
{
    if (!S || !d_b || !d_x || !result)
    {
        setError("l3k_mfs_pcg_solve: null argument");
        return -1;
    }
    if (int rc = mfsSolvable(S, pcg_single_rank, "l3k_mfs_pcg_solve"))
        return rc;
    return pcgSolve(mfsOp(S), d_b, d_x, d_minv, opts, result);
}
int l3k_mfs_pcg_solve_cols(l3k_mfs* S, const double* d_b, size_t ldb, double* d_x, size_t ldx, int ncols, const double* d_minv,
                           const l3k_cg_opts* opts, l3k_cg_result* results)
{
    if (int rc = pcgCheckCols("l3k_mfs_pcg_solve_cols", S, S ? size_t(S->rows->nOwnedDofs()) : 0, d_b, ldb, d_x, ldx, ncols, results))
        return rc;
    if (int rc = mfsSolvable(S, pcg_single_rank, "l3k_mfs_pcg_solve")) // (each column is an l3k_mfs_pcg_solve)
        return rc;
    return pcgSolveCols(mfsOp(S), d_b, ldb, d_x, ldx, ncols, d_minv, opts, results);
}
int l3k_mfs_cheb_create(l3k_mfs* S, const double* d_minv, const l3k_cheb_opts* opts, l3k_cheb** out)
{
    if (!S || !d_minv || !out)
    {
        setError("l3k_mfs_cheb_create: null argument");
        return -1;
    }
    if (int rc = mfsSolvable(S, cheb_single_rank, "l3k_mfs_cheb_create"))
        return rc;
    return chebCreate(mfsOp(S), "l3k_mfs_cheb_create", d_minv, opts, out);
}
int l3k_mfs_pcg_solve_cheb(l3k_mfs* S, const double* d_b, double* d_x, l3k_cheb* c, const l3k_cg_opts* opts, l3k_cg_result* result)
{
    if (!S || !d_b || !d_x || !c || !result)
    {
        setError("l3k_mfs_pcg_solve_cheb: null argument");
        return -1;
    }
    if (int rc = mfsSolvable(S, cheb_single_rank, "l3k_mfs_pcg_solve_cheb"))
        return rc;
    return l3k::solver::pcgSolvePrecond(mfsOp(S), "l3k_mfs_pcg_solve_cheb", d_b, d_x, chebPrecond(c), opts, result);
}
} // extern "C"
// ------------------------------------------------------------------------------------------------ collective solves
// The same loops on a partitioned operator (include/l3k.h; solve/BelosSolvers.hpp:116-122 in an MPI run).  Every refusal comes
// before the first collective call: a rank that returns -1 here has left no peer waiting inside an exchange
int l3k::solver::haloFitsSystem(const char* who, const l3k_mf* mf, const l3k_halo* h)
{
    if (l3k::halo::context(h) != mf->ctx)
    {
        setError("%s: the halo and the system belong to different contexts", who);
        return -1;
    }
    const int dpn = mf->mesh->dofs_per_node;
    if (l3k::halo::dofsPerNode(h) != dpn || l3k_halo_n_ghost_dofs(h) != mf->mesh->n_ghost_nodes * dpn)
    {
        setError("%s: the halo (%d dofs per node, %lld ghost dofs) does not match the mesh (%d, %lld)", who, l3k::halo::dofsPerNode(h),
                 (long long)l3k_halo_n_ghost_dofs(h), dpn, (long long)(mf->mesh->n_ghost_nodes * dpn));
        return -1;
    }
    return 0;
}
using l3k::solver::haloFitsSystem;
namespace
{
int distSolve(const LinOp& A, const char* who, const double* d_b, double* d_x, const double* d_minv, l3k_cheb* c, const l3k_cg_opts* opts,
              l3k_cg_result* result)
{
    if (A.n > 0 && (!d_b || !d_x))
    {
        setError("%s: null vector", who);
        return -1;
    }
    if (int rc = cgWorkspace(A.ctx))
        return rc;
    if (!c)
        return pcgSolve(A, d_b, d_x, d_minv, opts, result);
    if (c->op.object != A.object || c->op.halo != A.halo)
    {
        setError("%s: the preconditioner was created for another system", who);
        return -1;
    }
    if (d_minv && d_minv != c->minv)
    {
        setError("%s: d_minv is not the array the preconditioner was created on (pass that one, or NULL)", who);
        return -1;
    }
    return l3k::solver::pcgSolvePrecond(A, who, d_b, d_x, chebPrecond(c), opts, result);
}
} // namespace
extern "C" {
int l3k_pcg_solve_dist(l3k_mf* mf, l3k_halo* halo, const double* d_b, double* d_x, const double* d_minv, l3k_cheb* cheb,
                       const l3k_cg_opts* opts, l3k_cg_result* result)
{
    if (!mf || !halo || !result)
    {
        setError("l3k_pcg_solve_dist: null argument");
        return -1;
    }
    if (int rc = haloFitsSystem("l3k_pcg_solve_dist", mf, halo))
        return rc;
    return distSolve(l3k::solver::mfDistOp(mf, halo), "l3k_pcg_solve_dist", d_b, d_x, d_minv, cheb, opts, result);
}
int l3k_csr_dist_pcg_solve(l3k_csr_dist* D, const double* d_b, double* d_x, const double* d_minv, l3k_cheb* cheb, const l3k_cg_opts* opts,
                           l3k_cg_result* result)
{
    if (!D || !result)
    {
        setError("l3k_csr_dist_pcg_solve: null argument");
        return -1;
    }
    return distSolve(l3k::solver::csrDistOp(D), "l3k_csr_dist_pcg_solve", d_b, d_x, d_minv, cheb, opts, result);
}
int l3k_cheb_create_dist(l3k_mf* mf, l3k_halo* halo, const double* d_minv, const l3k_cheb_opts* opts, l3k_cheb** out)
{
    if (!mf || !halo || !out || (!d_minv && mf->mesh->nOwnedDofs() > 0))
    {
        setError("l3k_cheb_create_dist: null argument");
        return -1;
    }
    if (int rc = haloFitsSystem("l3k_cheb_create_dist", mf, halo))
        return rc;
    return chebCreate(l3k::solver::mfDistOp(mf, halo), "l3k_cheb_create_dist", d_minv, opts, out);
}
int l3k_csr_dist_cheb_create(l3k_csr_dist* D, const double* d_minv, const l3k_cheb_opts* opts, l3k_cheb** out)
{
    if (!D || !out || (!d_minv && l3k::csr::ownedRows(D) > 0))
    {
        setError("l3k_csr_dist_cheb_create: null argument");
        return -1;
    }
    return chebCreate(l3k::solver::csrDistOp(D), "l3k_csr_dist_cheb_create", d_minv, opts, out);
}
} // extern "C"
