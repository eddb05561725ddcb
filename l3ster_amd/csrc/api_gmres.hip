// api_gmres.hip -- restarted GMRES(m) of libl3k.so (include/l3k.h: l3k_gmres_*; the reference's Gmres, solve/BelosSolvers.hpp:124-130,
// with the restart options of solve/SolverInterface.hpp:26-37): right preconditioning, classical Gram-Schmidt with one
// re-orthogonalisation, written once over the operator value (LinOp, solver.hpp) for l3k_mf, l3k_mfs and l3k_csr on one rank and for
// the partitioned operators (l3k_mf with an l3k_halo, l3k_csr_dist), where every reducing pass is followed by one all-reduce.
// The kernels are in device/gmres.hpp.
#include "device/gmres.hpp"
#include "solver.hpp"

using namespace l3k::gmres;
using l3k::solver::LinOp;
using l3k::solver::Precond;

// the object behind l3k_gmres: one allocation, V | w | z | u (ld apart, ld a multiple of 4: the applies want aligned vectors), then
// the small arrays
struct l3k_gmres
{
    l3k_ctx*         ctx;
    int64_t          n, ld;
    int              m, ldh; // restart length; rows of H (m + 1)
    DevBuf< double > work;
    double *         V, *w, *z, *u, *H, *g, *cs, *sn, *h1, *h2, *t, *y, *partial, *sc;
};

namespace
{
constexpr l3k_gmres_opts gmres_default_opts{1e-6, 10000, 0, 1, 39}; // (opts == NULL, include/l3k.h)
const char* const        gmres_single_rank =
    "%s is the single-rank solver; this mesh has ghost nodes: partitioned systems call l3k_gmres_solve_dist";
inline int gmGrid(int64_t n)
{
    const int64_t g = (n + cg_threads - 1) / cg_threads;
    return int(g < 1 ? 1 : (g > cg_blocks ? cg_blocks : g));
}
inline bool overlap(const double* a, const double* b, int64_t n)
{
    return a < b + n && b < a + n;
}
// The route of a reducing pass over nb basis vectors (device/gmres.hpp): the row tile in LDS where nb columns of at least 16 rows
// fit the budget next to the 2 * 256 + T doubles of the shares, else the chunked sweeps.  L3K_GMRES_TILE in the environment (read
// once) is the switch of tools/bench_gmres.py: 0 takes the tile away, 16 / 32 / 64 set the budget in KB (default: tile_lds_kb)
struct PassPlan
{
    int    T, grid; // T == 0: chunked sweeps
    size_t lds;
};
constexpr int tile_lds_kb = 64;
PassPlan passPlan(int nb, int64_t n)
{
    static const int budget = [] { // doubles
        const char* e  = std::getenv("L3K_GMRES_TILE");
        const int   kb = e ? std::atoi(e) : tile_lds_kb;
        return (kb < 0 ? 0 : kb > 64 ? 64 : kb) * 128;
    }();
    if (nb >= gm_chunk && nb + 1 <= cg_threads)
        for (int T = cg_threads; T >= 16; T /= 2)
            if (int64_t(nb) * (T + 1) + 2 * cg_threads + T <= budget)
            {
                const int64_t tiles = n > 0 ? (n + T - 1) / T : 1; // (a rank that owns no row launches one workgroup, which writes 0)
                return {T, int(tiles < cg_blocks ? tiles : cg_blocks), size_t(int64_t(nb) * (T + 1) + 2 * cg_threads + T) * sizeof(double)};
            }
    return {0, gmGrid(n), 0};
}
// out[0 .. nb] <- V^T w, <w, w> (multiDot): first stage into `partial` ((nb + 1) * grid <= (nb + 1) * cg_blocks doubles), then the
// finish stage
int launchDots(l3k_ctx* ctx, double* partial, const double* V, size_t ld, int nb, const double* w, const double* mask, int64_t n,
               double* out, const double* sc)
{
    const PassPlan p = passPlan(nb, n);
    if (p.T)
        hipLaunchKernelGGL(tileKernel< false >, dim3(p.grid), dim3(cg_threads), p.lds, ctx->stream, V, ld, nb, const_cast< double* >(w), mask,
                           n, static_cast< const double* >(nullptr), partial, sc, p.T);
    else
        hipLaunchKernelGGL(multiDotKernel, dim3(p.grid), dim3(cg_threads), 0, ctx->stream, V, ld, nb, w, mask, n, partial, sc);
    hipLaunchKernelGGL(finishKernel, dim3(nb + 1), dim3(cg_threads), 0, ctx->stream, partial, p.grid, out, sc);
    L3K_HIP(hipGetLastError());
    return 0;
}
// w <- w - V h_in, out <- multiDot of the new w (projectRedot)
int launchProject(l3k_ctx* ctx, double* partial, const double* V, size_t ld, int nb, double* w, const double* mask, int64_t n,
                  const double* h_in, double* out, const double* sc)
{
    const PassPlan p = passPlan(nb, n);
    if (p.T)
        hipLaunchKernelGGL(tileKernel< true >, dim3(p.grid), dim3(cg_threads), p.lds, ctx->stream, V, ld, nb, w, mask, n, h_in, partial, sc, p.T);
    else
        hipLaunchKernelGGL(projectRedotKernel, dim3(p.grid), dim3(cg_threads), 0, ctx->stream, V, ld, nb, w, mask, n, h_in, partial, sc);
    hipLaunchKernelGGL(finishKernel, dim3(nb + 1), dim3(cg_threads), 0, ctx->stream, partial, p.grid, out, sc);
    L3K_HIP(hipGetLastError());
    return 0;
}
template < int mode >
int launchCombine(l3k_ctx* ctx, const double* V, size_t ld, int nb, const double* y, const double* minv, int64_t n, double* x)
{
    hipLaunchKernelGGL(combineKernel< mode >, dim3(gmGrid(n)), dim3(cg_threads), 0, ctx->stream, V, ld, nb, y, minv, n, x);
    L3K_HIP(hipGetLastError());
    return 0;
}
// the context's buffer for the partial sums of a piece: count doubles, grown on demand (what is on the stream finishes first)
int piecePartials(l3k_ctx* ctx, size_t count, double** out)
{
    if (ctx->gmres_partials_count < count)
    {
        L3K_HIP(hipStreamSynchronize(ctx->stream));
        if (ctx->gmres_partials)
            L3K_HIP(hipFree(ctx->gmres_partials));
        ctx->gmres_partials = nullptr, ctx->gmres_partials_count = 0;
        L3K_HIP(hipMalloc(reinterpret_cast< void** >(&ctx->gmres_partials), count * sizeof(double)));
        ctx->gmres_partials_count = count;
    }
    *out = ctx->gmres_partials;
    return 0;
}
int checkPiece(const char* who, const l3k_ctx* ctx, const void* V, size_t ld, int k, int64_t n, bool rest)
{
    if (!ctx || !V || !rest)
    {
        setError("%s: null argument", who);
        return -1;
    }
    if (k < 1 || n < 1)
    {
        setError("%s: k = %d and n = %lld must be at least 1", who, k, (long long)n);
        return -1;
    }
    if (ld % 4 != 0 || ld < size_t(n))
    {
        setError("%s: ld = %zu must be a multiple of 4 and at least n = %lld", who, ld, (long long)n);
        return -1;
    }
    return 0;
}
// The collective route (include/l3k.h): the halo's reduction block is held while a solve writes into it
struct ReduceHold
{
    l3k_halo* h;
    explicit ReduceHold(l3k_halo* halo) : h{halo}
    {
        if (h)
            l3k::halo::reduceHold(h, 1);
    }
    ReduceHold(const ReduceHold&)            = delete;
    ReduceHold& operator=(const ReduceHold&) = delete;
    ~ReduceHold()
    {
        if (h)
            l3k::halo::reduceHold(h, -1);
    }
};
// The solve (include/l3k.h).  Right preconditioner: P (cheb, pmg), else Jacobi d_minv, else none.  On a partitioned operator
// (A.halo; its reduce hook is allreduceRow) every reducing pass lands in this rank's row of the halo's block instead of `dst`, and
// the hook puts the sum over the ranks into `dst`: the kernels behind it read reduced values at the places they read today.  In a
// world of one there is no row, the passes land in `dst` and the hook enqueues nothing
int gmresSolve(l3k_gmres* G, const LinOp& A, const char* who, const double* d_b, double* d_x, const double* d_minv, const Precond* P,
               const l3k_gmres_opts* opts, l3k_gmres_result* result)
{
    if (G->ctx != A.ctx)
    {
        setError("%s: the workspace and the system belong to different contexts", who);
        return -1;
    }
    if (G->n != A.n)
    {
        setError("%s: the workspace was created for n = %lld, the operator has %lld rows", who, (long long)G->n, (long long)A.n);
        return -1;
    }
    if (P && (P->system != A.object || P->n != A.n))
    {
        setError("%s: the preconditioner was created for another system", who);
        return -1;
    }
    if (P && P->ld > G->ld) // (the scratch vectors handed to the preconditioner are G->ld apart)
    {
        setError("%s: the preconditioner's vectors are %lld apart, the workspace's %lld", who, (long long)P->ld, (long long)G->ld);
        return -1;
    }
    if (overlap(d_b, d_x, A.n))
    {
        setError("%s: b and x overlap", who);
        return -1;
    }
    const l3k_gmres_opts o   = opts ? *opts : gmres_default_opts;
    l3k_ctx* const       ctx = A.ctx;
    const hipStream_t    st  = ctx->stream;
    const int64_t        n = G->n, ld = G->ld;
    const int            m     = G->m, every = o.check_every > 0 ? o.check_every : 1;
    const double* const  mask  = P ? P->mask : d_minv;
    const int            grid  = gmGrid(n);
    const ReduceHold     hold{A.halo};
    double* const        row = A.halo ? l3k::halo::reduceRow(A.halo) : nullptr;
    const auto           land = [row](double* dst) { return row ? row : dst; };
    double               h[n_slots] = {};
    double               scale = 1., res = 0., est = 0.;
    int                  it = 0, cycles = 0, breakdown = 0;
    auto                 read = [&]() {
        L3K_HIP(hipMemcpyAsync(h, G->sc, sizeof h, hipMemcpyDeviceToHost, st));
        L3K_HIP(hipStreamSynchronize(st));
        return 0;
    };
    L3K_HIP(hipMemsetAsync(G->sc, 0, sizeof h, st));
    if (o.residual_scaling == 2) // sc[s_bb] = <b, b>
    {
        if (int rc = launchDots(ctx, G->partial, G->V, size_t(ld), 0, d_b, nullptr, n, land(G->sc + s_bb), nullptr))
            return rc;
        if (int rc = A.reduce(G->sc, s_bb, 1))
            return rc;
    }
    for (;; ++cycles)
    {
        // r = mask(b - A x) in v_0, beta
        if (int rc = A.apply(d_x, G->V))
            return rc;
        hipLaunchKernelGGL(residualKernel, dim3(grid), dim3(cg_threads), 0, st, G->V, d_b, mask, n, G->partial);
        hipLaunchKernelGGL(finishKernel, dim3(1), dim3(cg_threads), 0, st, G->partial, grid, land(G->sc + s_rr), nullptr);
        L3K_HIP(hipGetLastError());
        if (int rc = A.reduce(G->sc, s_rr, 1))
            return rc;
        if (int rc = read())
            return rc;
        const double beta = std::sqrt(h[s_rr]);
        if (cycles == 0)
        {
            if (o.residual_scaling == 1)
                scale = beta > 0. ? beta : 1.;
            else if (o.residual_scaling == 2)
                scale = std::sqrt(h[s_bb]) > 1e-300 ? std::sqrt(h[s_bb]) : 1e-300;
            est = beta / scale;
        }
        res = beta / scale;
        if (res <= o.tol || it >= o.max_iters || cycles > o.max_restarts || !(beta > 0.))
            break;
        hipLaunchKernelGGL(startCycleKernel, dim3(1), dim3(1), 0, st, G->sc, G->g);
        hipLaunchKernelGGL(scaleIntoKernel, dim3(grid), dim3(cg_threads), 0, st, G->V, G->V, n, G->sc, int(s_beta));
        L3K_HIP(hipGetLastError());
        const int steps = std::min(m, o.max_iters - it);
        int       kv    = 0;
        for (int k = 0; k < steps; ++k)
        {
            const double* vk = G->V + size_t(k) * ld;
            const double* z  = vk; // (no preconditioner: z = v_k, no copy)
            if (P)
            {
                if (int rc = P->apply(vk, G->z, G->w, G->u, nullptr))
                    return rc;
                z = G->z;
            }
            else if (d_minv)
            {
                hipLaunchKernelGGL(jacobiKernel, dim3(grid), dim3(cg_threads), 0, st, vk, d_minv, G->z, n);
                z = G->z;
            }
            if (int rc = A.apply(z, G->w))
                return rc;
            const int nb = k + 1;
            if (int rc = launchDots(ctx, G->partial, G->V, size_t(ld), nb, G->w, mask, n, land(G->h1), G->sc))
                return rc;
            if (int rc = A.reduce(G->h1, 0, nb + 1))
                return rc;
            if (int rc = launchProject(ctx, G->partial, G->V, size_t(ld), nb, G->w, mask, n, G->h1, land(G->h2), G->sc))
                return rc;
            if (int rc = A.reduce(G->h2, 0, nb + 1))
                return rc;
            if (int rc = launchProject(ctx, G->partial, G->V, size_t(ld), nb, G->w, mask, n, G->h2, land(G->t), G->sc))
                return rc;
            if (int rc = A.reduce(G->t, 0, nb + 1))
                return rc;
            hipLaunchKernelGGL(hessenbergKernel, dim3(1), dim3(cg_threads), 0, st, G->h1, G->h2, G->t, k, G->H, G->ldh, G->cs, G->sn, G->g,
                               G->sc);
            if (k + 1 < steps) // (the last step of a cycle needs no v_{k+1})
                hipLaunchKernelGGL(scaleIntoKernel, dim3(grid), dim3(cg_threads), 0, st, G->w, G->V + size_t(k + 1) * ld, n, G->sc, int(s_nu));
            L3K_HIP(hipGetLastError());
            if ((it + k + 1) % every == 0 || k + 1 == steps)
            {
                if (int rc = read())
                    return rc;
                kv  = int(h[s_kvalid]);
                est = h[s_est] / scale;
                if (h[s_breakdown] != 0. || est <= o.tol)
                    break;
            }
        }
        breakdown |= h[s_breakdown] != 0.;
        it += kv;
        // y = R^-1 g; x += M^-1 (V y)
        hipLaunchKernelGGL(triSolveKernel, dim3(1), dim3(cg_threads), 0, st, G->H, G->ldh, G->g, kv, G->y);
        L3K_HIP(hipGetLastError());
        if (!P)
        {
            if (int rc = launchCombine< 0 >(ctx, G->V, size_t(ld), kv, G->y, d_minv, n, d_x))
                return rc;
        }
        else
        {
            if (int rc = launchCombine< 1 >(ctx, G->V, size_t(ld), kv, G->y, nullptr, n, G->u))
                return rc;
            if (int rc = P->apply(G->u, G->z, G->w, G->V, nullptr)) // (u holds V y: the basis is free)
                return rc;
            if (int rc = launchCombine< 2 >(ctx, G->z, size_t(ld), 1, nullptr, mask, n, d_x))
                return rc;
        }
    }
    result->achieved_tol = res;
    result->estimate     = est;
    result->orth_loss    = h[s_orth];
    result->iterations   = it;
    result->restarts     = cycles > 1 ? cycles - 1 : 0; // (cycles run; the first one is no restart)
    result->converged    = res <= o.tol;
    result->breakdown    = breakdown;
    return 0;
}
int mfCheck(const char* who, l3k_gmres* G, const l3k_mf* mf, const double* d_b, const double* d_x, const void* precond, bool need_precond,
            const l3k_gmres_result* result)
{
    if (!G || !mf || !d_b || !d_x || !result || (need_precond && !precond))
    {
        setError("%s: null argument", who);
        return -1;
    }
    if (mf->mesh->n_ghost_nodes != 0)
    {
        setError(gmres_single_rank, who);
        return -1;
    }
    return 0;
}
int mfsCheck(const char* who, l3k_gmres* G, const l3k_mfs* S, const double* d_b, const double* d_x, const void* precond, bool need_precond,
             const l3k_gmres_result* result)
{
    if (!G || !S || !d_b || !d_x || !result || (need_precond && !precond))
    {
        setError("%s: null argument", who);
        return -1;
    }
    return l3k::solver::mfsSolvable(S, gmres_single_rank, who);
}
int csrCheck(const char* who, l3k_gmres* G, const l3k_csr* A, const double* d_b, const double* d_x, const void* precond, bool need_precond,
             const l3k_gmres_result* result)
{
    if (!G || !A || !d_b || !d_x || !result || (need_precond && !precond))
    {
        setError("%s: null argument", who);
        return -1;
    }
    return 0;
}
// l3k_gmres_create, and l3k_gmres_create_dist (one_rank == false): n is one rank's share of the rows then -- it may be 0, and it
// does not bound the restart length, which has to be the same on every rank
int createWorkspace(const char* who, bool one_rank, l3k_ctx* ctx, int64_t n, int restart_length, size_t max_bytes, l3k_gmres** out)
{
    if (!ctx || !out)
    {
        setError("%s: null argument", who);
        return -1;
    }
    if (n < (one_rank ? 1 : 0) || restart_length < 1)
    {
        setError("%s: n = %lld and restart_length = %d must be at least %s", who, (long long)n, restart_length, one_rank ? "1" : "0 and 1");
        return -1;
    }
    const int64_t m = one_rank ? std::min< int64_t >(restart_length, n) : restart_length; // (n rows span no more than n directions)
    if (m + 2 > hess_lds) // (the Hessenberg column of a step is rotated in LDS)
    {
        setError("%s: restart_length = %d above %d", who, restart_length, hess_lds - 2);
        return -1;
    }
    const int64_t ld = (n + 3) / 4 * 4;
    const size_t  small = size_t((m + 1) * m + (m + 1) + 2 * m + 3 * (m + 2) + (m + 1) + (m + 2) * int64_t(cg_blocks) + n_slots);
    const size_t  count = size_t((m + 1 + 3) * ld) + small;
    if (max_bytes != 0 && count * sizeof(double) > max_bytes)
    {
        setError("%s: the workspace of GMRES(%lld) on %lld rows needs %zu bytes, above max_bytes = %zu", who, (long long)m, (long long)n,
                 count * sizeof(double), max_bytes);
        return -1;
    }
    L3K_HIP(hipSetDevice(ctx->device));
    auto G = std::make_unique< l3k_gmres >();
    G->ctx = ctx, G->n = n, G->ld = ld, G->m = int(m), G->ldh = int(m + 1);
    if (int rc = G->work.alloc(count))
        return rc;
    L3K_HIP(hipMemsetAsync(G->work.ptr, 0, count * sizeof(double), ctx->stream));
    double* p = G->work.ptr;
    auto    take = [&](size_t c) {
        double* q = p;
        p += c;
        return q;
    };
    G->V = take(size_t((m + 1) * ld)), G->w = take(size_t(ld)), G->z = take(size_t(ld)), G->u = take(size_t(ld));
    G->H = take(size_t((m + 1) * m)), G->g = take(size_t(m + 1)), G->cs = take(size_t(m)), G->sn = take(size_t(m));
    G->h1 = take(size_t(m + 2)), G->h2 = take(size_t(m + 2)), G->t = take(size_t(m + 2)), G->y = take(size_t(m + 1));
    G->partial = take(size_t(m + 2) * cg_blocks), G->sc = take(n_slots);
    *out = G.release();
    return 0;
}
// The collective solves (include/l3k.h).  Every refusal comes before the first collective call
int distSolve(l3k_gmres* G, LinOp A, const char* who, const double* d_b, double* d_x, const double* d_minv, l3k_cheb* c,
              const l3k_gmres_opts* opts, l3k_gmres_result* result)
{
    if (A.n > 0 && (!d_b || !d_x))
    {
        setError("%s: null vector", who);
        return -1;
    }
    if (l3k::halo::context(A.halo) != A.ctx)
    {
        setError("%s: the halo and the system belong to different contexts", who);
        return -1;
    }
    if (c && (c->op.object != A.object || c->op.halo != A.halo))
    {
        setError("%s: the preconditioner was created for another system, or by a single-rank creator", who);
        return -1;
    }
    if (c && d_minv && d_minv != c->minv)
    {
        setError("%s: d_minv is not the array the preconditioner was created on (pass that one, or NULL)", who);
        return -1;
    }
    if (G->ctx == A.ctx && G->n == A.n && !overlap(d_b, d_x, A.n)) // (else gmresSolve refuses, and nothing is reserved)
        if (int rc = l3k::halo::reduceEnsure(A.halo, G->m + 1))
            return rc;
    A.reduce_fn = [](void* halo, double* d_vals, int count) { return l3k::halo::allreduceRow(static_cast< l3k_halo* >(halo), d_vals, count); };
    if (!c)
        return gmresSolve(G, A, who, d_b, d_x, d_minv, nullptr, opts, result);
    const Precond P = l3k::solver::chebPrecond(c);
    return gmresSolve(G, A, who, d_b, d_x, nullptr, &P, opts, result);
}
} // namespace

extern "C" {
int l3k_gmres_create(l3k_ctx* ctx, int64_t n, int restart_length, size_t max_bytes, l3k_gmres** out)
{
    return createWorkspace("l3k_gmres_create", true, ctx, n, restart_length, max_bytes, out);
}
int l3k_gmres_create_dist(l3k_ctx* ctx, int64_t n_owned, int restart_length, size_t max_bytes, l3k_gmres** out)
{
    return createWorkspace("l3k_gmres_create_dist", false, ctx, n_owned, restart_length, max_bytes, out);
}
int l3k_gmres_solve_dist(l3k_gmres* G, l3k_mf* mf, l3k_halo* halo, const double* d_b, double* d_x, const double* d_minv, l3k_cheb* cheb,
                         const l3k_gmres_opts* opts, l3k_gmres_result* result)
{
    if (!G || !mf || !halo || !result)
    {
        setError("l3k_gmres_solve_dist: null argument");
        return -1;
    }
    if (int rc = l3k::solver::haloFitsSystem("l3k_gmres_solve_dist", mf, halo))
        return rc;
    return distSolve(G, l3k::solver::mfDistOp(mf, halo), "l3k_gmres_solve_dist", d_b, d_x, d_minv, cheb, opts, result);
}
int l3k_csr_dist_gmres_solve(l3k_gmres* G, l3k_csr_dist* D, const double* d_b, double* d_x, const double* d_minv, l3k_cheb* cheb,
                             const l3k_gmres_opts* opts, l3k_gmres_result* result)
{
    if (!G || !D || !result)
    {
        setError("l3k_csr_dist_gmres_solve: null argument");
        return -1;
    }
    return distSolve(G, l3k::solver::csrDistOp(D), "l3k_csr_dist_gmres_solve", d_b, d_x, d_minv, cheb, opts, result);
}
int l3k_gmres_info_get(const l3k_gmres* G, l3k_gmres_info* out)
{
    if (!G || !out)
    {
        setError("l3k_gmres_info_get: null argument");
        return -1;
    }
    *out = {G->n, G->ld, G->m, G->work.n * sizeof(double)};
    return 0;
}
int l3k_gmres_destroy(l3k_gmres* G)
{
    delete G;
    return 0;
}
int l3k_gmres_solve(l3k_gmres* G, l3k_mf* mf, const double* d_b, double* d_x, const double* d_minv, const l3k_gmres_opts* opts,
                    l3k_gmres_result* result)
{
    if (int rc = mfCheck("l3k_gmres_solve", G, mf, d_b, d_x, nullptr, false, result))
        return rc;
    return gmresSolve(G, l3k::solver::mfOp(mf), "l3k_gmres_solve", d_b, d_x, d_minv, nullptr, opts, result);
}
int l3k_gmres_solve_cheb(l3k_gmres* G, l3k_mf* mf, const double* d_b, double* d_x, l3k_cheb* c, const l3k_gmres_opts* opts,
                         l3k_gmres_result* result)
{
    if (int rc = mfCheck("l3k_gmres_solve_cheb", G, mf, d_b, d_x, c, true, result))
        return rc;
    const Precond P = l3k::solver::chebPrecond(c);
    return gmresSolve(G, l3k::solver::mfOp(mf), "l3k_gmres_solve_cheb", d_b, d_x, nullptr, &P, opts, result);
}
int l3k_gmres_solve_pmg(l3k_gmres* G, l3k_mf* mf, const double* d_b, double* d_x, l3k_pmg* M, const l3k_gmres_opts* opts,
                        l3k_gmres_result* result)
{
    if (int rc = mfCheck("l3k_gmres_solve_pmg", G, mf, d_b, d_x, M, true, result))
        return rc;
    const Precond P = l3k::solver::pmgPrecond(M);
    return gmresSolve(G, l3k::solver::mfOp(mf), "l3k_gmres_solve_pmg", d_b, d_x, nullptr, &P, opts, result);
}
int l3k_csr_gmres_solve(l3k_gmres* G, l3k_csr* A, const double* d_b, double* d_x, const double* d_minv, const l3k_gmres_opts* opts,
                        l3k_gmres_result* result)
{
    if (int rc = csrCheck("l3k_csr_gmres_solve", G, A, d_b, d_x, nullptr, false, result))
        return rc;
    return gmresSolve(G, l3k::solver::csrOp(A), "l3k_csr_gmres_solve", d_b, d_x, d_minv, nullptr, opts, result);
}
int l3k_csr_gmres_solve_cheb(l3k_gmres* G, l3k_csr* A, const double* d_b, double* d_x, l3k_cheb* c, const l3k_gmres_opts* opts,
                             l3k_gmres_result* result)
{
    if (int rc = csrCheck("l3k_csr_gmres_solve_cheb", G, A, d_b, d_x, c, true, result))
        return rc;
    const Precond P = l3k::solver::chebPrecond(c);
    return gmresSolve(G, l3k::solver::csrOp(A), "l3k_csr_gmres_solve_cheb", d_b, d_x, nullptr, &P, opts, result);
}
int l3k_csr_gmres_solve_tri(l3k_gmres* G, l3k_csr* A, const double* d_b, double* d_x, l3k_tri* T, const l3k_gmres_opts* opts,
                            l3k_gmres_result* result)
{
    if (int rc = csrCheck("l3k_csr_gmres_solve_tri", G, A, d_b, d_x, T, true, result))
        return rc;
    if (int rc = l3k::solver::triReady(T, "l3k_csr_gmres_solve_tri"))
        return rc;
    const Precond P = l3k::solver::triPrecond(T);
    return gmresSolve(G, l3k::solver::csrOp(A), "l3k_csr_gmres_solve_tri", d_b, d_x, nullptr, &P, opts, result);
}
int l3k_mfs_gmres_solve(l3k_gmres* G, l3k_mfs* S, const double* d_b, double* d_x, const double* d_minv, const l3k_gmres_opts* opts,
                        l3k_gmres_result* result)
{
    if (int rc = mfsCheck("l3k_mfs_gmres_solve", G, S, d_b, d_x, nullptr, false, result))
        return rc;
    return gmresSolve(G, l3k::solver::mfsOp(S), "l3k_mfs_gmres_solve", d_b, d_x, d_minv, nullptr, opts, result);
}
int l3k_mfs_gmres_solve_cheb(l3k_gmres* G, l3k_mfs* S, const double* d_b, double* d_x, l3k_cheb* c, const l3k_gmres_opts* opts,
                             l3k_gmres_result* result)
{
    if (int rc = mfsCheck("l3k_mfs_gmres_solve_cheb", G, S, d_b, d_x, c, true, result))
        return rc;
    const Precond P = l3k::solver::chebPrecond(c);
    return gmresSolve(G, l3k::solver::mfsOp(S), "l3k_mfs_gmres_solve_cheb", d_b, d_x, nullptr, &P, opts, result);
}
// ------------------------------------------------------------------------------------------------ the pieces
// (no workspace object here: the partial sums go through a buffer of the context, grown on demand; the calls are asynchronous)
int l3k_gmres_multi_dot(l3k_ctx* ctx, const double* d_V, size_t ld, int k, const double* d_w, const double* d_mask, int64_t n, double* d_h)
{
    if (int rc = checkPiece("l3k_gmres_multi_dot", ctx, d_V, ld, k, n, d_w && d_h))
        return rc;
    double* partial = nullptr;
    if (int rc = piecePartials(ctx, size_t(k + 1) * cg_blocks, &partial))
        return rc;
    return launchDots(ctx, partial, d_V, ld, k, d_w, d_mask, n, d_h, nullptr);
}
int l3k_gmres_project(l3k_ctx* ctx, const double* d_V, size_t ld, int k, double* d_w, const double* d_mask, int64_t n, const double* d_h_in,
                      double* d_h_out)
{
    if (int rc = checkPiece("l3k_gmres_project", ctx, d_V, ld, k, n, d_w && d_h_in && d_h_out))
        return rc;
    double* partial = nullptr;
    if (int rc = piecePartials(ctx, size_t(k + 1) * cg_blocks, &partial))
        return rc;
    return launchProject(ctx, partial, d_V, ld, k, d_w, d_mask, n, d_h_in, d_h_out, nullptr);
}
int l3k_gmres_combine(l3k_ctx* ctx, const double* d_V, size_t ld, int k, const double* d_y, const double* d_minv, int64_t n, double* d_x)
{
    if (int rc = checkPiece("l3k_gmres_combine", ctx, d_V, ld, k, n, d_y && d_x))
        return rc;
    return launchCombine< 0 >(ctx, d_V, ld, k, d_y, d_minv, n, d_x);
}
} // extern "C"
