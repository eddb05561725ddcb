// api_tri.hip -- the triangular preconditioners of libl3k.so on a device CSR operator (include/l3k.h: l3k_tri_*): symmetric
// Gauss-Seidel and ILU(0), what the reference reaches through Ifpack2 (solve/Ifpack2Preconditioners.hpp:97-101,134-157; run by
// tests/SolverTests.cpp:221-232).  The symbolic phase is host/tri_levels.cpp, the kernels are in device/tri.hpp; this file owns the
// object, the launch sequences and the preconditioner value the PCG and GMRES loops take.
#include "csr_launch.hpp"
#include "device/tri.hpp"
#include "host/tri_levels.hpp"
#include "solver.hpp"

struct l3k_tri
{
    l3k_csr*     A = nullptr;
    l3k_tri_opts o{};
    int64_t      n = 0, n_active = 0, ld = 0;
    int          fuse_rows = 0;
    // one side of the diagonal: the level-ordered rows and the launches that walk them
    struct Side
    {
        l3k::host::TriLevels              lv;
        std::vector< l3k::host::TriLaunch > plan;
        DevBuf< int32_t >                 rows;
        DevBuf< int64_t >                 level_ptr;
    } lower, upper;
    DevBuf< int64_t >            diag_pos;
    DevBuf< double >             mask, y; // 1 on the active rows; the vector between the two solves of an apply
    DevBuf< double >             dinv;    // SGS: omega / a_ii
    DevBuf< double >             f;       // ILU0: the factor in A's pattern
    DevBuf< unsigned long long > status;
    int64_t                      n_bad = 0, first_bad = -1;
    bool                         factored = false;
};

namespace
{
using namespace l3k::tri;
using l3k::csr::csrGrid;
using l3k::csr::withLanes;

int uploadSide(l3k_tri::Side& s, int64_t fuse_rows, hipStream_t st)
{
    s.plan = l3k::host::triPlan(s.lv, fuse_rows);
    if (int rc = s.rows.upload(s.lv.rows.data(), s.lv.rows.size(), st))
        return rc;
    return s.level_ptr.upload(s.lv.level_ptr.data(), s.lv.level_ptr.size(), st);
}
// the launches of one solve: z <- T^-1 r on the active rows, 0 on the others
template < int MODE >
int launchSolve(l3k_tri* T, const l3k_tri::Side& s, const double* r, double* z)
{
    const l3k_csr* A  = T->A;
    hipStream_t    st = A->ctx->stream;
    if (T->n_active < T->n) // (the columns of empty rows are read as 0)
        L3K_HIP(hipMemsetAsync(z, 0, size_t(T->n) * sizeof(double), st));
    const bool      sgs = MODE == sgs_lower || MODE == sgs_upper;
    const SolveArgs a{A->row_ptr, A->col_ind, T->diag_pos.ptr, sgs ? A->values : T->f.ptr, T->dinv.ptr, r, z,
                      (2. - T->o.damping) / T->o.damping};
    withLanes(A->lanes, [&](auto L) {
        for (const auto& p : s.plan)
            if (p.fused)
                hipLaunchKernelGGL((triFusedSolveKernel< L(), MODE >), dim3(1), dim3(cg_threads), 0, st, a, s.rows.ptr, s.level_ptr.ptr, p.l0, p.l1);
            else
            {
                const int64_t first = s.lv.level_ptr[size_t(p.l0)], count = s.lv.level_ptr[size_t(p.l1)] - first;
                hipLaunchKernelGGL((triLevelSolveKernel< L(), MODE >), dim3(csrGrid(count, L())), dim3(cg_threads), 0, st, a, s.rows.ptr + first, count);
            }
        return 0;
    });
    L3K_HIP(hipGetLastError());
    return 0;
}
int solveLower(l3k_tri* T, const double* r, double* y)
{
    return T->o.kind == L3K_TRI_SGS ? launchSolve< sgs_lower >(T, T->lower, r, y) : launchSolve< ilu0_lower >(T, T->lower, r, y);
}
int solveUpper(l3k_tri* T, const double* y, double* z)
{
    return T->o.kind == L3K_TRI_SGS ? launchSolve< sgs_upper >(T, T->upper, y, z) : launchSolve< ilu0_upper >(T, T->upper, y, z);
}
// the refusals every call on vectors shares
int checkVectors(const l3k_tri* T, const char* who, const double* in, const double* out)
{
    if (!T || (T->n > 0 && (!in || !out)))
    {
        setError("%s: null argument", who);
        return -1;
    }
    if (!T->factored)
    {
        setError("%s: nothing to solve with (l3k_tri_factor has not run, or its last run failed)", who);
        return -1;
    }
    if (T->n > 0 && l3k::csr::overlap(in, size_t(T->n), out, size_t(T->n)))
    {
        setError("%s: the input and the output vector overlap", who);
        return -1;
    }
    return 0;
}
int applyUnchecked(l3k_tri* T, const double* r, double* z)
{
    if (T->n_active == 0)
    {
        if (T->n > 0)
            L3K_HIP(hipMemsetAsync(z, 0, size_t(T->n) * sizeof(double), T->A->ctx->stream));
        return 0;
    }
    if (int rc = solveLower(T, r, T->y.ptr))
        return rc;
    return solveUpper(T, T->y.ptr, z);
}
} // namespace

int l3k::solver::triReady(const l3k_tri* T, const char* who)
{
    if (!T->factored)
    {
        setError("%s: the preconditioner is not factored (l3k_tri_factor has not run, or its last run failed)", who);
        return -1;
    }
    return 0;
}

// the object as the preconditioner of pcgSolvePrecond and of the GMRES loop: the mask is the object's own
l3k::solver::Precond l3k::solver::triPrecond(l3k_tri* T)
{
    return {T, T->A, T->mask.ptr, T->n, T->ld, [](void* o, const double* r, double* z, double*, double*, double* s) {
                l3k_tri* t = static_cast< l3k_tri* >(o);
                if (int rc = l3k_tri_apply(t, r, z))
                    return rc;
                return s ? l3k::solver::dotInto(t->A->ctx, r, z, t->n, s, 2) : 0;
            }};
}

extern "C" {

int l3k_tri_create(l3k_csr* A, const l3k_tri_opts* opts, l3k_tri** out)
{
    if (!A || !out)
    {
        setError("l3k_tri_create: null argument");
        return -1;
    }
    const l3k_tri_opts o = opts ? *opts : l3k_tri_opts{L3K_TRI_SGS, 1., 0., 1., 0};
    if (o.kind != L3K_TRI_SGS && o.kind != L3K_TRI_ILU0)
    {
        setError("l3k_tri_create: kind = %d; it is L3K_TRI_SGS (0) or L3K_TRI_ILU0 (1)", o.kind);
        return -1;
    }
    if (o.kind == L3K_TRI_SGS && !(o.damping > 0. && o.damping < 2.))
    {
        setError("l3k_tri_create: damping = %g outside (0, 2)", o.damping);
        return -1;
    }
    if (o.fuse_rows < 0)
    {
        setError("l3k_tri_create: fuse_rows = %d is negative", o.fuse_rows);
        return -1;
    }
    hipStream_t st = A->ctx->stream;
    auto        T  = std::make_unique< l3k_tri >();
    T->A = A, T->o = o, T->n = A->n, T->ld = (A->n + 3) / 4 * 4;
    T->fuse_rows = o.fuse_rows ? o.fuse_rows : cg_threads / A->lanes;
    {
        std::vector< int64_t > row_ptr(size_t(A->n) + 1, 0);
        std::vector< int32_t > col_ind(size_t(A->info.nnz));
        if (A->n > 0)
            L3K_HIP(hipMemcpyAsync(row_ptr.data(), A->row_ptr, row_ptr.size() * sizeof(int64_t), hipMemcpyDeviceToHost, st));
        if (A->info.nnz > 0)
            L3K_HIP(hipMemcpyAsync(col_ind.data(), A->col_ind, col_ind.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        L3K_HIP(hipStreamSynchronize(st));
        const int64_t bad = l3k::host::triFirstRowWithoutDiagonal(A->n, row_ptr.data(), col_ind.data());
        if (bad >= 0)
        {
            setError("l3k_tri_create: the active row %lld has no stored diagonal entry", (long long)bad);
            return -1;
        }
        l3k::host::triLevels(A->n, row_ptr.data(), col_ind.data(), false, T->lower.lv);
        l3k::host::triLevels(A->n, row_ptr.data(), col_ind.data(), true, T->upper.lv);
    }
    T->n_active = int64_t(T->lower.lv.rows.size());
    if (int rc = uploadSide(T->lower, T->fuse_rows, st))
        return rc;
    if (int rc = uploadSide(T->upper, T->fuse_rows, st))
        return rc;
    const size_t n1 = size_t(A->n > 0 ? A->n : 1);
    if (int rc = T->diag_pos.alloc(n1))
        return rc;
    if (int rc = T->mask.alloc(n1))
        return rc;
    if (int rc = T->y.alloc(n1))
        return rc;
    if (int rc = T->status.alloc(status_words))
        return rc;
    if (o.kind == L3K_TRI_SGS)
    {
        if (int rc = T->dinv.alloc(n1))
            return rc;
    }
    else if (int rc = T->f.alloc(size_t(A->info.nnz > 0 ? A->info.nnz : 1)))
        return rc;
    if (A->n > 0)
        hipLaunchKernelGGL(triDiagPosKernel, dim3(csrGrid(A->n, 1)), dim3(cg_threads), 0, st, A->row_ptr, A->col_ind, A->n, T->diag_pos.ptr,
                           T->mask.ptr);
    L3K_HIP(hipGetLastError());
    L3K_HIP(hipStreamSynchronize(st)); // (the uploads read the object's host vectors, which stay, but a failed copy shows here)
    *out = T.release();
    return 0;
}

int l3k_tri_factor(l3k_tri* T)
{
    if (!T)
    {
        setError("l3k_tri_factor: null argument");
        return -1;
    }
    const l3k_csr* A  = T->A;
    hipStream_t    st = A->ctx->stream;
    T->factored       = false;
    T->n_bad          = 0;
    T->first_bad      = -1;
    if (T->n_active == 0)
    {
        T->factored = true;
        return 0;
    }
    L3K_HIP(hipMemsetAsync(T->status.ptr, 0, sizeof(unsigned long long), st));
    L3K_HIP(hipMemsetAsync(T->status.ptr + 1, 0xff, sizeof(unsigned long long), st));
    if (T->o.kind == L3K_TRI_SGS)
        hipLaunchKernelGGL(triRecipDiagKernel, dim3(csrGrid(T->n, 1)), dim3(cg_threads), 0, st, T->diag_pos.ptr, A->values, T->n, T->o.damping,
                           T->dinv.ptr, T->status.ptr);
    else
    {
        L3K_HIP(hipMemcpyAsync(T->f.ptr, A->values, size_t(A->info.nnz) * sizeof(double), hipMemcpyDeviceToDevice, st));
        if (T->o.absolute_threshold != 0. || T->o.relative_threshold != 1.)
            hipLaunchKernelGGL(triThresholdKernel, dim3(csrGrid(T->n, 1)), dim3(cg_threads), 0, st, T->diag_pos.ptr, T->n,
                               T->o.absolute_threshold, T->o.relative_threshold, T->f.ptr);
        const FactorArgs a{A->row_ptr, A->col_ind, T->diag_pos.ptr, T->f.ptr, T->status.ptr};
        const auto&      s = T->lower;
        withLanes(A->lanes, [&](auto L) {
            for (const auto& p : s.plan)
                if (p.fused)
                    hipLaunchKernelGGL((triFusedFactorKernel< L() >), dim3(1), dim3(cg_threads), 0, st, a, s.rows.ptr, s.level_ptr.ptr, p.l0, p.l1);
                else
                {
                    const int64_t first = s.lv.level_ptr[size_t(p.l0)], count = s.lv.level_ptr[size_t(p.l1)] - first;
                    hipLaunchKernelGGL((triLevelFactorKernel< L() >), dim3(csrGrid(count, L())), dim3(cg_threads), 0, st, a, s.rows.ptr + first, count);
                }
            return 0;
        });
    }
    L3K_HIP(hipGetLastError());
    unsigned long long h[status_words];
    L3K_HIP(hipMemcpyAsync(h, T->status.ptr, sizeof h, hipMemcpyDeviceToHost, st));
    L3K_HIP(hipStreamSynchronize(st));
    if (h[0] != 0)
    {
        T->n_bad     = int64_t(h[0]);
        T->first_bad = h[1] < uint64_t(T->n) ? int64_t(h[1]) : -1;
        setError("l3k_tri_factor: %lld %s zero or not finite, the first at row %lld", (long long)T->n_bad,
                 T->o.kind == L3K_TRI_SGS ? "diagonal entries are" : "pivots are", (long long)T->first_bad);
        return -2;
    }
    T->factored = true;
    return 0;
}

int l3k_tri_apply(l3k_tri* T, const double* d_r, double* d_z)
{
    if (int rc = checkVectors(T, "l3k_tri_apply", d_r, d_z))
        return rc;
    return applyUnchecked(T, d_r, d_z);
}
int l3k_tri_solve_lower(l3k_tri* T, const double* d_r, double* d_y)
{
    if (int rc = checkVectors(T, "l3k_tri_solve_lower", d_r, d_y))
        return rc;
    return solveLower(T, d_r, d_y);
}
int l3k_tri_solve_upper(l3k_tri* T, const double* d_y, double* d_z)
{
    if (int rc = checkVectors(T, "l3k_tri_solve_upper", d_y, d_z))
        return rc;
    return solveUpper(T, d_y, d_z);
}
int l3k_tri_values(const l3k_tri* T, double* d_out)
{
    if (!T || (!d_out && T->A->info.nnz > 0))
    {
        setError("l3k_tri_values: null argument");
        return -1;
    }
    if (T->o.kind != L3K_TRI_ILU0)
    {
        setError("l3k_tri_values: an SGS preconditioner has no factor values (it reads A's)");
        return -1;
    }
    if (T->A->info.nnz > 0)
        L3K_HIP(hipMemcpyAsync(d_out, T->f.ptr, size_t(T->A->info.nnz) * sizeof(double), hipMemcpyDeviceToDevice, T->A->ctx->stream));
    return 0;
}
int l3k_tri_info_get(const l3k_tri* T, l3k_tri_info* out)
{
    if (!T || !out)
    {
        setError("l3k_tri_info_get: null argument");
        return -1;
    }
    const size_t bytes = (T->lower.rows.n + T->upper.rows.n) * sizeof(int32_t) + (T->lower.level_ptr.n + T->upper.level_ptr.n + T->diag_pos.n) * sizeof(int64_t) +
                         (T->mask.n + T->y.n + T->dinv.n + T->f.n) * sizeof(double) + T->status.n * sizeof(unsigned long long);
    *out = {T->n,
            T->n_active,
            T->A->info.nnz,
            T->o.kind,
            T->A->lanes,
            T->lower.lv.n_levels,
            T->upper.lv.n_levels,
            std::max(T->lower.lv.max_rows, T->upper.lv.max_rows),
            int64_t(T->lower.plan.size()),
            int64_t(T->upper.plan.size()),
            bytes,
            T->n_bad,
            T->first_bad,
            T->factored ? 1 : 0};
    return 0;
}
int l3k_tri_destroy(l3k_tri* T)
{
    delete T;
    return 0;
}
int l3k_csr_pcg_solve_tri(l3k_csr* A, const double* d_b, double* d_x, l3k_tri* T, const l3k_cg_opts* opts, l3k_cg_result* result)
{
    if (!A || !d_b || !d_x || !T || !result)
    {
        setError("l3k_csr_pcg_solve_tri: null argument");
        return -1;
    }
    if (int rc = l3k::solver::triReady(T, "l3k_csr_pcg_solve_tri"))
        return rc;
    return l3k::solver::pcgSolvePrecond(l3k::solver::csrOp(A), "l3k_csr_pcg_solve_tri", d_b, d_x, l3k::solver::triPrecond(T), opts, result);
}
} // extern "C"
