// api_chol.hip -- the sparse direct solver of libl3k.so (include/l3k.h: l3k_chol_*): band Cholesky on a device CSR operator, what
// the reference reaches through Amesos2 (Klu2 / Lapack, solve/Amesos2Solvers.hpp:18-32: ordering and symbolic factorisation on the
// first call, numeric factorisation and solve on every call).  The symbolic phase is host/chol_symbolic.cpp, the kernels are in
// device/chol.hpp; this file owns the object and the launch sequences.
#include "csr_launch.hpp"
#include "device/chol.hpp"
#include "host/chol_symbolic.hpp"

struct l3k_chol
{
    l3k_csr*                     A = nullptr;
    l3k::host::CholSymbolic      sym;
    DevBuf< double >             L;       // the block storage
    DevBuf< int32_t >            perm, inv;
    DevBuf< int64_t >            col_off;
    DevBuf< unsigned long long > status;
    DevBuf< double >             w, scratch; // solve workspaces for ncols_cap columns
    int                          ncols_cap = 0;
    size_t                       ldw = 0, lds = 0;
    int64_t                      n_bad = 0, first_bad = -1;
    bool                         factored = false;
};

namespace
{
using namespace l3k::chol;
constexpr size_t default_max_bytes = size_t(8) << 30;

template < typename F >
int withBlock(int nb, F&& f)
{
    return nb == 64 ? f(std::integral_constant< int, 64 >{}) : f(std::integral_constant< int, 32 >{});
}
int ensureWorkspace(l3k_chol* c, int ncols)
{
    if (ncols <= c->ncols_cap)
        return 0;
    DevBuf< double > w, s;
    if (int rc = w.alloc(size_t(ncols) * c->ldw))
        return rc;
    if (int rc = s.alloc(size_t(ncols) * c->lds))
        return rc;
    c->w         = std::move(w);
    c->scratch   = std::move(s);
    c->ncols_cap = ncols;
    return 0;
}
} // namespace

extern "C" {

int l3k_chol_create(l3k_csr* A, const l3k_chol_opts* opts, l3k_chol** out)
{
    if (!A || !out)
    {
        setError("l3k_chol_create: null argument");
        return -1;
    }
    const l3k_chol_opts o  = opts ? *opts : l3k_chol_opts{0, 0};
    hipStream_t         st = A->ctx->stream;
    auto                c  = std::make_unique< l3k_chol >();
    c->A                   = A;
    {
        std::vector< int64_t > row_ptr(size_t(A->n) + 1, 0);
        std::vector< int32_t > col_ind(size_t(A->info.nnz));
        if (A->n > 0)
            L3K_HIP(hipMemcpyAsync(row_ptr.data(), A->row_ptr, row_ptr.size() * sizeof(int64_t), hipMemcpyDeviceToHost, st));
        if (A->info.nnz > 0)
            L3K_HIP(hipMemcpyAsync(col_ind.data(), A->col_ind, col_ind.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        L3K_HIP(hipStreamSynchronize(st));
        if (int rc = l3k::host::cholSymbolic(A->n, row_ptr.data(), col_ind.data(), o.block, c->sym, "l3k_chol_create"))
            return rc;
    }
    const auto& s = c->sym;
    if (int rc = l3k::host::cholCheckBytes(s, o.max_bytes ? o.max_bytes : default_max_bytes, "l3k_chol_create"))
        return rc;
    c->ldw = size_t(s.n_blocks) * s.nb;
    c->lds = size_t(s.max_height > 0 ? s.max_height : 1) * s.nb;
    if (int rc = c->L.alloc(s.factor_bytes / sizeof(double)))
        return rc;
    if (int rc = c->perm.upload(s.perm.data(), s.perm.size(), st))
        return rc;
    if (int rc = c->inv.upload(s.inv.data(), s.inv.size(), st))
        return rc;
    if (int rc = c->col_off.upload(s.col_off.data(), s.col_off.size(), st))
        return rc;
    if (int rc = c->status.alloc(status_words))
        return rc;
    if (int rc = ensureWorkspace(c.get(), 1))
        return rc;
    L3K_HIP(hipStreamSynchronize(st)); // the uploads read the object's host vectors, which stay, but a failed copy shows here
    *out = c.release();
    return 0;
}

int l3k_chol_factor(l3k_chol* c)
{
    if (!c)
    {
        setError("l3k_chol_factor: null argument");
        return -1;
    }
    const auto&   s  = c->sym;
    const l3k_csr* A = c->A;
    hipStream_t   st = A->ctx->stream;
    c->factored      = false;
    c->n_bad         = 0;
    c->first_bad     = -1;
    if (s.n_blocks == 0)
    {
        c->factored = true;
        return 0;
    }
    L3K_HIP(hipMemsetAsync(c->L.ptr, 0, s.factor_bytes, st));
    L3K_HIP(hipMemsetAsync(c->status.ptr, 0, status_words * sizeof(unsigned long long), st));
    withBlock(s.nb, [&](auto NB) {
        constexpr int     nb  = NB();
        constexpr int64_t nb2 = int64_t(nb) * nb;
        hipLaunchKernelGGL((cholFillKernel< nb >), dim3(l3k::csr::csrGrid(A->n, 1)), dim3(threads), 0, st, A->row_ptr, A->col_ind, A->values,
                           A->n, c->inv.ptr, c->col_off.ptr, c->L.ptr, s.n_active, s.n_blocks);
        for (int64_t K = 0; K < s.n_blocks; ++K)
        {
            double*       colK = c->L.ptr + s.col_off[size_t(K)] * nb2;
            const int64_t H    = s.heights[size_t(K)];
            hipLaunchKernelGGL((cholDiagKernel< nb >), dim3(1), dim3(threads), 0, st, colK, K * nb, c->status.ptr);
            if (H == 0)
                continue;
            hipLaunchKernelGGL((cholPanelKernel< nb >), dim3(unsigned(H)), dim3(threads), 0, st, colK);
            hipLaunchKernelGGL((cholUpdateKernel< nb >), dim3(unsigned(H * (H + 1) / 2)), dim3(threads), 0, st, c->L.ptr, c->col_off.ptr, K);
        }
        return 0;
    });
    L3K_HIP(hipGetLastError());
    unsigned long long h[status_words];
    L3K_HIP(hipMemcpyAsync(h, c->status.ptr, sizeof h, hipMemcpyDeviceToHost, st));
    L3K_HIP(hipStreamSynchronize(st));
    if (h[0] != 0)
    {
        c->n_bad     = int64_t(h[0]);
        c->first_bad = h[1] < uint64_t(s.n_active) ? s.perm[size_t(h[1])] : -1;
        setError("l3k_chol_factor: matrix is not positive definite (%lld non-positive or non-finite pivots, the first at row %lld)",
                 (long long)c->n_bad, (long long)c->first_bad);
        return -2;
    }
    c->factored = true;
    return 0;
}

int l3k_chol_solve(l3k_chol* c, const double* d_b, size_t ldb, double* d_x, size_t ldx, int ncols)
{
    if (!c || ncols < 1 || (c->sym.n > 0 && (!d_b || !d_x)))
    {
        setError("l3k_chol_solve: null argument or ncols < 1");
        return -1;
    }
    if (!c->factored)
    {
        setError("l3k_chol_solve: no factorisation to solve with (l3k_chol_factor has not run, or its last run failed)");
        return -1;
    }
    const auto& s = c->sym;
    if (ncols > 1 && (ldb < size_t(s.n) || ldx < size_t(s.n)))
    {
        setError("l3k_chol_solve: leading dimension smaller than the number of rows");
        return -1;
    }
    if (s.n_blocks == 0)
        return 0;
    if (int rc = ensureWorkspace(c, ncols))
        return rc;
    hipStream_t    st   = c->A->ctx->stream;
    const unsigned nc   = unsigned(ncols);
    const unsigned grid = unsigned(l3k::csr::csrGrid(int64_t(c->ldw), 1));
    double*        w    = c->w.ptr;
    hipLaunchKernelGGL(cholGatherKernel, dim3(grid, nc), dim3(threads), 0, st, d_b, ldb, w, c->ldw, c->perm.ptr, s.n_active, int64_t(c->ldw));
    withBlock(s.nb, [&](auto NB) {
        constexpr int     nb  = NB();
        constexpr int64_t nb2 = int64_t(nb) * nb;
        for (int64_t K = 0; K < s.n_blocks; ++K)
        {
            const double* colK = c->L.ptr + s.col_off[size_t(K)] * nb2;
            const int64_t H    = s.heights[size_t(K)];
            hipLaunchKernelGGL((cholFwdDiagKernel< nb >), dim3(nc), dim3(threads), 0, st, colK, w + K * nb, c->ldw);
            if (H > 0)
                hipLaunchKernelGGL((cholFwdUpdateKernel< nb >), dim3(unsigned(H), nc), dim3(threads), 0, st, colK, w + K * nb, c->ldw);
        }
        for (int64_t K = s.n_blocks - 1; K >= 0; --K)
        {
            const double* colK = c->L.ptr + s.col_off[size_t(K)] * nb2;
            const int64_t H    = s.heights[size_t(K)];
            if (H > 0)
                hipLaunchKernelGGL((cholBwdPartialKernel< nb >), dim3(unsigned(H), nc), dim3(threads), 0, st, colK, w + K * nb, c->ldw,
                                   c->scratch.ptr, c->lds);
            hipLaunchKernelGGL((cholBwdDiagKernel< nb >), dim3(nc), dim3(threads), 0, st, colK, w + K * nb, c->ldw, int(H), c->scratch.ptr,
                               c->lds);
        }
        return 0;
    });
    hipLaunchKernelGGL(cholScatterKernel, dim3(grid, nc), dim3(threads), 0, st, w, c->ldw, d_x, ldx, c->perm.ptr, s.n_active);
    L3K_HIP(hipGetLastError());
    return 0;
}

int l3k_chol_info_get(const l3k_chol* c, l3k_chol_info* out)
{
    if (!c || !out)
    {
        setError("l3k_chol_info_get: null argument");
        return -1;
    }
    const auto& s = c->sym;
    *out          = {s.n, s.n_active, s.n_blocks, s.nb, s.max_height, s.factor_bytes, s.factor_flops, s.update_flops,
                     c->n_bad, c->first_bad, c->factored ? 1 : 0};
    return 0;
}

int l3k_chol_destroy(l3k_chol* c)
{
    delete c;
    return 0;
}
} // extern "C"
