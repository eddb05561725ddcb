// api_csr.hip -- the device CSR operator of libl3k.so (include/l3k.h: l3k_csr_*): what the assembled and the condensed system hand to
// the solver layer.  The kernels are in device/csr.hpp; the solves on such an operator are in api_solver.hip.
#include "csr_launch.hpp"

namespace
{
using namespace l3k::csr;
using l3k::red::cg_blocks;

// NC columns of an apply
template < int L, int NC >
void launchApply(const l3k_csr* A, const double* d_x, size_t ldx, double* d_y, size_t ldy, double alpha, double beta)
{
    hipLaunchKernelGGL((csrApplyKernel< L, NC, false >), dim3(csrGrid(A->n, L)), dim3(cg_threads), 0, A->ctx->stream, A->row_ptr,
                       A->col_ind, A->values, A->n, d_x, ldx, d_y, ldy, alpha, beta, static_cast< double* >(nullptr));
}
} // namespace

extern "C" {

int l3k_csr_create(l3k_ctx* ctx, int64_t n, const int64_t* d_row_ptr, const int32_t* d_col_ind, const double* d_values,
                   int lanes_per_row, l3k_csr** out)
{
    if (!ctx || !d_row_ptr || !out || n < 0)
    {
        setError("l3k_csr_create: null argument or n < 0");
        return -1;
    }
    if (n > INT32_MAX)
    {
        setError("l3k_csr_create: n = %lld does not fit the 32-bit column indices", static_cast< long long >(n));
        return -1;
    }
    if (lanes_per_row != 0 && lanes_per_row != 4 && lanes_per_row != 16 && lanes_per_row != 64)
    {
        setError("l3k_csr_create: lanes_per_row = %d; it is 0 (choose) or 4, 16 or 64", lanes_per_row);
        return -1;
    }
    if (int rc = l3k::red::cgWorkspace(ctx))
        return rc;
    auto A = std::make_unique< l3k_csr >();
    if (int rc = A->flag.alloc(flag_words))
        return rc;
    // one validation pass (two kernels: row_ptr, then -- only if that passed -- the columns) and one readback
    unsigned long long* flag = A->flag.ptr;
    hipStream_t         st   = ctx->stream;
    L3K_HIP(hipMemsetAsync(flag, 0xff, sizeof *flag, st));
    L3K_HIP(hipMemsetAsync(flag + 1, 0, (flag_words - 1) * sizeof *flag, st));
    hipLaunchKernelGGL(csrCheckRowsKernel, dim3(csrGrid(n, 1)), dim3(cg_threads), 0, st, d_row_ptr, n, flag);
    if (d_col_ind && n > 0)
        hipLaunchKernelGGL(csrCheckColsKernel, dim3(csrGrid(n, 16)), dim3(cg_threads), 0, st, d_row_ptr, d_col_ind, n, flag);
    L3K_HIP(hipGetLastError());
    unsigned long long h[flag_words];
    L3K_HIP(hipMemcpyAsync(h, flag, sizeof h, hipMemcpyDeviceToHost, st));
    L3K_HIP(hipStreamSynchronize(st));
    if (h[0] != no_offence)
    {
        const long long row = static_cast< long long >(h[0] / 8);
        switch (h[0] % 8)
        {
        case first_row_ptr_not_zero: setError("l3k_csr_create: row_ptr[0] is not 0"); break;
        case row_ptr_decreasing: setError("l3k_csr_create: row_ptr decreases at row %lld", row); break;
        case column_out_of_range: setError("l3k_csr_create: row %lld has a column index outside [0, n)", row); break;
        default: setError("l3k_csr_create: the column indices of row %lld are not strictly ascending", row); break;
        }
        return -1;
    }
    const int64_t nnz = static_cast< int64_t >(h[3]);
    if (nnz > 0 && (!d_col_ind || !d_values))
    {
        setError("l3k_csr_create: null col_ind or values for a matrix of %lld entries", static_cast< long long >(nnz));
        return -1;
    }
    A->ctx     = ctx;
    A->n       = n;
    A->row_ptr = d_row_ptr;
    A->col_ind = d_col_ind;
    A->values  = d_values;
    const int64_t n_empty = static_cast< int64_t >(h[1]);
    A->info               = {n, nnz, n_empty, static_cast< int64_t >(h[2]), n > n_empty ? double(nnz) / double(n - n_empty) : 0., 0};
    A->lanes = A->info.lanes_per_row = lanes_per_row ? lanes_per_row : chooseLanes(A->info.mean_row_len);
    *out                             = A.release();
    return 0;
}
int l3k_csr_info_get(const l3k_csr* A, l3k_csr_info* out)
{
    if (!A || !out)
    {
        setError("l3k_csr_info_get: null argument");
        return -1;
    }
    *out = A->info;
    return 0;
}
int l3k_csr_apply(l3k_csr* A, const double* d_x, size_t ldx, double* d_y, size_t ldy, int ncols, double alpha, double beta)
{
    if (!A || ncols < 1 || (A->n > 0 && (!d_x || !d_y)))
    {
        setError("l3k_csr_apply: null argument or ncols < 1");
        return -1;
    }
    const size_t n = size_t(A->n);
    if (n == 0)
        return 0;
    if (ncols > 1 && (ldx < n || ldy < n))
    {
        setError("l3k_csr_apply: leading dimension smaller than the number of rows");
        return -1;
    }
    if (overlap(d_x, size_t(ncols - 1) * ldx + n, d_y, size_t(ncols - 1) * ldy + n))
    {
        setError("l3k_csr_apply: x and y overlap");
        return -1;
    }
    // passes of four, two or one columns: the columns of a pass share each load of col_ind and values
    for (int c = 0; c < ncols;)
    {
        const int     nc = ncols - c >= 4 ? 4 : ncols - c >= 2 ? 2 : 1;
        const double* x  = d_x + size_t(c) * ldx;
        double*       y  = d_y + size_t(c) * ldy;
        withLanes(A->lanes, [&](auto L) {
            if (nc == 4)
                launchApply< L(), 4 >(A, x, ldx, y, ldy, alpha, beta);
            else if (nc == 2)
                launchApply< L(), 2 >(A, x, ldx, y, ldy, alpha, beta);
            else
                launchApply< L(), 1 >(A, x, ldx, y, ldy, alpha, beta);
            return 0;
        });
        c += nc;
    }
    L3K_HIP(hipGetLastError());
    return 0;
}
int l3k_csr_apply_energy(l3k_csr* A, const double* d_x, double* d_y, double* d_s)
{
    if (!A || !d_s || (A->n > 0 && (!d_x || !d_y)))
    {
        setError("l3k_csr_apply_energy: null argument");
        return -1;
    }
    if (A->n > 0 && overlap(d_x, size_t(A->n), d_y, size_t(A->n)))
    {
        setError("l3k_csr_apply_energy: x and y overlap");
        return -1;
    }
    withLanes(A->lanes, [&](auto L) {
        const int g = csrGrid(A->n, L());
        hipLaunchKernelGGL((csrApplyKernel< L(), 1, true >), dim3(g), dim3(cg_threads), 0, A->ctx->stream, A->row_ptr, A->col_ind,
                           A->values, A->n, d_x, size_t(A->n), d_y, size_t(A->n), 1., 0., A->ctx->red_ws);
        l3k::red::launchFinish(A->ctx, g, d_s, {1});
        return 0;
    });
    L3K_HIP(hipGetLastError());
    return 0;
}
int l3k_csr_diag(l3k_csr* A, double* d_diag, double damping, double threshold, double* d_minv)
{
    if (!A)
    {
        setError("l3k_csr_diag: null argument");
        return -1;
    }
    if (A->n > 0 && (d_diag || d_minv))
        hipLaunchKernelGGL(csrDiagKernel, dim3(csrGrid(A->n, 1)), dim3(cg_threads), 0, A->ctx->stream, A->row_ptr, A->col_ind,
                           A->values, A->n, damping, threshold, d_diag, d_minv);
    L3K_HIP(hipGetLastError());
    return 0;
}
int l3k_csr_dirichlet(l3k_csr* A, double* d_values, const uint8_t* d_mask, const double* d_bc_vals, size_t ldg, double* d_rhs,
                      size_t ldr, int ncols)
{
    if (!A || ncols < 1 || (A->n > 0 && (!d_mask || !d_bc_vals || !d_rhs)) || (A->info.nnz > 0 && !d_values))
    {
        setError("l3k_csr_dirichlet: null argument or ncols < 1");
        return -1;
    }
    if (d_values != A->values)
    {
        setError("l3k_csr_dirichlet: d_values is not the values array the operator was created on");
        return -1;
    }
    const size_t n = size_t(A->n);
    if (n == 0)
        return 0;
    if (ncols > 1 && (ldg < n || ldr < n))
    {
        setError("l3k_csr_dirichlet: leading dimension smaller than the number of rows");
        return -1;
    }
    unsigned long long* flag = A->flag.ptr;
    hipStream_t         st   = A->ctx->stream;
    L3K_HIP(hipMemsetAsync(flag, 0xff, sizeof *flag, st));
    hipLaunchKernelGGL(csrDirichletCheckKernel, dim3(csrGrid(A->n, 1)), dim3(cg_threads), 0, st, A->row_ptr, A->col_ind, A->n, d_mask,
                       flag);
    L3K_HIP(hipGetLastError());
    unsigned long long h = 0;
    L3K_HIP(hipMemcpyAsync(&h, flag, sizeof h, hipMemcpyDeviceToHost, st));
    L3K_HIP(hipStreamSynchronize(st));
    if (h != no_offence) // (the reference dereferences end() here, bcs/DirichletBC.hpp:104-108)
    {
        setError("l3k_csr_dirichlet: the Dirichlet row %lld has no stored diagonal entry; nothing was changed",
                 static_cast< long long >(h));
        return -1;
    }
    withLanes(A->lanes, [&](auto L) {
        hipLaunchKernelGGL((csrDirichletKernel< L() >), dim3(csrGrid(A->n, L())), dim3(cg_threads), 0, st, A->row_ptr, A->col_ind,
                           d_values, A->n, d_mask, d_bc_vals, ldg, d_rhs, ldr, ncols);
        return 0;
    });
    L3K_HIP(hipGetLastError());
    return 0;
}
int l3k_csr_destroy(l3k_csr* A)
{
    delete A;
    return 0;
}
} // extern "C"
