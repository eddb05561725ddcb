// api_csr_dist.hip -- the distributed CSR operator of libl3k.so (include/l3k.h: l3k_csr_dist_*, l3k_csr_dirichlet_dist): the
// assembled and the condensed system on a partitioned mesh in front of the solver layer.
//
// Sub-assembled form: every rank keeps the matrix A_r of its own elements over its local dofs [owned | ghost];
// A = sum_r R_r^T A_r R_r is never formed and no matrix entry travels.  The reference exports the ghost rows of the matrix once,
// at endAssembly (Tpetra::CrsMatrix::fillComplete behind algsys/AssembledSystem.hpp); here the ghost rows of y are export-added
// at every apply, on the schedule of l3k_mf_apply_dist (api_halo.hip; algsys/MatrixFreeSystem.hpp:1020-1140), with the exchanges
// of the existing halo (comm/ImportExport.hpp:295-372, :402-470).  The kernels are in device/csr_dist.hpp.
#include "csr_launch.hpp"
#include "device/csr_dist.hpp"

struct l3k_csr_dist
{
    l3k_csr*          A    = nullptr;
    l3k_halo*         halo = nullptr;
    int64_t           n_owned = 0, n_ghost = 0;
    int64_t           n_rows[l3k::csr::n_row_classes] = {0, 0, 0};
    DevBuf< int32_t > rows[l3k::csr::n_row_classes]; // ascending row lists: interior, border, ghost
    DevBuf< double >  diag_ws;                       // [n_owned + n_ghost]: the local diagonal of l3k_csr_dist_diag
    DevBuf< double >  energy_ws;                     // block sums of l3k_csr_dist_apply_energy (allocated by its first call)
};

namespace
{
using namespace l3k::csr;
namespace halo = l3k::halo;

// the three row lists of D, by an ordered compaction in three launches and one readback (creation only)
int buildRowLists(l3k_csr_dist* D)
{
    const l3k_csr* A = D->A;
    const int64_t  n = A->n;
    if (n == 0)
        return 0;
    hipStream_t   s      = A->ctx->stream;
    const int64_t per    = (n + l3k::red::cg_blocks - 1) / l3k::red::cg_blocks;
    const int64_t chunk  = (per + cg_threads - 1) / cg_threads * cg_threads;
    const int     blocks = int((n + chunk - 1) / chunk);
    DevBuf< int > counts;
    if (int rc = counts.alloc(size_t(blocks + 1) * n_row_classes))
        return rc;
    int* const totals = counts.ptr + size_t(blocks) * n_row_classes;
    hipLaunchKernelGGL(csrRowClassCountKernel, dim3(blocks), dim3(cg_threads), 0, s, A->row_ptr, A->col_ind, n, D->n_owned, chunk, counts.ptr);
    hipLaunchKernelGGL(csrRowClassScanKernel, dim3(1), dim3(64), 0, s, counts.ptr, blocks, totals);
    L3K_HIP(hipGetLastError());
    int h[n_row_classes];
    L3K_HIP(hipMemcpyAsync(h, totals, sizeof h, hipMemcpyDeviceToHost, s));
    L3K_HIP(hipStreamSynchronize(s));
    if (int64_t(h[0]) + h[1] != D->n_owned || h[2] != D->n_ghost)
    {
        setError("l3k_csr_dist_create: the row classes (%d interior, %d border, %d ghost) do not add up to %lld owned and %lld ghost rows",
                 h[0], h[1], h[2], (long long)D->n_owned, (long long)D->n_ghost);
        return -3;
    }
    for (int c = 0; c < n_row_classes; ++c)
    {
        D->n_rows[c] = h[c];
        if (int rc = D->rows[c].alloc(size_t(h[c])))
            return rc;
    }
    hipLaunchKernelGGL(csrRowClassFillKernel, dim3(blocks), dim3(cg_threads), 0, s, A->row_ptr, A->col_ind, n, D->n_owned, chunk, counts.ptr,
                       D->rows[0].ptr, D->rows[1].ptr, D->rows[2].ptr);
    L3K_HIP(hipGetLastError());
    L3K_HIP(hipStreamSynchronize(s)); // (counts is a local)
    return 0;
}
// NC columns of the rows rows[0 .. n_rows) of D's local matrix
template < int L, int NC, bool SPLIT >
void launchRows(const l3k_csr_dist* D, const int32_t* rows, int64_t n_rows, const double* x, size_t ldx, const double* xg, size_t ldxg,
                double* y, size_t ldy, double* yg, size_t ldyg, double alpha, double beta)
{
    const l3k_csr* A = D->A;
    hipLaunchKernelGGL((csrDistApplyKernel< L, NC, SPLIT >), dim3(csrGrid(n_rows, L)), dim3(cg_threads), 0, A->ctx->stream, A->row_ptr,
                       A->col_ind, A->values, rows, n_rows, D->n_owned, x, ldx, xg, ldxg, y, ldy, yg, ldyg, alpha, beta);
}
// all columns of a row list (or of a slice of one) in l3k_csr_apply's passes of four, two or one
template < bool SPLIT >
void applyRows(const l3k_csr_dist* D, const int32_t* rows, int64_t n_rows, int ncols, const double* x, size_t ldx, const double* xg,
               size_t ldxg, double* y, size_t ldy, double* yg, size_t ldyg, double alpha, double beta)
{
    if (n_rows == 0)
        return;
    for (int c = 0; c < ncols;)
    {
        const int     nc  = ncols - c >= 4 ? 4 : ncols - c >= 2 ? 2 : 1;
        const double* xc  = x + size_t(c) * ldx;
        const double* xgc = xg ? xg + size_t(c) * ldxg : nullptr;
        double*       yc  = y + size_t(c) * ldy;
        double*       ygc = yg ? yg + size_t(c) * ldyg : nullptr;
        withLanes(D->A->lanes, [&](auto L) {
            if (nc == 4)
                launchRows< L(), 4, SPLIT >(D, rows, n_rows, xc, ldx, xgc, ldxg, yc, ldy, ygc, ldyg, alpha, beta);
            else if (nc == 2)
                launchRows< L(), 2, SPLIT >(D, rows, n_rows, xc, ldx, xgc, ldxg, yc, ldy, ygc, ldyg, alpha, beta);
            else
                launchRows< L(), 1, SPLIT >(D, rows, n_rows, xc, ldx, xgc, ldxg, yc, ldy, ygc, ldyg, alpha, beta);
            return 0;
        });
        c += nc;
    }
}
// l3k_csr_dist_apply_energy: the launches that leave block sums of x_i y_i write a workspace of the operator's own, one segment
// behind the other -- the two slices of the interior list (each with the grid the plain apply gives it), the border pass, the
// neighbours' messages
constexpr int energy_interior_blocks = l3k::red::cg_blocks, energy_border_blocks = 3 * l3k::red::cg_blocks / 8,
              energy_received_blocks = 3 * l3k::red::cg_blocks / 8;
constexpr size_t energy_ws_doubles   = 2 * energy_interior_blocks + energy_border_blocks + energy_received_blocks;
// one column of a slice of the interior list with the block sums of x_i y_i into partial[0 .. returned blocks)
int applyInteriorDot(const l3k_csr_dist* D, const int32_t* rows, int64_t n_rows, const double* x, double* y, double* partial)
{
    if (n_rows == 0)
        return 0;
    const l3k_csr* A = D->A;
    return withLanes(A->lanes, [&](auto L) {
        const int g = std::min(csrGrid(n_rows, L()), energy_interior_blocks);
        hipLaunchKernelGGL((csrDistApplyKernel< L(), 1, false, true >), dim3(g), dim3(cg_threads), 0, A->ctx->stream, A->row_ptr, A->col_ind,
                           A->values, rows, n_rows, D->n_owned, x, size_t(0), static_cast< const double* >(nullptr), size_t(0), y, size_t(0),
                           static_cast< double* >(nullptr), size_t(0), 1., 0., partial);
        return g;
    });
}
// y <- alpha A x + beta y on the owned rows (l3k_csr_dist_apply).  d_s != nullptr (one column, alpha = 1, beta = 0:
// l3k_csr_dist_apply_energy): the same launches in the same order, the interior ones in their WITH_DOT instance, and behind the
// unpack-add the border pass and the finishing block: s[1] <- this rank's <x, y>
int distApply(l3k_csr_dist* D, const char* who, const double* d_x, size_t ldx, double* d_y, size_t ldy, int ncols, double alpha, double beta,
              double* d_s)
{
    l3k_halo* h   = D->halo;
    l3k_ctx*  ctx = D->A->ctx;
    // a rank that owns nothing (no row, no neighbour) takes part and returns; its timing slot is filled like everybody's
    if (D->A->n == 0 && !halo::hasNeighbours(h))
    {
        L3K_HIP(hipSetDevice(ctx->device));
        if (hipEvent_t* tev = halo::timingSlot(h))
            for (int k = 0; k < 6; ++k)
                L3K_HIP(hipEventRecord(tev[k], ctx->stream));
        if (d_s)
        {
            l3k::red::launchFinish(ctx, 0, d_s, {1}); // (its share of <x, A x> is 0)
            L3K_HIP(hipGetLastError());
        }
        return 0;
    }
    const size_t no = size_t(D->n_owned);
    if (no > 0 && (!d_x || !d_y))
    {
        setError("%s: null vector", who);
        return -1;
    }
    if (ncols > 1 && (ldx < no || ldy < no))
    {
        setError("%s: leading dimension smaller than the number of owned rows", who);
        return -1;
    }
    if (no > 0 && overlap(d_x, size_t(ncols - 1) * ldx + no, d_y, size_t(ncols - 1) * ldy + no))
    {
        setError("%s: x and y overlap", who);
        return -1;
    }
    L3K_HIP(hipSetDevice(ctx->device));
    hipStream_t s  = ctx->stream;
    double *    xg = nullptr, *yg = nullptr;
    size_t      ldg = 1;
    if (int rc = halo::buffers(h, ncols, &xg, &yg, &ldg))
        return rc;
    hipEvent_t* tev   = halo::timingSlot(h);
    const auto  stamp = [&](int k) { return tev ? hipEventRecord(tev[k], s) : hipSuccess; };
    const int32_t* interior = D->rows[row_interior].ptr;
    // (a rank without neighbours has no exchange to hide: its interior list goes in one launch -- the split costs a launch's ramp
    // and drain)
    const int64_t ni = D->n_rows[row_interior], half = halo::hasNeighbours(h) ? ni / 2 : ni;
    if (d_s && !D->energy_ws.ptr)
        if (int rc = D->energy_ws.alloc(energy_ws_doubles))
            return rc;
    double* const partial = D->energy_ws.ptr;
    int           blocks  = 0; // of partial sums left so far (d_s != nullptr)
    // ---- import: pack, post; the first half of the interior rows runs meanwhile
    if (int rc = halo::beginImport(h, d_x, ldx, ncols, xg, ldg))
        return rc;
    L3K_HIP(stamp(0));
    if (d_s)
        blocks += applyInteriorDot(D, interior, half, d_x, d_y, partial);
    else
        applyRows< false >(D, interior, half, ncols, d_x, ldx, nullptr, 0, d_y, ldy, nullptr, 0, alpha, beta);
    L3K_HIP(stamp(1));
    // ---- border rows read the imported ghosts; ghost rows write the export buffer (every entry of it: no zeroing)
    if (int rc = halo::waitImport(h))
        return rc;
    L3K_HIP(stamp(2));
    applyRows< true >(D, D->rows[row_border].ptr, D->n_rows[row_border], ncols, d_x, ldx, xg, ldg, d_y, ldy, yg, ldg, alpha, beta);
    applyRows< true >(D, D->rows[row_ghost].ptr, D->n_rows[row_ghost], ncols, d_x, ldx, xg, ldg, d_y, ldy, yg, ldg, alpha, beta);
    L3K_HIP(stamp(3));
    // ---- export: post; the second half of the interior rows runs meanwhile
    if (int rc = halo::beginExport(h, ncols, yg, ldg))
        return rc;
    L3K_HIP(stamp(4));
    if (d_s)
        blocks += applyInteriorDot(D, interior + half, ni - half, d_x, d_y, partial + blocks);
    else
        applyRows< false >(D, interior + half, ni - half, ncols, d_x, ldx, nullptr, 0, d_y, ldy, nullptr, 0, alpha, beta);
    L3K_HIP(stamp(5));
    L3K_HIP(hipGetLastError());
    if (int rc = halo::endExport(h, d_y, ldy, ncols))
        return rc;
    if (d_s)
    {
        // the border rows are complete now: their share; the interior rows that a neighbour's message added into: what it added;
        // then the sum of all block sums in the order they were laid out
        if (const int64_t nb = D->n_rows[row_border]; nb > 0)
        {
            const int g = int(std::min< int64_t >((nb + cg_threads - 1) / cg_threads, energy_border_blocks));
            hipLaunchKernelGGL(csrDistBorderDotKernel, dim3(g), dim3(cg_threads), 0, s, D->rows[row_border].ptr, nb, d_x, d_y, partial + blocks);
            blocks += g;
        }
        const int n_nbrs = halo::nNeighbours(h);
        if (n_nbrs > energy_received_blocks)
        {
            setError("%s: %d neighbours, more than the %d block sums kept for their messages", who, n_nbrs, energy_received_blocks);
            return -3;
        }
        for (int k = 0; k < n_nbrs; ++k)
        {
            const int32_t* rows = nullptr;
            const double*  vals = nullptr;
            int64_t        n    = 0;
            halo::received(h, k, &rows, &vals, &n);
            if (n == 0)
                continue;
            const int g = int(std::min< int64_t >((n + cg_threads - 1) / cg_threads, energy_received_blocks / n_nbrs));
            hipLaunchKernelGGL(csrDistReceivedDotKernel, dim3(g), dim3(cg_threads), 0, s, D->A->row_ptr, D->A->col_ind, D->n_owned, rows, vals,
                               n, d_x, partial + blocks);
            blocks += g;
        }
        hipLaunchKernelGGL(l3k::red::cgFinishKernel, dim3(1), dim3(cg_threads), 0, s, partial, blocks, d_s, 1, -1);
        L3K_HIP(hipGetLastError());
    }
    return 0;
}
} // namespace

l3k_halo* l3k::csr::haloOf(const l3k_csr_dist* D)
{
    return D->halo;
}
l3k_ctx* l3k::csr::contextOf(const l3k_csr_dist* D)
{
    return D->A->ctx;
}
int64_t l3k::csr::ownedRows(const l3k_csr_dist* D)
{
    return D->n_owned;
}

extern "C" {
int l3k_csr_dist_create(l3k_csr* A, l3k_halo* h, int64_t n_owned, l3k_csr_dist** out)
{
    if (!A || !h || !out)
    {
        setError("l3k_csr_dist_create: null argument");
        return -1;
    }
    if (halo::context(h) != A->ctx)
    {
        setError("l3k_csr_dist_create: the halo and the operator belong to different contexts");
        return -1;
    }
    const int64_t n_ghost = l3k_halo_n_ghost_dofs(h);
    if (n_owned < 0 || A->n != n_owned + n_ghost)
    {
        setError("l3k_csr_dist_create: the operator has n = %lld rows, n_owned = %lld and the halo's %lld ghost dofs make %lld",
                 (long long)A->n, (long long)n_owned, (long long)n_ghost, (long long)(n_owned + n_ghost));
        return -1;
    }
    L3K_HIP(hipSetDevice(A->ctx->device));
    auto D     = std::make_unique< l3k_csr_dist >();
    D->A       = A;
    D->halo    = h;
    D->n_owned = n_owned;
    D->n_ghost = n_ghost;
    if (int rc = buildRowLists(D.get()))
        return rc;
    if (int rc = D->diag_ws.alloc(size_t(A->n)))
        return rc;
    *out = D.release();
    return 0;
}
int l3k_csr_dist_info_get(const l3k_csr_dist* D, l3k_csr_dist_info* out)
{
    if (!D || !out)
    {
        setError("l3k_csr_dist_info_get: null argument");
        return -1;
    }
    *out = {D->n_owned,     D->n_ghost,     D->n_rows[row_interior], D->n_rows[row_border], D->n_rows[row_ghost],
            D->rows[row_interior].ptr, D->rows[row_border].ptr, D->rows[row_ghost].ptr, D->A};
    return 0;
}
int l3k_csr_dist_apply(l3k_csr_dist* D, const double* d_x, size_t ldx, double* d_y, size_t ldy, int ncols, double alpha, double beta)
{
    if (!D || ncols < 1)
    {
        setError("l3k_csr_dist_apply: null argument or ncols < 1");
        return -1;
    }
    return distApply(D, "l3k_csr_dist_apply", d_x, ldx, d_y, ldy, ncols, alpha, beta, nullptr);
}
int l3k_csr_dist_apply_energy(l3k_csr_dist* D, const double* d_x, double* d_y, double* d_s)
{
    if (!D || !d_s)
    {
        setError("l3k_csr_dist_apply_energy: null argument");
        return -1;
    }
    if (int rc = l3k::red::cgWorkspace(D->A->ctx))
        return rc;
    const size_t ld = size_t(D->n_owned > 0 ? D->n_owned : 1);
    return distApply(D, "l3k_csr_dist_apply_energy", d_x, ld, d_y, ld, 1, 1., 0., d_s);
}
int l3k_csr_dist_diag(l3k_csr_dist* D, double* d_diag, double damping, double threshold, double* d_minv)
{
    if (!D)
    {
        setError("l3k_csr_dist_diag: null argument");
        return -1;
    }
    const l3k_csr* A = D->A;
    if (A->n == 0 && !halo::hasNeighbours(D->halo))
        return 0;
    if (D->n_owned > 0 && !d_diag && !d_minv)
    {
        setError("l3k_csr_dist_diag: neither d_diag nor d_minv given (the call is collective: every rank asks for something)");
        return -1;
    }
    L3K_HIP(hipSetDevice(A->ctx->device));
    hipStream_t s     = A->ctx->stream;
    double*     owned = d_diag ? d_diag : D->diag_ws.ptr;
    double*     ghost = D->diag_ws.ptr + D->n_owned;
    if (A->n > 0)
        hipLaunchKernelGGL(csrDistDiagKernel, dim3(csrGrid(A->n, 1)), dim3(cg_threads), 0, s, A->row_ptr, A->col_ind, A->values, A->n,
                           D->n_owned, owned, ghost);
    L3K_HIP(hipGetLastError());
    const size_t ldg = size_t(D->n_ghost > 0 ? D->n_ghost : 1), ldo = size_t(D->n_owned > 0 ? D->n_owned : 1);
    if (int rc = halo::beginExport(D->halo, 1, ghost, ldg))
        return rc;
    if (int rc = halo::endExport(D->halo, owned, ldo, 1))
        return rc;
    if (d_minv && D->n_owned > 0)
        hipLaunchKernelGGL(csrDistMinvKernel, dim3(csrGrid(D->n_owned, 1)), dim3(cg_threads), 0, s, A->row_ptr, D->n_owned, owned, damping,
                           threshold, d_minv);
    L3K_HIP(hipGetLastError());
    return 0;
}
int l3k_csr_dirichlet_dist(l3k_csr* A, double* d_values, const uint8_t* d_mask, const double* d_bc_vals_local, size_t ldg, double* d_rhs,
                           size_t ldr, int ncols, int64_t n_owned)
{
    if (!A || ncols < 1 || (A->n > 0 && (!d_mask || !d_bc_vals_local || !d_rhs)) || (A->info.nnz > 0 && !d_values))
    {
        setError("l3k_csr_dirichlet_dist: null argument or ncols < 1");
        return -1;
    }
    if (d_values != A->values)
    {
        setError("l3k_csr_dirichlet_dist: d_values is not the values array the operator was created on");
        return -1;
    }
    if (n_owned < 0 || n_owned > A->n)
    {
        setError("l3k_csr_dirichlet_dist: n_owned = %lld outside [0, n = %lld]", (long long)n_owned, (long long)A->n);
        return -1;
    }
    const size_t n = size_t(A->n);
    if (n == 0)
        return 0;
    if (ncols > 1 && (ldg < n || ldr < n))
    {
        setError("l3k_csr_dirichlet_dist: leading dimension smaller than the number of local rows");
        return -1;
    }
    L3K_HIP(hipSetDevice(A->ctx->device));
    unsigned long long* flag = A->flag.ptr;
    hipStream_t         st   = A->ctx->stream;
    L3K_HIP(hipMemsetAsync(flag, 0xff, sizeof *flag, st));
    if (n_owned > 0)
        hipLaunchKernelGGL(csrDistDirichletCheckKernel, dim3(csrGrid(n_owned, 1)), dim3(cg_threads), 0, st, A->row_ptr, A->col_ind, n_owned,
                           d_mask, flag);
    L3K_HIP(hipGetLastError());
    unsigned long long h = 0;
    L3K_HIP(hipMemcpyAsync(&h, flag, sizeof h, hipMemcpyDeviceToHost, st));
    L3K_HIP(hipStreamSynchronize(st));
    if (h != no_offence)
    {
        setError("l3k_csr_dirichlet_dist: the owned Dirichlet row %lld has no stored diagonal entry; nothing was changed",
                 static_cast< long long >(h));
        return -1;
    }
    withLanes(A->lanes, [&](auto L) {
        hipLaunchKernelGGL((csrDistDirichletKernel< L() >), dim3(csrGrid(A->n, L())), dim3(cg_threads), 0, st, A->row_ptr, A->col_ind,
                           d_values, A->n, n_owned, d_mask, d_bc_vals_local, ldg, d_rhs, ldr, ncols);
        return 0;
    });
    L3K_HIP(hipGetLastError());
    return 0;
}
int l3k_csr_dist_destroy(l3k_csr_dist* D)
{
    delete D;
    return 0;
}
} // extern "C"
