// api_mfs.hip -- l3k_mfs of libl3k.so (include/l3k.h): the matrix-free sum of several domain and boundary terms over one set of rows.
// A term on some of the elements is an ordinary l3k_mf on an ordinary l3k_mesh over the same nodes, so the element kernels run as
// they are; what is new here is small: the comparison of two Dirichlet masks, the coverage mask of the terms, the Jacobi inverse that
// is zero outside it.
#include "solver.hpp"

namespace
{
constexpr int                mfs_threads = 256;
constexpr unsigned long long no_index    = ~0ull;
// the first index at which two byte masks differ (a null mask reads as zeros) -> *first, which the caller set to no_index
__global__ __launch_bounds__(mfs_threads) void maskDiffKernel(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, int64_t n,
                                                              unsigned long long* __restrict__ first)
{
    const int64_t stride = int64_t(gridDim.x) * mfs_threads;
    for (int64_t i = int64_t(blockIdx.x) * mfs_threads + threadIdx.x; i < n; i += stride)
        if ((a ? a[i] : uint8_t{0}) != (b ? b[i] : uint8_t{0}))
        {
            atomicMin(first, static_cast< unsigned long long >(i)); // (a thread's indices ascend: its first hit is its lowest)
            break;
        }
}
struct FieldInds
{
    int v[l3k::dev::max_unknowns];
};
// active[node * dpn + fi[u]] = 1 for every node of the `count` listed elements (face_elem != null: of the elements face_elem[i], the
// elements of a boundary term's sides) and every unknown u of the term.  One thread per (element, node), grid-stride: correct for
// any grid.  Several threads may store the same 1 into one byte
__global__ __launch_bounds__(mfs_threads) void coverageKernel(const uint32_t* __restrict__ elem_nodes, const int64_t* __restrict__ face_elem,
                                                              int64_t count, int N, int64_t n_nodes, int dpn, FieldInds fi, int U,
                                                              uint8_t* __restrict__ active)
{
    const int64_t items = count * N, stride = int64_t(gridDim.x) * mfs_threads;
    for (int64_t i = int64_t(blockIdx.x) * mfs_threads + threadIdx.x; i < items; i += stride)
    {
        const int64_t at = i / N, e = face_elem ? face_elem[at] : at;
        const int64_t node = elem_nodes[e * N + (i - at * N)];
        if (node < n_nodes)
            for (int u = 0; u < U; ++u)
                active[node * dpn + fi.v[u]] = 1;
    }
}
// *count += the non-zero bytes of mask[0, n)
__global__ __launch_bounds__(mfs_threads) void countActiveKernel(const uint8_t* __restrict__ mask, int64_t n, unsigned long long* __restrict__ count)
{
    __shared__ unsigned sh[mfs_threads];
    unsigned            acc    = 0;
    const int64_t       stride = int64_t(gridDim.x) * mfs_threads;
    for (int64_t i = int64_t(blockIdx.x) * mfs_threads + threadIdx.x; i < n; i += stride)
        acc += mask[i] != 0;
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int w = mfs_threads / 2; w > 0; w >>= 1)
    {
        if (int(threadIdx.x) < w)
            sh[threadIdx.x] += sh[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0 && sh[0] != 0)
        atomicAdd(count, static_cast< unsigned long long >(sh[0]));
}
// NativeJacobiImpl::init (solve/NativePreconditioners.hpp:75-96) on the active rows, 0 on the others: the mask decides, not the value
__global__ __launch_bounds__(mfs_threads) void maskedJacobiInverseKernel(const double* __restrict__ d, const uint8_t* __restrict__ active, int64_t n,
                                                                         double damping, double threshold, double* __restrict__ out)
{
    const int64_t stride = int64_t(gridDim.x) * mfs_threads;
    for (int64_t i = int64_t(blockIdx.x) * mfs_threads + threadIdx.x; i < n; i += stride)
    {
        const double v = d[i], a = fabs(v);
        out[i]         = active[i] ? (v < 0. ? -damping : damping) / (a > threshold ? a : threshold) : 0.;
    }
}
// the project's grid rule for workgroups that stride over their work (stridedGrid, objects.hpp), one thread per item
unsigned itemGrid(const l3k_ctx* ctx, int64_t items)
{
    return stridedGrid(ctx, (items + mfs_threads - 1) / mfs_threads);
}
int64_t nodesPerElement(const l3k_mesh* m)
{
    const int64_t n1 = m->order + 1;
    return m->dim == 2 ? n1 * n1 : n1 * n1 * n1;
}
int setDevice(const l3k_ctx* ctx)
{
    int cur = -1;
    if (hipGetDevice(&cur) != hipSuccess || cur != ctx->device) // (several contexts in one process)
        L3K_HIP(hipSetDevice(ctx->device));
    return 0;
}
// the refusals of an add that the term's mesh decides: 0, or -1 with the error set
int checkTermMesh(l3k_mfs* S, const char* who, const KernelTerm& t)
{
    const l3k_mesh *r = S->rows, *m = t.mesh;
    if (S->finalized)
    {
        setError("%s: the system is finalized: no more terms", who);
        return -1;
    }
    if (t.ctx != S->ctx || m->ctx != S->ctx)
    {
        setError("%s: the term belongs to another context", who);
        return -1;
    }
    if (m->dim != r->dim || m->order != r->order)
    {
        setError("%s: the term's mesh has dim %d and order %d, the rows dim %d and order %d", who, m->dim, m->order, r->dim, r->order);
        return -1;
    }
    if (m->n_owned_nodes != r->n_owned_nodes || m->n_ghost_nodes != r->n_ghost_nodes)
    {
        setError("%s: the term's mesh has %lld owned and %lld ghost nodes, the rows %lld and %lld: not a mesh over the same nodes", who,
                 (long long)m->n_owned_nodes, (long long)m->n_ghost_nodes, (long long)r->n_owned_nodes, (long long)r->n_ghost_nodes);
        return -1;
    }
    if (m->dofs_per_node != r->dofs_per_node)
    {
        setError("%s: the term's mesh has dofs_per_node = %d, the rows %d", who, m->dofs_per_node, r->dofs_per_node);
        return -1;
    }
    if (t.n_rhs < S->n_rhs)
    {
        setError("%s: the term has n_rhs = %d, the system %d", who, t.n_rhs, S->n_rhs);
        return -1;
    }
    if (m == r || (!m->dirichlet.ptr && !r->dirichlet.ptr))
        return 0;
    if (int rc = setDevice(S->ctx))
        return rc;
    const int64_t      n     = r->nLocalDofs();
    unsigned long long first = no_index;
    hipStream_t        s     = S->ctx->stream;
    L3K_HIP(hipMemcpyAsync(S->word.ptr, &first, sizeof first, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(maskDiffKernel, dim3(itemGrid(S->ctx, n)), dim3(mfs_threads), 0, s, m->dirichlet.ptr, r->dirichlet.ptr, n, S->word.ptr);
    L3K_HIP(hipGetLastError());
    L3K_HIP(hipMemcpyAsync(&first, S->word.ptr, sizeof first, hipMemcpyDeviceToHost, s));
    L3K_HIP(hipStreamSynchronize(s));
    if (first != no_index)
    {
        setError("%s: the Dirichlet mask of the term's mesh differs from that of the rows, first at dof %llu (node %llu, dof %llu of the node)",
                 who, first, first / unsigned(r->dofs_per_node), first % unsigned(r->dofs_per_node));
        return -1;
    }
    return 0;
}
int requireFinalized(const l3k_mfs* S, const char* who)
{
    if (S->finalized)
        return 0;
    setError("%s: call l3k_mfs_finalize first", who);
    return -1;
}
// `which` of a domain launch as the sides of a boundary term see it (l3k_mf_apply_elems): all sides of interior elements go with the
// first half of the interior; -1: none
int sideClass(int which)
{
    return which == 4 ? -1 : (which == 3 ? 0 : which);
}
// what the operands of an apply decide for every term, before anything is written
int checkApply(const l3k_mfs* S, const char* who, int ncols, const double* d_x, size_t ldx, const double* d_xghost, size_t ldxg, const double* d_y,
               size_t ldy, const double* d_yghost, size_t ldyg)
{
    if (int rc = requireFinalized(S, who))
        return rc;
    if (int rc = checkColumns(ncols, S->n_rhs))
        return rc;
    if (ldx < size_t(S->rows->nOwnedDofs()) || ldy < size_t(S->rows->nOwnedDofs()))
    {
        setError("leading dimension smaller than the number of owned dofs");
        return -1;
    }
    for (const auto& t : S->terms)
    {
        if (t.mf)
        {
            if (int rc = checkApplyOperands(t.mf, ncols, d_x, ldx, d_xghost, ldxg, d_y, ldy, d_yghost, ldyg))
                return rc;
        }
        else if (int rc = checkFieldsSet(t.bnd))
            return rc;
    }
    return 0;
}
} // namespace

l3k::solver::LinOp l3k::solver::mfsOp(l3k_mfs* S)
{
    return {S->ctx, S->rows->nOwnedDofs(), S,
            [](const LinOp& op, const double* x, double* y) {
                return l3k_mfs_apply(static_cast< l3k_mfs* >(op.object), x, size_t(op.n), y, size_t(op.n), 1, 1., 0.);
            },
            [](const LinOp& op, const double* x, double* y, double* s) {
                return l3k_mfs_apply_energy(static_cast< l3k_mfs* >(op.object), x, y, s);
            }};
}

extern "C" {
int l3k_mfs_create(l3k_mesh* rows, int n_rhs, l3k_mfs** out)
{
    if (!rows || !out)
    {
        setError("l3k_mfs_create: null argument");
        return -1;
    }
    if (n_rhs < 1)
    {
        setError("n_rhs must be >= 1");
        return -1;
    }
    if (int rc = setDevice(rows->ctx))
        return rc;
    auto S   = std::make_unique< l3k_mfs >();
    S->ctx   = rows->ctx;
    S->rows  = rows;
    S->n_rhs = n_rhs;
    if (int rc = S->word.alloc(1))
        return rc;
    *out = S.release();
    return 0;
}
int l3k_mfs_add_domain(l3k_mfs* S, l3k_mf* term)
{
    if (!S || !term)
    {
        setError("l3k_mfs_add_domain: null argument");
        return -1;
    }
    if (!term->boundary_terms.empty())
    {
        setError("l3k_mfs_add_domain: the term has %zu attached boundary terms: add them with l3k_mfs_add_boundary", term->boundary_terms.size());
        return -1;
    }
    if (int rc = checkTermMesh(S, "l3k_mfs_add_domain", *term))
        return rc;
    S->terms.push_back({term, nullptr});
    return 0;
}
int l3k_mfs_add_boundary(l3k_mfs* S, l3k_bnd* term)
{
    if (!S || !term)
    {
        setError("l3k_mfs_add_boundary: null argument");
        return -1;
    }
    if (int rc = checkTermMesh(S, "l3k_mfs_add_boundary", *term))
        return rc;
    S->terms.push_back({nullptr, term});
    return 0;
}
int l3k_mfs_finalize(l3k_mfs* S)
{
    if (!S)
    {
        setError("l3k_mfs_finalize: null argument");
        return -1;
    }
    if (S->finalized)
    {
        setError("l3k_mfs_finalize: the system is finalized already");
        return -1;
    }
    if (int rc = setDevice(S->ctx))
        return rc;
    const l3k_mesh* r = S->rows;
    hipStream_t     s = S->ctx->stream;
    DevBuf< uint8_t > active;
    if (int rc = active.alloc(size_t(r->nLocalDofs())))
        return rc;
    if (active.n > 0)
        L3K_HIP(hipMemsetAsync(active.ptr, 0, active.n, s));
    L3K_HIP(hipMemsetAsync(S->word.ptr, 0, sizeof(unsigned long long), s));
    for (const auto& t : S->terms)
    {
        const KernelTerm& k     = t.mf ? static_cast< const KernelTerm& >(*t.mf) : *t.bnd;
        const l3k_mesh*   m     = k.mesh;
        const int64_t     count = t.mf ? m->n_elems : t.bnd->n_faces;
        const int64_t     N     = nodesPerElement(m);
        if (count == 0)
            continue;
        FieldInds fi{};
        for (int u = 0; u < k.kp.n_unknowns; ++u)
            fi.v[u] = k.field_inds[u];
        hipLaunchKernelGGL(coverageKernel, dim3(itemGrid(S->ctx, count * N)), dim3(mfs_threads), 0, s, m->elem_nodes.ptr,
                           t.mf ? nullptr : t.bnd->face_elem.ptr, count, int(N), r->n_owned_nodes + r->n_ghost_nodes, r->dofs_per_node, fi,
                           k.kp.n_unknowns, active.ptr);
    }
    if (r->nOwnedDofs() > 0)
        hipLaunchKernelGGL(countActiveKernel, dim3(itemGrid(S->ctx, r->nOwnedDofs())), dim3(mfs_threads), 0, s, active.ptr, r->nOwnedDofs(),
                           S->word.ptr);
    L3K_HIP(hipGetLastError());
    unsigned long long n_active = 0;
    L3K_HIP(hipMemcpyAsync(&n_active, S->word.ptr, sizeof n_active, hipMemcpyDeviceToHost, s));
    L3K_HIP(hipStreamSynchronize(s));
    S->active        = std::move(active);
    S->n_active_rows = int64_t(n_active);
    S->finalized     = true;
    return 0;
}
int l3k_mfs_info_get(const l3k_mfs* S, l3k_mfs_info* out)
{
    if (!S || !out)
    {
        setError("l3k_mfs_info_get: null argument");
        return -1;
    }
    *out = {int64_t(S->terms.size()), S->rows->nOwnedDofs(), S->n_active_rows, int64_t(S->rows->owned_dirichlet_rows.n), S->n_rhs,
            S->finalized ? 1 : 0};
    return 0;
}
int l3k_mfs_active(const l3k_mfs* S, uint8_t* d_mask)
{
    if (!S || (!d_mask && S->rows->nLocalDofs() > 0))
    {
        setError("l3k_mfs_active: null argument");
        return -1;
    }
    if (int rc = requireFinalized(S, "l3k_mfs_active"))
        return rc;
    if (S->active.n > 0)
        L3K_HIP(hipMemcpyAsync(d_mask, S->active.ptr, S->active.n, hipMemcpyDeviceToDevice, S->ctx->stream));
    return 0;
}
int l3k_mfs_destroy(l3k_mfs* S)
{
    delete S;
    return 0;
}

int l3k_mfs_scale(l3k_mfs* S, double* d_y, size_t ldy, int ncols, double beta)
{
    if (!S || !d_y)
    {
        setError("l3k_mfs_scale: null argument");
        return -1;
    }
    return scaleRows(S->ctx, d_y, ldy, S->rows->nOwnedDofs(), ncols, beta);
}
int l3k_mfs_apply_elems(l3k_mfs* S, int which, const double* d_x, size_t ldx, const double* d_xghost, size_t ldxg, double* d_y, size_t ldy,
                        double* d_yghost, size_t ldyg, int ncols, double alpha, double beta)
{
    if (!S || !d_x || !d_y)
    {
        setError("l3k_mfs_apply_elems: null argument");
        return -1;
    }
    if (which < 0 || which > 4)
    {
        setError("which must be 0 (interior), 1 (border), 2 (all), 3 or 4 (first / second half of the interior)");
        return -1;
    }
    if (int rc = checkApply(S, "l3k_mfs_apply_elems", ncols, d_x, ldx, d_xghost, ldxg, d_y, ldy, d_yghost, ldyg))
        return rc;
    for (const auto& t : S->terms)
    {
        if (t.mf)
        {
            if (int rc = mfApplyElems(t.mf, which, d_x, ldx, d_xghost, ldxg, d_y, ldy, d_yghost, ldyg, ncols, alpha, beta, 0))
                return rc;
        }
        else if (sideClass(which) >= 0)
            if (int rc = l3k_bnd_apply(t.bnd, sideClass(which), d_x, ldx, d_xghost, ldxg, d_y, ldy, d_yghost, ldyg, ncols, alpha))
                return rc;
    }
    return 0;
}
int l3k_mfs_dirichlet_rows(l3k_mfs* S, const double* d_x, size_t ldx, double* d_y, size_t ldy, int ncols, double alpha)
{
    if (!S || !d_x || !d_y)
    {
        setError("l3k_mfs_dirichlet_rows: null argument");
        return -1;
    }
    return dirichletRowsOf(S->ctx, S->rows, d_x, ldx, d_y, ldy, ncols, alpha);
}
int l3k_mfs_apply(l3k_mfs* S, const double* d_x, size_t ldx, double* d_y, size_t ldy, int ncols, double alpha, double beta)
{
    if (!S || !d_x || !d_y)
    {
        setError("l3k_mfs_apply: null argument");
        return -1;
    }
    if (S->rows->n_ghost_nodes != 0)
    {
        setError("l3k_mfs_apply is the single-rank form; the rows have ghost nodes: use the split-phase entry points");
        return -1;
    }
    // (a refused call leaves y as it was: the refusals come before the scaling pass)
    if (int rc = checkApply(S, "l3k_mfs_apply", ncols, d_x, ldx, nullptr, 0, d_y, ldy, nullptr, 0))
        return rc;
    if (int rc = l3k_mfs_scale(S, d_y, ldy, ncols, beta))
        return rc;
    if (int rc = l3k_mfs_apply_elems(S, 2, d_x, ldx, nullptr, 0, d_y, ldy, nullptr, 0, ncols, alpha, beta))
        return rc;
    return l3k_mfs_dirichlet_rows(S, d_x, ldx, d_y, ldy, ncols, alpha);
}
int l3k_mfs_apply_energy(l3k_mfs* S, const double* d_x, double* d_y, double* d_s)
{
    if (!S || !d_x || !d_y || !d_s)
    {
        setError("l3k_mfs_apply_energy: null argument");
        return -1;
    }
    const int64_t n = S->rows->nOwnedDofs();
    if (int rc = l3k_mfs_apply(S, d_x, size_t(n), d_y, size_t(n), 1, 1., 0.))
        return rc;
    return l3k_cg_dot_pap(S->ctx, d_x, d_y, n, d_s);
}
int l3k_mfs_diag_rhs(l3k_mfs* S, int which, const double* d_dirichlet_vals, size_t ldg, double* d_diag, double* d_rhs, size_t ldr,
                     double* d_diag_ghost, double* d_rhs_ghost, size_t ldrg, int finalize)
{
    if (!S || !d_rhs)
    {
        setError("l3k_mfs_diag_rhs: null argument");
        return -1;
    }
    if (which < 0 || which > 4)
    {
        setError("which must be 0 (interior), 1 (border), 2 (all), 3 or 4 (first / second half of the interior)");
        return -1;
    }
    if (int rc = requireFinalized(S, "l3k_mfs_diag_rhs"))
        return rc;
    for (const auto& t : S->terms) // (every term forms all of its own columns, as alone)
        if ((t.mf ? t.mf->n_rhs : t.bnd->n_rhs) != S->n_rhs)
        {
            setError("l3k_mfs_diag_rhs: a term has n_rhs = %d, the system %d: the right-hand sides of the sum need terms of the system's n_rhs",
                     t.mf ? t.mf->n_rhs : t.bnd->n_rhs, S->n_rhs);
            return -1;
        }
    for (const auto& t : S->terms)
    {
        if (t.mf)
        {
            if (int rc = l3k_mf_diag_rhs(t.mf, which, d_dirichlet_vals, ldg, d_diag, d_rhs, ldr, d_diag_ghost, d_rhs_ghost, ldrg, 0))
                return rc;
        }
        else if (sideClass(which) >= 0)
            if (int rc = l3k_bnd_diag_rhs(t.bnd, sideClass(which), d_dirichlet_vals, ldg, d_diag, d_rhs, ldr, d_diag_ghost, d_rhs_ghost, ldrg))
                return rc;
    }
    return finalize && d_diag ? dirichletFinalizeOf(S->ctx, S->rows, d_dirichlet_vals, ldg, d_diag, d_rhs, ldr, S->n_rhs) : 0;
}
int l3k_mfs_jacobi_inverse(l3k_mfs* S, const double* d_diag, double damping, double threshold, double* d_minv)
{
    const int64_t n = S ? S->rows->nOwnedDofs() : 0;
    if (!S || (n > 0 && (!d_diag || !d_minv)))
    {
        setError("l3k_mfs_jacobi_inverse: null argument");
        return -1;
    }
    if (int rc = requireFinalized(S, "l3k_mfs_jacobi_inverse"))
        return rc;
    if (n > 0)
        hipLaunchKernelGGL(maskedJacobiInverseKernel, dim3(itemGrid(S->ctx, n)), dim3(mfs_threads), 0, S->ctx->stream, d_diag, S->active.ptr, n,
                           damping, threshold, d_minv);
    L3K_HIP(hipGetLastError());
    return 0;
}
} // extern "C"
