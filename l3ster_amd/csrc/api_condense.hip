// api_condense.hip -- static condensation of the element-internal dofs on the assembled path (the reference's
// CondensationPolicy::ElementBoundary: algsys/StaticCondensationManager.hpp:322-350 condenseSystem, :352-408 endAssembly,
// :410-470 recoverSolution).
//
// Element systems are formed by l3k_local_assemble into buffers of the system (row-major K_e, column-major F_e), the
// condensation kernels of the system's (order, unknowns) shape (device/condense.hpp, Instance::condense) eliminate the internal
// dofs in place, and S_e / g_e leave the device only through l3k_condense_local: l3k_condense_global sums them into the caller's
// CSR graph with the primary-node scatter below (the hand-off of device/csr_scatter.hpp), pipelined on two streams as l3k_assemble_global is.  Recovery is stateless: it
// forms and eliminates the element systems again (the reference caches K_ii^-1 K_ib per element: 4.5 MB at order 6).
#include "objects.hpp"
#include "device/condense.hpp"
#include "device/csr_scatter.hpp"

namespace
{
using l3k::dev::CondenseArgs;
using l3k::dev::primaryNodeOf;

constexpr int cond_nb = 32; // CondShape::NB: pivots per panel (the factored diagonal blocks take Ni U x NB doubles per element)

struct CondScatterArgs : l3k::dev::CsrSink // (the condensed system: row_ptr, col_ind, values, rhs, ldr, n_missing)
{
    const uint32_t* elem_nodes;
    const uint8_t*  dirichlet; // per local dof, or null
    const double *  K, *F;     // eliminated element systems: row-major K_e (Schur block mirrored), column-major F_e
    const int*      fail;      // per element: its pivot failed (nothing of it is scattered)
    int64_t         first;
    int             n, NN, Np, dpn, n_rhs, skip_dirichlet;
    int             field_inds[l3k::dev::max_unknowns];
};

// The primary-node variant of api_assembled.hip's assembledScatterKernel: one wave per (element, PRIMARY row node), the U rows of
// the node, the lanes over the primary columns (b', u') of the row; the entries stay where the condensation left them, in the
// element's row-major K_e (rows and columns of primary dofs: S_e), so rows of internal dofs are never touched.  The search rule
// is that of device/csr_scatter.hpp.
template < int U >
__global__ __launch_bounds__(64) void condensedScatterKernel(const CondScatterArgs a)
{
    const int       Nd = a.NN * U, Nbd = a.Np * U;
    const int64_t   e  = blockIdx.x / a.Np;
    const int       q  = int(blockIdx.x - e * a.Np);
    if (a.fail[e])
        return;
    const uint32_t* en   = a.elem_nodes + (a.first + e) * a.NN;
    const int       b    = primaryNodeOf(q, a.n);
    const int       lane = threadIdx.x;
    l3k::dev::NodeRows< U > rows(int64_t(en[b]) * a.dpn, a.field_inds, a.dirichlet, a.skip_dirichlet);
    if (a.F && a.rhs)
        rows.addRhs(a, lane, a.n_rhs, a.F + e * a.n_rhs * Nd + b * U, Nd);
    if (!a.K || !a.values)
        return;
    rows.loadRanges(a.row_ptr);
    const double* Kb      = a.K + (e * Nd + int64_t(b) * U) * Nd; // rows (b, 0 .. U-1)
    unsigned      missing = 0;
    for (int j = lane; j < Nbd; j += 64)
    {
        const int     qp  = j / U, up = j - qp * U, bp = primaryNodeOf(qp, a.n);
        const int64_t col = int64_t(en[bp]) * a.dpn + a.field_inds[up];
        if (a.skip_dirichlet && a.dirichlet && a.dirichlet[col])
            continue;
        const double* Kj = Kb + bp * U + up; // (one pointer per lane: the rows' addresses are not kept in registers across the loop)
        missing += rows.addEntry(a, col, [&](int u) { return Kj[int64_t(u) * Nd]; });
    }
    csrCountMissing(a, missing);
}

struct CondShapeH // the host's view of CondShape
{
    int n, NN, Np, Nd, Nid, Nbd;
    CondShapeH(int p, int U)
        : n(p + 1), NN(n * n * n), Np(NN - (p - 1) * (p - 1) * (p - 1)), Nd(NN * U), Nid((NN - Np) * U), Nbd(Np * U)
    {
    }
};

const l3k::dev::Instance* condInstance(const l3k_mf* mf, const char* what)
{
    const auto* inst = instanceFor(mf, mf->n_rhs);
    if (inst && !inst->condense)
    {
        setError("%s: this shape has no condensation kernels", what);
        return nullptr;
    }
    return inst;
}
// doubles per element of a sub-batch: K_e, F_e (R columns), the factored diagonal blocks, the pivot flag (an int in a double)
size_t perElem(const CondShapeH& sh, int R)
{
    return size_t(sh.Nd) * sh.Nd + size_t(sh.Nd) * R + size_t(sh.Nid) * cond_nb + 1;
}
// elements per sub-batch for `bytes` per half, within the launch-size limits of the condensation kernels
int64_t subBatch(const CondShapeH& sh, int R, size_t bytes, int64_t count)
{
    int64_t       nb    = int64_t(bytes / (perElem(sh, R) * sizeof(double)));
    nb                  = nb < 1 ? 1 : (nb > count ? count : nb);
    const int64_t tiles = int64_t((sh.Nd + R + 63) / 64) * ((sh.Nd + R + 63) / 64);
    while (nb > 1 && (nb * tiles > int64_t(0x7fffffff) || nb * sh.Nbd > int64_t(0x7fffffff) || nb * sh.Np > int64_t(0x7fffffff)))
        nb /= 2;
    return nb;
}
// the system's condensation buffers: two halves of `doubles` (second stream and events on request) and the pivot counter
int ensureBufs(l3k_mf* mf, size_t doubles, bool two_streams)
{
    if (int rc = mf->gcond.ensure(doubles, two_streams))
        return rc;
    if (!mf->cond_nfail)
        L3K_HIP(hipMalloc(reinterpret_cast< void** >(&mf->cond_nfail), sizeof(unsigned)));
    return 0;
}
// the pieces of a half for nb elements
struct Half
{
    double *K, *F, *Rd;
    int*    fail;
};
Half halfOf(double* base, const CondShapeH& sh, int R, int64_t nb)
{
    Half h;
    h.K    = base;
    h.F    = R ? base + size_t(nb) * sh.Nd * sh.Nd : nullptr;
    h.Rd   = base + size_t(nb) * sh.Nd * sh.Nd + size_t(nb) * sh.Nd * R;
    h.fail = reinterpret_cast< int* >(h.Rd + size_t(nb) * sh.Nid * cond_nb);
    return h;
}
// element systems of [first, first + n) into the half (l3k_local_assemble: every assembly route, the degenerate-element error)
int formSystems(l3k_mf* mf, const Half& h, const CondShapeH& sh, int R, int64_t first, int64_t n)
{
    hipStream_t s = mf->ctx->stream;
    if (h.F)
        L3K_HIP(hipMemsetAsync(h.F, 0, sizeof(double) * size_t(n) * sh.Nd * R, s));
    if (int rc = l3k_local_assemble(mf, first, n, h.K, h.F, nullptr))
        return rc;
    L3K_HIP(hipMemsetAsync(h.fail, 0, sizeof(int) * size_t(n), s));
    return 0;
}
CondenseArgs condArgs(const l3k_mf* mf, const Half& h, int R, int64_t n)
{
    CondenseArgs a{};
    a.K     = h.K;
    a.F     = h.F;
    a.Rd    = h.Rd;
    a.fail  = h.fail;
    a.nfail = mf->cond_nfail;
    a.count = n;
    a.n_rhs = R;
    return a;
}
int readPivotFlag(l3k_mf* mf, hipStream_t s)
{
    unsigned h = 0;
    L3K_HIP(hipMemcpyAsync(&h, mf->cond_nfail, sizeof h, hipMemcpyDeviceToHost, s));
    L3K_HIP(hipStreamSynchronize(s));
    if (h)
    {
        setError("non-positive pivot in the element-internal block");
        return -2;
    }
    return 0;
}

int launchCondensedScatter(l3k_mf* mf, int64_t first, int64_t count, const Half& h, const CondShapeH& sh, const int64_t* d_row_ptr,
                           const int32_t* d_col_ind, double* d_values, double* d_rhs, size_t ldr, int skip_dirichlet,
                           unsigned long long* d_count, hipStream_t s)
{
    const l3k_mesh* m = mf->mesh;
    CondScatterArgs a{};
    a.elem_nodes     = m->elem_nodes.ptr;
    a.dirichlet      = m->dirichlet.ptr;
    a.K              = h.K;
    a.F              = h.F;
    a.fail           = h.fail;
    a.row_ptr        = d_row_ptr;
    a.col_ind        = d_col_ind;
    a.values         = d_values;
    a.rhs            = d_rhs;
    a.ldr            = ldr;
    a.n_missing      = d_count;
    a.first          = first;
    a.n              = sh.n;
    a.NN             = sh.NN;
    a.Np             = sh.Np;
    a.dpn            = m->dofs_per_node;
    a.n_rhs          = mf->n_rhs;
    a.skip_dirichlet = skip_dirichlet;
    for (int u = 0; u < l3k::dev::max_unknowns; ++u)
        a.field_inds[u] = mf->field_inds[u];
    const dim3 grid(unsigned(count * sh.Np));
    const int  rc = l3k::dev::withUnknowns< 8 >(mf->kp.n_unknowns, [&](auto u) {
        return l3k::dev::launchKernel< 0 >("condensedScatterKernel", condensedScatterKernel< u() >, grid, dim3(64), 0, s, a);
    });
    if (rc == l3k::dev::not_instantiated)
    {
        setError("l3k_condense_global: %d unknowns not supported (1..8)", mf->kp.n_unknowns);
        return -1;
    }
    return rc;
}
} // namespace

extern "C" {
int l3k_condense_local(l3k_mf* mf, int64_t first, int64_t count, double* d_S, double* d_G)
{
    if (!mf)
    {
        setError("null mf");
        return -1;
    }
    const l3k_mesh* m = mf->mesh;
    if (int rc = refuseQuads(m, "l3k_condense_local"))
        return rc;
    if (int rc = checkRange(m, first, count))
        return rc;
    if (count == 0 || (!d_S && !d_G))
        return 0;
    const auto* inst = condInstance(mf, "l3k_condense_local");
    if (!inst)
        return -4;
    const CondShapeH sh(m->order, mf->kp.n_unknowns);
    const int        R  = d_G ? mf->n_rhs : 0;
    const int64_t    nb = subBatch(sh, R, size_t(1) << 30, count);
    L3K_HIP(hipSetDevice(mf->ctx->device));
    if (int rc = ensureBufs(mf, nb * perElem(sh, R), false))
        return rc;
    hipStream_t s = mf->ctx->stream;
    L3K_HIP(hipMemsetAsync(mf->cond_nfail, 0, sizeof(unsigned), s));
    const Half h = halfOf(mf->gcond.buf[0], sh, R, nb);
    for (int64_t done = 0; done < count;)
    {
        const int64_t n = count - done < nb ? count - done : nb;
        if (int rc = formSystems(mf, h, sh, R, first + done, n))
            return rc;
        CondenseArgs a = condArgs(mf, h, R, n);
        a.S            = d_S ? d_S + size_t(done) * sh.Nbd * sh.Nbd : nullptr;
        a.G            = d_G ? d_G + size_t(done) * R * sh.Nbd : nullptr;
        if (int rc = inst->condense(a, s))
            return rc;
        done += n;
    }
    return readPivotFlag(mf, s);
}

int l3k_condense_global(l3k_mf* mf, int64_t first, int64_t count, const int64_t* d_row_ptr, const int32_t* d_col_ind,
                        double* d_values, double* d_rhs, size_t ldr, int skip_dirichlet, size_t workspace_bytes, int64_t* n_missing)
{
    if (!mf || !d_row_ptr || !d_col_ind || !d_values)
    {
        setError("l3k_condense_global: null argument");
        return -1;
    }
    const l3k_mesh* m = mf->mesh;
    if (int rc = refuseQuads(m, "l3k_condense_global"))
        return rc;
    if (int rc = checkRange(m, first, count))
        return rc;
    const int64_t n_local_dofs = (m->n_owned_nodes + m->n_ghost_nodes) * m->dofs_per_node;
    if (d_rhs && ldr < size_t(n_local_dofs))
    {
        setError("rhs leading dimension smaller than the number of local dofs");
        return -1;
    }
    if (n_missing)
        *n_missing = 0;
    if (count == 0)
        return 0;
    const auto* inst = condInstance(mf, "l3k_condense_global");
    if (!inst)
        return -4;
    const CondShapeH sh(m->order, mf->kp.n_unknowns);
    const int        R = d_rhs ? mf->n_rhs : 0;
    if (workspace_bytes == 0)
        workspace_bytes = size_t(2) << 30;
    int64_t nb = subBatch(sh, R, workspace_bytes / 2, count);
    // at least ~8 sub-batches per call where the batch stays large enough for full launches (the overlap needs several)
    if (const int64_t eighth = (count + 7) / 8; nb > eighth && eighth >= 512)
        nb = eighth;
    L3K_HIP(hipSetDevice(mf->ctx->device));
    if (int rc = ensureBufs(mf, nb * perElem(sh, R), true))
        return rc;
    auto&               g       = mf->gcond;
    hipStream_t         sa      = mf->ctx->stream;
    unsigned long long* d_count = n_missing ? mf->ctx->missCounter() : nullptr;
    if (d_count)
        L3K_HIP(hipMemsetAsync(d_count, 0, sizeof(unsigned long long), sa));
    L3K_HIP(hipMemsetAsync(mf->cond_nfail, 0, sizeof(unsigned), sa));
    // (a degenerate element ends the loop: -2 once the scatters in flight are done)
    if (int rc = runSubBatches(
            g, sa, first, count, nb,
            [&](int k, int64_t at, int64_t n) {
                const Half h = halfOf(g.buf[k], sh, R, nb);
                if (int rc = formSystems(mf, h, sh, R, at, n))
                    return rc;
                CondenseArgs a = condArgs(mf, h, R, n);
                a.mirror       = 1;
                return inst->condense(a, sa);
            },
            [&](int k, int64_t at, int64_t n) {
                return launchCondensedScatter(mf, at, n, halfOf(g.buf[k], sh, R, nb), sh, d_row_ptr, d_col_ind, d_values, d_rhs, ldr,
                                              skip_dirichlet, d_count, g.second);
            }))
        return rc;
    unsigned long long hcount = 0;
    if (d_count)
        L3K_HIP(hipMemcpyAsync(&hcount, d_count, sizeof hcount, hipMemcpyDeviceToHost, sa));
    L3K_HIP(hipStreamSynchronize(sa));
    if (n_missing)
        *n_missing = int64_t(hcount);
    return readPivotFlag(mf, sa);
}

int l3k_condensed_recover(l3k_mf* mf, int64_t first, int64_t count, double* d_x, size_t ldx)
{
    if (!mf || !d_x)
    {
        setError("l3k_condensed_recover: null argument");
        return -1;
    }
    const l3k_mesh* m = mf->mesh;
    if (int rc = refuseQuads(m, "l3k_condensed_recover"))
        return rc;
    if (int rc = checkRange(m, first, count))
        return rc;
    const int64_t n_local_dofs = (m->n_owned_nodes + m->n_ghost_nodes) * m->dofs_per_node;
    if (ldx < size_t(n_local_dofs))
    {
        setError("x leading dimension smaller than the number of local dofs");
        return -1;
    }
    const CondShapeH sh(m->order, mf->kp.n_unknowns);
    if (count == 0 || sh.Nid == 0)
        return 0;
    const auto* inst = condInstance(mf, "l3k_condensed_recover");
    if (!inst)
        return -4;
    const int     R  = mf->n_rhs;
    const int64_t nb = subBatch(sh, R, size_t(1) << 30, count);
    L3K_HIP(hipSetDevice(mf->ctx->device));
    if (int rc = ensureBufs(mf, nb * perElem(sh, R), false))
        return rc;
    hipStream_t s = mf->ctx->stream;
    L3K_HIP(hipMemsetAsync(mf->cond_nfail, 0, sizeof(unsigned), s));
    const Half h = halfOf(mf->gcond.buf[0], sh, R, nb);
    for (int64_t done = 0; done < count;)
    {
        const int64_t n = count - done < nb ? count - done : nb;
        if (int rc = formSystems(mf, h, sh, R, first + done, n))
            return rc;
        CondenseArgs a = condArgs(mf, h, R, n);
        a.recover      = 1;
        a.elem_nodes   = m->elem_nodes.ptr;
        a.first        = first + done;
        a.dpn          = m->dofs_per_node;
        for (int u = 0; u < l3k::dev::max_unknowns; ++u)
            a.field_inds[u] = mf->field_inds[u];
        a.x   = d_x;
        a.ldx = ldx;
        if (int rc = inst->condense(a, s))
            return rc;
        done += n;
    }
    return readPivotFlag(mf, s);
}
} // extern "C"
