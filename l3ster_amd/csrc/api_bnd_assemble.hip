// api_bnd_assemble.hip -- boundary equation kernels in the assembled and condensed paths (hexes).
//
// Reference: the boundary overload of assembleGlobalSystem (algsys/AssembleGlobalSystem.hpp:55-96): per BoundaryElementView one
// assembleLocalSystem (the local system of the whole element from the side quadrature, AssembleLocalSystem.hpp:77-216), handed to
// the same condensation manager / scatter as a domain element's; with CondensationPolicy::ElementBoundary the side matrix is thus
// added to the element's blocks before the internal dofs are eliminated (StaticCondensationManager.hpp:354-407, :322-346).  Here:
//   l3k_bnd_local_assemble    K_s, F_s of a range of a term's sides (device/boundary_assemble.hpp, write mode)
//   l3k_bnd_assemble_global   ... formed in sub-batches and summed into the caller's CSR values / rhs by the row-major scatter kernel
//   l3k_mf_assemble_boundary  the switch: l3k_local_assemble (and with it the three condensation calls) accumulates the sides of its
//                             elements into K_e, F_e; l3k_assemble_global runs the standalone route for the sides of its elements
#include "objects.hpp"

#include <algorithm>
#include <numeric>

namespace
{
// node rows of the sides' elements: out[i][:] = elem_nodes[face_elem[i]][:]
__global__ __launch_bounds__(256) void gatherSideNodesKernel(const uint32_t* __restrict__ elem_nodes, const int64_t* __restrict__ face_elem,
                                                             int64_t n_faces, int NN, uint32_t* __restrict__ out)
{
    const int64_t total = n_faces * NN;
    for (int64_t t = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; t < total; t += int64_t(gridDim.x) * blockDim.x)
    {
        const int64_t i = t / NN;
        out[t]          = elem_nodes[face_elem[i] * NN + (t - i * NN)];
    }
}

int nodesPerElem(const l3k_mesh* m)
{
    const int N1 = m->order + 1;
    return m->dim == 2 ? N1 * N1 : N1 * N1 * N1;
}
int uploadSideList(l3k_bnd* b, l3k_bnd::SideList& l, const std::vector< int64_t >& elem, const std::vector< uint8_t >& side,
                   const std::vector< uint8_t >* rank)
{
    L3K_HIP(hipSetDevice(b->ctx->device));
    hipStream_t s = b->ctx->stream;
    if (int rc = l.elem.upload(elem.data(), elem.size(), s))
        return rc;
    if (int rc = l.side.upload(side.data(), side.size(), s))
        return rc;
    if (rank)
        if (int rc = l.rank.upload(rank->data(), rank->size(), s))
            return rc;
    const int NN = nodesPerElem(b->mesh);
    if (int rc = l.nodes.alloc(elem.size() * size_t(NN)))
        return rc;
    if (!elem.empty())
    {
        hipLaunchKernelGGL(gatherSideNodesKernel, dim3(gridFor(int64_t(elem.size()) * NN)), dim3(256), 0, s, b->mesh->elem_nodes.ptr, l.elem.ptr,
                           int64_t(elem.size()), NN, l.nodes.ptr);
        L3K_HIP(hipGetLastError());
    }
    L3K_HIP(hipStreamSynchronize(s)); // (the host vectors may be temporaries)
    l.built = true;
    return 0;
}
} // namespace
// the list in the caller's order on the device
int sideListInOrder(l3k_bnd* b)
{
    if (b->in_order.built)
        return 0;
    return uploadSideList(b, b->in_order, b->list_elem, b->list_side, nullptr);
}
namespace
{
// ... stably sorted by element, with the rank of each side among the sides of its element (the order of the list)
int ensureByElem(l3k_bnd* b)
{
    if (b->by_elem.built)
        return 0;
    const size_t          n = b->list_elem.size();
    std::vector< size_t > order(n);
    std::iota(order.begin(), order.end(), size_t{0});
    std::stable_sort(order.begin(), order.end(), [&](size_t x, size_t y) { return b->list_elem[x] < b->list_elem[y]; });
    std::vector< int64_t > elem(n);
    std::vector< uint8_t > side(n), rank(n);
    for (size_t i = 0; i < n; ++i)
    {
        elem[i] = b->list_elem[order[i]];
        side[i] = b->list_side[order[i]];
        const size_t r = i > 0 && elem[i - 1] == elem[i] ? size_t(rank[i - 1]) + 1 : 0;
        if (r > 255)
        {
            setError("boundary term lists more than 256 sides of element %lld", (long long)elem[i]);
            return -1;
        }
        rank[i] = uint8_t(r);
    }
    if (int rc = uploadSideList(b, b->by_elem, elem, side, &rank))
        return rc;
    b->by_elem_host.swap(elem);
    b->by_elem_rank.swap(rank);
    return 0;
}

struct SideShape
{
    int     Nd, R;
    int64_t max_sides; // of one launch (grid limits of the side matrix kernel and of the scatter)
    size_t  coef;      // coefficient doubles per side
};
const l3k::dev::BoundaryInstance* sideInstance(const l3k_bnd* b, const char* what, SideShape& sh)
{
    const auto* inst = boundaryInstanceFor(b, b->n_rhs, what);
    if (!inst)
        return nullptr;
    if (!inst->assemble)
    {
        setError("%s: this boundary kernel shape has no assembly launcher", what);
        return nullptr;
    }
    const int NN = nodesPerElem(b->mesh);
    sh.Nd        = NN * b->kp.n_unknowns;
    sh.R         = b->n_rhs;
    const int64_t ntl = (sh.Nd + 63) / 64, npair = ntl * (ntl + 1) / 2;
    sh.max_sides = std::min(int64_t(0x7fffffff) / npair, int64_t(0x7fffffff) / 64 / sh.Nd);
    sh.max_sides = sh.max_sides < 1 ? 1 : sh.max_sides;
    sh.coef      = inst->assemble_ws_doubles;
    return inst;
}
l3k::dev::SideAsmArgs sideArgs(const l3k_bnd* b, const l3k_bnd::SideList& l)
{
    l3k::dev::SideAsmArgs a{};
    a.elem_nodes = b->mesh->elem_nodes.ptr;
    a.elem_verts = b->mesh->elem_verts.ptr;
    a.tables     = b->tables.ptr;
    a.fields     = b->fields;
    a.ldf        = b->ldf;
    a.time       = b->time;
    a.face_elem  = l.elem.ptr;
    a.face_side  = l.side.ptr;
    a.face_rank  = l.rank.ptr;
    return a;
}
int ensureCoef(l3k_bnd* b, size_t doubles)
{
    if (b->coef_ws.n >= doubles)
        return 0;
    b->coef_ws = DevBuf< double >{};
    return b->coef_ws.alloc(doubles);
}

// The sides [lo, lo + count) of list `l` of the term, formed in sub-batches and summed into the CSR values / rhs
int sidesIntoGlobal(l3k_bnd* b, const l3k_bnd::SideList& l, int64_t lo, int64_t count, const int64_t* d_row_ptr, const int32_t* d_col_ind,
                    double* d_values, double* d_rhs, size_t ldr, int skip_dirichlet, size_t workspace_bytes, int64_t* n_missing,
                    const char* what)
{
    if (count == 0)
        return 0;
    SideShape   sh;
    const auto* inst = sideInstance(b, what, sh);
    if (!inst)
        return -4;
    if (int rc = checkFieldsSet(b, what))
        return rc;
    L3K_HIP(hipSetDevice(b->ctx->device));
    const size_t per_side = sizeof(double) * (size_t(sh.Nd) * sh.Nd + size_t(sh.Nd) * sh.R + sh.coef);
    if (workspace_bytes == 0)
        workspace_bytes = size_t(1) << 30;
    int64_t nb = int64_t(workspace_bytes / 2 / per_side);
    nb         = nb < 1 ? 1 : (nb > count ? count : nb);
    nb         = nb > sh.max_sides ? sh.max_sides : nb;
    const size_t kd = size_t(nb) * sh.Nd * sh.Nd, fd = d_rhs ? size_t(nb) * sh.Nd * sh.R : 0, wd = size_t(nb) * sh.coef;
    auto&        g  = b->gasm;
    if (int rc = g.ensure(kd + fd + wd, true))
        return rc;
    hipStream_t         sa      = b->ctx->stream;
    unsigned long long* d_count = n_missing ? b->ctx->missCounter() : nullptr;
    if (d_count)
        L3K_HIP(hipMemsetAsync(d_count, 0, sizeof(unsigned long long), sa));
    if (int rc = runSubBatches(
            g, sa, lo, count, nb,
            [&](int k, int64_t at, int64_t n) {
                l3k::dev::SideAsmArgs a = sideArgs(b, l);
                a.face_begin            = at;
                a.face_count            = n;
                a.K                     = g.buf[k];
                a.F                     = d_rhs ? g.buf[k] + kd : nullptr;
                a.coef                  = g.buf[k] + kd + fd;
                return inst->assemble(a, b->blobPtr(), sa);
            },
            [&](int k, int64_t at, int64_t n) {
                return launchAssembledScatterRows(b->ctx, b->mesh, l.nodes.ptr, b->kp.n_unknowns, b->n_rhs, b->field_inds, at, n, g.buf[k],
                                                  d_rhs ? g.buf[k] + kd : nullptr, d_row_ptr, d_col_ind, d_values, d_rhs, ldr, skip_dirichlet,
                                                  d_count, g.second, 0);
            }))
        return rc;
    if (d_count)
    {
        unsigned long long h = 0;
        L3K_HIP(hipMemcpyAsync(&h, d_count, sizeof h, hipMemcpyDeviceToHost, sa));
        L3K_HIP(hipStreamSynchronize(sa));
        *n_missing += int64_t(h);
    }
    return 0;
}
// positions [lo, hi) of the term's element-sorted list whose elements lie in [first, first + count)
void sideRangeOf(const l3k_bnd* b, int64_t first, int64_t count, int64_t& lo, int64_t& hi)
{
    const auto& e = b->by_elem_host;
    lo            = std::lower_bound(e.begin(), e.end(), first) - e.begin();
    hi            = std::lower_bound(e.begin(), e.end(), first + count) - e.begin();
}
} // namespace

int checkAssembleBoundary(const l3k_mf* mf, const char* what)
{
    for (size_t t = 0; t < mf->boundary_terms.size(); ++t)
    {
        const l3k_bnd* b = mf->boundary_terms[t];
        if (b->kp.n_unknowns != mf->kp.n_unknowns)
        {
            setError("%s: attached boundary term %zu has n_unknowns = %d, the system has %d (l3k_mf_assemble_boundary is on)", what, t,
                     b->kp.n_unknowns, mf->kp.n_unknowns);
            return -1;
        }
        for (int u = 0; u < mf->kp.n_unknowns; ++u)
            if (b->field_inds[u] != mf->field_inds[u])
            {
                setError("%s: attached boundary term %zu has field_inds[%d] = %d, the system has %d (l3k_mf_assemble_boundary is on)", what,
                         t, u, b->field_inds[u], mf->field_inds[u]);
                return -1;
            }
        if (b->n_rhs != mf->n_rhs)
        {
            setError("%s: attached boundary term %zu has n_rhs = %d, the system has %d (l3k_mf_assemble_boundary is on)", what, t, b->n_rhs,
                     mf->n_rhs);
            return -1;
        }
        SideShape sh;
        if (!sideInstance(b, what, sh))
            return -1;
        if (int rc = checkFieldsSet(b, what))
            return rc;
    }
    return 0;
}

int accumulateBoundarySides(l3k_mf* mf, int64_t first, int64_t count, double* d_K, double* d_F)
{
    if (!d_K && !d_F)
        return 0;
    hipStream_t s = mf->ctx->stream;
    for (l3k_bnd* b : mf->boundary_terms) // attachment order; within a term the order of its list (the rounds below)
    {
        if (int rc = ensureByElem(b))
            return rc;
        int64_t lo, hi;
        sideRangeOf(b, first, count, lo, hi);
        if (hi == lo)
            continue;
        SideShape   sh;
        const auto* inst = sideInstance(b, "l3k_local_assemble", sh);
        if (!inst)
            return -4;
        for (int64_t at = lo; at < hi;)
        {
            // whole elements per launch: a cut between two sides of one element would restart the rounds in the middle of its sides
            int64_t end = std::min(hi, at + sh.max_sides);
            while (end < hi && end > at + 1 && b->by_elem_host[size_t(end)] == b->by_elem_host[size_t(end - 1)])
                --end;
            if (end < hi && b->by_elem_host[size_t(end)] == b->by_elem_host[size_t(end - 1)])
            {
                setError("l3k_local_assemble: the sides of element %lld do not fit one launch", (long long)b->by_elem_host[size_t(at)]);
                return -1;
            }
            const int64_t n = end - at;
            if (int rc = ensureCoef(b, size_t(n) * sh.coef))
                return rc;
            int rounds = 0;
            for (int64_t i = at; i < end; ++i)
                rounds = std::max(rounds, int(b->by_elem_rank[size_t(i)]) + 1);
            l3k::dev::SideAsmArgs a = sideArgs(b, b->by_elem);
            a.face_begin            = at;
            a.face_count            = n;
            a.K                     = d_K;
            a.F                     = d_F;
            a.coef                  = b->coef_ws.ptr;
            a.elem_base             = first;
            a.accumulate            = 1;
            for (a.round = 0; a.round < rounds; ++a.round)
                if (int rc = inst->assemble(a, b->blobPtr(), s))
                    return rc;
            at = end;
        }
    }
    return 0;
}

int assembleGlobalBoundarySides(l3k_mf* mf, int64_t first, int64_t count, const int64_t* d_row_ptr, const int32_t* d_col_ind, double* d_values,
                                double* d_rhs, size_t ldr, int skip_dirichlet, size_t workspace_bytes, int64_t* n_missing)
{
    int64_t dummy = 0;
    for (l3k_bnd* b : mf->boundary_terms)
    {
        if (int rc = ensureByElem(b))
            return rc;
        int64_t lo, hi;
        sideRangeOf(b, first, count, lo, hi);
        if (int rc = sidesIntoGlobal(b, b->by_elem, lo, hi - lo, d_row_ptr, d_col_ind, d_values, d_rhs, ldr, skip_dirichlet, workspace_bytes,
                                     n_missing ? n_missing : &dummy, "l3k_assemble_global"))
            return rc;
    }
    return 0;
}

extern "C" {
int l3k_bnd_local_assemble(l3k_bnd* bnd, int64_t first, int64_t count, double* d_K, double* d_F)
{
    if (!bnd)
    {
        setError("l3k_bnd_local_assemble: null bnd");
        return -1;
    }
    if (int rc = refuseQuads(bnd->mesh, "l3k_bnd_local_assemble"))
        return rc;
    if (first < 0 || count < 0 || first + count > bnd->n_faces)
    {
        setError("l3k_bnd_local_assemble: side range [%lld, %lld) outside [0, %lld)", (long long)first, (long long)(first + count),
                 (long long)bnd->n_faces);
        return -1;
    }
    if (count == 0 || (!d_K && !d_F))
        return 0;
    SideShape   sh;
    const auto* inst = sideInstance(bnd, "l3k_bnd_local_assemble", sh);
    if (!inst)
        return -4;
    if (int rc = checkFieldsSet(bnd, "l3k_bnd_local_assemble"))
        return rc;
    if (int rc = sideListInOrder(bnd))
        return rc;
    L3K_HIP(hipSetDevice(bnd->ctx->device));
    for (int64_t done = 0; done < count;)
    {
        const int64_t n = std::min(count - done, sh.max_sides);
        if (int rc = ensureCoef(bnd, size_t(n) * sh.coef))
            return rc;
        l3k::dev::SideAsmArgs a = sideArgs(bnd, bnd->in_order);
        a.face_begin            = first + done;
        a.face_count            = n;
        a.K                     = d_K ? d_K + size_t(done) * sh.Nd * sh.Nd : nullptr;
        a.F                     = d_F ? d_F + size_t(done) * sh.Nd * sh.R : nullptr;
        a.coef                  = bnd->coef_ws.ptr;
        if (int rc = inst->assemble(a, bnd->blobPtr(), bnd->ctx->stream))
            return rc;
        done += n;
        if (done < count) // (the next launch reuses, and may regrow, the coefficient workspace)
            L3K_HIP(hipStreamSynchronize(bnd->ctx->stream));
    }
    return 0;
}

int l3k_bnd_assemble_global(l3k_bnd* bnd, int64_t first, int64_t count, const int64_t* d_row_ptr, const int32_t* d_col_ind, double* d_values,
                            double* d_rhs, size_t ldr, int skip_dirichlet, size_t workspace_bytes, int64_t* n_missing)
{
    if (!bnd)
    {
        setError("l3k_bnd_assemble_global: null bnd");
        return -1;
    }
    if (!d_row_ptr || !d_col_ind || !d_values)
    {
        setError("l3k_bnd_assemble_global: null argument (row_ptr, col_ind and values are needed)");
        return -1;
    }
    const l3k_mesh* m = bnd->mesh;
    if (int rc = refuseQuads(m, "l3k_bnd_assemble_global"))
        return rc;
    if (first < 0 || count < 0 || first + count > bnd->n_faces)
    {
        setError("l3k_bnd_assemble_global: side range [%lld, %lld) outside [0, %lld)", (long long)first, (long long)(first + count),
                 (long long)bnd->n_faces);
        return -1;
    }
    if (d_rhs && ldr < size_t(m->nLocalDofs()))
    {
        setError("l3k_bnd_assemble_global: rhs leading dimension smaller than the number of local dofs");
        return -1;
    }
    if (n_missing)
        *n_missing = 0;
    if (count == 0)
        return 0;
    if (int rc = sideListInOrder(bnd))
        return rc;
    return sidesIntoGlobal(bnd, bnd->in_order, first, count, d_row_ptr, d_col_ind, d_values, d_rhs, ldr, skip_dirichlet, workspace_bytes,
                           n_missing, "l3k_bnd_assemble_global");
}

int l3k_mf_assemble_boundary(l3k_mf* mf, int on)
{
    if (!mf)
    {
        setError("l3k_mf_assemble_boundary: null mf");
        return -1;
    }
    if (on)
        if (int rc = refuseQuads(mf->mesh, "l3k_mf_assemble_boundary"))
            return rc;
    mf->assemble_boundary = on != 0;
    return 0;
}
} // extern "C"
