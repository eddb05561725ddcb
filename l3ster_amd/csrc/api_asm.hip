// api_asm.hip -- the assembled system as one object (include/l3k.h: l3k_asm_*), on hexes and on quads.
//
// Reference: algsys::AssembledSystem (algsys/AssembledSystem.hpp): beginAssembly / assembleProblem(domain kernel | boundary kernel) /
// endAssembly, then the solver on the matrix.  The object owns the CSR arrays of the full graph of its mesh and the right-hand sides.
// Hexes go through the existing entry points (l3k_local_assemble, l3k_bnd_local_assemble, l3k_assemble_global,
// l3k_bnd_assemble_global: the same launchers, and the sub-batch pipelines of the TERMS, sized by the object's workspace_bytes); quads
// through the element and side kernels of device/quad_assemble.hpp in front of the row-major scatter kernel of api_assembled.hip, on
// the object's own sub-batch pipeline (sumQuadSystems below; runSubBatches, objects.hpp).
//
// A system made by l3k_asm_create_condensed (quads) eliminates the element-internal dofs: the same pipeline, with the split kernel
// of device/quad_condense.hpp in the scatter's place, a per-element store of the internal rows that l3k_asm_begin zeroes and
// l3k_asm_end factors, and l3k_asm_recover / l3k_asm_schur_updates on the factored store.  Scatter, split and
// elimination put their entries into the CSR arrays by the one rule of device/csr_scatter.hpp.
//
// A system made by l3k_asm_create_dist lives on one rank's part of a partitioned mesh: the same arrays over the local dofs
// [owned | ghost], filled by the same rank-local calls; l3k_asm_end is then collective and hands out a distributed operator
// (api_csr_dist.hip; DESIGN.md 4.20: the sub-assembled form).
#include "objects.hpp"

#include "device/quad_condense.hpp"

#include <algorithm>

struct l3k_asm
{
    l3k_ctx*           ctx  = nullptr;
    l3k_mesh*          mesh = nullptr;
    std::vector< int > field_inds;
    int                n_rhs = 1, state = L3K_ASM_NEW;
    size_t             workspace_bytes = 0, ldr = 0;
    int64_t            n = 0, nnz = 0, n_missing = 0;
    DevBuf< int64_t >  row_ptr;
    DevBuf< int32_t >  col_ind;
    DevBuf< double >   values, rhs, zero_vals;
    SubBatchPipe       pipe;
    l3k_csr*           csr = nullptr;
    // a partitioned system (l3k_asm_create_dist): the exchange, the operator over [owned | ghost], the prescribed values over the local dofs
    l3k_halo*          halo    = nullptr;
    l3k_csr_dist*      dist    = nullptr;
    int64_t            n_owned = 0;
    DevBuf< double >   g_local;
    // static condensation: the store [n_elems][Nis][LD] of the internal rows [K_ii | K_ib | F_i], LD = Nis + Nbs + n_rhs
    bool               condensed = false, eliminated = false;
    int                Us = 0, Nis = 0, Nbs = 0, LD = 0, team = l3k::dev::cond_threads;
    int64_t            n_failed = 0;
    DevBuf< double >   store;
    DevBuf< int >      d_fields;
    DevBuf< unsigned > d_nfail;
    ~l3k_asm()
    {
        if (dist)
            (void)l3k_csr_dist_destroy(dist);
        if (csr)
            (void)l3k_csr_destroy(csr);
    }
};

namespace
{
int nodesPerElem(const l3k_mesh* m)
{
    const int N1 = m->order + 1;
    return m->dim == 2 ? N1 * N1 : N1 * N1 * N1;
}
// the side arguments of a term over its list in the caller's order
l3k::dev::SideAsmArgs sideArgsInOrder(const l3k_bnd* b)
{
    l3k::dev::SideAsmArgs a{};
    a.elem_nodes = b->mesh->elem_nodes.ptr;
    a.elem_verts = b->mesh->elem_verts.ptr;
    a.tables     = b->tables.ptr;
    a.fields     = b->fields;
    a.ldf        = b->ldf;
    a.time       = b->time;
    a.face_elem  = b->in_order.elem.ptr;
    a.face_side  = b->in_order.side.ptr;
    a.face_rank  = b->in_order.rank.ptr;
    return a;
}
const l3k::dev::Instance* quadElementInstance(const l3k_mf* mf, const char* what)
{
    const auto* inst = instanceFor(mf, mf->n_rhs);
    if (inst && !inst->assemble)
    {
        setError("%s: this kernel shape has no assembly launcher", what);
        return nullptr;
    }
    return inst;
}
const l3k::dev::BoundaryInstance* quadSideInstance(const l3k_bnd* b, const char* what)
{
    const auto* inst = boundaryInstanceFor(b, b->n_rhs, what);
    if (inst && !inst->assemble)
    {
        setError("%s: this boundary kernel shape has no assembly launcher", what);
        return nullptr;
    }
    return inst;
}
int checkSideRange(const l3k_bnd* b, int64_t first, int64_t count, const char* what)
{
    if (first < 0 || count < 0 || first + count > b->n_faces)
    {
        setError("%s: side range [%lld, %lld) outside [0, %lld)", what, (long long)first, (long long)(first + count), (long long)b->n_faces);
        return -1;
    }
    return 0;
}
// sub-batch size of systems of `per_system` bytes in two halves of the workspace, at most `cap` (launch limits) and `count`
int64_t subBatch(size_t workspace_bytes, size_t per_system, int64_t count, int64_t cap)
{
    if (workspace_bytes == 0)
        workspace_bytes = size_t(1) << 30;
    int64_t nb = int64_t(workspace_bytes / 2 / per_system);
    nb         = std::min(nb, std::min(count, cap));
    return nb < 1 ? 1 : nb;
}
// the split of a sub-batch of a condensed system: primary block -> CSR arrays, internal rows -> the store (quad_condense.hpp);
// d_elem_of: the elements of side systems (several of one element may share the launch: atomics), nullptr for element systems
int launchQuadSplit(l3k_asm* A, const KernelTerm& t, const uint32_t* d_nodes, const int64_t* d_elem_of, int64_t at, int64_t n, const double* d_K,
                    const double* d_F, unsigned long long* d_count, hipStream_t s)
{
    const l3k_mesh*        m = A->mesh;
    const int              n1d = m->order + 1;
    l3k::dev::QuadSplitArgs a{};
    a.nodes     = d_nodes;
    a.elem_of   = d_elem_of;
    a.K         = d_K;
    a.F         = d_F;
    a.row_ptr   = A->row_ptr.ptr;
    a.col_ind   = A->col_ind.ptr;
    a.values    = A->values.ptr;
    a.rhs       = A->rhs.ptr;
    a.store     = A->store.ptr;
    a.ldr       = A->ldr;
    a.n_missing = d_count;
    a.first     = at;
    a.count     = n;
    a.n1d       = n1d;
    a.dpn       = m->dofs_per_node;
    a.n_rhs     = t.n_rhs;
    a.Us        = A->Us;
    a.Nis       = A->Nis;
    a.LD        = A->LD;
    for (int u = 0; u < t.kp.n_unknowns; ++u)
    {
        a.field_inds[u] = t.field_inds[u];
        a.slot[u] = int(std::lower_bound(A->field_inds.begin(), A->field_inds.end(), t.field_inds[u]) - A->field_inds.begin()); // (checkTerm: present)
    }
    const int64_t blocks = n * n1d * n1d; // (subBatch caps n)
    const int rc = l3k::dev::withUnknowns< 8 >(t.kp.n_unknowns, [&](auto u) {
        return l3k::dev::launchKernel< 0 >("quadSplitKernel", d_elem_of ? l3k::dev::quadSplitKernel< u(), true > : l3k::dev::quadSplitKernel< u(), false >,
                                           dim3(unsigned(blocks)), dim3(64), 0, s, a);
    });
    if (rc == l3k::dev::not_instantiated)
    {
        setError("l3k_asm_add: %d unknowns not supported (1..8)", t.kp.n_unknowns);
        return -1;
    }
    return rc;
}
// The quad route of both l3k_asm_add_* calls: the local systems [first, first + count) of a term -- Nd = NN U dofs each, their node
// rows d_nodes[first + i] -- formed by form(at, n, d_K, d_F, d_flag) on the context's stream into one half of the object's pipeline
// while the other half is summed into the object's arrays on the second stream.  Entries outside the graph are added to
// A->n_missing; -2 if a forming kernel raised a half's degenerate-element flag.  d_elem_of: the elements of side systems (a
// condensed system files their internal rows under them), nullptr for element systems
template < typename Form >
int sumQuadSystems(l3k_asm* A, const KernelTerm& t, const uint32_t* d_nodes, const int64_t* d_elem_of, int64_t first, int64_t count, Form&& form)
{
    const l3k_mesh* m = A->mesh;
    L3K_HIP(hipSetDevice(A->ctx->device));
    const int     NN = nodesPerElem(m), U = t.kp.n_unknowns, Nd = NN * U, R = t.n_rhs;
    const size_t  kd1 = size_t(Nd) * Nd, fd1 = size_t(Nd) * R;
    const int64_t nb  = subBatch(A->workspace_bytes, sizeof(double) * (kd1 + fd1), count, int64_t(0x7fffffff) / NN);
    const size_t  kd = size_t(nb) * kd1, fd = size_t(nb) * fd1;
    auto&         g  = A->pipe;
    if (int rc = g.ensure(kd + fd + 1, true))
        return rc;
    hipStream_t         sa      = A->ctx->stream;
    unsigned long long* d_count = A->ctx->missCounter();
    L3K_HIP(hipMemsetAsync(d_count, 0, sizeof(unsigned long long), sa));
    double* const flag[2] = {g.buf[0] + kd + fd, g.buf[1] + kd + fd}; // the degenerate-element flag of each half
    for (int k = 0; k < 2; ++k)
        L3K_HIP(hipMemsetAsync(flag[k], 0, sizeof(double), sa));
    if (int rc = runSubBatches(
            g, sa, first, count, nb, [&](int k, int64_t at, int64_t n) { return form(at, n, g.buf[k], g.buf[k] + kd, flag[k]); },
            [&](int k, int64_t at, int64_t n) {
                if (A->condensed)
                    return launchQuadSplit(A, t, d_nodes, d_elem_of, at, n, g.buf[k], g.buf[k] + kd, d_count, g.second);
                return launchAssembledScatterRows(A->ctx, m, d_nodes, U, R, t.field_inds, at, n, g.buf[k], g.buf[k] + kd, A->row_ptr.ptr,
                                                  A->col_ind.ptr, A->values.ptr, A->rhs.ptr, A->ldr, 0, d_count, g.second, 0);
            }))
        return rc;
    int64_t   missing = 0;
    const int rc      = readDegenerateFlags(sa, flag[0], flag[1], d_count, &missing);
    A->n_missing += missing;
    return rc;
}
// a condensed system whose store l3k_asm_end has factored takes no more terms and no second elimination
int checkNotEliminated(const l3k_asm* A, const char* what)
{
    if (A->condensed && A->eliminated)
    {
        setError("%s: the element-internal blocks of this system were eliminated by l3k_asm_end; l3k_asm_begin starts the next assembly", what);
        return -1;
    }
    return 0;
}
// what the term of an l3k_asm_add_* call must share with the system (KernelTerm: both kinds of term)
int checkTerm(const l3k_asm* A, const KernelTerm& t, const char* what)
{
    if (A->state != L3K_ASM_OPEN)
    {
        setError("%s: the system is not open (l3k_asm_begin opens it, l3k_asm_end closes it)", what);
        return -1;
    }
    if (t.kp.dimension != A->mesh->dim)
    {
        setError("%s: a term of dimension %d on a system of dimension %d%s", what, t.kp.dimension, A->mesh->dim, quadsNote(A->mesh));
        return -1;
    }
    if (t.mesh != A->mesh || t.ctx != A->ctx)
    {
        setError("%s: the term lives on another mesh than the system", what);
        return -1;
    }
    for (int u = 0; u < t.kp.n_unknowns; ++u)
        if (!std::binary_search(A->field_inds.begin(), A->field_inds.end(), t.field_inds[u]))
        {
            setError("%s: the term's field_inds[%d] = %d is not among the system's field_inds (not a subset)", what, u, t.field_inds[u]);
            return -1;
        }
    if (t.n_rhs != A->n_rhs)
    {
        setError("%s: the term has n_rhs = %d, the system %d", what, t.n_rhs, A->n_rhs);
        return -1;
    }
    return checkNotEliminated(A, what);
}
// l3k_asm_recover / l3k_asm_schur_updates: a closed condensed system
int checkFactoredStore(const l3k_asm* A, const char* what)
{
    if (!A->condensed)
    {
        setError("%s: the system is not condensed (l3k_asm_create_condensed makes one that is)", what);
        return -1;
    }
    if (A->state != L3K_ASM_CLOSED)
    {
        setError("%s: the system is not closed (l3k_asm_end factors the element-internal blocks and closes it)", what);
        return -1;
    }
    return 0;
}
l3k::dev::QuadCondArgs condArgs(const l3k_asm* A, int64_t first, int64_t count)
{
    l3k::dev::QuadCondArgs a{};
    a.store      = A->store.ptr;
    a.elem_nodes = A->mesh->elem_nodes.ptr;
    a.fields     = A->d_fields.ptr;
    a.first      = first;
    a.count      = count;
    a.n1d        = A->mesh->order + 1;
    a.dpn        = A->mesh->dofs_per_node;
    a.n_rhs      = A->n_rhs;
    a.Us         = A->Us;
    a.Nis        = A->Nis;
    a.Nbs        = A->Nbs;
    a.LD         = A->LD;
    a.team       = A->team;
    return a;
}
unsigned condGrid(const l3k_asm* A, int64_t count)
{
    const int per_wg = l3k::dev::cond_threads / A->team;
    return unsigned((count + per_wg - 1) / per_wg);
}
// l3k_asm_end on a condensed system: the elimination pass over all elements; -2 where a pivot test failed
int eliminateStore(l3k_asm* A)
{
    A->eliminated = true;
    A->n_failed   = 0;
    const int64_t ne = A->mesh->n_elems;
    if (A->Nis == 0 || ne == 0)
        return 0;
    hipStream_t              s = A->ctx->stream;
    l3k::dev::QuadCondArgs   a = condArgs(A, 0, ne);
    a.row_ptr                  = A->row_ptr.ptr;
    a.col_ind                  = A->col_ind.ptr;
    a.values                   = A->values.ptr;
    a.rhs                      = A->rhs.ptr;
    a.ldr                      = A->ldr;
    a.n_failed                 = A->d_nfail.ptr;
    a.n_missing                = A->ctx->missCounter();
    L3K_HIP(hipMemsetAsync(a.n_failed, 0, sizeof(unsigned), s));
    L3K_HIP(hipMemsetAsync(a.n_missing, 0, sizeof(unsigned long long), s));
    const size_t lds = sizeof(double) * size_t(l3k::dev::cond_threads / A->team) * A->Nis * A->LD;
    const int    rc  = lds <= l3k::dev::cond_lds_bytes
                           ? l3k::dev::launchKernel("quadEliminateKernel", l3k::dev::quadEliminateKernel< true >, dim3(condGrid(A, ne)),
                                                    dim3(l3k::dev::cond_threads), lds, s, a)
                           : l3k::dev::launchKernel("quadEliminateKernel", l3k::dev::quadEliminateKernel< false >, dim3(condGrid(A, ne)),
                                                    dim3(l3k::dev::cond_threads), 0, s, a);
    if (rc)
        return rc;
    unsigned           nfail   = 0;
    unsigned long long missing = 0;
    L3K_HIP(hipMemcpyAsync(&nfail, a.n_failed, sizeof nfail, hipMemcpyDeviceToHost, s));
    L3K_HIP(hipMemcpyAsync(&missing, a.n_missing, sizeof missing, hipMemcpyDeviceToHost, s));
    L3K_HIP(hipStreamSynchronize(s));
    A->n_missing += int64_t(missing);
    A->n_failed = nfail;
    if (nfail)
    {
        setError("l3k_asm_end: non-positive pivot in the element-internal block of %u of %lld elements; the system stays open "
                 "(l3k_asm_begin starts over)", nfail, (long long)ne);
        return -2;
    }
    return 0;
}
// The collective tail of l3k_asm_end on a partitioned system, behind the rank-local elimination and the local operator: the
// prescribed values imported to the ghost rows, the Dirichlet step with the owner rule, the ghost rows of rhs export-added into
// their owners' rows and zeroed, the distributed operator (created once: its row lists depend on the graph only)
int endDistributed(l3k_asm* A, const double* d_vals_owned, size_t ldg)
{
    hipStream_t   s = A->ctx->stream;
    const int64_t n = A->n, no = A->n_owned, ng = n - no;
    if (A->mesh->dirichlet.ptr && n > 0)
    {
        if (!A->g_local.ptr)
            if (int rc = A->g_local.alloc(size_t(A->n_rhs) * size_t(n)))
                return rc;
        L3K_HIP(hipMemsetAsync(A->g_local.ptr, 0, sizeof(double) * A->g_local.n, s));
        if (d_vals_owned) // (NULL: homogeneous on every rank -- nothing to import)
        {
            if (no > 0)
                L3K_HIP(hipMemcpy2DAsync(A->g_local.ptr, sizeof(double) * size_t(n), d_vals_owned, sizeof(double) * ldg, sizeof(double) * size_t(no),
                                         size_t(A->n_rhs), hipMemcpyDeviceToDevice, s));
            if (int rc = l3k_halo_import(A->halo, A->g_local.ptr, size_t(n), A->n_rhs, A->g_local.ptr + no, size_t(n)))
                return rc;
        }
        if (int rc = l3k_csr_dirichlet_dist(A->csr, A->values.ptr, A->mesh->dirichlet.ptr, A->g_local.ptr, size_t(n), A->rhs.ptr, A->ldr,
                                            A->n_rhs, no))
            return rc;
    }
    if (n > 0)
    {
        if (int rc = l3k_halo_export_add(A->halo, A->rhs.ptr + no, A->ldr, A->n_rhs, A->rhs.ptr, A->ldr))
            return rc;
        if (ng > 0)
            L3K_HIP(hipMemset2DAsync(A->rhs.ptr + no, sizeof(double) * A->ldr, 0, sizeof(double) * size_t(ng), size_t(A->n_rhs), s));
    }
    if (!A->dist)
        if (int rc = l3k_csr_dist_create(A->csr, A->halo, no, &A->dist))
            return rc;
    A->state = L3K_ASM_CLOSED;
    return 0;
}
} // namespace

extern "C" {
int l3k_asm_element_systems(l3k_mf* term, int64_t first, int64_t count, double* d_K, double* d_F)
{
    if (!term)
    {
        setError("l3k_asm_element_systems: null argument");
        return -1;
    }
    const l3k_mesh* m = term->mesh;
    if (m->dim != 2)
        return l3k_local_assemble(term, first, count, d_K, d_F, nullptr);
    if (int rc = checkRange(m, first, count))
        return rc;
    if (count == 0 || (!d_K && !d_F))
        return 0;
    const auto* inst = quadElementInstance(term, "l3k_asm_element_systems");
    if (!inst)
        return -4;
    l3k::dev::ElemArgs a;
    if (int rc = assemblyArgs(term, first, count, a))
        return rc;
    L3K_HIP(hipSetDevice(term->ctx->device));
    double* flag = nullptr;
    if (int rc = assemblyWorkspace(term, inst, count, flag))
        return rc;
    a.K         = d_K;
    a.F         = d_F;
    a.workspace = flag;
    if (int rc = inst->assemble(a, term->blobPtr(), term->ctx->stream))
        return rc;
    return readDegenerateFlags(term->ctx->stream, flag);
}

int l3k_asm_side_systems(l3k_bnd* term, int64_t first, int64_t count, double* d_K, double* d_F)
{
    if (!term)
    {
        setError("l3k_asm_side_systems: null argument");
        return -1;
    }
    if (term->mesh->dim != 2)
        return l3k_bnd_local_assemble(term, first, count, d_K, d_F);
    if (int rc = checkSideRange(term, first, count, "l3k_asm_side_systems"))
        return rc;
    if (count == 0 || (!d_K && !d_F))
        return 0;
    const auto* inst = quadSideInstance(term, "l3k_asm_side_systems");
    if (!inst)
        return -4;
    if (int rc = checkFieldsSet(term, "l3k_asm_side_systems"))
        return rc;
    if (int rc = sideListInOrder(term))
        return rc;
    L3K_HIP(hipSetDevice(term->ctx->device));
    l3k::dev::SideAsmArgs a = sideArgsInOrder(term);
    a.face_begin            = first;
    a.face_count            = count;
    a.K                     = d_K;
    a.F                     = d_F;
    return inst->assemble(a, term->blobPtr(), term->ctx->stream);
}

} // extern "C"
namespace
{
// l3k_asm_create (`condensed` = false: the full graph) and l3k_asm_create_condensed (quads: the graph of the primary nodes and the store)
// and l3k_asm_create_dist (`dist`: with the halo of a partitioned mesh, whose ghost nodes are then accepted)
int createSystem(const char* what, bool condensed, l3k_mesh* mesh, int n_fields, const int* field_inds, int n_rhs, size_t workspace_bytes,
                 l3k_asm** out, bool dist = false, l3k_halo* halo = nullptr)
{
    if (!mesh || !out || (dist && !halo))
    {
        setError("%s: null argument", what);
        return -1;
    }
    if (n_fields < 0 || (n_fields > 0 && !field_inds) || (n_fields == 0 && field_inds))
    {
        setError("%s: n_fields = %d with %s field_inds; it is 1 .. dofs_per_node indices, or 0 and NULL for all dofs", what, n_fields,
                 field_inds ? "non-null" : "null");
        return -1;
    }
    if (n_rhs < 1)
    {
        setError("%s: n_rhs = %d; it is at least 1", what, n_rhs);
        return -1;
    }
    if (dist)
    {
        if (l3k::halo::context(halo) != mesh->ctx)
        {
            setError("%s: the halo and the mesh belong to different contexts", what);
            return -1;
        }
        if (l3k::halo::dofsPerNode(halo) != mesh->dofs_per_node || l3k_halo_n_ghost_dofs(halo) != mesh->n_ghost_nodes * mesh->dofs_per_node)
        {
            setError("%s: the halo (%d dofs per node, %lld ghost dofs) does not match the mesh (%d dofs per node, %lld ghost dofs)", what,
                     l3k::halo::dofsPerNode(halo), (long long)l3k_halo_n_ghost_dofs(halo), mesh->dofs_per_node,
                     (long long)(mesh->n_ghost_nodes * mesh->dofs_per_node));
            return -1;
        }
    }
    else if (mesh->n_ghost_nodes > 0)
    {
        setError("%s: a partitioned mesh (%lld ghost nodes): the assembled system and its CSR operator are single-rank", what,
                 (long long)mesh->n_ghost_nodes);
        return -1;
    }
    if (condensed && mesh->dim != 2)
    {
        setError("%s: a hex mesh: the condensed assembled system is for quads; hexes are condensed by l3k_condense_global", what);
        return -1;
    }
    L3K_HIP(hipSetDevice(mesh->ctx->device));
    if (dist && mesh->n_elems == 0 && mesh->nLocalDofs() == 0)
    {
        // a rank that owns nothing: the system of no rows (row_ptr = {0}), so that the rank takes part in every call and returns
        auto A             = std::make_unique< l3k_asm >();
        A->ctx             = mesh->ctx;
        A->mesh            = mesh;
        A->n_rhs           = n_rhs;
        A->halo            = halo;
        A->workspace_bytes = workspace_bytes;
        A->condensed       = condensed;
        const int U        = n_fields ? n_fields : mesh->dofs_per_node;
        for (int u = 0; u < U; ++u)
            A->field_inds.push_back(field_inds ? field_inds[u] : u);
        if (int rc = A->row_ptr.alloc(1))
            return rc;
        L3K_HIP(hipMemsetAsync(A->row_ptr.ptr, 0, sizeof(int64_t), mesh->ctx->stream));
        L3K_HIP(hipStreamSynchronize(mesh->ctx->stream));
        *out = A.release();
        return 0;
    }
    const int          n1d = mesh->order + 1, Np = 4 * mesh->order;
    DevBuf< uint32_t > prim; // the primary node rows: the elements of the condensed graph (alive until the fill has run)
    l3k_graph*         g = nullptr;
    if (condensed)
    {
        if (int rc = prim.alloc(size_t(mesh->n_elems) * Np))
            return rc;
        if (mesh->n_elems > 0)
            if (int rc = l3k::dev::launchKernel("quadPrimaryNodesKernel", l3k::dev::quadPrimaryNodesKernel, dim3(gridFor(mesh->n_elems * Np)),
                                                dim3(256), 0, mesh->ctx->stream, static_cast< const uint32_t* >(mesh->elem_nodes.ptr),
                                                mesh->n_elems, n1d, prim.ptr))
                return rc;
        if (int rc = graphCreateOn(mesh, prim.ptr, Np, Np, 0, n_fields, field_inds, &g))
            return rc;
    }
    else if (int rc = l3k_graph_create(mesh, n_fields, field_inds, L3K_GRAPH_FULL, &g)) // (the rules of field_inds are the graph's)
        return rc;
    const auto     drop_graph = [&](int rc) { (void)l3k_graph_destroy(g); return rc; };
    l3k_graph_info gi;
    if (int rc = l3k_graph_info_get(g, &gi))
        return drop_graph(rc);
    auto A             = std::make_unique< l3k_asm >();
    A->ctx             = mesh->ctx;
    A->mesh            = mesh;
    A->n_rhs           = n_rhs;
    A->halo            = dist ? halo : nullptr;
    A->n_owned         = mesh->nOwnedDofs();
    A->workspace_bytes = workspace_bytes;
    A->n               = gi.n;
    A->nnz             = gi.nnz;
    A->ldr             = size_t(gi.n);
    const int U        = n_fields ? n_fields : mesh->dofs_per_node;
    for (int u = 0; u < U; ++u)
        A->field_inds.push_back(field_inds ? field_inds[u] : u);
    if (int rc = A->row_ptr.alloc(size_t(gi.n) + 1))
        return drop_graph(rc);
    if (int rc = A->col_ind.alloc(size_t(gi.nnz)))
        return drop_graph(rc);
    if (int rc = A->values.alloc(size_t(gi.nnz)))
        return drop_graph(rc);
    if (int rc = A->rhs.alloc(size_t(n_rhs) * A->ldr))
        return drop_graph(rc);
    if (int rc = l3k_graph_fill(g, A->row_ptr.ptr, A->col_ind.ptr))
        return drop_graph(rc);
    if (condensed)
    {
        const int Ni = (mesh->order - 1) * (mesh->order - 1);
        A->condensed = true;
        A->Us        = U;
        A->Nis       = Ni * U;
        A->Nbs       = Np * U;
        A->LD        = A->Nis + A->Nbs + n_rhs;
        A->team      = A->Nis <= 4 ? 16 : (A->Nis <= 32 ? 64 : l3k::dev::cond_threads);
        if (int rc = A->store.alloc(size_t(mesh->n_elems) * A->Nis * A->LD))
            return drop_graph(rc);
        if (int rc = A->d_fields.upload(A->field_inds.data(), A->field_inds.size(), A->ctx->stream))
            return drop_graph(rc);
        if (int rc = A->d_nfail.alloc(1))
            return drop_graph(rc);
    }
    // values and rhs <- 0; the graph object's buffers feed the fill: synchronise before it goes
    hipStream_t s   = A->ctx->stream;
    hipError_t  err = gi.nnz ? hipMemsetAsync(A->values.ptr, 0, sizeof(double) * size_t(gi.nnz), s) : hipSuccess;
    if (err == hipSuccess && gi.n)
        err = hipMemsetAsync(A->rhs.ptr, 0, sizeof(double) * size_t(n_rhs) * A->ldr, s);
    if (err == hipSuccess && A->store.n)
        err = hipMemsetAsync(A->store.ptr, 0, sizeof(double) * A->store.n, s);
    if (err == hipSuccess)
        err = hipStreamSynchronize(s);
    (void)l3k_graph_destroy(g);
    if (err != hipSuccess)
    {
        setError("%s: zeroing the arrays failed: %s", what, hipGetErrorString(err));
        return -3;
    }
    *out = A.release();
    return 0;
}
} // namespace
extern "C" {
int l3k_asm_create(l3k_mesh* mesh, int n_fields, const int* field_inds, int n_rhs, size_t workspace_bytes, l3k_asm** out)
{
    return createSystem("l3k_asm_create", false, mesh, n_fields, field_inds, n_rhs, workspace_bytes, out);
}
int l3k_asm_create_condensed(l3k_mesh* mesh, int n_fields, const int* field_inds, int n_rhs, size_t workspace_bytes, l3k_asm** out)
{
    return createSystem("l3k_asm_create_condensed", true, mesh, n_fields, field_inds, n_rhs, workspace_bytes, out);
}
int l3k_asm_create_dist(l3k_mesh* mesh, l3k_halo* halo, int n_fields, const int* field_inds, int n_rhs, size_t workspace_bytes, int condensed,
                        l3k_asm** out)
{
    return createSystem("l3k_asm_create_dist", condensed != 0, mesh, n_fields, field_inds, n_rhs, workspace_bytes, out, true, halo);
}

int l3k_asm_begin(l3k_asm* A)
{
    if (!A)
    {
        setError("l3k_asm_begin: null argument");
        return -1;
    }
    L3K_HIP(hipSetDevice(A->ctx->device));
    hipStream_t s = A->ctx->stream;
    if (A->nnz)
        L3K_HIP(hipMemsetAsync(A->values.ptr, 0, sizeof(double) * size_t(A->nnz), s));
    if (A->n)
        L3K_HIP(hipMemsetAsync(A->rhs.ptr, 0, sizeof(double) * size_t(A->n_rhs) * A->ldr, s));
    if (A->store.n)
        L3K_HIP(hipMemsetAsync(A->store.ptr, 0, sizeof(double) * A->store.n, s));
    A->eliminated = false;
    A->n_failed   = 0;
    A->n_missing = 0;
    A->state     = L3K_ASM_OPEN;
    return 0;
}

int l3k_asm_add_domain(l3k_asm* A, l3k_mf* term, int64_t first, int64_t count)
{
    const char* const what = "l3k_asm_add_domain";
    if (!A || !term)
    {
        setError("%s: null argument", what);
        return -1;
    }
    if (int rc = checkTerm(A, *term, what))
        return rc;
    if (assemblesBoundary(term))
    {
        setError("%s: the term has l3k_mf_assemble_boundary on; add its boundary terms with l3k_asm_add_boundary instead", what);
        return -1;
    }
    const l3k_mesh* m = A->mesh;
    if (int rc = checkRange(m, first, count))
        return rc;
    if (count == 0)
        return 0;
    int64_t missing = 0;
    if (m->dim != 2)
    {
        const auto* inst = instanceFor(term, term->n_rhs);
        if (!inst)
            return -4;
        if (!inst->assemble)
        {
            setError("%s: this kernel shape has no assembly launcher", what);
            return -1;
        }
        const int rc = l3k_assemble_global(term, first, count, A->row_ptr.ptr, A->col_ind.ptr, A->values.ptr, A->rhs.ptr, A->ldr, 0,
                                           A->workspace_bytes, &missing);
        A->n_missing += missing;
        return rc;
    }
    const auto* inst = quadElementInstance(term, what);
    if (!inst)
        return -4;
    return sumQuadSystems(A, *term, m->elem_nodes.ptr, nullptr, first, count, [&](int64_t at, int64_t n, double* d_K, double* d_F, double* d_flag) {
        l3k::dev::ElemArgs a;
        if (int rc = assemblyArgs(term, at, n, a))
            return rc;
        a.K         = d_K;
        a.F         = d_F;
        a.workspace = d_flag;
        return inst->assemble(a, term->blobPtr(), A->ctx->stream);
    });
}

int l3k_asm_add_boundary(l3k_asm* A, l3k_bnd* term, int64_t first, int64_t count)
{
    const char* const what = "l3k_asm_add_boundary";
    if (!A || !term)
    {
        setError("%s: null argument", what);
        return -1;
    }
    if (int rc = checkTerm(A, *term, what))
        return rc;
    if (int rc = checkSideRange(term, first, count, what))
        return rc;
    if (count == 0)
        return 0;
    const l3k_mesh* m       = A->mesh;
    int64_t         missing = 0;
    if (m->dim != 2)
    {
        const auto* inst = boundaryInstanceFor(term, term->n_rhs, what);
        if (!inst)
            return -4;
        if (!inst->assemble)
        {
            setError("%s: this boundary kernel shape has no assembly launcher", what);
            return -1;
        }
        const int rc = l3k_bnd_assemble_global(term, first, count, A->row_ptr.ptr, A->col_ind.ptr, A->values.ptr, A->rhs.ptr, A->ldr, 0,
                                               A->workspace_bytes, &missing);
        A->n_missing += missing;
        return rc;
    }
    const auto* inst = quadSideInstance(term, what);
    if (!inst)
        return -4;
    if (int rc = checkFieldsSet(term, what))
        return rc;
    if (int rc = sideListInOrder(term))
        return rc;
    return sumQuadSystems(A, *term, term->in_order.nodes.ptr, term->in_order.elem.ptr, first, count, [&](int64_t at, int64_t n, double* d_K, double* d_F, double*) {
        l3k::dev::SideAsmArgs a = sideArgsInOrder(term);
        a.face_begin            = at;
        a.face_count            = n;
        a.K                     = d_K;
        a.F                     = d_F;
        return inst->assemble(a, term->blobPtr(), A->ctx->stream);
    });
}

int l3k_asm_end(l3k_asm* A, const double* d_dirichlet_vals, size_t ldg)
{
    if (!A)
    {
        setError("l3k_asm_end: null argument");
        return -1;
    }
    if (A->state != L3K_ASM_OPEN)
    {
        setError("l3k_asm_end: the system is not open (l3k_asm_begin opens it)");
        return -1;
    }
    if (A->halo && d_dirichlet_vals && ldg < size_t(A->n_owned))
    {
        setError("l3k_asm_end: leading dimension of the prescribed values (%zu) smaller than the number of owned dofs (%lld)", ldg,
                 (long long)A->n_owned);
        return -1;
    }
    if (!A->halo && d_dirichlet_vals && ldg < size_t(A->n))
    {
        setError("l3k_asm_end: leading dimension of the prescribed values (%zu) smaller than the number of dofs (%lld)", ldg, (long long)A->n);
        return -1;
    }
    L3K_HIP(hipSetDevice(A->ctx->device));
    if (int rc = checkNotEliminated(A, "l3k_asm_end"))
        return rc;
    if (A->condensed)
        if (int rc = eliminateStore(A))
            return rc;
    if (!A->csr) // (the operator keeps the pointers of the object's arrays: created once, valid for every later assembly)
        if (int rc = l3k_csr_create(A->ctx, A->n, A->row_ptr.ptr, A->col_ind.ptr, A->values.ptr, 0, &A->csr))
            return rc;
    if (A->halo)
        return endDistributed(A, d_dirichlet_vals, ldg);
    if (A->mesh->dirichlet.ptr && A->n > 0)
    {
        const double* g = d_dirichlet_vals;
        if (!g)
        {
            if (!A->zero_vals.ptr)
            {
                if (int rc = A->zero_vals.alloc(size_t(A->n_rhs) * size_t(A->n)))
                    return rc;
                L3K_HIP(hipMemsetAsync(A->zero_vals.ptr, 0, sizeof(double) * A->zero_vals.n, A->ctx->stream));
            }
            g   = A->zero_vals.ptr;
            ldg = size_t(A->n);
        }
        if (int rc = l3k_csr_dirichlet(A->csr, A->values.ptr, A->mesh->dirichlet.ptr, g, ldg, A->rhs.ptr, A->ldr, A->n_rhs))
            return rc;
    }
    A->state = L3K_ASM_CLOSED;
    return 0;
}

int l3k_asm_info_get(const l3k_asm* A, l3k_asm_info* out)
{
    if (!A || !out)
    {
        setError("l3k_asm_info_get: null argument");
        return -1;
    }
    *out = {A->n, A->nnz, A->n_missing, A->ldr, A->n_rhs, A->state, A->row_ptr.ptr, A->col_ind.ptr, A->values.ptr, A->rhs.ptr,
            A->state == L3K_ASM_CLOSED ? A->csr : nullptr};
    return 0;
}

int l3k_asm_dist_info_get(const l3k_asm* A, l3k_asm_dist_info* out)
{
    if (!A || !out)
    {
        setError("l3k_asm_dist_info_get: null argument");
        return -1;
    }
    if (!A->halo)
    {
        setError("l3k_asm_dist_info_get: the system is not partitioned (l3k_asm_create_dist makes one that is)");
        return -1;
    }
    *out = {A->n_owned, A->n - A->n_owned, A->state == L3K_ASM_CLOSED ? A->dist : nullptr};
    return 0;
}

int l3k_asm_cond_info_get(const l3k_asm* A, l3k_asm_cond_info* out)
{
    if (!A || !out)
    {
        setError("l3k_asm_cond_info_get: null argument");
        return -1;
    }
    *out = {};
    if (A->condensed)
        *out = {1, 4 * A->mesh->order, (A->mesh->order - 1) * (A->mesh->order - 1), A->mesh->n_elems, int64_t(A->store.n * sizeof(double)),
                A->n_failed};
    return 0;
}

int l3k_asm_recover(l3k_asm* A, double* d_x, size_t ldx)
{
    const char* const what = "l3k_asm_recover";
    if (!A || (!d_x && !(A->halo && A->n == 0)))
    {
        setError("%s: null argument", what);
        return -1;
    }
    if (int rc = checkFactoredStore(A, what))
        return rc;
    if (A->halo && A->n == 0) // (a rank that owns nothing)
        return 0;
    if (ldx < size_t(A->n))
    {
        setError("%s: leading dimension of x (%zu) smaller than the number of dofs (%lld)", what, ldx, (long long)A->n);
        return -1;
    }
    const int64_t ne = A->mesh->n_elems;
    L3K_HIP(hipSetDevice(A->ctx->device));
    if (A->halo) // (collective: the primary dofs of ghost nodes come from their owners; internal dofs are always owned)
        if (int rc = l3k_halo_import(A->halo, d_x, ldx, A->n_rhs, d_x + A->n_owned, ldx))
            return rc;
    if (A->Nis == 0 || ne == 0)
        return 0;
    l3k::dev::QuadCondArgs a = condArgs(A, 0, ne);
    a.x                      = d_x;
    a.ldx                    = ldx;
    const size_t lds = sizeof(double) * size_t(l3k::dev::cond_threads / A->team) * (A->Nbs + 2 * A->Nis);
    if (int rc = l3k::dev::launchKernel("quadRecoverKernel", l3k::dev::quadRecoverKernel, dim3(condGrid(A, ne)), dim3(l3k::dev::cond_threads), lds,
                                        A->ctx->stream, a))
        return rc;
    L3K_HIP(hipStreamSynchronize(A->ctx->stream));
    return 0;
}

int l3k_asm_schur_updates(l3k_asm* A, int64_t first, int64_t count, double* d_W, double* d_w)
{
    const char* const what = "l3k_asm_schur_updates";
    if (!A)
    {
        setError("%s: null argument", what);
        return -1;
    }
    if (int rc = checkFactoredStore(A, what))
        return rc;
    if (int rc = checkRange(A->mesh, first, count))
        return rc;
    if (count == 0 || (!d_W && !d_w))
        return 0;
    L3K_HIP(hipSetDevice(A->ctx->device));
    hipStream_t s = A->ctx->stream;
    if (A->Nis == 0) // order 1: nothing to eliminate
    {
        if (d_W)
            L3K_HIP(hipMemsetAsync(d_W, 0, sizeof(double) * size_t(count) * A->Nbs * A->Nbs, s));
        if (d_w)
            L3K_HIP(hipMemsetAsync(d_w, 0, sizeof(double) * size_t(count) * A->n_rhs * A->Nbs, s));
    }
    else
    {
        l3k::dev::QuadCondArgs a = condArgs(A, first, count);
        a.outW                   = d_W;
        a.outw                   = d_w;
        if (int rc = l3k::dev::launchKernel("quadSchurOutKernel", l3k::dev::quadSchurOutKernel, dim3(condGrid(A, count)),
                                            dim3(l3k::dev::cond_threads), 0, s, a))
            return rc;
    }
    L3K_HIP(hipStreamSynchronize(s));
    return 0;
}

int l3k_asm_destroy(l3k_asm* A)
{
    delete A;
    return 0;
}
} // extern "C"
