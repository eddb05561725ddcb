// api.hip -- the extern "C" surface of libl3k.so (include/l3k.h) plus the small vector kernels around the element
// kernels (scale, Dirichlet rows, pack / unpack-add).  No CPU fallback: without a usable HIP device every device entry
// point fails with an error.
#include "objects.hpp"
#include "device/launch.hpp"
#include "host/mesh_plan.hpp"

#include <algorithm>
#include <cmath>

using l3k::api::KernelMeta;
using l3k::api::findKernel;
using l3k::api::findResidual;

// ------------------------------------------------------------------------------------------------ small kernels
namespace
{
// y <- beta*y (beta == 0: y <- 0, NaN-safe like putScalar(0.), algsys/MatrixFreeSystem.hpp:1038)
__global__ void scaleKernel(double* __restrict__ y, size_t ld, int64_t rows, int ncols, double beta)
{
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    for (int c = 0; c < ncols; ++c)
    {
        double* col = y + ld * c;
        for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < rows; i += stride)
            col[i] = beta == 0. ? 0. : col[i] * beta;
    }
}
// y[d] += alpha*x[d] on owned Dirichlet rows (algsys/MatrixFreeSystem.hpp:1087-1098)
__global__ void dirichletRowsKernel(const int64_t* __restrict__ rows, int64_t n, const double* __restrict__ x, size_t ldx,
                                    double* __restrict__ y, size_t ldy, int ncols, double alpha)
{
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += stride)
    {
        const int64_t d = rows[i];
        for (int c = 0; c < ncols; ++c)
            y[d + ldy * c] += alpha * x[d + ldx * c];
    }
}
// diag = 1, rhs = g on owned Dirichlet rows (algsys/MatrixFreeSystem.hpp:911-915)
__global__ void dirichletFinalizeKernel(const int64_t* __restrict__ rows, int64_t n, const double* __restrict__ g, size_t ldg,
                                        double* __restrict__ diag, double* __restrict__ rhs, size_t ldr, int ncols)
{
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += stride)
    {
        const int64_t d = rows[i];
        diag[d]         = 1.;
        for (int c = 0; c < ncols; ++c)
            rhs[d + ldr * c] = g ? g[d + ldg * c] : 0.;
    }
}
// comm::Import pack / comm::Export unpack (comm/ImportExport.hpp:356-372, 448-470)
__global__ void packKernel(const double* __restrict__ src, size_t ld, int ncols, const int32_t* __restrict__ idx, int64_t n,
                           double* __restrict__ dst)
{
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += stride)
    {
        const int64_t r = idx[i];
        for (int c = 0; c < ncols; ++c)
            dst[i + n * c] = src[r + ld * c];
    }
}
__global__ void unpackAddKernel(const double* __restrict__ src, int64_t n, const int32_t* __restrict__ idx,
                                double* __restrict__ dst, size_t ld, int ncols)
{
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += stride)
    {
        const int64_t r = idx[i];
        for (int c = 0; c < ncols; ++c)
            dst[r + ld * c] += src[i + n * c];
    }
}
} // namespace

namespace
{
const std::vector< KernelMeta >& kernelMetas()
{
    static const std::vector< KernelMeta > metas = [] {
        std::vector< KernelMeta > m;
#define L3K_X(id, T, name)                                                                                             \
    m.push_back({id, {T::params.dimension, T::params.n_equations, T::params.n_unknowns, T::params.n_fields, T::params.n_rhs}, \
                 name, std::is_empty_v< T > ? size_t{0} : sizeof(T)});
        L3K_FOR_EACH_KERNEL(L3K_X)
#undef L3K_X
#define L3K_X(id, T, name)                                                                                             \
    m.push_back({id, {T::params.dimension, T::params.n_equations, T::params.n_unknowns, T::params.n_fields, T::params.n_rhs}, \
                 name, std::is_empty_v< T > ? size_t{0} : sizeof(T), true});
        L3K_FOR_EACH_BOUNDARY_KERNEL(L3K_X)
#undef L3K_X
        return m;
    }();
    return metas;
}
const std::vector< KernelMeta >& residualMetas()
{
    static const std::vector< KernelMeta > metas = [] {
        std::vector< KernelMeta > m;
#define L3K_X(id, T, name)                                                                                             \
    m.push_back({id, {T::params.dimension, T::params.n_equations, T::params.n_unknowns, T::params.n_fields, T::params.n_rhs}, \
                 name, std::is_empty_v< T > ? size_t{0} : sizeof(T)});
        L3K_FOR_EACH_RESIDUAL_KERNEL(L3K_X)
#undef L3K_X
        return m;
    }();
    return metas;
}
// kernels announced by plugins (l3k_plugin_load): metadata materialised on first sight
const KernelMeta* fromPlugin(int id, bool residual)
{
    struct Seen
    {
        KernelMeta meta;
        bool       residual;
    };
    static std::vector< std::unique_ptr< Seen > > seen;
    for (const auto& k : seen)
        if (k->meta.id == id && k->residual == residual)
            return &k->meta;
    const auto* pk = l3k::dev::findPluginKernel(id, residual);
    if (!pk)
        return nullptr;
    seen.push_back(std::make_unique< Seen >(Seen{KernelMeta{pk->id,
                                                            {pk->dimension, pk->n_equations, pk->n_unknowns, pk->n_fields, pk->n_rhs},
                                                            pk->name, pk->param_bytes, pk->kind == 1},
                                                 residual}));
    return &seen.back()->meta;
}
} // namespace

namespace l3k::api
{
const KernelMeta* findResidual(int id)
{
    for (const auto& k : residualMetas())
        if (k.id == id)
            return &k;
    return fromPlugin(id, true);
}
const KernelMeta* findKernel(int id)
{
    for (const auto& k : kernelMetas())
        if (k.id == id)
            return &k;
    return fromPlugin(id, false);
}
} // namespace l3k::api

#ifdef L3K_ABLATION
// stage timeline of the single-wave kernel (tools/kbench.py --stamps): 256 iterations x 16 cycle counters of workgroup 0
namespace
{
constexpr int n_stamps = 256 * 16 + 2 * 4096; // + start / end clock of every workgroup (up to 4096)
long long*    debugStamps()
{
    static long long* buf = [] {
        long long* p = nullptr;
        if (std::getenv("L3K_STAMPS") && hipMalloc(&p, n_stamps * sizeof(long long)) == hipSuccess)
            (void)hipMemset(p, 0, n_stamps * sizeof(long long));
        return p;
    }();
    return buf;
}
} // namespace
extern "C" int l3k_debug_stamps(long long* host, int n)
{
    long long* p = debugStamps();
    if (!p || n > n_stamps)
        return -1;
    return hipMemcpy(host, p, n * sizeof(long long), hipMemcpyDeviceToHost) == hipSuccess ? 0 : -3;
}
#endif

namespace
{

// ElemArgs::scratch_alloc: the context's scratch arena, at least `bytes` large (kernels in flight on the context's stream may
// still use the old arena when it has to grow: hipFree waits for them)
double* contextScratch(void* owner, size_t bytes)
{
    auto* ctx = static_cast< l3k_ctx* >(owner);
    if (bytes <= ctx->scratch_bytes)
        return ctx->scratch;
    if (ctx->scratch)
        (void)hipFree(ctx->scratch);
    ctx->scratch       = nullptr;
    ctx->scratch_bytes = 0;
    if (hipMalloc(reinterpret_cast< void** >(&ctx->scratch), bytes) != hipSuccess)
        return nullptr;
    ctx->scratch_bytes = bytes;
    return ctx->scratch;
}

// What `which` selects of items that come in two classes (interior first: n_first of n_total): the classes it covers and
// its range.  3 / 4 = first / second half of the first class (one half overlaps the import, the other the export); colour
// by colour these become: all of the class / nothing.  valid = false: no such `which`
struct WhichRange
{
    bool    valid, classes[2];
    int64_t begin, count;
};
WhichRange rangeOf(int which, int64_t n_first, int64_t n_total)
{
    switch (which)
    {
    case 0: return {true, {true, false}, 0, n_first};
    case 1: return {true, {false, true}, n_first, n_total - n_first};
    case 2: return {true, {true, true}, 0, n_total};
    case 3: return {true, {true, false}, 0, n_first / 2};
    case 4: return {true, {false, false}, n_first / 2, n_first - n_first / 2};
    default: return {};
    }
}
// A colour plan walked: one launch per non-empty colour of the classes covered, in (class, colour) order
template < typename Set, typename Launch >
int walkColourPlan(const std::vector< int64_t > (&det_ptr)[2], const bool (&classes)[2], Set&& set, Launch&& launch)
{
    for (int cls = 0; cls < 2; ++cls)
        if (classes[cls])
            for (size_t c = 0; c + 1 < det_ptr[cls].size(); ++c)
            {
                const int64_t count = det_ptr[cls][c + 1] - det_ptr[cls][c];
                set(det_ptr[cls][c], count);
                if (count > 0)
                    if (int rc = launch())
                        return rc;
            }
    return 0;
}

// the operands every launch of a term takes: the mesh arrays, the tables, the fields, the time and the dof layout
void termArgs(const KernelTerm& t, l3k::dev::ElemArgs& a)
{
    const l3k_mesh* m = t.mesh;
    a                 = {};
    a.elem_nodes      = m->elem_nodes.ptr;
    a.elem_verts      = m->elem_verts.ptr;
    a.dirichlet       = m->dirichlet.ptr;
    a.tables          = t.tables.ptr;
    a.fields          = t.fields;
    a.ldf             = t.ldf;
    a.n_owned_dofs    = m->nOwnedDofs();
    a.time            = t.time;
    a.dofs_per_node   = m->dofs_per_node;
    for (int u = 0; u < l3k::dev::max_unknowns; ++u)
        a.field_inds[u] = t.field_inds[u];
}
// ... the vectors of an apply (owned rows and ghost rows of x and y) and of a diag / rhs pass
void applyOperands(l3k::dev::ElemArgs& a, const double* d_x, size_t ldx, const double* d_xghost, size_t ldxg, double* d_y, size_t ldy,
                   double* d_yghost, size_t ldyg, double alpha)
{
    a.x = d_x, a.xg = d_xghost, a.y = d_y, a.yg = d_yghost;
    a.ldx = ldx, a.ldxg = ldxg, a.ldy = ldy, a.ldyg = ldyg;
    a.alpha = alpha;
}
void diagRhsOperands(l3k::dev::ElemArgs& a, const double* d_dirichlet_vals, size_t ldg, double* d_diag, double* d_rhs, size_t ldr,
                     double* d_diag_ghost, double* d_rhs_ghost, size_t ldrg)
{
    a.dirichlet_vals = d_dirichlet_vals;
    a.ldg            = ldg;
    a.y = d_rhs, a.ldy = ldr, a.yg = d_rhs_ghost, a.ldyg = ldrg;
    a.diag = d_diag, a.diag_g = d_diag_ghost;
}
// `energy` (applies): where a single-column launch adds x^T A x, l3k_mf_energy_begin's target; only the apply kernel reads it
int fillArgs(l3k_mf* mf, int which, int ncols, l3k::dev::ElemArgs& a, double* energy = nullptr)
{
    const l3k_mesh* m = mf->mesh;
    termArgs(*mf, a);
    a.elem_flags      = m->elem_flags.ptr;
    a.exclusive_node_begin = m->exclusive_begin;
    a.exclusive_node_end   = m->exclusive_end;
    a.slot_tab             = m->slot_tab.ptr;
    a.all_affine           = m->all_affine ? 1 : 0;
    a.tune                 = &mf->ctx->tune;
    a.scratch_alloc        = &contextScratch;
    a.scratch_owner        = mf->ctx;
    // dynamic batch distribution of the single-wave kernel (l3k_tuning::static_deal: the static deal)
    a.work_counters        = mf->ctx->tune.static_deal ? nullptr : mf->ctx->work_counters;
    a.energy        = ncols == 1 ? energy : nullptr;
    a.energy_done   = &mf->energy_done;
    a.n_shell              = m->n_shell;
    a.tables_host     = mf->tables_host.data();
#ifdef L3K_ABLATION // (tools/kbench.py's switches exist in the ablation build only)
    static const int dbg_flags = [] {
        const char* e = std::getenv("L3K_DEBUG_FLAGS");
        return e ? std::atoi(e) : 0;
    }();
    a.dbg    = dbg_flags;
    a.stamps = debugStamps();
#endif
    a.dense  = mf->dense;
    a.ref_z0 = mf->ctx->reference_z0 ? 1 : 0;
    const WhichRange r = rangeOf(which, m->n_interior, m->n_elems);
    if (!r.valid)
    {
        setError("which must be 0 (interior), 1 (border), 2 (all), 3 or 4 (first / second half of the interior)");
        return -1;
    }
    a.elem_begin = r.begin;
    a.elem_count = r.count;
    if (int rc = checkFieldsSet(mf))
        return rc;
    return checkColumns(ncols, mf->n_rhs);
}
} // namespace
// ... of a LocalAssembly launch: all columns of the elements [first, first + count), written from position 0 of the output
int assemblyArgs(l3k_mf* mf, int64_t first, int64_t count, l3k::dev::ElemArgs& a)
{
    if (int rc = fillArgs(mf, 2, mf->n_rhs, a))
        return rc;
    a.elem_begin     = first;
    a.elem_count     = count;
    a.elem_begin_out = 0;
    return 0;
}
const l3k::dev::Instance* instanceFor(const l3k_mf* mf, int ncols)
{
    const auto* inst = l3k::dev::findInstance(mf->kernel_id, mf->mesh->order, mf->nq, ncols);
    if (!inst)
        setError("no device instantiation for kernel %d, order %d, nq %d, ncols %d: add it to L3K_FOR_EACH_INSTANCE "
                 "(l3ster_amd/csrc/user_kernels.hpp) and rebuild",
                 mf->kernel_id, mf->mesh->order, mf->nq, ncols);
    return inst;
}
const l3k::dev::BoundaryInstance* boundaryInstanceFor(const l3k_bnd* b, int ncols, const char* what)
{
    const auto* inst = l3k::dev::findBoundaryInstance(b->kernel_id, b->mesh->order, b->nq, ncols);
    if (!inst)
        setError("%s%sno device instantiation for boundary kernel %d, order %d, nq %d, ncols %d: add it to "
                 "L3K_FOR_EACH_BOUNDARY_INSTANCE (l3ster_amd/csrc/user_kernels.hpp) and rebuild",
                 what ? what : "", what ? ": " : "", b->kernel_id, b->mesh->order, b->nq, ncols);
    return inst;
}
namespace
{
// How an apply of `ncols` columns is launched (l3k_mf_apply_elems launches the plan, l3k_mf_route describes it): through the
// ncols-column instance; else, as the reference does when fewer columns than n_rhs are passed
// (algsys/MatrixFreeSystem.hpp:1124-1138), through the single-column one -- for a dense dof layout all columns in one pass over
// the elements (node ids, flags and the work ticket once per element, MatrixFreeSystem.hpp:678-688; l3k_tuning::column_by_column
// switches it off for cross-checks), otherwise column by column.
enum class ColumnPlan
{
    instance,
    one_pass,
    per_column
};
const l3k::dev::Instance* planColumns(const l3k_mf* mf, int ncols, ColumnPlan& plan)
{
    plan = ColumnPlan::instance;
    if (const auto* inst = l3k::dev::findInstance(mf->kernel_id, mf->mesh->order, mf->nq, ncols))
        return inst;
    const auto* inst = instanceFor(mf, 1);
    plan = inst && inst->apply_cols && mf->dense && !mf->ctx->deterministic && !mf->ctx->tune.column_by_column ? ColumnPlan::one_pass
                                                                                                            : ColumnPlan::per_column;
    return inst;
}
} // namespace
// LocalAssembly: mf->ws grown to the coefficient workspace of `count` elements; flag = its trailing double, which the assembly
// kernels set on a degenerate element, cleared on the context's stream
int assemblyWorkspace(l3k_mf* mf, const l3k::dev::Instance* inst, int64_t count, double*& flag)
{
    const size_t need = inst->assemble_ws_doubles * size_t(count) + 1;
    if (need > mf->ws_doubles)
    {
        if (mf->ws)
            L3K_HIP(hipFree(mf->ws));
        mf->ws = nullptr;
        L3K_HIP(hipMalloc(reinterpret_cast< void** >(&mf->ws), need * sizeof(double)));
        mf->ws_doubles = need;
    }
    flag = mf->ws + need - 1;
    L3K_HIP(hipMemsetAsync(flag, 0, sizeof(double), mf->ctx->stream));
    return 0;
}
// ... and the flag (or the two of a pipeline's halves) read back on s, which is synchronised: -2 if one is set.  The miss counter of
// l3k_assemble_global rides on the same synchronisation
int readDegenerateFlags(hipStream_t s, const double* d_flag0, const double* d_flag1, const unsigned long long* d_count, int64_t* n_missing)
{
    double             flags[2] = {0., 0.};
    unsigned long long h        = 0;
    L3K_HIP(hipMemcpyAsync(&flags[0], d_flag0, sizeof(double), hipMemcpyDeviceToHost, s));
    if (d_flag1)
        L3K_HIP(hipMemcpyAsync(&flags[1], d_flag1, sizeof(double), hipMemcpyDeviceToHost, s));
    if (d_count)
        L3K_HIP(hipMemcpyAsync(&h, d_count, sizeof h, hipMemcpyDeviceToHost, s));
    L3K_HIP(hipStreamSynchronize(s));
    if (n_missing)
        *n_missing = int64_t(h);
    if (flags[0] != 0. || flags[1] != 0.)
    {
        setError("Encountered degenerate element ( |J| <= 0 )"); // algsys/AssembleLocalSystem.hpp:249
        return -2;
    }
    return 0;
}
namespace
{
// F_e = sum_q w detJ B_q^T f_q into d_F: the sum-factorised RHS-mode kernel without Dirichlet lifting, element-local output
void elementLocalRhs(l3k::dev::ElemArgs& a, double* d_F)
{
    a.dirichlet      = nullptr;
    a.elem_flags     = nullptr;
    a.dirichlet_vals = nullptr;
    a.diag           = nullptr;
    a.local_out      = 1;
    a.y              = d_F; // unused for addressing in local_out mode, must be non-null
}
} // namespace

namespace
{
int bndArgs(const l3k_bnd* b, int which, int ncols, l3k::dev::ElemArgs& a)
{
    termArgs(*b, a);
    a.face_elem = b->face_elem.ptr;
    a.face_side = b->face_side.ptr;
    const WhichRange r = rangeOf(which, b->n_interior_faces, b->n_faces);
    if (which > 2 || !r.valid) // (sides have no halves)
    {
        setError("which must be 0 (sides of interior elements), 1 (of border elements) or 2 (all)");
        return -1;
    }
    a.face_begin = r.begin;
    a.face_count = r.count;
    if (int rc = checkFieldsSet(b))
        return rc;
    return checkColumns(ncols, b->n_rhs);
}
// the launch ranges of a side call: the caller's range, or in deterministic mode one launch per colour of the classes it
// covers (the ELEMENTS of the sides of one colour share no node: the order of the additions to a row is the order of the launches)
template < typename F >
int forEachSideRange(const l3k_bnd* b, int which, l3k::dev::ElemArgs& a, F&& launch)
{
    if (!b->ctx->deterministic)
        return launch(a);
    if (b->det_ptr[0].empty())
    {
        setError("deterministic mode was enabled after this boundary term was created: create it with the mode on");
        return -1;
    }
    return walkColourPlan(
        b->det_ptr, rangeOf(which, b->n_interior_faces, b->n_faces).classes, [&](int64_t begin, int64_t count) { a.face_begin = begin, a.face_count = count; },
        [&] { return launch(a); });
}
int bndApplyImpl(l3k_bnd* b, int which, const double* d_x, size_t ldx, const double* d_xghost, size_t ldxg, double* d_y,
                 size_t ldy, double* d_yghost, size_t ldyg, int ncols, double alpha)
{
    l3k::dev::ElemArgs a;
    if (int rc = bndArgs(b, which, ncols, a))
        return rc;
    const l3k_mesh* m = b->mesh;
    if (ldx < size_t(m->nOwnedDofs()) || ldy < size_t(m->nOwnedDofs()))
    {
        setError("leading dimension smaller than the number of owned dofs");
        return -1;
    }
    if (m->n_ghost_nodes > 0 && which != 0 && (!d_xghost || !d_yghost))
    {
        setError("mesh has ghost nodes: sides of border elements need the ghost import/export buffers");
        return -1;
    }
    applyOperands(a, d_x, ldx, d_xghost, ldxg, d_y, ldy, d_yghost, ldyg, alpha);
    const auto* inst = boundaryInstanceFor(b, ncols);
    if (!inst)
        return -4;
    return forEachSideRange(b, which, a, [&](l3k::dev::ElemArgs& r) { return inst->apply(r, b->blobPtr(), b->ctx->stream); });
}
int bndDiagRhsImpl(l3k_bnd* b, int which, const double* d_dirichlet_vals, size_t ldg, double* d_diag, double* d_rhs,
                   size_t ldr, double* d_diag_ghost, double* d_rhs_ghost, size_t ldrg)
{
    l3k::dev::ElemArgs a;
    if (int rc = bndArgs(b, which, b->n_rhs, a))
        return rc;
    if (b->mesh->n_ghost_nodes > 0 && which != 0 && (!d_rhs_ghost || (d_diag && !d_diag_ghost)))
    {
        setError("mesh has ghost nodes: sides of border elements need the ghost diag / rhs buffers");
        return -1;
    }
    diagRhsOperands(a, d_dirichlet_vals, ldg, d_diag, d_rhs, ldr, d_diag_ghost, d_rhs_ghost, ldrg);
    const auto* inst = boundaryInstanceFor(b, b->n_rhs);
    if (!inst)
        return -4;
    return forEachSideRange(b, which, a, [&](l3k::dev::ElemArgs& r) { return inst->diag_rhs(r, b->blobPtr(), b->ctx->stream); });
}
} // namespace

// ------------------------------------------------------------------------------------------------ C ABI

namespace
{
// Greedy colouring of the elements by their corner nodes (two conforming hexes share a node iff they share a corner), class
// by class in element order; the element arrays are copied in (class, colour, element) order.  A launch over one colour of
// one class adds at most once to any row, so the order of the additions to a row is the order of the launches.
int buildDeterministicPlan(l3k_mesh& m, const l3k_mesh_desc* d, const std::vector< uint8_t >& flags)
{
    const int     n1 = d->order + 1, nv = 1 << d->dim;
    const int64_t N  = d->dim == 2 ? int64_t(n1) * n1 : int64_t(n1) * n1 * n1;
    m.det_corner_nodes = l3k::host::cornerNodes(d->dim, d->order, d->n_elems, d->elem_nodes); // (kept: the colouring of boundary sides)
    std::vector< int64_t > self(static_cast< size_t >(d->n_elems)); // (every element is its own item)
    for (int64_t e = 0; e < d->n_elems; ++e)
        self[e] = e;
    l3k::host::ColourPlan plan;
    if (int rc = l3k::host::colourItems(d->n_elems, d->n_interior_elems, self.data(), m.det_corner_nodes.data(), nv, "", plan))
        return rc;
    const auto& order = plan.order;
    std::swap(m.det_ptr, plan.ptr);
    std::vector< uint32_t > nodes(static_cast< size_t >(d->n_elems * N));
    const int               nvd = nv * 3; // vertex doubles per element
    std::vector< double >   verts(static_cast< size_t >(d->n_elems) * nvd);
    std::vector< uint8_t >  fl(flags.empty() ? 0 : static_cast< size_t >(d->n_elems));
    for (int64_t i = 0; i < d->n_elems; ++i)
    {
        const int64_t e = order[i];
        std::copy_n(d->elem_nodes + e * N, N, nodes.begin() + i * N);
        std::copy_n(d->elem_verts + e * nvd, nvd, verts.begin() + i * nvd);
        if (!fl.empty())
            fl[i] = flags[e];
    }
    hipStream_t s = m.ctx->stream;
    if (int rc = m.det_elem_nodes.upload(nodes.data(), nodes.size(), s))
        return rc;
    if (int rc = m.det_elem_verts.upload(verts.data(), verts.size(), s))
        return rc;
    if (!fl.empty())
        if (int rc = m.det_elem_flags.upload(fl.data(), fl.size(), s))
            return rc;
    L3K_HIP(hipStreamSynchronize(s)); // (the staging vectors are locals)
    m.det_colour = std::move(plan.colour);
    m.det_built  = true;
    return 0;
}
// the launch ranges of an element call: the caller's range as it is, or in deterministic mode the colours of the classes
// it covers, on the permuted element arrays (the two halves of the interior, which = 3 / 4, become: all of it / nothing)
template < typename F >
int forEachLaunchRange(const l3k_mf* mf, int which, l3k::dev::ElemArgs& a, F&& launch)
{
    const l3k_mesh* m = mf->mesh;
    if (!mf->ctx->deterministic)
        return launch(a);
    if (!m->det_built)
    {
        setError("deterministic mode was enabled after this mesh was created: create the mesh with the mode on");
        return -1;
    }
    a.elem_nodes = m->det_elem_nodes.ptr;
    a.elem_verts = m->det_elem_verts.ptr;
    a.elem_flags = m->det_elem_flags.ptr;
    a.energy     = nullptr; // (the fused <x, A x> is an atomic accumulation: the caller takes the fixed-order dot product)
    return walkColourPlan(
        m->det_ptr, rangeOf(which, m->n_interior, m->n_elems).classes, [&](int64_t begin, int64_t count) { a.elem_begin = begin, a.elem_count = count; },
        [&] { return launch(a); });
}
} // namespace

extern "C" {

int l3k_version(void)
{
    return L3K_VERSION;
}
const char* l3k_last_error(void)
{
    return l3k::dev::lastError();
}

int l3k_gll_nodes(int n, double* x)
{
    if (n < 2 || !x)
    {
        setError("l3k_gll_nodes: need n >= 2");
        return -1;
    }
    const auto v = l3k::host::gllNodes(n);
    std::copy(v.begin(), v.end(), x);
    return 0;
}
int l3k_gl_rule(int nq, double* x, double* w)
{
    if (nq < 1 || !x || !w)
    {
        setError("l3k_gl_rule: need nq >= 1");
        return -1;
    }
    std::vector< double > xv, wv;
    l3k::host::glRule(nq, xv, wv);
    std::copy(xv.begin(), xv.end(), x);
    std::copy(wv.begin(), wv.end(), w);
    return 0;
}
int l3k_n_qps1d(int p, int value_order, int derivative_order)
{
    return value_order * p + derivative_order * (p - 1) + 1;
}
int l3k_basis_1d(int p, int nq, double* I, double* D)
{
    if (p < 1 || nq < 1 || !I || !D)
    {
        setError("l3k_basis_1d: bad arguments");
        return -1;
    }
    std::vector< double > Iv, Dv;
    l3k::host::basis1d(p, nq, Iv, Dv);
    std::copy(Iv.begin(), Iv.end(), I);
    std::copy(Dv.begin(), Dv.end(), D);
    return 0;
}
int l3k_interp_1d(int p_from, int p_to, double* out)
{
    if (p_from < 1 || p_from > 8 || p_to < 1 || p_to > 8 || !out)
    {
        setError("l3k_interp_1d: orders must lie in 1 .. 8 and out must not be null");
        return -1;
    }
    const auto v = l3k::host::interp1d(p_from, p_to);
    std::copy(v.begin(), v.end(), out);
    return 0;
}
int l3k_colloc_deriv(int nq, double* C)
{
    if (nq < 1 || !C)
    {
        setError("l3k_colloc_deriv: bad arguments");
        return -1;
    }
    const auto v = l3k::host::collocDeriv(nq);
    std::copy(v.begin(), v.end(), C);
    return 0;
}

int l3k_kernel_info(int kernel_id, l3k_kparams* params, const char** name, size_t* param_bytes)
{
    const auto* k = findKernel(kernel_id);
    if (!k)
    {
        setError("unknown kernel id %d", kernel_id);
        return -1;
    }
    if (params)
        *params = k->kp;
    if (name)
        *name = k->name;
    if (param_bytes)
        *param_bytes = k->bytes;
    return 0;
}
int l3k_plugin_load(const char* path)
{
    if (!path)
    {
        setError("l3k_plugin_load: null path");
        return -1;
    }
    // the plugin's static registrars call registerPluginKernel / registerInstance / ... of THIS library
    void* h = dlopen(path, RTLD_NOW | RTLD_LOCAL);
    if (!h)
    {
        setError("l3k_plugin_load: %s", dlerror());
        return -1;
    }
    return 0;
}
int l3k_instance_count(void)
{
    return l3k::dev::instanceCount();
}
int l3k_instance_info(int i, int* kernel_id, int* order, int* nq, int* ncols)
{
    const auto* inst = l3k::dev::instanceAt(i);
    if (!inst)
    {
        setError("instance index %d out of range", i);
        return -1;
    }
    *kernel_id = inst->kernel_id;
    *order     = inst->order;
    *nq        = inst->nq;
    *ncols     = inst->ncols;
    return 0;
}

int l3k_ctx_create(int hip_device, void* hip_stream, l3k_ctx** out)
{
    if (!out)
    {
        setError("l3k_ctx_create: out is null");
        return -1;
    }
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count < 1)
    {
        setError("no HIP device available: libl3k has no CPU fallback (the device path is the product)");
        return -2;
    }
    if (hip_device < 0 || hip_device >= count)
    {
        setError("hip_device %d outside [0,%d)", hip_device, count);
        return -1;
    }
    L3K_HIP(hipSetDevice(hip_device));
    auto* ctx = new l3k_ctx{hip_device, static_cast< hipStream_t >(hip_stream)};
    // the ONLY place the product reads the environment: initial values of the context's settings (include/l3k.h: l3k_tuning)
    if (const char* e = std::getenv("L3K_DETERMINISTIC"))
        ctx->deterministic = std::atoi(e) != 0;
    const auto flag = [](const char* name, int& field) {
        if (const char* e = std::getenv(name))
            field = *e != '\0' && std::strcmp(e, "0") != 0;
    };
    if (const char* e = std::getenv("L3K_GENERIC_BELOW"))
        ctx->tune.generic_below = std::atoll(e);
    if (const char* e = std::getenv("L3K_FAST_WAVES_PER_CU"))
        ctx->tune.waves_per_cu = std::atoi(e) > 0 ? std::atoi(e) : 0;
    flag("L3K_FAST_STATIC", ctx->tune.static_deal);
    flag("L3K_NO_AFFINE", ctx->tune.no_affine);
    flag("L3K_COLUMN_BY_COLUMN", ctx->tune.column_by_column);
    flag("L3K_ASSEMBLE_DENSE", ctx->tune.assemble_dense);
    flag("L3K_ASM_TWO_LAUNCHES", ctx->tune.assemble_two_launches);
    flag("L3K_SCATTER_PER_ENTRY", ctx->tune.scatter_per_entry);
    flag("L3K_ASM_DIRECT_STORE", ctx->tune.assemble_direct_store);
    flag("L3K_ASM_NO_SYMMETRISE", ctx->tune.assemble_no_symmetrise);
    // the context's own device buffers are allocated here, with its device current: a later call may come from a thread
    // whose current device is another one (several contexts in one process: thread-emulated ranks, a multi-GPU C++ host)
    if (hipMalloc(reinterpret_cast< void** >(&ctx->work_counters), 9 * 128) != hipSuccess ||
        hipMalloc(reinterpret_cast< void** >(&ctx->red_ws), sizeof(double) * 2 * l3k_cg_blocks) != hipSuccess)
    {
        delete ctx;
        setError("l3k_ctx_create: hipMalloc of the context buffers failed");
        return -3;
    }
    *out = ctx;
    return 0;
}
int l3k_ctx_set_stream(l3k_ctx* ctx, void* hip_stream)
{
    if (!ctx)
    {
        setError("null ctx");
        return -1;
    }
    ctx->stream = static_cast< hipStream_t >(hip_stream);
    return 0;
}
int l3k_ctx_set_deterministic(l3k_ctx* ctx, int on)
{
    if (!ctx)
    {
        setError("null ctx");
        return -1;
    }
    ctx->deterministic = on != 0;
    return 0;
}
int l3k_ctx_set_reference_z0(l3k_ctx* ctx, int on)
{
    if (!ctx)
    {
        setError("null context");
        return -1;
    }
    ctx->reference_z0 = on != 0;
    return 0;
}
int l3k_ctx_get_tuning(const l3k_ctx* ctx, l3k_tuning* out)
{
    if (!ctx || !out)
    {
        setError("l3k_ctx_get_tuning: null argument");
        return -1;
    }
    *out = ctx->tune;
    return 0;
}
int l3k_ctx_set_tuning(l3k_ctx* ctx, const l3k_tuning* in)
{
    if (!ctx || !in)
    {
        setError("l3k_ctx_set_tuning: null argument");
        return -1;
    }
    if (in->generic_below < 0 || in->waves_per_cu < 0 || in->waves_per_cu > 64)
    {
        setError("l3k_ctx_set_tuning: generic_below must be >= 0 and waves_per_cu in [0, 64]");
        return -1;
    }
    ctx->tune = *in;
    return 0;
}
int l3k_ctx_synchronize(l3k_ctx* ctx)
{
    if (!ctx)
    {
        setError("null ctx");
        return -1;
    }
    L3K_HIP(hipStreamSynchronize(ctx->stream));
    return 0;
}
int l3k_ctx_destroy(l3k_ctx* ctx)
{
    delete ctx;
    return 0;
}

int l3k_mesh_create(l3k_ctx* ctx, const l3k_mesh_desc* d, l3k_mesh** out)
{
    if (!ctx || !d || !out)
    {
        setError("l3k_mesh_create: null argument");
        return -1;
    }
    if (d->dim != 2 && d->dim != 3)
    {
        setError("l3k_mesh_create: dim must be 2 (quads) or 3 (hexes), got %d", d->dim);
        return -1;
    }
    if (d->order < 1 || d->n_elems < 0 || d->n_interior_elems < 0 || d->n_interior_elems > d->n_elems ||
        d->dofs_per_node < 1 || d->n_owned_nodes < 0 || d->n_ghost_nodes < 0 || !d->elem_nodes || !d->elem_verts)
    {
        setError("l3k_mesh_create: inconsistent descriptor");
        return -1;
    }
    const int     dim     = d->dim;
    const int64_t N       = dim == 2 ? int64_t(d->order + 1) * (d->order + 1) : int64_t(d->order + 1) * (d->order + 1) * (d->order + 1);
    const int     nvd     = (1 << dim) * 3; // vertex coordinates per element: [2^dim][3]
    const int64_t n_nodes = d->n_owned_nodes + d->n_ghost_nodes;
    if (n_nodes * d->dofs_per_node >= (int64_t(1) << 31) * 8)
    {
        setError("too many local dofs");
        return -1;
    }
    l3k::host::MeshPlan plan; // (host staging: outlives the synchronisation below)
    if (int rc = l3k::host::analyseMesh(d, plan))
        return rc;
    L3K_HIP(hipSetDevice(ctx->device));
    auto m             = std::make_unique< l3k_mesh >();
    m->ctx             = ctx;
    m->dim             = d->dim;
    m->order           = d->order;
    m->dofs_per_node   = d->dofs_per_node;
    m->n_elems         = d->n_elems;
    m->n_interior      = d->n_interior_elems;
    m->n_owned_nodes   = d->n_owned_nodes;
    m->n_ghost_nodes   = d->n_ghost_nodes;
    m->exclusive_begin = plan.exclusive_begin;
    m->exclusive_end   = plan.exclusive_end;
    m->n_shell         = plan.n_shell;
    m->all_affine      = plan.all_affine;
    if (int rc = m->elem_nodes.upload(d->elem_nodes, size_t(d->n_elems * N), ctx->stream))
        return rc;
    if (int rc = m->elem_verts.upload(d->elem_verts, size_t(d->n_elems) * nvd, ctx->stream))
        return rc;
    if (int rc = m->slot_tab.upload(plan.slot_tab.data(), plan.slot_tab.size(), ctx->stream))
        return rc;
    if (d->dirichlet)
    {
        if (int rc = m->dirichlet.upload(d->dirichlet, size_t(n_nodes * d->dofs_per_node), ctx->stream))
            return rc;
        if (int rc = m->owned_dirichlet_rows.upload(plan.owned_dirichlet_rows.data(), plan.owned_dirichlet_rows.size(), ctx->stream))
            return rc;
    }
    if (int rc = m->elem_flags.upload(plan.elem_flags.data(), plan.elem_flags.size(), ctx->stream))
        return rc;
    if (ctx->deterministic)
        if (int rc = buildDeterministicPlan(*m, d, plan.elem_flags))
            return rc;
    L3K_HIP(hipStreamSynchronize(ctx->stream)); // host arrays may be freed by the caller after return
    *out = m.release();
    return 0;
}
int l3k_mesh_destroy(l3k_mesh* mesh)
{
    delete mesh;
    return 0;
}

int l3k_mf_create(l3k_ctx* ctx, l3k_mesh* mesh, int kernel_id, const void* kparam_blob, size_t kparam_bytes,
                  const l3k_asmopts* opts, const int* field_inds, int n_rhs, l3k_mf** out)
{
    if (!ctx || !mesh || !out)
    {
        setError("l3k_mf_create: null argument");
        return -1;
    }
    const auto* k = findKernel(kernel_id);
    if (!k)
    {
        setError("unknown kernel id %d", kernel_id);
        return -1;
    }
    if (k->boundary)
    {
        setError("kernel %s is a boundary equation kernel: use l3k_bnd_create", k->name);
        return -1;
    }
    if (int rc = checkKernelDim(k->kp, mesh))
        return rc;
    if (int rc = checkParamBlock(*k, kparam_blob, kparam_bytes))
        return rc;
    if (n_rhs < 1)
    {
        setError("n_rhs must be >= 1");
        return -1;
    }
    const int nq = quadraturePoints(mesh, opts);
    if (int rc = checkCollocation(nq, mesh))
        return rc;
    auto mf = std::make_unique< l3k_mf >();
    mf->init(ctx, mesh, *k, nq, n_rhs, kparam_blob, kparam_bytes);
    if (k->kp.n_unknowns > l3k::dev::max_unknowns)
    {
        setError("n_unknowns > %d unsupported", l3k::dev::max_unknowns);
        return -1;
    }
    if (int rc = resolveFieldInds(field_inds, k->kp.n_unknowns, mesh, mf->field_inds))
        return rc;
    mf->dense = k->kp.n_unknowns == mesh->dofs_per_node;
    for (int u = 0; u < k->kp.n_unknowns; ++u)
        mf->dense = mf->dense && mf->field_inds[u] == u;
    // rows of nodes touched by one element only are written (not accumulated) by the element kernel, see l3k_mf_scale
    mf->fuse = mf->dense && mesh->exclusive_end > mesh->exclusive_begin;
    L3K_HIP(hipSetDevice(ctx->device));
    if (int rc = uploadTables(mesh, nq, ctx->stream, mf->tables_host, mf->tables))
        return rc;
    L3K_HIP(hipStreamSynchronize(ctx->stream));
    *out = mf.release();
    return 0;
}
int l3k_mf_destroy(l3k_mf* mf)
{
    delete mf;
    return 0;
}
int l3k_mf_set_fields(l3k_mf* mf, const double* d_soa, size_t ld)
{
    if (!mf)
    {
        setError("null mf");
        return -1;
    }
    return setFields(*mf, d_soa, ld);
}
int l3k_mf_set_time(l3k_mf* mf, double time)
{
    if (!mf)
    {
        setError("null mf");
        return -1;
    }
    mf->time = time;
    return 0;
}

extern "C++" int checkApplyOperands(const l3k_mf* mf, int ncols, const double* d_x, size_t ldx, const double* d_xghost, size_t ldxg, const double* d_y,
                       size_t ldy, const double* d_yghost, size_t ldyg)
{
    const l3k_mesh* m = mf->mesh;
    if (int rc = checkFieldsSet(mf))
        return rc;
    if (int rc = checkColumns(ncols, mf->n_rhs))
        return rc;
    if (ldx < size_t(m->nOwnedDofs()) || ldy < size_t(m->nOwnedDofs()))
    {
        setError("leading dimension smaller than the number of owned dofs");
        return -1;
    }
    // the kernels move a node's dofs with 16-byte accesses (and run 18 % slower when a node's row straddles a 32-byte
    // boundary: profiles/r01_kbench_vector_alignment.log)
    const auto misaligned = [](const void* p, size_t ld, int nc) {
        return reinterpret_cast< uintptr_t >(p) % 16 != 0 || (nc > 1 && (ld * sizeof(double)) % 16 != 0);
    };
    // only the one-wave kernel uses 16-byte accesses: it takes dense dof layouts with an even number of unknowns
    // (FastCfg::feasible); every other shape runs the generic kernel with 8-byte accesses
    if (mf->dense && mf->kp.n_unknowns % 2 == 0 &&
        (misaligned(d_x, ldx, ncols) || misaligned(d_y, ldy, ncols) ||
         (m->n_ghost_nodes > 0 && d_xghost && misaligned(d_xghost, ldxg, ncols)) ||
         (m->n_ghost_nodes > 0 && d_yghost && misaligned(d_yghost, ldyg, ncols))))
    {
        setError("vectors must be 16-byte aligned (columns too: even leading dimensions); 32-byte alignment is faster");
        return -1;
    }
    return 0;
}

int l3k_last_fast_launch(unsigned* variant)
{
    if (!variant)
    {
        setError("l3k_last_fast_launch: null argument");
        return -1;
    }
    *variant = l3k::dev::lastFastLaunch();
    return 0;
}

int l3k_mf_route(l3k_mf* mf, int which, int ncols, int with_energy, char* buf, size_t n)
{
    if (!mf || !buf || n == 0)
    {
        setError("l3k_mf_route: null argument");
        return -1;
    }
    buf[0] = '\0';
    // (with_energy: any non-null device pointer, nothing is launched; with boundary terms attached l3k_mf_energy_begin does not
    // arm the accumulation, and the route says so)
    l3k::dev::ElemArgs a;
    double* const      energy = with_energy ? (mf->boundary_terms.empty() ? reinterpret_cast< double* >(mf->ctx->red_ws) : nullptr)
                                            : mf->energy_target;
    if (int rc = fillArgs(mf, which, ncols, a, energy))
        return rc;
    if (mf->ctx->deterministic)
        a.energy = nullptr; // (forEachLaunchRange)
    const l3k_mesh* m = mf->mesh;
    // the pointer relations the launcher looks at: ghost rows in buffers of their own whenever the mesh has ghost nodes and the
    // launch covers border elements (l3k_mf_apply_elems is given separate import / export buffers)
    static const double dummy[2] = {0., 0.};
    a.x = a.y = nullptr;
    a.xg = a.yg = (m->n_ghost_nodes > 0 && (which == 1 || which == 2)) ? const_cast< double* >(dummy) : nullptr;
    a.fuse_beta = mf->fuse;
    ColumnPlan  plan;
    const auto* inst = planColumns(mf, ncols, plan);
    if (!inst)
        return -4;
    if (plan == ColumnPlan::one_pass)
        a.n_cols = ncols;
    if (!inst->route)
    {
        setError("this instance carries no route description");
        return -4;
    }
    if (int rc2 = inst->route(a, buf, n))
        return rc2;
    const size_t len = std::strlen(buf);
    if (const auto* meta = l3k::api::findKernel(mf->kernel_id))
        std::snprintf(buf + len, n - len, " [kernel %d \"%s\"%s%s%s]", mf->kernel_id, meta->name,
                      plan == ColumnPlan::per_column ? ", column by column" : "",
                      mf->ctx->deterministic ? ", deterministic: one launch per colour" : "", mf->ctx->reference_z0 ? ", reference z=0" : "");
    return 0;
}

extern "C++" int scaleRows(l3k_ctx* ctx, double* d_y, size_t ldy, int64_t rows, int ncols, double beta)
{
    if (beta == 1. || rows <= 0)
        return 0;
    hipLaunchKernelGGL(scaleKernel, dim3(gridFor(rows)), dim3(256), 0, ctx->stream, d_y, ldy, rows, ncols, beta);
    L3K_HIP(hipGetLastError());
    return 0;
}
int l3k_mf_scale(l3k_mf* mf, double* d_y, size_t ldy, int ncols, double beta)
{
    if (!mf || !d_y)
    {
        setError("l3k_mf_scale: null argument");
        return -1;
    }
    const l3k_mesh* m    = mf->mesh;
    const int64_t   rows = m->nOwnedDofs();
    // rows of exclusive nodes are left to the element kernel (it writes alpha*A*x + beta*y there)
    const int64_t r0 = mf->fuse ? m->exclusive_begin * m->dofs_per_node : rows;
    const int64_t r1 = mf->fuse ? m->exclusive_end * m->dofs_per_node : rows;
    if (int rc = scaleRows(mf->ctx, d_y, ldy, r0, ncols, beta))
        return rc;
    return scaleRows(mf->ctx, d_y + r1, ldy, rows - r1, ncols, beta);
}

int l3k_mf_apply_elems(l3k_mf* mf, int which, const double* d_x, size_t ldx, const double* d_xghost, size_t ldxg,
                       double* d_y, size_t ldy, double* d_yghost, size_t ldyg, int ncols, double alpha, double beta)
{
    return mfApplyElems(mf, which, d_x, ldx, d_xghost, ldxg, d_y, ldy, d_yghost, ldyg, ncols, alpha, beta, mf && mf->fuse);
}
extern "C++" int mfApplyElems(l3k_mf* mf, int which, const double* d_x, size_t ldx, const double* d_xghost, size_t ldxg, double* d_y, size_t ldy,
                              double* d_yghost, size_t ldyg, int ncols, double alpha, double beta, int fuse)
{
    if (!mf || !d_x || !d_y)
    {
        setError("l3k_mf_apply_elems: null argument");
        return -1;
    }
    int cur_dev = -1;
    if (hipGetDevice(&cur_dev) != hipSuccess || cur_dev != mf->ctx->device) // (several contexts in one process)
        L3K_HIP(hipSetDevice(mf->ctx->device));
    l3k::dev::ElemArgs a;
    if (int rc = fillArgs(mf, which, ncols, a, mf->energy_target))
        return rc;
    if (a.elem_count > 0 && (a.energy || mf->energy_target)) // (armed but ncols > 1: a.energy is null, never "fused")
        ++mf->energy_expected;
    const l3k_mesh* m = mf->mesh;
    if (int rc = checkApplyOperands(mf, ncols, d_x, ldx, d_xghost, ldxg, d_y, ldy, d_yghost, ldyg))
        return rc;
    if (m->n_ghost_nodes > 0 && (which == 1 || which == 2) && (!d_xghost || !d_yghost))
    {
        setError("mesh has ghost nodes: border elements need the ghost import/export buffers");
        return -1;
    }
    applyOperands(a, d_x, ldx, d_xghost, ldxg, d_y, ldy, d_yghost, ldyg, alpha);
    a.beta      = beta;
    a.fuse_beta = fuse;
    const auto  launch = [&](const l3k::dev::Instance* inst, l3k::dev::ElemArgs& ac) {
        return forEachLaunchRange(mf, which, ac, [&](l3k::dev::ElemArgs& r) { return inst->apply(r, mf->blobPtr(), mf->ctx->stream); });
    };
    ColumnPlan  plan;
    const auto* inst = planColumns(mf, ncols, plan);
    if (!inst)
        return -4;
    int rc = 0;
    if (plan == ColumnPlan::instance)
        rc = launch(inst, a);
    else if (plan == ColumnPlan::one_pass)
    {
        a.n_cols = ncols;
        a.energy = nullptr;
        rc       = inst->apply_cols(a, mf->blobPtr(), mf->ctx->stream);
    }
    else
        rc = l3k::dev::forEachColumn(a, ncols, [&](l3k::dev::ElemArgs& ac) { return launch(inst, ac); });
    if (rc)
        return rc;
    // boundary equation kernels registered on this system act on the sides of the same element range
    // (the halves of the interior: all sides of interior elements go with the first half)
    if (which != 4)
        for (l3k_bnd* b : mf->boundary_terms)
            if (int rc = bndApplyImpl(b, which == 3 ? 0 : which, d_x, ldx, d_xghost, ldxg, d_y, ldy, d_yghost, ldyg, ncols, alpha))
                return rc;
    return 0;
}

extern "C++" int dirichletRowsOf(l3k_ctx* ctx, const l3k_mesh* m, const double* d_x, size_t ldx, double* d_y, size_t ldy, int ncols, double alpha)
{
    const auto& rows = m->owned_dirichlet_rows;
    if (rows.n == 0)
        return 0;
    hipLaunchKernelGGL(dirichletRowsKernel, dim3(gridFor(int64_t(rows.n))), dim3(256), 0, ctx->stream, rows.ptr,
                       int64_t(rows.n), d_x, ldx, d_y, ldy, ncols, alpha);
    L3K_HIP(hipGetLastError());
    return 0;
}
int l3k_mf_dirichlet_rows(l3k_mf* mf, const double* d_x, size_t ldx, double* d_y, size_t ldy, int ncols, double alpha)
{
    if (!mf || !d_x || !d_y)
    {
        setError("l3k_mf_dirichlet_rows: null argument");
        return -1;
    }
    return dirichletRowsOf(mf->ctx, mf->mesh, d_x, ldx, d_y, ldy, ncols, alpha);
}

// s[1] += sum over the owned Dirichlet rows of x_d^2 (their share of x^T A x: those rows of the operator are the identity)
__global__ void dirichletEnergyKernel(const int64_t* __restrict__ rows, int64_t n, const double* __restrict__ x, double* __restrict__ s1)
{
    __shared__ double sh[256];
    double            acc = 0.;
    for (int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x; i < n; i += int64_t(gridDim.x) * 256)
        acc += x[rows[i]] * x[rows[i]];
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1)
    {
        if (int(threadIdx.x) < w)
            sh[threadIdx.x] += sh[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0 && sh[0] != 0.)
        unsafeAtomicAdd(s1, sh[0]);
}

int l3k_mf_energy_begin(l3k_mf* mf, double* d_s)
{
    if (!mf || !d_s)
    {
        setError("l3k_mf_energy_begin: null argument");
        return -1;
    }
    L3K_HIP(hipMemsetAsync(d_s + 1, 0, sizeof(double), mf->ctx->stream));
    // the element kernel accumulates x^T A x only on its single-wave route and only for domain kernels
    mf->energy_target   = mf->boundary_terms.empty() ? d_s + 1 : nullptr;
    mf->energy_done     = 0;
    mf->energy_expected = 0;
    return 0;
}
int l3k_mf_energy_end(l3k_mf* mf, const double* d_x, int* fused)
{
    if (!mf || !d_x || !fused)
    {
        setError("l3k_mf_energy_end: null argument");
        return -1;
    }
    double* const s1  = mf->energy_target;
    *fused            = s1 != nullptr && mf->energy_done == mf->energy_expected;
    mf->energy_target = nullptr;
    const auto& rows  = mf->mesh->owned_dirichlet_rows;
    if (*fused && rows.n > 0)
    {
        const int64_t nr = int64_t(rows.n);
        hipLaunchKernelGGL(dirichletEnergyKernel, dim3(unsigned(std::min< int64_t >((nr + 255) / 256, 1024))), dim3(256), 0,
                           mf->ctx->stream, rows.ptr, nr, d_x, s1);
        L3K_HIP(hipGetLastError());
    }
    return 0;
}
int l3k_mf_apply_energy(l3k_mf* mf, const double* d_x, double* d_y, double* d_s)
{
    if (!mf || !d_x || !d_y || !d_s)
    {
        setError("l3k_mf_apply_energy: null argument");
        return -1;
    }
    const size_t n = size_t(mf->mesh->nOwnedDofs());
    if (int rc = l3k_mf_energy_begin(mf, d_s))
        return rc;
    const int rc = l3k_mf_apply(mf, d_x, n, d_y, n, 1, 1., 0.);
    int       fused = 0;
    if (int rc2 = l3k_mf_energy_end(mf, d_x, &fused))
        return rc2;
    if (rc)
        return rc;
    return fused ? 0 : l3k_cg_dot_pap(mf->ctx, d_x, d_y, int64_t(n), d_s); // (the dot product overwrites s[1])
}

int l3k_mf_apply(l3k_mf* mf, const double* d_x, size_t ldx, double* d_y, size_t ldy, int ncols, double alpha, double beta)
{
    if (!mf)
    {
        setError("null mf");
        return -1;
    }
    if (mf->mesh->n_ghost_nodes != 0)
    {
        setError("l3k_mf_apply is the single-rank form; this mesh has ghost nodes: use the split-phase entry points");
        return -1;
    }
    if (!d_x || !d_y)
    {
        setError("l3k_mf_apply: null argument");
        return -1;
    }
    // (a refused call leaves y as it was: the refusals come before the scaling pass)
    if (int rc = checkApplyOperands(mf, ncols, d_x, ldx, nullptr, 0, d_y, ldy, nullptr, 0))
        return rc;
    if (int rc = l3k_mf_scale(mf, d_y, ldy, ncols, beta))
        return rc;
    if (int rc = l3k_mf_apply_elems(mf, 2, d_x, ldx, nullptr, 0, d_y, ldy, nullptr, 0, ncols, alpha, beta))
        return rc;
    return l3k_mf_dirichlet_rows(mf, d_x, ldx, d_y, ldy, ncols, alpha);
}

int l3k_pack_rows(l3k_ctx* ctx, const double* d_src, size_t ld, int ncols, const int32_t* d_idx, int64_t n, double* d_dst)
{
    if (!ctx || (n > 0 && (!d_src || !d_idx || !d_dst)))
    {
        setError("l3k_pack_rows: null argument");
        return -1;
    }
    if (n <= 0)
        return 0;
    hipLaunchKernelGGL(packKernel, dim3(gridFor(n)), dim3(256), 0, ctx->stream, d_src, ld, ncols, d_idx, n, d_dst);
    L3K_HIP(hipGetLastError());
    return 0;
}
int l3k_unpack_add_rows(l3k_ctx* ctx, const double* d_src, int64_t n, const int32_t* d_idx, double* d_dst, size_t ld,
                        int ncols)
{
    if (!ctx || (n > 0 && (!d_src || !d_idx || !d_dst)))
    {
        setError("l3k_unpack_add_rows: null argument");
        return -1;
    }
    if (n <= 0)
        return 0;
    hipLaunchKernelGGL(unpackAddKernel, dim3(gridFor(n)), dim3(256), 0, ctx->stream, d_src, n, d_idx, d_dst, ld, ncols);
    L3K_HIP(hipGetLastError());
    return 0;
}

int l3k_mf_diag_rhs(l3k_mf* mf, int which, const double* d_dirichlet_vals, size_t ldg, double* d_diag, double* d_rhs,
                    size_t ldr, double* d_diag_ghost, double* d_rhs_ghost, size_t ldrg, int finalize)
{
    if (!mf || !d_rhs)
    {
        setError("l3k_mf_diag_rhs: null argument");
        return -1;
    }
    l3k::dev::ElemArgs a;
    if (int rc = fillArgs(mf, which, mf->n_rhs, a))
        return rc;
    diagRhsOperands(a, d_dirichlet_vals, ldg, d_diag, d_rhs, ldr, d_diag_ghost, d_rhs_ghost, ldrg);
    if (mf->mesh->n_ghost_nodes > 0 && which != 0 && (!d_rhs_ghost || (d_diag && !d_diag_ghost)))
    {
        setError("mesh has ghost nodes: border elements need the ghost diag / rhs buffers");
        return -1;
    }
    const auto* inst = instanceFor(mf, mf->n_rhs);
    if (!inst)
        return -4;
    if (int rc = forEachLaunchRange(mf, which, a, [&](l3k::dev::ElemArgs& r) {
            return inst->diag_rhs(r, mf->blobPtr(), mf->ctx->stream);
        }))
        return rc;
    for (l3k_bnd* b : mf->boundary_terms)
        if (int rc = bndDiagRhsImpl(b, which, d_dirichlet_vals, ldg, d_diag, d_rhs, ldr, d_diag_ghost, d_rhs_ghost, ldrg))
            return rc;
    return finalize && d_diag ? l3k_mf_dirichlet_finalize(mf, d_dirichlet_vals, ldg, d_diag, d_rhs, ldr) : 0;
}

int l3k_mf_dirichlet_finalize(l3k_mf* mf, const double* d_dirichlet_vals, size_t ldg, double* d_diag, double* d_rhs, size_t ldr)
{
    if (!mf || !d_diag || !d_rhs)
    {
        setError("l3k_mf_dirichlet_finalize: null argument");
        return -1;
    }
    return dirichletFinalizeOf(mf->ctx, mf->mesh, d_dirichlet_vals, ldg, d_diag, d_rhs, ldr, mf->n_rhs);
}
extern "C++" int dirichletFinalizeOf(l3k_ctx* ctx, const l3k_mesh* m, const double* d_dirichlet_vals, size_t ldg, double* d_diag, double* d_rhs,
                                     size_t ldr, int n_rhs)
{
    const auto& rows = m->owned_dirichlet_rows;
    if (rows.n == 0)
        return 0;
    hipLaunchKernelGGL(dirichletFinalizeKernel, dim3(gridFor(int64_t(rows.n))), dim3(256), 0, ctx->stream, rows.ptr, int64_t(rows.n),
                       d_dirichlet_vals, ldg, d_diag, d_rhs, ldr, n_rhs);
    L3K_HIP(hipGetLastError());
    return 0;
}

// K_e of [first, first + count) into d_K (row-major) through the tiled layout: sub-batches formed on the context's stream into one
// of the system's two halves, turned on the second stream (runSubBatches, objects.hpp)
static int assembleRowMajorViaTiled(l3k_mf* mf, const l3k::dev::Instance* inst, int64_t first, int64_t count, double* d_K)
{
    const l3k_mesh* m  = mf->mesh;
    const int       N1 = m->order + 1, U = mf->kp.n_unknowns, Nd = N1 * N1 * N1 * U;
    const size_t    mat = size_t(Nd) * Nd; // doubles per matrix
    // sub-batches of <= 1.5 GiB of tiled matrices per buffer (large launches: the kernels of the route are all memory-bound, so their
    // overlap on the two streams buys little and small sub-batches only add launch tails: tools/r04_stored_subbatch.py)
    int64_t nb = int64_t((size_t(1536) << 20) / (mat * sizeof(double)));
    nb         = nb < 1 ? 1 : nb;
    if (mf->ctx->tune.assemble_sub_batch > 0)
        nb = mf->ctx->tune.assemble_sub_batch;
    nb = nb > count ? count : nb;
    const size_t kd = size_t(nb) * mat, wd = inst->assemble_ws_doubles * size_t(nb) + 1;
    auto&        g  = mf->gasm;
    L3K_HIP(hipSetDevice(mf->ctx->device));
    if (int rc = g.ensure(kd + wd, true))
        return rc;
    hipStream_t sa   = mf->ctx->stream;
    // bitwise symmetric matrices, as the reference returns them: the x-major tiled layout and the one-pass mirroring transposition
    // (api_assembled.hip).  l3k_tuning::assemble_no_symmetrise: the plain tiled layout and the plain transposition (K[i][j] and
    // K[j][i] then differ by rounding) -- the cross-check of the former
    const bool sym = !mf->ctx->tune.assemble_no_symmetrise;
    // (the flags of degenerate elements: the trailing double of each half's coefficient workspace)
    double* const flag[2] = {g.buf[0] + kd + wd - 1, g.buf[1] + kd + wd - 1};
    for (int k = 0; k < 2; ++k)
        L3K_HIP(hipMemsetAsync(flag[k], 0, sizeof(double), sa));
    if (int rc = runSubBatches(
            g, sa, first, count, nb,
            [&](int k, int64_t at, int64_t n) {
                l3k::dev::ElemArgs a;
                if (int rc = assemblyArgs(mf, at, n, a))
                    return rc;
                a.K              = g.buf[k];
                a.K_tiled        = sym ? 2 : 1;
                a.workspace      = g.buf[k] + kd + size_t(nb - n) * inst->assemble_ws_doubles; // (the flag keeps one position per half)
                return inst->assemble(a, mf->blobPtr(), sa);
            },
            [&](int k, int64_t at, int64_t n) { // the transposition
                double* out = d_K + size_t(at - first) * mat;
                return sym ? launchTiledXToRowMajorSym(U, N1, n, g.buf[k], out, g.second) : launchTiledToRowMajor(U, N1, n, g.buf[k], out, g.second);
            }))
        return rc;
    return readDegenerateFlags(sa, flag[0], flag[1]);
}

int l3k_local_assemble(l3k_mf* mf, int64_t first, int64_t count, double* d_K, double* d_F, double* d_checksum)
{
    if (!mf)
    {
        setError("null mf");
        return -1;
    }
    const l3k_mesh* m = mf->mesh;
    if (int rc = refuseQuads(m, "l3k_local_assemble"))
        return rc;
    if (int rc = checkRange(m, first, count))
        return rc;
    if (count == 0)
        return 0;
    const bool sides = assemblesBoundary(mf);
    if (sides)
    {
        if (int rc = checkAssembleBoundary(mf, "l3k_local_assemble"))
            return rc;
        if (d_checksum)
        {
            setError("l3k_local_assemble: no checksum with l3k_mf_assemble_boundary on (the streaming checksum has no stored matrix to "
                     "add the side matrices to)");
            return -1;
        }
    }
    const auto* inst = instanceFor(mf, mf->n_rhs);
    if (!inst)
        return -4;
    l3k::dev::ElemArgs a;
    if (int rc = assemblyArgs(mf, first, count, a))
        return rc;
    a.K              = d_K;
    a.F              = d_F;
    a.checksum       = d_checksum;
    hipStream_t s    = mf->ctx->stream;
    // Stored row-major matrices: formed in the tiled layout (coalesced stores) and turned by a transposition kernel on a second
    // stream, sub-batch by sub-batch -- the assembly kernels cannot fill the 64-byte lines of a row-major K_e (four workgroups and
    // two iterations per line: 3.9 x write traffic).  l3k_tuning::assemble_direct_store keeps the direct store (cross-check).
    const l3k_tuning& tune = mf->ctx->tune;
    // (orders >= 4, or on request: below, a matrix is a few KB and the direct store wins -- order 2: 12.9 M against 6.7 M matrices/s,
    // profiles/r04_stored_assembly.jsonl)
    const bool via_tiled = d_K && inst->assemble_tiled && mf->kp.n_unknowns <= 4 && m->order <= 7 && !tune.assemble_dense &&
                           !tune.assemble_two_launches && !tune.assemble_direct_store && (m->order >= 4 || tune.assemble_sub_batch > 0);
    if (via_tiled)
    {
        if (int rc = assembleRowMajorViaTiled(mf, inst, first, count, d_K))
            return rc;
        a.K = nullptr; // (a checksum asked for beside K comes from a streaming pass below)
    }
    if (a.K || d_checksum)
    {
        double* flag = nullptr;
        if (int rc = assemblyWorkspace(mf, inst, count, flag))
            return rc;
        a.workspace = mf->ws;
        if (d_checksum)
            L3K_HIP(hipMemsetAsync(d_checksum, 0, sizeof(double) * size_t(count), s));
        if (int rc = inst->assemble(a, mf->blobPtr(), s))
            return rc;
        if (int rc = readDegenerateFlags(s, flag))
            return rc;
    }
    if (d_F)
    {
        elementLocalRhs(a, d_F);
        if (int rc = inst->diag_rhs(a, mf->blobPtr(), s))
            return rc;
    }
    if (sides) // the finished row-major K_e, F_e take the side systems of their elements (on the tiled route: after the transposition)
        return accumulateBoundarySides(mf, first, count, d_K, d_F);
    return 0;
}
// K_e of the elements [first, first + count) in the TILED layout (include/l3k.h): what l3k_assemble_global keeps between its two kernels
int l3k_local_assemble_tiled(l3k_mf* mf, int64_t first, int64_t count, double* d_Kt)
{
    if (!mf || !d_Kt)
    {
        setError("l3k_local_assemble_tiled: null argument");
        return -1;
    }
    const l3k_mesh* m = mf->mesh;
    if (int rc = refuseQuads(m, "l3k_local_assemble_tiled"))
        return rc;
    if (assemblesBoundary(mf))
    {
        setError("l3k_local_assemble_tiled: not with l3k_mf_assemble_boundary on (the side matrices are added to row-major element "
                 "matrices: use l3k_local_assemble)");
        return -1;
    }
    if (int rc = checkRange(m, first, count))
        return rc;
    if (count == 0)
        return 0;
    const auto* inst = instanceFor(mf, mf->n_rhs);
    if (!inst)
        return -4;
    if (!inst->assemble_tiled)
    {
        setError("l3k_local_assemble_tiled: this shape has no sum-factorised assembly kernel");
        return -1;
    }
    l3k::dev::ElemArgs a;
    if (int rc = assemblyArgs(mf, first, count, a))
        return rc;
    a.K              = d_Kt;
    a.K_tiled        = 1;
    hipStream_t s    = mf->ctx->stream;
    double*     flag = nullptr;
    if (int rc = assemblyWorkspace(mf, inst, count, flag))
        return rc;
    a.workspace = mf->ws;
    if (int rc = inst->assemble(a, mf->blobPtr(), s))
        return rc;
    return readDegenerateFlags(s, flag);
}
// assembleGlobalSystem (algsys/AssembleGlobalSystem.hpp:20-53: per element assembleLocalSystem -> scatterLocalSystem) for the
// elements [first, first + count) as ONE call: sub-batches of element systems are formed into one of two workspace buffers on the
// context's stream while the previous sub-batch is summed into the CSR values on a second stream -- the assembly kernels are
// bound by the FP64 pipe, the scatter by the memory-side atomic units, so the two overlap (runSubBatches, objects.hpp).
int l3k_assemble_global(l3k_mf* mf, int64_t first, int64_t count, const int64_t* d_row_ptr, const int32_t* d_col_ind,
                        double* d_values, double* d_rhs, size_t ldr, int skip_dirichlet, size_t workspace_bytes, int64_t* n_missing)
{
    if (!mf || !d_row_ptr || !d_col_ind || !d_values)
    {
        setError("l3k_assemble_global: null argument");
        return -1;
    }
    const l3k_mesh* m = mf->mesh;
    if (int rc = refuseQuads(m, "l3k_assemble_global"))
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
    const bool sides = assemblesBoundary(mf);
    if (sides)
        if (int rc = checkAssembleBoundary(mf, "l3k_assemble_global"))
            return rc;
    const auto* inst = instanceFor(mf, mf->n_rhs);
    if (!inst)
        return -4;
    L3K_HIP(hipSetDevice(mf->ctx->device));
    // element matrices between the two kernels in the tiled layout where the sum-factorised assembly kernel exists (its stores
    // coalesce, the scatter transposes a row through LDS); the dense cross-check kernel writes the reference's row-major layout
    const int    tiled = inst->assemble_tiled && mf->kp.n_unknowns <= 4 && m->order <= 7 && !mf->ctx->tune.assemble_dense ? 1 : 0;
    const int    N1 = m->order + 1, Nd = N1 * N1 * N1 * mf->kp.n_unknowns, R = mf->n_rhs;
    const size_t per_elem = sizeof(double) * (size_t(Nd) * Nd + size_t(Nd) * R + inst->assemble_ws_doubles);
    if (workspace_bytes == 0)
        workspace_bytes = size_t(1) << 30;
    int64_t nb = int64_t(workspace_bytes / 2 / per_elem);
    nb         = nb < 1 ? 1 : (nb > count ? count : nb);
    // at least ~8 sub-batches per call where the batch stays large enough for full launches (the overlap needs several)
    if (const int64_t eighth = (count + 7) / 8; nb > eighth && eighth >= 512)
        nb = eighth;
    while (nb * Nd > int64_t(0x7fffffff) / 64 && nb > 1) // (launch-size limits of the kernels)
        nb /= 2;
    const size_t kd = size_t(nb) * Nd * Nd, fd = d_rhs ? size_t(nb) * Nd * R : 0, wd = inst->assemble_ws_doubles * size_t(nb) + 1;
    auto&        g  = mf->gasm;
    if (int rc = g.ensure(kd + fd + wd, true))
        return rc;
    hipStream_t         sa      = mf->ctx->stream;
    unsigned long long* d_count = n_missing ? mf->ctx->missCounter() : nullptr;
    if (d_count)
        L3K_HIP(hipMemsetAsync(d_count, 0, sizeof(unsigned long long), sa));
    // (the flags of degenerate elements: the trailing double of each half's coefficient workspace, set by the kernels)
    double* const flag[2] = {g.buf[0] + kd + fd + wd - 1, g.buf[1] + kd + fd + wd - 1};
    for (int k = 0; k < 2; ++k)
        L3K_HIP(hipMemsetAsync(flag[k], 0, sizeof(double), sa));
    if (int rc = runSubBatches(
            g, sa, first, count, nb,
            [&](int k, int64_t at, int64_t n) {
                l3k::dev::ElemArgs a;
                if (int rc = assemblyArgs(mf, at, n, a))
                    return rc;
                a.K              = g.buf[k];
                a.K_tiled        = tiled;
                a.F              = d_rhs ? g.buf[k] + kd : nullptr;
                a.checksum       = nullptr;
                // (the kernels keep the degenerate-element flag behind the coefficients of THEIR elem_count elements: a short last
                // sub-batch works in the tail of the half, so that the flag has one position per half)
                a.workspace      = g.buf[k] + kd + fd + size_t(nb - n) * inst->assemble_ws_doubles;
                if (int rc = inst->assemble(a, mf->blobPtr(), sa))
                    return rc;
                if (!d_rhs)
                    return 0;
                L3K_HIP(hipMemsetAsync(a.F, 0, sizeof(double) * size_t(n) * Nd * R, sa));
                elementLocalRhs(a, a.F);
                return inst->diag_rhs(a, mf->blobPtr(), sa);
            },
            [&](int k, int64_t at, int64_t n) {
                return launchAssembledScatter(mf, at, n, g.buf[k], d_rhs ? g.buf[k] + kd : nullptr, d_row_ptr, d_col_ind, d_values, d_rhs, ldr,
                                              skip_dirichlet, d_count, g.second, tiled);
            }))
        return rc;
    if (int rc = readDegenerateFlags(sa, flag[0], flag[1], d_count, n_missing))
        return rc;
    if (sides) // the domain route above is the tiled one; the sides of the range's elements follow through the standalone side route
        return assembleGlobalBoundarySides(mf, first, count, d_row_ptr, d_col_ind, d_values, d_rhs, ldr, skip_dirichlet, workspace_bytes,
                                           n_missing);
    return 0;
}
// ------------------------------------------------------------------------------------------------ boundary terms
int l3k_bnd_create(l3k_ctx* ctx, l3k_mesh* mesh, int kernel_id, const void* kparam_blob, size_t kparam_bytes,
                   const l3k_asmopts* opts, const int* field_inds, int n_rhs, int64_t n_faces, const int64_t* face_elem,
                   const uint8_t* face_side, l3k_bnd** out)
{
    if (!ctx || !mesh || !out || n_faces < 0 || (n_faces > 0 && (!face_elem || !face_side)))
    {
        setError("l3k_bnd_create: bad argument");
        return -1;
    }
    const auto* k = findKernel(kernel_id);
    if (!k || !k->boundary)
    {
        setError("kernel id %d is not a boundary equation kernel", kernel_id);
        return -1;
    }
    if (int rc = checkKernelDim(k->kp, mesh))
        return rc;
    if (int rc = checkParamBlock(*k, kparam_blob, kparam_bytes))
        return rc;
    if (n_rhs < 1 || k->kp.n_unknowns > l3k::dev::max_unknowns)
    {
        setError("n_rhs must be >= 1 and n_unknowns <= %d", l3k::dev::max_unknowns);
        return -1;
    }
    if (int rc = l3k::host::checkSides(mesh->dim, mesh->n_elems, n_faces, face_elem, face_side))
        return rc;
    auto b = std::make_unique< l3k_bnd >();
    b->init(ctx, mesh, *k, quadraturePoints(mesh, opts), n_rhs, kparam_blob, kparam_bytes);
    if (int rc = resolveFieldInds(field_inds, k->kp.n_unknowns, mesh, b->field_inds))
        return rc;
    std::vector< int64_t > fe;
    std::vector< uint8_t > fs;
    b->n_interior_faces = l3k::host::interiorSidesFirst(mesh->n_interior, n_faces, face_elem, face_side, fe, fs);
    b->n_faces          = n_faces;
    b->list_elem.assign(face_elem, face_elem + n_faces); // (the caller's order: what the assembly entry points index)
    b->list_side.assign(face_side, face_side + n_faces);
    if (ctx->deterministic)
    {
        // greedy colouring of the sides by ALL 2^dim corner nodes of their elements: the side kernel scatter-adds over every
        // node of the element (the normal derivative couples all of them, device/boundary.hpp, device/quad_boundary.hpp), so
        // two sides may share a colour only if their elements share no node -- for conforming hexes / quads: no corner.
        // (Colouring by the side's own four corners let the z- side of a corner element and the x- side of the element stacked
        // on it into one launch.)  Class by class; the lists are stored in (class, colour) order
        if (!mesh->det_built)
        {
            setError("deterministic mode was enabled after this mesh was created: create the mesh with the mode on");
            return -1;
        }
        l3k::host::ColourPlan plan;
        if (int rc = l3k::host::colourItems(n_faces, b->n_interior_faces, fe.data(), mesh->det_corner_nodes.data(), 1 << mesh->dim,
                                            " for the boundary sides", plan))
            return rc;
        std::vector< int64_t > fe2(fe.size());
        std::vector< uint8_t > fs2(fs.size());
        for (size_t i = 0; i < fe.size(); ++i)
            fe2[i] = fe[size_t(plan.order[i])], fs2[i] = fs[size_t(plan.order[i])];
        std::swap(b->det_ptr, plan.ptr);
        fe.swap(fe2);
        fs.swap(fs2);
    }
    L3K_HIP(hipSetDevice(ctx->device));
    std::vector< double > block; // (host staging: outlives the synchronisation below)
    if (int rc = uploadTables(mesh, b->nq, ctx->stream, block, b->tables))
        return rc;
    if (int rc = b->face_elem.upload(fe.data(), fe.size(), ctx->stream))
        return rc;
    if (int rc = b->face_side.upload(fs.data(), fs.size(), ctx->stream))
        return rc;
    L3K_HIP(hipStreamSynchronize(ctx->stream));
    *out = b.release();
    return 0;
}
int l3k_bnd_destroy(l3k_bnd* bnd)
{
    delete bnd;
    return 0;
}
int l3k_bnd_set_fields(l3k_bnd* bnd, const double* d_soa, size_t ld)
{
    if (!bnd)
    {
        setError("null bnd");
        return -1;
    }
    return setFields(*bnd, d_soa, ld);
}
int l3k_bnd_set_time(l3k_bnd* bnd, double time)
{
    if (!bnd)
    {
        setError("null bnd");
        return -1;
    }
    bnd->time = time;
    return 0;
}
int l3k_bnd_apply(l3k_bnd* bnd, int which, const double* d_x, size_t ldx, const double* d_xghost, size_t ldxg, double* d_y,
                  size_t ldy, double* d_yghost, size_t ldyg, int ncols, double alpha)
{
    if (!bnd || !d_x || !d_y)
    {
        setError("l3k_bnd_apply: null argument");
        return -1;
    }
    return bndApplyImpl(bnd, which, d_x, ldx, d_xghost, ldxg, d_y, ldy, d_yghost, ldyg, ncols, alpha);
}
int l3k_bnd_diag_rhs(l3k_bnd* bnd, int which, const double* d_dirichlet_vals, size_t ldg, double* d_diag, double* d_rhs,
                     size_t ldr, double* d_diag_ghost, double* d_rhs_ghost, size_t ldrg)
{
    if (!bnd || !d_rhs)
    {
        setError("l3k_bnd_diag_rhs: null argument");
        return -1;
    }
    return bndDiagRhsImpl(bnd, which, d_dirichlet_vals, ldg, d_diag, d_rhs, ldr, d_diag_ghost, d_rhs_ghost, ldrg);
}
int l3k_mf_attach_boundary(l3k_mf* mf, l3k_bnd* bnd)
{
    if (!mf || !bnd)
    {
        setError("l3k_mf_attach_boundary: null argument");
        return -1;
    }
    if (bnd->mesh != mf->mesh)
    {
        setError("boundary term and system live on different meshes");
        return -1;
    }
    if (bnd->n_rhs != mf->n_rhs)
    {
        setError("boundary term has n_rhs = %d, system has %d", bnd->n_rhs, mf->n_rhs);
        return -1;
    }
    mf->boundary_terms.push_back(bnd);
    return 0;
}

} // extern "C"
