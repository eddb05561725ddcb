// objects.hpp -- the objects behind the opaque handles of include/l3k.h and the helpers the api_*.hip files share.
#ifndef L3K_OBJECTS_HPP
#define L3K_OBJECTS_HPP

#include "l3k.h"

#include "device/common.hpp"
#include "host/tables.hpp"
#include "user_kernels.hpp"

#include <hip/hip_runtime.h>

#include <dlfcn.h>

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <type_traits>
#include <string>
#include <utility>
#include <vector>

namespace l3k::dev
{
const char* lastError();
}
using l3k::dev::setError;

#define L3K_HIP(call)                                                                                                  \
    do                                                                                                                 \
    {                                                                                                                  \
        const hipError_t err_ = (call);                                                                                \
        if (err_ != hipSuccess)                                                                                        \
        {                                                                                                              \
            setError("%s failed: %s (%s:%d)", #call, hipGetErrorString(err_), __FILE__, __LINE__);                     \
            return -3;                                                                                                 \
        }                                                                                                              \
    } while (0)


namespace l3k::api
{
inline unsigned gridFor(int64_t n, int block = 256)
{
    const int64_t g = (n + block - 1) / block;
    return static_cast< unsigned >(g < 1 ? 1 : (g > 8192 ? 8192 : g));
}

template < typename T >
struct DevBuf
{
    T*     ptr = nullptr;
    size_t n   = 0;
    DevBuf()   = default;
    DevBuf(const DevBuf&)            = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : ptr{o.ptr}, n{o.n}
    {
        o.ptr = nullptr;
        o.n   = 0;
    }
    DevBuf& operator=(DevBuf&& o) noexcept
    {
        if (this != &o)
        {
            if (ptr)
                (void)hipFree(ptr);
            ptr   = o.ptr;
            n     = o.n;
            o.ptr = nullptr;
            o.n   = 0;
        }
        return *this;
    }
    ~DevBuf()
    {
        if (ptr)
            (void)hipFree(ptr);
    }
    int alloc(size_t count)
    {
        n = count;
        if (count == 0)
            return 0;
        L3K_HIP(hipMalloc(reinterpret_cast< void** >(&ptr), count * sizeof(T)));
        return 0;
    }
    int upload(const T* host, size_t count, hipStream_t s)
    {
        n = count;
        if (count == 0)
            return 0;
        L3K_HIP(hipMalloc(reinterpret_cast< void** >(&ptr), count * sizeof(T)));
        L3K_HIP(hipMemcpyAsync(ptr, host, count * sizeof(T), hipMemcpyHostToDevice, s));
        return 0;
    }
};
} // namespace l3k::api
using l3k::api::DevBuf;
using l3k::api::gridFor;

inline constexpr int l3k_cg_blocks = 1024; // blocks of the PCG's two-stage reductions (api_solver.hip)
struct l3k_ctx
{
    int         device;
    hipStream_t stream;
    // bitwise-reproducible mode (L3K_DETERMINISTIC=1 or l3k_ctx_set_deterministic): element launches go colour by colour
    // (no two elements of a launch share a node), so every row of y receives its contributions in a fixed order
    bool        deterministic = false;
    // l3k_ctx_set_reference_z0: matrix-free applies hand domain kernels Point{x, y, 0.} as the reference's hex sum-factorisation
    // path does (algsys/SumFactorization.hpp:732); default: the true point (what its local-element path passes)
    bool        reference_z0 = false;
    l3k_tuning  tune = l3k::dev::defaultTuning(); // launch-route settings (the environment is read once, in l3k_ctx_create)
    double*     red_ws = nullptr; // per-block partial sums of the PCG dot products (cg_blocks * 2 doubles)
    uint32_t*   work_counters = nullptr; // batch counters of the single-wave element kernel (8 x 128 bytes) + one more line:
    // the counter of l3k_assembled_scatter's entries outside the graph (no allocation per call)
    unsigned long long* missCounter() const { return reinterpret_cast< unsigned long long* >(work_counters + 8 * 32); }
    // global-memory working sets of the element kernels whose buffers exceed the LDS (ElemArgs::scratch): grown on demand
    double* scratch       = nullptr;
    size_t  scratch_bytes = 0;
    // partial sums of the GMRES pieces, which are called without a workspace object (l3k_gmres_multi_dot, l3k_gmres_project): grown on demand
    double* gmres_partials       = nullptr;
    size_t  gmres_partials_count = 0;
    ~l3k_ctx()
    {
        if (gmres_partials)
            (void)hipFree(gmres_partials);
        if (red_ws)
            (void)hipFree(red_ws);
        if (work_counters)
            (void)hipFree(work_counters);
        if (scratch)
            (void)hipFree(scratch);
    }
};
// workgroups of a launch whose workgroups stride over `count` items (the p-multigrid transfers, the rows of l3k_graph): the
// tuning's waves per CU where set (4 waves per workgroup), else the cap of the solver's vector kernels
inline unsigned stridedGrid(const l3k_ctx* ctx, int64_t count)
{
    int64_t cap = l3k_cg_blocks;
    if (ctx->tune.waves_per_cu > 0)
        cap = int64_t(ctx->tune.waves_per_cu) * l3k::dev::deviceComputeUnits() / 4;
    cap = cap < 1 ? 1 : cap;
    return unsigned(count < 1 ? 1 : (count < cap ? count : cap));
}
struct l3k_mesh
{
    l3k_ctx*            ctx;
    int                 dim, order, dofs_per_node;
    int64_t             n_elems, n_interior, n_owned_nodes, n_ghost_nodes;
    DevBuf< uint32_t >  elem_nodes;
    DevBuf< double >    elem_verts;
    DevBuf< uint8_t >   dirichlet;
    DevBuf< int64_t >   owned_dirichlet_rows;
    DevBuf< uint8_t >   elem_flags;
    int64_t             exclusive_begin = 0, exclusive_end = 0;
    // scatter order of the single-wave kernel: slot_tab[lane * 8 + k] = scatter slot of local node lane + (p+1)^2 * k; slots
    // [0, n_shell) are the element's non-internal nodes in ascending node-id order of a typical element (runs of contiguous
    // rows in y), slots [n_shell, N) its internal nodes = exactly the nodes of [exclusive_begin, exclusive_end)
    DevBuf< uint16_t >  slot_tab;
    int                 n_shell = 0;
    bool                all_affine = false; // every element is a parallelepiped (flags bit 1 of all elements)
    // deterministic mode: copies of the element arrays with the elements of each class (interior, border) sorted by colour;
    // det_ptr[0][c] .. det_ptr[0][c + 1] = interior elements of colour c, det_ptr[1][...] the border ones (positions in the
    // permuted arrays, which keep the interior elements first)
    bool                   det_built = false;
    DevBuf< uint32_t >     det_elem_nodes;
    DevBuf< double >       det_elem_verts;
    DevBuf< uint8_t >      det_elem_flags;
    std::vector< int64_t > det_ptr[2];
    std::vector< uint8_t >  det_colour; // host, [n_elems] in the ORIGINAL element order: the colour of each element
    std::vector< uint32_t > det_corner_nodes; // host, [n_elems][2^dim] in the ORIGINAL element order: colouring of boundary sides
    int64_t nOwnedDofs() const { return n_owned_nodes * dofs_per_node; }
    int64_t nLocalDofs() const { return (n_owned_nodes + n_ghost_nodes) * dofs_per_node; }
};
// Entry points without quad kernels (LocalAssembly and the assembled path) refuse quad meshes up front: -1 and the reason, and
// no hex kernel ever sees quad data
inline int refuseQuads(const l3k_mesh* m, const char* what)
{
    if (m && m->dim == 2)
    {
        setError("%s: quads (dim = 2) are not supported here; the device runs the matrix-free apply, diag / rhs, boundary terms, "
                 "integrals and values at nodes on quads", what);
        return -1;
    }
    return 0;
}
// appended to a dimension mismatch on a quad mesh: " (quads)"
inline const char* quadsNote(const l3k_mesh* m)
{
    return m->dim == 2 ? " (quads)" : "";
}
// ... and element ranges outside the mesh: -1
inline int checkRange(const l3k_mesh* m, int64_t first, int64_t count)
{
    if (first < 0 || count < 0 || first + count > m->n_elems)
    {
        setError("element range [%lld, %lld) outside [0, %lld)", (long long)first, (long long)(first + count), (long long)m->n_elems);
        return -1;
    }
    return 0;
}
struct l3k_bnd;
namespace l3k::api
{
struct KernelMeta
{
    int         id;
    l3k_kparams kp;
    const char* name;
    size_t      bytes;
    bool        boundary = false;
};
// registered equation kernels (built in or announced by a plugin) / residual kernels by id; nullptr if unknown
const KernelMeta* findKernel(int id);
const KernelMeta* findResidual(int id);
} // namespace l3k::api
// What a domain system (l3k_mf) and a boundary term (l3k_bnd) share: an equation kernel on a mesh with its operands
struct KernelTerm
{
    l3k_ctx*            ctx  = nullptr;
    l3k_mesh*           mesh = nullptr;
    int                 kernel_id = 0, nq = 0, n_rhs = 0;
    l3k_kparams         kp{};
    std::vector< char > blob;
    int                 field_inds[l3k::dev::max_unknowns] = {};
    DevBuf< double >    tables;
    const double*       fields = nullptr;
    size_t              ldf    = 0;
    double              time   = 0.;
    const void* blobPtr() const { return blob.empty() ? nullptr : blob.data(); } // the kernel's parameter block, if it has one
    void        init(l3k_ctx* c, l3k_mesh* m, const l3k::api::KernelMeta& k, int nq_, int n_rhs_, const void* kparam_blob, size_t kparam_bytes)
    {
        ctx = c, mesh = m, kernel_id = k.id, nq = nq_, n_rhs = n_rhs_, kp = k.kp;
        if (kparam_blob)
            blob.assign(static_cast< const char* >(kparam_blob), static_cast< const char* >(kparam_blob) + kparam_bytes);
    }
};
// The checks of what comes from outside, one each (0, or -1 with the error set); every entry point calls the ones it makes
inline int checkKernelDim(const l3k_kparams& kp, const l3k_mesh* mesh)
{
    if (kp.dimension == mesh->dim)
        return 0;
    setError("kernel dimension %d != mesh dimension %d%s", kp.dimension, mesh->dim, quadsNote(mesh));
    return -1;
}
inline int checkParamBlock(const l3k::api::KernelMeta& k, const void* kparam_blob, size_t kparam_bytes)
{
    if (!kparam_blob || kparam_bytes == k.bytes)
        return 0;
    setError("kernel %s expects a %zu-byte parameter block, got %zu", k.name, k.bytes, kparam_bytes);
    return -1;
}
// out[u] = field_inds[u] (null: u) for the kernel's unknowns, each inside [0, dofs_per_node)
inline int resolveFieldInds(const int* field_inds, int n_unknowns, const l3k_mesh* mesh, int* out)
{
    for (int u = 0; u < n_unknowns; ++u)
    {
        const int fi = field_inds ? field_inds[u] : u;
        if (fi < 0 || fi >= mesh->dofs_per_node)
        {
            setError("field_inds[%d] = %d outside [0, dofs_per_node = %d)", u, fi, mesh->dofs_per_node);
            return -1;
        }
        out[u] = fi;
    }
    return 0;
}
// quadrature points per direction from the assembly options (null: value order 1)
inline int quadraturePoints(const l3k_mesh* mesh, const l3k_asmopts* opts)
{
    const l3k_asmopts o = opts ? *opts : l3k_asmopts{1, 0, 0};
    return l3k_n_qps1d(mesh->order, o.value_order, o.derivative_order);
}
inline int checkCollocation(int nq, const l3k_mesh* mesh)
{
    if (nq >= mesh->order + 1)
        return 0;
    setError("nq = %d < p+1 = %d: the collocation-derivative device algorithm needs nq >= p+1", nq, mesh->order + 1);
    return -1;
}
// the 1-D table block of (order, nq) into `block` and from there to the device; `block` must outlive the copy on s
inline int uploadTables(const l3k_mesh* mesh, int nq, hipStream_t s, std::vector< double >& block, DevBuf< double >& tables)
{
    block = l3k::host::deviceTableBlock(mesh->order, nq);
    return tables.upload(block.data(), block.size(), s);
}
// the fields a kernel reads were set (T = l3k_mf / l3k_bnd names the kernel kind and the setter; `what`: optional prefix)
template < typename T >
int checkFieldsSet(const T* t, const char* what = nullptr)
{
    if (t->kp.n_fields == 0 || t->fields)
        return 0;
    setError("%s%s%s reads %d external fields but %s was not called", what ? what : "", what ? ": " : "", T::kernel_noun, t->kp.n_fields,
             T::fields_setter);
    return -1;
}
inline int checkColumns(int ncols, int n_rhs)
{
    if (ncols >= 1 && ncols <= n_rhs)
        return 0;
    setError("number of columns (%d) must be in [1, n_rhs = %d]", ncols, n_rhs); // algsys/MatrixFreeSystem.hpp:1035-1037
    return -1;
}
// l3k_*_set_fields: SoA fields with a leading dimension of at least the local nodes (null: none)
inline int setFields(KernelTerm& t, const double* d_soa, size_t ld)
{
    if (d_soa && ld < size_t(t.mesh->n_owned_nodes + t.mesh->n_ghost_nodes))
    {
        setError("field leading dimension %zu < number of local nodes", ld);
        return -1;
    }
    t.fields = d_soa;
    t.ldf    = ld;
    return 0;
}
// The sub-batch pipeline of the assembled path (runSubBatches below): two halves of element-system buffers, a
// second stream that consumes half i & 1 while the context's stream forms sub-batch i + 1 into the other, and the events that
// order the reuse of the halves.  Kept across calls (allocating gigabytes per call cost more than the pipeline saved)
struct SubBatchPipe
{
    double*     buf[2]  = {nullptr, nullptr};
    size_t      doubles = 0; // per half
    hipStream_t second  = nullptr;
    hipEvent_t  formed[2] = {nullptr, nullptr}, consumed[2] = {nullptr, nullptr};
    SubBatchPipe()                               = default;
    SubBatchPipe(const SubBatchPipe&)            = delete;
    SubBatchPipe& operator=(const SubBatchPipe&) = delete;
    ~SubBatchPipe()
    {
        for (int k = 0; k < 2; ++k)
        {
            if (buf[k])
                (void)hipFree(buf[k]);
            if (formed[k])
                (void)hipEventDestroy(formed[k]);
            if (consumed[k])
                (void)hipEventDestroy(consumed[k]);
        }
        if (second)
            (void)hipStreamDestroy(second);
    }
    // two halves of at least `need` doubles (both freed, then both allocated); the second stream and the events on first request
    int ensure(size_t need, bool two_streams)
    {
        if (doubles < need)
        {
            for (int k = 0; k < 2; ++k)
            {
                if (buf[k])
                    L3K_HIP(hipFree(buf[k]));
                buf[k] = nullptr;
            }
            doubles = 0;
            for (int k = 0; k < 2; ++k)
                L3K_HIP(hipMalloc(reinterpret_cast< void** >(&buf[k]), need * sizeof(double)));
            doubles = need;
        }
        if (two_streams && !second)
        {
            L3K_HIP(hipStreamCreateWithFlags(&second, hipStreamNonBlocking));
            for (int k = 0; k < 2; ++k)
            {
                L3K_HIP(hipEventCreateWithFlags(&formed[k], hipEventDisableTiming));
                L3K_HIP(hipEventCreateWithFlags(&consumed[k], hipEventDisableTiming));
            }
        }
        return 0;
    }
};
struct l3k_mf : KernelTerm
{
    static constexpr const char *kernel_noun = "kernel", *fields_setter = "l3k_mf_set_fields";
    std::vector< l3k_bnd* > boundary_terms; // attached boundary equation kernels (not owned)
    std::vector< double > tables_host;
    bool                dense = false, fuse = false;
    double*             energy_target = nullptr; // l3k_mf_apply_energy: where the element kernel adds x^T A x (device)
    int                 energy_done   = 0;       // ... how many element launches did (the launcher counts)
    int                 energy_expected = 0;     // ... of how many non-empty ones: equal = fused, else the caller takes a dot product
    double*             ws = nullptr; // LocalAssembly workspace (grown on demand)
    size_t              ws_doubles = 0;
    // Two pipelines, not one, because they nest: l3k_condense_global forms its sub-batches through l3k_local_assemble, whose stored
    // row-major route runs a whole pipeline on gasm (as l3k_assemble_global does) while the outer one is mid-flight on gcond
    SubBatchPipe gasm, gcond;
    // l3k_mf_assemble_boundary: the assembled and condensed entry points work on K_e + sum K_s, F_e + sum F_s over the attached sides
    bool         assemble_boundary = false;
    unsigned*    cond_nfail = nullptr; // the condensation's device counter of elements with a non-positive pivot
    ~l3k_mf()
    {
        if (ws)
            (void)hipFree(ws);
        if (cond_nfail)
            (void)hipFree(cond_nfail);
    }
};
// Sub-batches of at most nb of the elements [first, first + count) through the pipe: form(k, at, n) enqueues on `main` (the
// context's stream) what fills half k with the elements [at, at + n), consume(k, at, n) enqueues on p.second what reads it.  On
// return `main` is ordered after everything consumed.  A non-zero return of either callable or a failing HIP call ends the loop;
// the first error is the one returned, after both streams have drained: nothing queued can touch the halves or the caller's
// arrays once this has returned, whatever the outcome.
template < typename Form, typename Consume >
int runSubBatches(SubBatchPipe& p, hipStream_t main, int64_t first, int64_t count, int64_t nb, Form&& form, Consume&& consume)
{
    const auto step = [&](int i, int64_t at, int64_t n) -> int {
        const int k = i & 1;
        if (i >= 2)
            L3K_HIP(hipStreamWaitEvent(main, p.consumed[k], 0)); // the consumer of sub-batch i - 2 has read this half
        if (int rc = form(k, at, n))
            return rc;
        L3K_HIP(hipEventRecord(p.formed[k], main));
        L3K_HIP(hipStreamWaitEvent(p.second, p.formed[k], 0));
        if (int rc = consume(k, at, n))
            return rc;
        L3K_HIP(hipEventRecord(p.consumed[k], p.second));
        return 0;
    };
    const auto join = [&](int n_sub) -> int { // later work on the context's stream sees what the consumers wrote
        for (int k = 0; k < 2 && k < n_sub; ++k)
            L3K_HIP(hipStreamWaitEvent(main, p.consumed[k], 0));
        return 0;
    };
    int rc = 0, i = 0;
    for (int64_t done = 0; done < count && !rc; ++i)
    {
        const int64_t n = count - done < nb ? count - done : nb;
        rc              = step(i, first + done, n);
        done += n;
    }
    if (!rc)
        rc = join(i);
    if (rc)
    {
        (void)hipStreamSynchronize(p.second);
        (void)hipStreamSynchronize(main);
    }
    return rc;
}

// a square CSR matrix on the device (api_csr.hip): the caller's three arrays, validated once at creation, nothing copied
struct l3k_csr
{
    l3k_ctx*        ctx;
    int64_t         n;
    const int64_t*  row_ptr;
    const int32_t*  col_ind;
    const double*   values;
    int             lanes; // of a wave64 per row: 4, 16 or 64
    l3k_csr_info    info;
    DevBuf< unsigned long long > flag; // the word the checking kernels report through (validation, l3k_csr_dirichlet)
};

// api_halo.hip: the steps of an overlapped exchange, for the operators that live outside that file (api_csr_dist.hip: the
// schedule of l3k_mf_apply_dist around row launches).  All of them queue work and return; 0 or the error code with the message set
namespace l3k::halo
{
l3k_ctx* context(const l3k_halo* h);
int      dofsPerNode(const l3k_halo* h);
bool     hasNeighbours(const l3k_halo* h);
// the halo's own ghost buffers for `ncols` columns: xg (import target) and yg (export source), [ncols][ldg], ldg >= 1
int buffers(l3k_halo* h, int ncols, double** xg, double** yg, size_t* ldg);
// pack the owned rows the neighbours read and post the import into ghost [ncols][ldg] behind the work queued so far
int beginImport(l3k_halo* h, const double* d_owned, size_t ld, int ncols, double* d_ghost, size_t ldg);
// the context's stream waits for the posted import
int waitImport(l3k_halo* h);
// post the export of ghost [ncols][ldg] behind the work queued so far
int beginExport(l3k_halo* h, int ncols, const double* d_ghost, size_t ldg);
// the context's stream waits for the posted export, then the received rows are added into d_owned (neighbour list order)
int endExport(l3k_halo* h, double* d_owned, size_t ld, int ncols);
// the six events of the next timed apply (l3k_halo_timing_begin), or nullptr when none is left
hipEvent_t* timingSlot(l3k_halo* h);
// what the last export of ONE column brought from neighbour k < nNeighbours(h): the owned rows it added into (the neighbour's send
// list) and the values it added, n of each; valid behind endExport until the next export
int  nNeighbours(const l3k_halo* h);
// The block of l3k_halo_allreduce_sum_n for a solve that writes its sums into it.  reduceEnsure: a capacity of at least `capacity`
// (l3k_halo_reduce_reserve unless there is one).  reduceHold(+1 / -1): a solve is using the block, l3k_halo_reduce_reserve leaves it
// alone.  reduceRow: this rank's row of the block -- what a reducing kernel may write its finished sums into, no copy in front of
// the messages -- or nullptr in a world of one, where nothing is reduced.  allreduceRow: d_out[0 .. count) <- the sum over the
// ranks of the rows' first `count` values, in rank order, behind what the context's stream holds (nothing in a world of one)
int     reduceEnsure(l3k_halo* h, int capacity);
void    reduceHold(l3k_halo* h, int delta);
double* reduceRow(const l3k_halo* h);
int     allreduceRow(l3k_halo* h, double* d_out, int count);
void received(const l3k_halo* h, int k, const int32_t** d_rows, const double** d_vals, int64_t* n);
} // namespace l3k::halo
// api_csr_dist.hip: what the collective solves (api_solver.hip) need of a distributed CSR operator
namespace l3k::csr
{
l3k_halo* haloOf(const l3k_csr_dist* D);
l3k_ctx*  contextOf(const l3k_csr_dist* D);
int64_t   ownedRows(const l3k_csr_dist* D);
} // namespace l3k::csr

// a boundary equation kernel on a list of element sides (assembleProblem(kernel, boundary_ids) of the reference)
struct l3k_bnd : KernelTerm
{
    static constexpr const char *kernel_noun = "boundary kernel", *fields_setter = "l3k_bnd_set_fields";
    DevBuf< int64_t >     face_elem; // sides of interior elements first
    DevBuf< uint8_t >     face_side;
    int64_t               n_faces = 0, n_interior_faces = 0;
    // deterministic mode: the two classes of sides sorted by colour (sides of one colour share no node); det_ptr[cls][c] ..
    // det_ptr[cls][c + 1] = positions of colour c in face_elem / face_side
    std::vector< int64_t > det_ptr[2];
    // ---- assembly of the side systems (api_bnd_assemble.hip): two more orders of the list, built on first use
    struct SideList
    {
        DevBuf< int64_t >  elem;
        DevBuf< uint8_t >  side, rank; // rank: position of the side among the sides of its element (sorted list only)
        DevBuf< uint32_t > nodes;      // [n_faces][N]: the node rows of the sides' elements, what the scatter kernel indexes
        bool               built = false;
    };
    std::vector< int64_t > list_elem; // host: the list in the order l3k_bnd_create was given
    std::vector< uint8_t > list_side;
    SideList               in_order;  // ... in that order on the device
    SideList               by_elem;   // ... stably sorted by element
    std::vector< int64_t > by_elem_host; // host: the elements of by_elem
    std::vector< uint8_t > by_elem_rank; // host: the ranks of by_elem
    SubBatchPipe           gasm;         // the sub-batch pipeline of l3k_bnd_assemble_global
    DevBuf< double >       coef_ws;      // coefficient workspace of l3k_bnd_local_assemble and of the accumulating route
};

// the sum of several terms over one set of rows (api_mfs.hip): domain and boundary terms in the order they were added, on `rows` or
// on meshes over the same nodes; nothing is owned but the coverage mask
struct l3k_mfs
{
    struct Term
    {
        l3k_mf*  mf; // exactly one of the two
        l3k_bnd* bnd;
    };
    l3k_ctx*            ctx;
    l3k_mesh*           rows;
    int                 n_rhs;
    bool                finalized = false;
    std::vector< Term > terms;
    DevBuf< uint8_t >   active; // [n_local_dofs]: 1 where a term has an entry (l3k_mfs_finalize)
    DevBuf< unsigned long long > word; // what the checking and counting kernels report through
    int64_t             n_active_rows = 0;
};
// api.hip: l3k_mf_apply_elems with the fused store of the exclusive rows switched by the caller (`fuse`: l3k_mf::fuse for a system
// on its own; 0 inside a sum, where every row is accumulated and none written); the system itself is not modified
int mfApplyElems(l3k_mf* mf, int which, const double* d_x, size_t ldx, const double* d_xghost, size_t ldxg, double* d_y, size_t ldy,
                 double* d_yghost, size_t ldyg, int ncols, double alpha, double beta, int fuse);
// api.hip: y <- beta y on the first `rows` rows of `ncols` columns (beta == 1: nothing), and y += alpha x on the owned Dirichlet rows
// of a mesh, on the context's stream
int scaleRows(l3k_ctx* ctx, double* d_y, size_t ldy, int64_t rows, int ncols, double beta);
int dirichletRowsOf(l3k_ctx* ctx, const l3k_mesh* m, const double* d_x, size_t ldx, double* d_y, size_t ldy, int ncols, double alpha);
// ... and diag = 1, rhs = g (null: 0) there, the last step of a diag / rhs pass
int dirichletFinalizeOf(l3k_ctx* ctx, const l3k_mesh* m, const double* d_dirichlet_vals, size_t ldg, double* d_diag, double* d_rhs, size_t ldr,
                        int n_rhs);
// api.hip: the system's device instantiation for `ncols` columns, or nullptr with the error set (callers return -4)
const l3k::dev::Instance* instanceFor(const l3k_mf* mf, int ncols);
// ... of a boundary term (`what`: optional prefix of the message)
const l3k::dev::BoundaryInstance* boundaryInstanceFor(const l3k_bnd* b, int ncols, const char* what = nullptr);
// api.hip: the refusals of an apply that its operands alone decide (fields set, number of columns, leading dimensions, alignment
// of x, y and, where given, the ghost buffers): 0, or -1 with the error set.  The apply entry points call it before their first launch
int checkApplyOperands(const l3k_mf* mf, int ncols, const double* d_x, size_t ldx, const double* d_xghost, size_t ldxg, const double* d_y,
                       size_t ldy, const double* d_yghost, size_t ldyg);
// api_assembled.hip: `count` element matrices from the tiled layout of l3k_local_assemble_tiled to the row-major one, on stream s
int launchTiledToRowMajor(int U, int N1, int64_t count, const double* d_Kt, double* d_K, hipStream_t s);
// ... and the upper triangles overwritten by the mirrored lower ones (bitwise symmetric matrices, as the reference's)
int launchTiledXToRowMajorSym(int U, int N1, int64_t count, const double* d_Kt, double* d_K, hipStream_t s);
// api_assembled.hip: the batch scatter of element systems into CSR values on a given stream
int launchAssembledScatter(l3k_mf* mf, int64_t first, int64_t count, const double* d_K, const double* d_F, const int64_t* d_row_ptr,
                           const int32_t* d_col_ind, double* d_values, double* d_rhs, size_t ldr, int skip_dirichlet,
                           unsigned long long* d_count, hipStream_t s, int tiled);
// ... of systems whose node rows are d_nodes[first + e] (element systems: the mesh's elem_nodes; side systems: the node rows of the
// sides' elements) with the unknowns, right-hand sides and dofs of the caller's term
int launchAssembledScatterRows(const l3k_ctx* ctx, const l3k_mesh* m, const uint32_t* d_nodes, int n_unknowns, int n_rhs, const int* field_inds,
                               int64_t first, int64_t count, const double* d_K, const double* d_F, const int64_t* d_row_ptr,
                               const int32_t* d_col_ind, double* d_values, double* d_rhs, size_t ldr, int skip_dirichlet,
                               unsigned long long* d_count, hipStream_t s, int tiled);
// api.hip: the arguments of a LocalAssembly launch of the elements [first, first + count): all columns, output from slot 0
int assemblyArgs(l3k_mf* mf, int64_t first, int64_t count, l3k::dev::ElemArgs& a);
// ... mf->ws grown to the coefficient workspace of `count` elements; flag = its trailing double, which the assembly kernels set on a
// degenerate element, cleared on the context's stream
int assemblyWorkspace(l3k_mf* mf, const l3k::dev::Instance* inst, int64_t count, double*& flag);
// ... and the flag (or the two of a pipeline's halves) and the miss counter read back on s, which is synchronised: -2 if a flag is set
int readDegenerateFlags(hipStream_t s, const double* d_flag0, const double* d_flag1 = nullptr, const unsigned long long* d_count = nullptr,
                        int64_t* n_missing = nullptr);
// api_graph.hip: l3k_graph_create's builder on any table of node rows of the mesh (the argument checks of field_inds are its own)
struct l3k_graph;
int graphCreateOn(l3k_mesh* mesh, const uint32_t* d_elem_nodes, int N, int Ns, int condensed, int n_fields, const int* field_inds,
                  l3k_graph** out);
// api_bnd_assemble.hip: the term's list of sides on the device in the order it was given (l3k_bnd::in_order), built on first use
int sideListInOrder(l3k_bnd* b);
// api_bnd_assemble.hip: with l3k_mf_assemble_boundary on and terms attached, the refusals of `what` (0, or -1 with the error set) ...
int checkAssembleBoundary(const l3k_mf* mf, const char* what);
inline bool assemblesBoundary(const l3k_mf* mf)
{
    return mf->assemble_boundary && !mf->boundary_terms.empty();
}
// ... K_e += sum K_s, F_e += sum F_s over the attached sides of the elements [first, first + count) on the context's stream: d_K
// [count][Nd][Nd] row-major, d_F [count][n_rhs][Nd], either may be null
int accumulateBoundarySides(l3k_mf* mf, int64_t first, int64_t count, double* d_K, double* d_F);
// ... the side systems of every attached term on the elements [first, first + count) summed into the CSR values / rhs (the
// standalone route of l3k_bnd_assemble_global); entries outside the graph are added to *n_missing
int assembleGlobalBoundarySides(l3k_mf* mf, int64_t first, int64_t count, const int64_t* d_row_ptr, const int32_t* d_col_ind, double* d_values,
                                double* d_rhs, size_t ldr, int skip_dirichlet, size_t workspace_bytes, int64_t* n_missing);
#endif
