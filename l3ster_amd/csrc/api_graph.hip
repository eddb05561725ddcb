// api_graph.hip -- the device builder of the CSR sparsity graph of libl3k.so (include/l3k.h: l3k_graph_*): what produces the
// d_row_ptr / d_col_ind that l3k_assembled_scatter, l3k_assemble_global, l3k_condense_global and l3k_csr_create take.  The kernels
// and the algorithm are in device/graph.hpp.
#include "objects.hpp"

#include "device/graph.hpp"

#include <rocprim/rocprim.hpp>

using namespace l3k::graph;

struct l3k_graph
{
    l3k_ctx*                     ctx;
    GraphArgs                    args{};
    l3k_graph_info               info{};
    DevBuf< int >                field_inds;
    DevBuf< int64_t >            elem_ptr, node_off;
    DevBuf< uint32_t >           cnt, elem_of, deg, scratch_nodes, scratch;
    DevBuf< unsigned long long > stats;
    DevBuf< char >               scan_tmp;
    unsigned                     scratch_grid = 0;
};

namespace
{
// in-place exclusive sum of the int64 array d [count]; the temporary storage is the object's (grown on demand)
int scanInPlace(l3k_graph* g, int64_t* d, size_t count)
{
    size_t bytes = 0;
    L3K_HIP(rocprim::exclusive_scan(nullptr, bytes, d, d, int64_t(0), count, rocprim::plus< int64_t >(), g->ctx->stream));
    if (!g->scan_tmp.ptr || bytes > g->scan_tmp.n)
    {
        g->scan_tmp = DevBuf< char >();
        if (int rc = g->scan_tmp.alloc(bytes ? bytes : 1))
            return rc;
    }
    L3K_HIP(rocprim::exclusive_scan(g->scan_tmp.ptr, bytes, d, d, int64_t(0), count, rocprim::plus< int64_t >(), g->ctx->stream));
    return 0;
}
// the row kernel over the nodes whose keys fit the LDS, or (scratch) over the list of the others
template < bool FILL >
void launchRows(const l3k_graph* g, const GraphArgs& a, bool scratch)
{
    if (scratch)
        hipLaunchKernelGGL((graphRowKernel< FILL, true >), dim3(g->scratch_grid), dim3(graph_threads), 0, g->ctx->stream, a);
    else
        hipLaunchKernelGGL((graphRowKernel< FILL, false >), dim3(stridedGrid(g->ctx, a.n_nodes)), dim3(graph_threads), 0, g->ctx->stream, a);
}
// deg -> node_off (scanned) and the statistics of deg; then the block of statistics on the host (synchronises)
int degreesToOffsets(l3k_graph* g, unsigned long long (&h)[stat_words], int64_t& nnz)
{
    GraphArgs&  a  = g->args;
    hipStream_t st = g->ctx->stream;
    L3K_HIP(hipMemsetAsync(a.stats + stat_max_deg, 0, 2 * sizeof *a.stats, st)); // stat_max_deg, stat_n_coupled
    hipLaunchKernelGGL(graphDegStatsKernel, dim3(gridFor(a.n_nodes + 1, graph_threads)), dim3(graph_threads), 0, st, a);
    L3K_HIP(hipGetLastError());
    if (int rc = scanInPlace(g, a.node_off, size_t(a.n_nodes + 1)))
        return rc;
    L3K_HIP(hipMemcpyAsync(h, a.stats, sizeof h, hipMemcpyDeviceToHost, st));
    L3K_HIP(hipMemcpyAsync(&nnz, a.node_off + a.n_nodes, sizeof nnz, hipMemcpyDeviceToHost, st));
    L3K_HIP(hipStreamSynchronize(st));
    return 0;
}
} // namespace

// The graph of the node rows d_elem_nodes [n_elems][N] of `mesh`, of which the Ns selected ones couple (all of them, or with
// `condensed` the primary nodes of a hex): l3k_graph_create on the mesh's own rows, and the condensed graph of a quad mesh on the
// rows of its primary nodes (api_asm.hip), which must outlive the fill
int graphCreateOn(l3k_mesh* mesh, const uint32_t* d_elem_nodes, int N, int Ns, int condensed, int n_fields, const int* field_inds,
                  l3k_graph** out)
{
    const int dpn = mesh->dofs_per_node;
    if (n_fields < 0 || n_fields > dpn || (n_fields > 0 && !field_inds) || (n_fields == 0 && field_inds))
    {
        setError("l3k_graph_create: n_fields = %d with %s field_inds; it is 1 .. dofs_per_node = %d indices, or 0 and NULL for all dofs",
                 n_fields, field_inds ? "non-null" : "null", dpn);
        return -1;
    }
    const int          U = n_fields ? n_fields : dpn;
    std::vector< int > fi(static_cast< size_t >(U));
    for (int u = 0; u < U; ++u)
    {
        fi[u] = field_inds ? field_inds[u] : u;
        if (fi[u] < 0 || fi[u] >= dpn || (u > 0 && fi[u] <= fi[u - 1]))
        {
            setError("l3k_graph_create: field_inds[%d] = %d; the indices are strictly ascending and inside [0, dofs_per_node = %d)", u,
                     fi[u], dpn);
            return -1;
        }
    }
    const int64_t n_nodes = mesh->n_owned_nodes + mesh->n_ghost_nodes, n = n_nodes * dpn;
    if (n > INT32_MAX)
    {
        setError("l3k_graph_create: n = %lld does not fit the 32-bit column indices", static_cast< long long >(n));
        return -1;
    }
    const int n1d = mesh->order + 1;
    if (mesh->n_elems > int64_t(UINT32_MAX))
    {
        setError("l3k_graph_create: %lld elements do not fit the 32-bit node -> element table", static_cast< long long >(mesh->n_elems));
        return -1;
    }
    l3k_ctx*    ctx = mesh->ctx;
    hipStream_t st  = ctx->stream;
    auto        g   = std::make_unique< l3k_graph >();
    g->ctx          = ctx;
    if (int rc = g->field_inds.upload(fi.data(), fi.size(), st))
        return rc;
    if (int rc = g->elem_ptr.alloc(size_t(n_nodes + 1)))
        return rc;
    if (int rc = g->node_off.alloc(size_t(n_nodes + 1)))
        return rc;
    if (int rc = g->cnt.alloc(size_t(n_nodes)))
        return rc;
    if (int rc = g->deg.alloc(size_t(n_nodes)))
        return rc;
    if (int rc = g->elem_of.alloc(size_t(mesh->n_elems) * Ns))
        return rc;
    if (int rc = g->stats.alloc(stat_words + 1)) // + the cursor of the scratch list
        return rc;
    GraphArgs& a = g->args;
    a.elem_nodes = d_elem_nodes;
    a.n_elems    = mesh->n_elems;
    a.n_nodes    = n_nodes;
    a.N          = N;
    a.Ns         = Ns;
    a.n1d        = n1d;
    a.condensed  = condensed;
    a.U          = U;
    a.dpn        = dpn;
    a.field_inds = g->field_inds.ptr;
    a.elem_ptr   = g->elem_ptr.ptr;
    a.cnt        = g->cnt.ptr;
    a.elem_of    = g->elem_of.ptr;
    a.deg        = g->deg.ptr;
    a.node_off   = g->node_off.ptr;
    a.stats      = g->stats.ptr;

    // 1. node -> element table
    const int64_t n_keys = mesh->n_elems * Ns;
    L3K_HIP(hipMemsetAsync(a.stats, 0, (stat_words + 1) * sizeof *a.stats, st));
    if (n_nodes > 0)
    {
        L3K_HIP(hipMemsetAsync(a.cnt, 0, size_t(n_nodes) * sizeof *a.cnt, st));
        L3K_HIP(hipMemsetAsync(a.deg, 0, size_t(n_nodes) * sizeof *a.deg, st));
    }
    if (n_keys > 0)
        hipLaunchKernelGGL(graphCountKernel, dim3(gridFor(n_keys, graph_threads)), dim3(graph_threads), 0, st, a);
    hipLaunchKernelGGL(graphNodeStatsKernel, dim3(gridFor(n_nodes + 1, graph_threads)), dim3(graph_threads), 0, st, a);
    L3K_HIP(hipGetLastError());
    if (int rc = scanInPlace(g.get(), a.elem_ptr, size_t(n_nodes + 1)))
        return rc;
    if (n_keys > 0)
        hipLaunchKernelGGL(graphFillTableKernel, dim3(gridFor(n_keys, graph_threads)), dim3(graph_threads), 0, st, a);
    // 2. the degrees of the nodes whose keys fit the LDS, the offsets and the one readback
    if (n_nodes > 0)
        launchRows< false >(g.get(), a, false);
    L3K_HIP(hipGetLastError());
    unsigned long long h[stat_words];
    int64_t            nnz = 0;
    if (int rc = degreesToOffsets(g.get(), h, nnz))
        return rc;
    if (h[stat_n_scratch] > 0)
    {
        // 3. some key lists exceed the LDS: the list of those nodes, one slice of global scratch per workgroup, their degrees, and
        // the offsets and the readback once more
        if (h[stat_max_keys] > (1ull << 30))
        {
            setError("l3k_graph_create: a node of %llu elements has %llu keys; at most 2^30 are sorted",
                     static_cast< unsigned long long >(h[stat_max_elems]), static_cast< unsigned long long >(h[stat_max_keys]));
            return -1;
        }
        int64_t stride = 1;
        while (stride < int64_t(h[stat_max_keys]))
            stride <<= 1;
        a.n_scratch      = int64_t(h[stat_n_scratch]);
        a.scratch_stride = stride;
        g->scratch_grid  = stridedGrid(ctx, a.n_scratch);
        if (int rc = g->scratch_nodes.alloc(size_t(a.n_scratch)))
            return rc;
        if (int rc = g->scratch.alloc(size_t(stride) * g->scratch_grid))
            return rc;
        a.scratch_nodes = g->scratch_nodes.ptr;
        a.scratch       = g->scratch.ptr;
        hipLaunchKernelGGL(graphScratchListKernel, dim3(gridFor(n_nodes, graph_threads)), dim3(graph_threads), 0, st, a,
                           g->scratch_nodes.ptr, a.stats + stat_words);
        launchRows< false >(g.get(), a, true);
        L3K_HIP(hipGetLastError());
        if (int rc = degreesToOffsets(g.get(), h, nnz))
            return rc;
    }
    const int64_t n_coupled = int64_t(h[stat_n_coupled]);
    g->info                 = {n,
                               nnz,
                               n - n_coupled * U,
                               int64_t(h[stat_max_deg]) * U,
                               int64_t(h[stat_n_scratch]),
                               int64_t(g->field_inds.n * sizeof(int) + (g->elem_ptr.n + g->node_off.n) * sizeof(int64_t) +
                          (g->cnt.n + g->elem_of.n + g->deg.n + g->scratch_nodes.n + g->scratch.n) * sizeof(uint32_t) +
                          g->stats.n * sizeof(unsigned long long) + g->scan_tmp.n),
                               int(h[stat_max_elems]),
                               lds_key_capacity};
    *out = g.release();
    return 0;
}

extern "C" {

int l3k_graph_create(l3k_mesh* mesh, int n_fields, const int* field_inds, int kind, l3k_graph** out)
{
    if (!mesh || !out)
    {
        setError("l3k_graph_create: null argument");
        return -1;
    }
    if (kind != L3K_GRAPH_FULL && kind != L3K_GRAPH_CONDENSED)
    {
        setError("l3k_graph_create: kind = %d; it is L3K_GRAPH_FULL (0) or L3K_GRAPH_CONDENSED (1)", kind);
        return -1;
    }
    if (kind == L3K_GRAPH_CONDENSED)
        if (int rc = refuseQuads(mesh, "l3k_graph_create(L3K_GRAPH_CONDENSED)"))
            return rc;
    const int n1d = mesh->order + 1, N = mesh->dim == 2 ? n1d * n1d : n1d * n1d * n1d;
    const int inner = mesh->order - 1, Ns = kind == L3K_GRAPH_CONDENSED ? N - inner * inner * inner : N;
    return graphCreateOn(mesh, mesh->elem_nodes.ptr, N, Ns, kind == L3K_GRAPH_CONDENSED, n_fields, field_inds, out);
}
int l3k_graph_info_get(const l3k_graph* g, l3k_graph_info* out)
{
    if (!g || !out)
    {
        setError("l3k_graph_info_get: null argument");
        return -1;
    }
    *out = g->info;
    return 0;
}
int l3k_graph_fill(l3k_graph* g, int64_t* d_row_ptr, int32_t* d_col_ind)
{
    if (!g || !d_row_ptr)
    {
        setError("l3k_graph_fill: null argument");
        return -1;
    }
    if (g->info.nnz > 0 && !d_col_ind)
    {
        setError("l3k_graph_fill: null col_ind for a graph of %lld entries", static_cast< long long >(g->info.nnz));
        return -1;
    }
    GraphArgs a = g->args;
    a.row_ptr   = d_row_ptr;
    a.col_ind   = d_col_ind;
    hipLaunchKernelGGL(graphRowPtrKernel, dim3(gridFor(g->info.n + 1, graph_threads)), dim3(graph_threads), 0, g->ctx->stream, a);
    if (g->info.nnz > 0)
    {
        launchRows< true >(g, a, false);
        if (a.n_scratch > 0)
            launchRows< true >(g, a, true);
    }
    L3K_HIP(hipGetLastError());
    return 0;
}
int l3k_graph_destroy(l3k_graph* g)
{
    delete g;
    return 0;
}
} // extern "C"
