// graph.hpp -- the CSR sparsity graph of a mesh, built on the device (include/l3k.h: l3k_graph_*).  What the reference computes in
// algsys/SparsityGraph.hpp:26-81 (computeLocalGraph: over-allocated rows, filled with duplicates, then sorted and de-duplicated
// row by row) is done here at NODE level: the set of nodes b that share an element with the row node a is the same for every
// dof of a, so the dofs appear only in the final stores.
//
//   1. node -> element table: a count per (element, selected local node) with an integer atomicAdd, an exclusive scan, a fill
//      through one atomic cursor per node.  The order of a node's elements is whatever the atomics give; every row is sorted.
//      "Selected" = all N local nodes (L3K_GRAPH_FULL) or the primary ones (L3K_GRAPH_CONDENSED, primaryNodeOf of condense.hpp).
//   2. graphRowKernel< FILL, SCRATCH >: one workgroup per row node.  It gathers the selected node ids of the node's m elements
//      (m Ns keys of 32 bits), sorts them in place with a bitonic network over the next power of two (padding 0xFFFFFFFF, which
//      is no node: n < 2^31), marks the first key of every run of equal keys and compacts with a workgroup prefix sum.  FILL =
//      false stores the number of distinct keys, FILL = true the U rows of the node; both run the same code up to the stores.
//   3. The keys live in the LDS (SCRATCH = false, nodes with m Ns <= lds_key_capacity) or in the workgroup's slice of a global
//      buffer (SCRATCH = true, the GS pattern of sumfact_apply.hpp), which walks the list of the nodes that did not fit.
// Integer atomics and plain vector loads / stores only.  Nothing here grows with n_elems Ns^2 or with nnz.
#ifndef L3K_DEVICE_GRAPH_HPP
#define L3K_DEVICE_GRAPH_HPP

#include "common.hpp"
#include "condense.hpp"

namespace l3k::graph
{
constexpr int      graph_threads    = 256;
// 4096 keys = 16 KiB of LDS per workgroup: eight workgroups of four waves fill the 32 wave slots of a CU and take 128 of its
// 160 KiB, so the wave slots, not the LDS, bound the occupancy.  8 elements of order 6 (2744 keys) fit; DESIGN.md 4.14
constexpr int      lds_key_capacity = 4096;
constexpr uint32_t pad_key          = 0xFFFFFFFFu;

// slots of the statistics word block
enum
{
    stat_max_elems = 0, // largest number of elements at a node
    stat_n_scratch,     // nodes whose key list exceeds lds_key_capacity
    stat_max_keys,      // largest key list (m Ns)
    stat_max_deg,       // largest number of coupled nodes
    stat_n_coupled,     // nodes with at least one coupled node
    stat_words
};

struct GraphArgs
{
    const uint32_t* elem_nodes; // [n_elems][N]
    int64_t         n_elems, n_nodes;
    int             N, Ns, n1d, condensed; // nodes per element, selected ones, nodes per direction, kind
    int             U, dpn;
    const int*      field_inds; // [U] device
    int64_t*        elem_ptr;   // [n_nodes + 1] node -> first entry of elem_of
    uint32_t*       cnt;        // [n_nodes] elements per node (the fill's cursor on the way)
    uint32_t*       elem_of;    // [n_elems Ns]
    uint32_t*       deg;        // [n_nodes] coupled nodes per node
    int64_t*        node_off;   // [n_nodes + 1] first entry of the node's U rows in col_ind
    unsigned long long* stats;  // [stat_words]
    const uint32_t* scratch_nodes; // [n_scratch] the nodes of the SCRATCH route
    int64_t         n_scratch;
    uint32_t*       scratch;       // [grid][scratch_stride] key buffers of the SCRATCH route
    int64_t         scratch_stride;
    int64_t*        row_ptr; // the caller's arrays (fill only)
    int32_t*        col_ind;
};

// element-local index of the q-th selected node
__device__ __forceinline__ int selectedNode(int q, int n1d, int condensed)
{
    return condensed ? l3k::dev::primaryNodeOf(q, n1d) : q;
}

__device__ __forceinline__ unsigned long long waveMax(unsigned long long v)
{
    for (int o = 32; o > 0; o >>= 1)
    {
        const unsigned long long w = __shfl_xor(v, o);
        v                          = w > v ? w : v;
    }
    return v;
}
__device__ __forceinline__ unsigned long long waveSum(unsigned long long v)
{
    for (int o = 32; o > 0; o >>= 1)
        v += __shfl_xor(v, o);
    return v;
}

// 1a. cnt[node] += 1 for every (element, selected local node)
__global__ void __launch_bounds__(graph_threads) graphCountKernel(GraphArgs a)
{
    const int64_t total = a.n_elems * a.Ns;
    for (int64_t i = int64_t(blockIdx.x) * graph_threads + threadIdx.x; i < total; i += int64_t(gridDim.x) * graph_threads)
    {
        const int64_t e = i / a.Ns;
        const int     q = int(i - e * a.Ns);
        atomicAdd(&a.cnt[a.elem_nodes[e * a.N + selectedNode(q, a.n1d, a.condensed)]], 1u);
    }
}
// 1b. the counts widened for the scan (entry n_nodes: 0, the scan leaves the total there), their statistics, the cursors zeroed
__global__ void __launch_bounds__(graph_threads) graphNodeStatsKernel(GraphArgs a)
{
    unsigned long long mx = 0, ns = 0;
    for (int64_t i = int64_t(blockIdx.x) * graph_threads + threadIdx.x; i <= a.n_nodes; i += int64_t(gridDim.x) * graph_threads)
    {
        const uint32_t m = i < a.n_nodes ? a.cnt[i] : 0u;
        a.elem_ptr[i]    = m;
        if (i < a.n_nodes)
            a.cnt[i] = 0;
        mx = m > mx ? m : mx;
        ns += int64_t(m) * a.Ns > lds_key_capacity;
    }
    mx = waveMax(mx);
    ns = waveSum(ns);
    if ((threadIdx.x & 63) == 0)
    {
        atomicMax(&a.stats[stat_max_elems], mx);
        atomicMax(&a.stats[stat_max_keys], mx * a.Ns);
        if (ns)
            atomicAdd(&a.stats[stat_n_scratch], ns);
    }
}
// 1c. elem_of[elem_ptr[node] + cursor[node]++] = element
__global__ void __launch_bounds__(graph_threads) graphFillTableKernel(GraphArgs a)
{
    const int64_t total = a.n_elems * a.Ns;
    for (int64_t i = int64_t(blockIdx.x) * graph_threads + threadIdx.x; i < total; i += int64_t(gridDim.x) * graph_threads)
    {
        const int64_t  e    = i / a.Ns;
        const int      q    = int(i - e * a.Ns);
        const uint32_t node = a.elem_nodes[e * a.N + selectedNode(q, a.n1d, a.condensed)];
        const uint32_t pos  = atomicAdd(&a.cnt[node], 1u);
        a.elem_of[a.elem_ptr[node] + pos] = uint32_t(e);
    }
}
// the nodes of the SCRATCH route, in the order the atomics give (each is sorted on its own: the order does not matter)
__global__ void __launch_bounds__(graph_threads) graphScratchListKernel(GraphArgs a, uint32_t* list, unsigned long long* cursor)
{
    for (int64_t i = int64_t(blockIdx.x) * graph_threads + threadIdx.x; i < a.n_nodes; i += int64_t(gridDim.x) * graph_threads)
        if ((a.elem_ptr[i + 1] - a.elem_ptr[i]) * a.Ns > lds_key_capacity)
            list[atomicAdd(cursor, 1ull)] = uint32_t(i);
}

// 2. one workgroup per row node (workgroups stride over the nodes, or over the list of the SCRATCH route)
template < bool FILL, bool SCRATCH >
__global__ void __launch_bounds__(graph_threads) graphRowKernel(GraphArgs a)
{
    __shared__ uint32_t lds_keys[SCRATCH ? 1 : lds_key_capacity];
    __shared__ uint32_t wave_total[graph_threads / 64];
    uint32_t* const     keys = SCRATCH ? a.scratch + int64_t(blockIdx.x) * a.scratch_stride : lds_keys;
    const int           tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t       n_rows = SCRATCH ? a.n_scratch : a.n_nodes;
    for (int64_t r = blockIdx.x; r < n_rows; r += gridDim.x)
    {
        const int64_t node = SCRATCH ? int64_t(a.scratch_nodes[r]) : r;
        const int64_t eb   = a.elem_ptr[node];
        const int     nk   = int((a.elem_ptr[node + 1] - eb) * a.Ns); // keys of this node (uniform over the workgroup; < 2^30: the host checks)
        if (!SCRATCH && nk > lds_key_capacity)
            continue; // the SCRATCH launch serves it
        if (nk == 0)
        {
            if (!FILL && tid == 0)
                a.deg[node] = 0;
            continue;
        }
        int P = 1;
        while (P < nk)
            P <<= 1;
        for (int i = tid; i < P; i += graph_threads)
        {
            uint32_t key = pad_key;
            if (i < nk)
            {
                const int m = i / a.Ns;
                const int q = i - m * a.Ns;
                key = a.elem_nodes[int64_t(a.elem_of[eb + m]) * a.N + selectedNode(q, a.n1d, a.condensed)];
            }
            keys[i] = key;
        }
        __syncthreads();
        // bitonic network, ascending
        for (int k = 2; k <= P; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1)
            {
                for (int i = tid; i < P; i += graph_threads)
                {
                    const int l = i ^ j;
                    if (l > i)
                    {
                        const uint32_t x = keys[i], y = keys[l];
                        if (((i & k) == 0) == (x > y))
                        {
                            keys[i] = y;
                            keys[l] = x;
                        }
                    }
                }
                __syncthreads();
            }
        // heads of the runs of equal keys, compacted to the front in chunks of one key per thread.  A head moves to a position <=
        // its own, inside its chunk or an earlier one; the last key of a chunk (the left neighbour of the next chunk's first) is
        // rewritten only by itself, with its own value
        uint32_t n_distinct = 0;
        for (int base = 0; base < nk; base += graph_threads)
        {
            const int      i    = base + tid;
            const uint32_t key  = i < nk ? keys[i] : pad_key;
            const bool     head = i < nk && (i == 0 || keys[i - 1] != key);
            const unsigned long long mask = __ballot(head);
            if (lane == 0)
                wave_total[wave] = uint32_t(__popcll(mask));
            __syncthreads();
            uint32_t before = 0, chunk = 0;
            for (int w = 0; w < graph_threads / 64; ++w)
            {
                before += w < wave ? wave_total[w] : 0u;
                chunk += wave_total[w];
            }
            if constexpr (FILL)
                if (head)
                    keys[n_distinct + before + uint32_t(__popcll(mask & ((1ull << lane) - 1ull)))] = key;
            n_distinct += chunk;
            __syncthreads();
        }
        if constexpr (FILL)
        {
            // rows (node, field_inds[u]), u = 0 .. U-1, are adjacent in col_ind (the rows between them are empty) and equal: U
            // copies of the n_distinct U columns b dpn + field_inds[u'], b ascending, u' ascending within b
            const int64_t row_len = int64_t(n_distinct) * a.U, total = row_len * a.U, off = a.node_off[node];
            for (int64_t i = tid; i < total; i += graph_threads)
            {
                const int64_t t = i % row_len, b = t / a.U;
                a.col_ind[off + i] = int32_t(int64_t(keys[b]) * a.dpn + a.field_inds[t - b * a.U]);
            }
            __syncthreads(); // the next node's gather overwrites the keys
        }
        else if (tid == 0)
            a.deg[node] = n_distinct;
    }
}

// node_off[a] = deg[a] U^2 for the scan (entry n_nodes: 0) and the statistics of deg
__global__ void __launch_bounds__(graph_threads) graphDegStatsKernel(GraphArgs a)
{
    unsigned long long mx = 0, nc = 0;
    for (int64_t i = int64_t(blockIdx.x) * graph_threads + threadIdx.x; i <= a.n_nodes; i += int64_t(gridDim.x) * graph_threads)
    {
        const uint32_t d = i < a.n_nodes ? a.deg[i] : 0u;
        a.node_off[i]    = int64_t(d) * a.U * a.U;
        mx = d > mx ? d : mx;
        nc += d > 0;
    }
    mx = waveMax(mx);
    nc = waveSum(nc);
    if ((threadIdx.x & 63) == 0)
    {
        atomicMax(&a.stats[stat_max_deg], mx);
        if (nc)
            atomicAdd(&a.stats[stat_n_coupled], nc);
    }
}
// row_ptr of the dof rows: row (a, f) starts rank(f) deg[a] U entries into the node's segment, rank(f) = the number of
// field_inds below f (the rows outside field_inds are empty)
__global__ void __launch_bounds__(graph_threads) graphRowPtrKernel(GraphArgs a)
{
    const int64_t n = a.n_nodes * a.dpn;
    for (int64_t i = int64_t(blockIdx.x) * graph_threads + threadIdx.x; i <= n; i += int64_t(gridDim.x) * graph_threads)
    {
        const int64_t node = i / a.dpn;
        const int     f    = int(i - node * a.dpn);
        int           rank = 0;
        for (int u = 0; u < a.U; ++u)
            rank += a.field_inds[u] < f;
        a.row_ptr[i] = a.node_off[node] + (node < a.n_nodes ? int64_t(rank) * a.deg[node] * a.U : 0);
    }
}
} // namespace l3k::graph
#endif
