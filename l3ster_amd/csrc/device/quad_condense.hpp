// quad_condense.hpp -- static condensation of the element-internal dofs on quad meshes, as a mode of the assembled system
// (include/l3k.h: l3k_asm_create_condensed; the reference's StaticCondensationManager< ElementBoundary >,
// algsys/StaticCondensationManager.hpp:259-473).  STATEFUL, as the reference: the object keeps, per element, the internal rows
//     [ K_ii | K_ib | F_i ]        Nis = Ni Us rows of LD = Nis + Nbs + R doubles, Ni = (p-1)^2, Nbs = 4 p Us
// over the system's Us fields (dofs node-major q Us + s, primary and internal nodes each in ascending element-local index), and
// every local system of every term is SPLIT into it on the way to the CSR arrays:
//   1. quadSplitKernel:     one wave per (local system, row node), the lanes over the row's entries as in assembledScatterKernel
//                           (api_assembled.hip): a primary row sums its primary columns into the condensed graph and F_b into the
//                           rhs (the node rows and the search rule of csr_scatter.hpp, no Dirichlet skip), an internal row is added
//                           to the element's slot of the store.  K_bi is dropped: it is K_ib^T.
//   2. quadEliminateKernel: a TEAM of 16, 64 or 256 threads per element, 256 / team elements per workgroup (an order-2 block of 3
//                           unknowns is 3 x 3: one workgroup per element would idle 61 of 64 lanes).  The slot is copied to the
//                           LDS where teams x slot fits cond_lds_bytes, else it is worked on in place in global memory (same body).
//                           Right-looking Cholesky of the augmented rows on the upper triangle: row k scaled by 1 / sqrt(pivot),
//                           then the rank-1 update of the rows below it -- the K_ib and F_i columns ride along, which leaves
//                           [ L^T | W = L^-1 K_ib | h = L^-1 F_i ] in the slot.  Then schurProduct: W^T W and W^T h by FMAs over k
//                           ascending (fma(W[k][a], W[k][b], .) and its mirror image are the same operation: bitwise symmetric),
//                           subtracted from the CSR values and the rhs with the addressing of kernel 1 (csrFind of csr_scatter.hpp:
//                           the guess is the position next to the node's previous field).
//   3. quadRecoverKernel:   y = h - W x_b, back substitution with L^T column by column, plain stores: one writer per dof, a fixed
//                           summation order.
//   4. quadSchurOutKernel:  schurProduct of a factored store into the caller's arrays instead of the CSR.
// A pivot that is not a positive finite number (tested on the bits, condense.hpp) stops its element: no update, counted.
// Runtime sizes and dynamic LDS: one instance per kernel for every order and number of fields.
#ifndef L3K_DEVICE_QUAD_CONDENSE_HPP
#define L3K_DEVICE_QUAD_CONDENSE_HPP

#include "common.hpp"
#include "condense.hpp"
#include "csr_scatter.hpp"
#include "launch.hpp"

namespace l3k::dev
{
// LDS a workgroup of the elimination kernel may take for its elements' slots; shapes above it (one slot: order 6 with 4 fields,
// order 7 with 3, order 8 with 2 and more) are eliminated in place in global memory
constexpr size_t cond_lds_bytes = 128 * 1024;
constexpr int    cond_threads   = 256;

// q-th primary node of a quad with n = p + 1 nodes per direction, ascending: the row y = 0, the two ends of the rows 0 < y < p,
// the row y = p; and the inverse
__host__ __device__ constexpr int quadPrimaryNodeOf(int q, int n)
{
    const int p = n - 1;
    if (q < n)
        return q;
    q -= n;
    if (q < 2 * (p - 1))
        return ((q % 2) ? p : 0) + n * (1 + q / 2);
    return n * p + (q - 2 * (p - 1));
}
__host__ __device__ constexpr bool quadIsPrimary(int b, int n)
{
    const int ix = b % n, iy = b / n;
    return ix == 0 || ix == n - 1 || iy == 0 || iy == n - 1;
}
// position of local node b in its list: among the primary nodes, or among the internal ones ((ix-1) + (p-1)(iy-1))
__host__ __device__ constexpr int quadSplitIndex(int b, int n)
{
    const int p = n - 1, ix = b % n, iy = b / n;
    if (iy == 0)
        return ix;
    if (iy == p)
        return n + 2 * (p - 1) + ix;
    if (ix == 0 || ix == p)
        return n + 2 * (iy - 1) + (ix == p);
    return (ix - 1) + (p - 1) * (iy - 1);
}

// the primary node rows [n_elems][4 p] of a quad mesh: what the graph builder of graph.hpp takes as the elements of the condensed graph
__global__ void __launch_bounds__(256) quadPrimaryNodesKernel(const uint32_t* __restrict__ elem_nodes, int64_t n_elems, int n1d,
                                                              uint32_t* __restrict__ out)
{
    const int     Np    = 4 * (n1d - 1);
    const int64_t total = n_elems * Np;
    for (int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x; i < total; i += int64_t(gridDim.x) * 256)
    {
        const int64_t e = i / Np;
        out[i]          = elem_nodes[e * n1d * n1d + quadPrimaryNodeOf(int(i - e * Np), n1d)];
    }
}

struct QuadSplitArgs : CsrSink // (the condensed system: row_ptr, col_ind, values, rhs, ldr, n_missing)
{
    const uint32_t* nodes;     // [.][NN] node rows of the local systems (element systems: the mesh's; side systems: the sides' elements')
    const int64_t*  elem_of;   // [.] element of local system i, or nullptr: i itself
    const double *  K, *F;     // the sub-batch: [count][Nd][Nd] row-major, [count][R][Nd]
    double*         store;
    int64_t         first, count;
    int             n1d, dpn, n_rhs, Us, Nis, LD;
    int             field_inds[max_unknowns]; // of the term's unknowns
    int             slot[max_unknowns];       // ... and their positions among the system's fields
};

template < bool ATOMIC >
__device__ __forceinline__ void storeAdd(double* p, double v)
{
    if constexpr (ATOMIC)
        unsafeAtomicAdd(p, v);
    else
        *p += v;
}

// ATOMIC = false: no two local systems of the launch belong to one element (a domain term); true: sides
template < int U, bool ATOMIC >
__global__ __launch_bounds__(64) void quadSplitKernel(const QuadSplitArgs a)
{
    const int       n = a.n1d, NN = n * n, Nd = NN * U;
    const int64_t   e    = blockIdx.x / NN; // local system of the batch
    const int       b    = int(blockIdx.x - e * NN);
    const uint32_t* en   = a.nodes + (a.first + e) * NN;
    const int       lane = threadIdx.x;
    const double*   Kb   = a.K ? a.K + (e * Nd + int64_t(b) * U) * Nd : nullptr; // rows (b, 0 .. U-1)
    if (!quadIsPrimary(b, n))
    {
        const int64_t elem = a.elem_of ? a.elem_of[a.first + e] : a.first + e;
        double* const rows = a.store + (elem * a.Nis + int64_t(quadSplitIndex(b, n)) * a.Us) * a.LD; // + slot[u] * LD
        if (a.F)
            for (int t = lane; t < a.n_rhs * U; t += 64)
            {
                const int r = t / U, u = t - r * U;
                storeAdd< ATOMIC >(rows + int64_t(a.slot[u]) * a.LD + (a.LD - a.n_rhs) + r, a.F[(e * a.n_rhs + r) * Nd + b * U + u]);
            }
        if (!Kb)
            return;
        for (int j = lane; j < Nd; j += 64)
        {
            const int bp = j / U, q = quadSplitIndex(bp, n);
            const int col = (quadIsPrimary(bp, n) ? a.Nis : 0) + q * a.Us + a.slot[j - bp * U];
#pragma unroll
            for (int u = 0; u < U; ++u)
                storeAdd< ATOMIC >(rows + int64_t(a.slot[u]) * a.LD + col, Kb[int64_t(u) * Nd + j]);
        }
        return;
    }
    NodeRows< U > rows(int64_t(en[b]) * a.dpn, a.field_inds, nullptr, 0); // (no Dirichlet skip: every row is live)
    if (a.F)
        rows.addRhs(a, lane, a.n_rhs, a.F + e * a.n_rhs * Nd + b * U, Nd);
    if (!Kb)
        return;
    rows.loadRanges(a.row_ptr);
    unsigned missing = 0;
    for (int j = lane; j < Nd; j += 64)
    {
        const int bp = j / U;
        if (!quadIsPrimary(bp, n))
            continue;
        const int64_t col = int64_t(en[bp]) * a.dpn + a.field_inds[j - bp * U];
        missing += rows.addEntry(a, col, [&](int u) { return Kb[int64_t(u) * Nd + j]; });
    }
    csrCountMissing(a, missing);
}

struct QuadCondArgs : CsrSink // (elimination: the condensed system -- row_ptr, col_ind, values, rhs, ldr, n_missing)
{
    double*         store;      // [n_elems][Nis][LD]
    const uint32_t* elem_nodes; // [n_elems][n1d^2]
    const int*      fields;     // [Us] the system's field_inds (device)
    int64_t         first, count; // the elements of the launch
    int             n1d, dpn, n_rhs, Us, Nis, Nbs, LD, team;
    unsigned*       n_failed;   // elimination: elements whose pivot test failed
    // updates out: [count][Nbs][Nbs], [count][R][Nbs], either may be null
    double *outW, *outw;
    // recovery
    double* x;
    size_t  ldx;
};

// local dof row of the a-th primary (internal) dof of an element
__device__ __forceinline__ int64_t condDof(const QuadCondArgs& a, const uint32_t* en, int i, bool primary)
{
    const int q = i / a.Us, m = a.n1d - 2, b = primary ? quadPrimaryNodeOf(q, a.n1d) : (1 + q % m) + a.n1d * (1 + q / m);
    return int64_t(en[b]) * a.dpn + a.fields[i - q * a.Us];
}

// W^T W and W^T h of a factored slot M by the team's threads t of T: scattered (negated) into the CSR arrays, or written to
// out (OUT) for the element at position `at` of the launch
template < bool OUT >
__device__ __forceinline__ void schurProduct(const QuadCondArgs& a, const double* M, const uint32_t* en, int64_t at, int t, int T)
{
    const int     Np = a.Nbs / a.Us, LD = a.LD;
    const double* W  = M + a.Nis;
    unsigned      missing = 0;
    if (OUT ? a.outW != nullptr : a.values != nullptr)
        for (int i = t; i < a.Nbs * Np; i += T) // (row dof ar, column node bq), bq fastest
        {
            const int ar = i / Np, bq = i - ar * Np;
            int64_t   rb = 0, re = 0, pos = 0, col0 = 0;
            if constexpr (!OUT)
            {
                const int64_t row = condDof(a, en, ar, true);
                rb                = a.row_ptr[row];
                re                = a.row_ptr[row + 1];
                col0              = int64_t(en[quadPrimaryNodeOf(bq, a.n1d)]) * a.dpn;
                pos               = csrLowerBound(a.col_ind, rb, re, col0 + a.fields[0]);
            }
            for (int s = 0; s < a.Us; ++s)
            {
                const int br  = bq * a.Us + s;
                double    acc = 0.;
                for (int k = 0; k < a.Nis; ++k)
                    acc = fma(W[k * LD + ar], W[k * LD + br], acc);
                if constexpr (OUT)
                    a.outW[(at * a.Nbs + ar) * a.Nbs + br] = acc;
                else
                {
                    // (the columns of one node are adjacent in a row of the graph, fields ascending: the guess of csrFind)
                    const int64_t ps = csrFind(a.col_ind, rb, re, pos + s, col0 + a.fields[s]);
                    if (ps >= 0)
                        unsafeAtomicAdd(a.values + ps, -acc);
                    else
                        ++missing;
                }
            }
        }
    if (OUT ? a.outw != nullptr : a.rhs != nullptr)
        for (int i = t; i < a.Nbs * a.n_rhs; i += T)
        {
            const int r = i / a.Nbs, ar = i - r * a.Nbs;
            double    acc = 0.;
            for (int k = 0; k < a.Nis; ++k)
                acc = fma(W[k * LD + ar], M[k * LD + a.Nis + a.Nbs + r], acc);
            if constexpr (OUT)
                a.outw[(at * a.n_rhs + r) * a.Nbs + ar] = acc;
            else
                unsafeAtomicAdd(a.rhs + size_t(r) * a.ldr + condDof(a, en, ar, true), -acc);
        }
    csrCountMissing(a, missing);
}

// Every loop bound below depends on the shape alone, so the teams of a workgroup (and the idle team of a last workgroup) meet at
// every barrier.  LDS: the slots of the workgroup's teams live in dynamic LDS for the duration
template < bool LDS >
__global__ __launch_bounds__(cond_threads) void quadEliminateKernel(const QuadCondArgs a)
{
    extern __shared__ double cond_lds[];
    const int     T = a.team, team = threadIdx.x / T, t = threadIdx.x - team * T;
    const int64_t at   = int64_t(blockIdx.x) * (cond_threads / T) + team;
    const bool    live = at < a.count;
    const int64_t elem = a.first + (live ? at : 0);
    const int     Nis = a.Nis, LD = a.LD, slot = Nis * LD;
    double* const G = a.store + elem * slot;
    double* const M = LDS ? cond_lds + team * slot : G;
    if (LDS && live)
        for (int i = t; i < slot; i += T)
            M[i] = G[i];
    const int cw = T < 64 ? T : 64, rw = T / cw, tc = t % cw, tr = t / cw; // lanes along a row, row groups
    bool      ok = live;
    for (int k = 0; k < Nis; ++k)
    {
        __syncthreads(); // the update of step k - 1 (or the copy) is complete
        const double d = M[k * LD + k];
        ok             = ok && positiveFinite(d);
        const double l = sqrt(d);
        if (ok)
            for (int j = k + 1 + t; j < LD; j += T)
                M[k * LD + j] /= l;
        __syncthreads();
        if (ok)
        {
            if (t == 0)
                M[k * LD + k] = l;
            for (int i = k + 1 + tr; i < Nis; i += rw)
            {
                const double f = M[k * LD + i];
                for (int j = i + tc; j < LD; j += cw)
                    M[i * LD + j] = fma(-f, M[k * LD + j], M[i * LD + j]);
            }
        }
    }
    __syncthreads();
    if (!ok)
    {
        if (live && t == 0)
            atomicAdd(a.n_failed, 1u);
        return; // (no barrier below)
    }
    schurProduct< false >(a, M, a.elem_nodes + elem * a.n1d * a.n1d, at, t, T);
    if (LDS)
        for (int i = t; i < slot; i += T)
            G[i] = M[i];
}

__global__ __launch_bounds__(cond_threads) void quadSchurOutKernel(const QuadCondArgs a)
{
    const int     T = a.team, team = threadIdx.x / T, t = threadIdx.x - team * T;
    const int64_t at = int64_t(blockIdx.x) * (cond_threads / T) + team;
    if (at >= a.count)
        return;
    const int64_t elem = a.first + at;
    schurProduct< true >(a, a.store + elem * a.Nis * a.LD, a.elem_nodes + elem * a.n1d * a.n1d, at, t, T);
}

// dynamic LDS: per team x_b [Nbs], y [Nis], x_i [Nis]
__global__ __launch_bounds__(cond_threads) void quadRecoverKernel(const QuadCondArgs a)
{
    extern __shared__ double cond_lds[];
    const int     T = a.team, team = threadIdx.x / T, t = threadIdx.x - team * T;
    const int64_t at   = int64_t(blockIdx.x) * (cond_threads / T) + team;
    const bool    live = at < a.count;
    const int64_t elem = a.first + (live ? at : 0);
    const int     Nis = a.Nis, Nbs = a.Nbs, LD = a.LD;
    const double*   M  = a.store + elem * Nis * LD;
    const uint32_t* en = a.elem_nodes + elem * a.n1d * a.n1d;
    double* const   xb = cond_lds + team * (Nbs + 2 * Nis);
    double* const   y  = xb + Nbs;
    double* const   xi = y + Nis;
    for (int r = 0; r < a.n_rhs; ++r)
    {
        double* const xr = a.x + size_t(r) * a.ldx;
        if (live)
            for (int i = t; i < Nbs; i += T)
                xb[i] = xr[condDof(a, en, i, true)];
        __syncthreads();
        if (live)
            for (int k = t; k < Nis; k += T)
            {
                double acc = M[k * LD + Nis + Nbs + r];
                for (int i = 0; i < Nbs; ++i)
                    acc = fma(-M[k * LD + Nis + i], xb[i], acc);
                y[k] = acc;
            }
        __syncthreads();
        for (int k = Nis - 1; k >= 0; --k) // L^T x_i = y, column by column from the last
        {
            if (live)
            {
                const double xk = y[k] / M[k * LD + k];
                for (int j = t; j < k; j += T)
                    y[j] = fma(-M[j * LD + k], xk, y[j]);
                if (t == 0)
                    xi[k] = xk;
            }
            __syncthreads();
        }
        if (live)
            for (int k = t; k < Nis; k += T)
                xr[condDof(a, en, k, false)] = xi[k];
        __syncthreads();
    }
}
} // namespace l3k::dev
#endif
