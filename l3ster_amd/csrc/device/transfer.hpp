// transfer.hpp -- the inter-order transfer of the p-multigrid levels: prolongation x_f <- P x_c and restriction r_c <- P^T r_f between
// two node sets of the SAME elements (orders p_f > p_c), as sum-factorised sweeps with the 1-D table of l3k_interp_1d.
//
// One element per workgroup of 256 threads (4 waves), workgroups walk the elements with a grid stride.  A node's dofs_per_node
// components move together, in groups of `group` components where the LDS would not hold them all.  Two LDS buffers alternate
// between the sweeps.  The x rows are stored with an ODD stride (n | 1): in the x sweep the lanes of a wave run over the rows, so
// their reads and writes are a row stride apart and an odd stride in doubles spreads them over all banks; in the y and z sweeps
// the lanes run along x and the accesses are contiguous.  The weights are read from LDS: in the x sweep a wave's lanes share the
// output index, so W is one address per wave (a broadcast); in the y and z sweeps a wave spans several output indices (the y sweep
// has B = n | 1 <= 9 lanes per index) and reads as many W addresses.  Not tuned further: the transfers are O(n^4) per element.
// Where n is even the padding slot at the end of each x row (index n of stride n | 1) is never read or written: the x sweep fills
// ix < n only and the y and z sweeps skip the slot.
//
// P is made well defined by the OWNERSHIP of the fine nodes: owner[node] = the lowest fine element that contains the node.  An
// element writes (prolongation) or reads (restriction) only the fine nodes it owns, so P has one row per fine dof -- the values of
// the coarse basis of the owning element at the node -- and the restriction is its exact transpose, without multiplicity weights.
//
// Partitioned meshes (the GHOST instantiations, behind l3k_transfer_*): a vector of a level is two buffers, owned rows and ghost
// rows, and `local dof < n_owned_dofs` selects the buffer as in the element kernels.  Only OWNED fine nodes take part in the
// ownership table (ghost fine nodes keep the fill value, which no element index equals, so no element handles them): the owned
// fine nodes of all ranks are the global fine nodes once each, hence the rows of the ranks' P are the rows of the global P.  The
// fine side therefore never addresses a ghost row; the coarse side reads (prolongation) or accumulates into (restriction) owned
// and ghost rows, and the caller's exchange -- import before, export-add after -- completes the global product.
#ifndef L3K_DEVICE_TRANSFER_HPP
#define L3K_DEVICE_TRANSFER_HPP

#include "common.hpp"

#include <type_traits>

namespace l3k::dev
{
constexpr int transfer_threads = 256;

struct TransferArgs
{
    int             dim, nf, nc, U, group; // nodes per direction of the two orders; dofs per node; components per pass
    int64_t         elem_begin, elem_count;
    const int64_t*  elem_list;  // positions [elem_begin, elem_begin + elem_count) name the fine elements; nullptr: themselves
    const int64_t*  elem_map;   // coarse element of a fine one; nullptr: the same index
    const uint32_t* nodes_f;    // [n_elems][nf^dim]
    const uint32_t* nodes_c;    // [n_elems][nc^dim]
    const uint8_t*  dirichlet_f; // byte masks over the dofs, or nullptr
    const uint8_t*  dirichlet_c;
    const int32_t*  owner;      // [fine nodes]
    const double*   table;      // weights W[j * n_out + i] from input index j to output index i of a sweep
    const double*   frozen;     // prolongation: fine rows with frozen[row] == 0 are left alone (the smoother's minv), or nullptr
    const double*   src;
    double*         dst;
    int             add;        // prolongation: dst += P src instead of dst = P src
};
// ... of the GHOST instantiations (a struct of its own: the single-rank kernels keep their kernel arguments and with them their
// code): the coarse vector's ghost rows -- read by the prolongation, accumulated into by the restriction -- and the numbers of
// owned dofs of the two levels
struct TransferGhostArgs : TransferArgs
{
    const double* src_ghost;
    double*       dst_ghost;
    int64_t       n_owned_dofs_f, n_owned_dofs_c; // (the fine count states the contract: every fine dof touched is below it)
};

// out[a * sa_out + i * B + b] = sum_j W[j * n_out + i] in[a * sa_in + j * B + b] for a < A, i < n_out, b < B.  B == 1 (the x sweep): the
// lanes run over a; otherwise over b, which then runs over x rows of nx values at stride sx: the padding slots (b % sx >= nx) hold
// nothing and are skipped
__device__ __forceinline__ void transferSweep(const double* __restrict__ in, double* __restrict__ out, const double* __restrict__ W,
                                              int A, int n_in, int n_out, int B, int sa_in, int sa_out, int nx, int sx)
{
    const int total = A * n_out * B;
    for (int o = threadIdx.x; o < total; o += transfer_threads)
    {
        int a, i, b;
        if (B == 1)
        {
            a = o % A;
            i = o / A;
            b = 0;
        }
        else
        {
            b           = o % B;
            const int t = o / B;
            i           = t % n_out;
            a           = t / n_out;
            if (b % sx >= nx)
                continue;
        }
        const double* src = in + a * sa_in + b;
        double        acc = 0.;
        for (int j = 0; j < n_in; ++j)
            acc += W[j * n_out + i] * src[j * B];
        out[a * sa_out + i * B + b] = acc;
    }
    __syncthreads();
}

inline __host__ __device__ int transferPow(int n, int dim)
{
    return dim == 2 ? n * n : n * n * n;
}
// doubles of one LDS buffer per component: the largest intermediate, fine rows with the padded x stride
inline __host__ __device__ int transferBufDoubles(int nf, int dim)
{
    return (nf | 1) * (dim == 2 ? nf : nf * nf);
}
inline size_t transferLdsBytes(int nf, int nc, int dim, int group)
{
    return sizeof(double) * (size_t(2) * group * transferBufDoubles(nf, dim) + size_t(nf) * nc);
}

// RESTRICT == false: dst (fine) = or += P src (coarse);  RESTRICT == true: dst (coarse) += P^T src (fine), atomically.
// GHOST: the coarse dofs >= n_owned_dofs_c live in src_ghost / dst_ghost (the fine side is the same code: an element handles
// owned fine nodes only, the ownership table sees to it)
template < bool RESTRICT, bool GHOST = false >
__global__ __launch_bounds__(transfer_threads) void transferKernel(std::conditional_t< GHOST, TransferGhostArgs, TransferArgs > a)
{
    extern __shared__ double lds[];
    const int nf = a.nf, nc = a.nc, U = a.U, dim = a.dim;
    const int nz_f = dim == 2 ? 1 : nf, nz_c = dim == 2 ? 1 : nc;
    const int sxf = nf | 1, sxc = nc | 1; // padded x strides
    const int Nf = transferPow(nf, dim), Nc = transferPow(nc, dim);
    const int per = transferBufDoubles(nf, dim); // doubles per component and buffer
    double*   W    = lds;
    double*   buf0 = lds + nf * nc;
    double*   buf1 = buf0 + a.group * per;
    for (int i = threadIdx.x; i < nf * nc; i += transfer_threads)
        W[i] = a.table[i];
    __syncthreads();
    for (int64_t pos = blockIdx.x; pos < a.elem_count; pos += gridDim.x)
    {
        const int64_t   ef = a.elem_list ? a.elem_list[a.elem_begin + pos] : a.elem_begin + pos;
        const int64_t   ec = a.elem_map ? a.elem_map[ef] : ef;
        const uint32_t* nf_ids = a.nodes_f + ef * Nf;
        const uint32_t* nc_ids = a.nodes_c + ec * Nc;
        for (int c0 = 0; c0 < U; c0 += a.group)
        {
            const int g = U - c0 < a.group ? U - c0 : a.group;
            if constexpr (!RESTRICT)
            {
                // gather the coarse values (Dirichlet dofs read as 0): buf0[c][kz][jy][ix, stride sxc]
                const int cs = nz_c * nc * sxc;
                for (int t = threadIdx.x; t < g * Nc; t += transfer_threads)
                {
                    const int     c = t % g, ln = t / g;
                    const int64_t dof = int64_t(nc_ids[ln]) * U + c0 + c;
                    double        v   = 0.;
                    if (!(a.dirichlet_c && a.dirichlet_c[dof]))
                    {
                        if constexpr (GHOST)
                            v = dof < a.n_owned_dofs_c ? a.src[dof] : a.src_ghost[dof - a.n_owned_dofs_c];
                        else
                            v = a.src[dof];
                    }
                    buf0[c * cs + (ln / nc) * sxc + ln % nc] = v;
                }
                __syncthreads();
                // x: rows (c, kz, jy) of nc -> nf;  y: (c, kz) x nc -> nf with B = sxf;  z: c x nc -> nf with B = sxf * nf
                transferSweep(buf0, buf1, W, g * nz_c * nc, nc, nf, 1, sxc, sxf, nf, sxf);
                transferSweep(buf1, buf0, W, g * nz_c, nc, nf, sxf, nc * sxf, nf * sxf, nf, sxf);
                double* res = buf0;
                if (dim == 3)
                {
                    transferSweep(buf0, buf1, W, g, nc, nf, sxf * nf, nc * sxf * nf, nf * sxf * nf, nf, sxf);
                    res = buf1;
                }
                // one writer per fine dof: the owning element, plain stores
                const int fs = nz_f * nf * sxf;
                for (int t = threadIdx.x; t < g * Nf; t += transfer_threads)
                {
                    const int      c = t % g, ln = t / g;
                    const uint32_t node = nf_ids[ln];
                    if (a.owner[node] != int32_t(ef))
                        continue;
                    const int64_t dof = int64_t(node) * U + c0 + c;
                    if (a.frozen && !((__double_as_longlong(a.frozen[dof]) & 0x7fffffffffffffffLL) != 0))
                        continue;
                    const bool   fixed = a.dirichlet_f && a.dirichlet_f[dof];
                    const double v     = fixed ? 0. : res[c * fs + (ln / nf) * sxf + ln % nf];
                    if (a.add)
                    {
                        if (!fixed)
                            a.dst[dof] += v;
                    }
                    else
                        a.dst[dof] = v;
                }
                __syncthreads();
            }
            else
            {
                // gather the fine values this element owns (other nodes and Dirichlet dofs read as 0; never loaded, so that
                // nothing stored there can reach the sums): buf0[c][kz][jy][ix, stride sxf]
                const int fs = nz_f * nf * sxf;
                for (int t = threadIdx.x; t < g * Nf; t += transfer_threads)
                {
                    const int      c = t % g, ln = t / g;
                    const uint32_t node = nf_ids[ln];
                    const int64_t  dof  = int64_t(node) * U + c0 + c;
                    double         v    = 0.;
                    if (a.owner[node] == int32_t(ef) && !(a.dirichlet_f && a.dirichlet_f[dof]))
                        v = a.src[dof];
                    buf0[c * fs + (ln / nf) * sxf + ln % nf] = v;
                }
                __syncthreads();
                // the transposed sweeps in the reverse order: z, y, then x
                double *in = buf0, *out = buf1;
                if (dim == 3)
                {
                    transferSweep(in, out, W, g, nf, nc, sxf * nf, nf * sxf * nf, nc * sxf * nf, nf, sxf);
                    double* t = in;
                    in        = out;
                    out       = t;
                }
                transferSweep(in, out, W, g * nz_c, nf, nc, sxf, nf * sxf, nc * sxf, nf, sxf);
                transferSweep(out, in, W, g * nz_c * nc, nf, nc, 1, sxf, sxc, nf, sxf);
                const int cs = nz_c * nc * sxc;
                for (int t = threadIdx.x; t < g * Nc; t += transfer_threads)
                {
                    const int     c = t % g, ln = t / g;
                    const int64_t dof = int64_t(nc_ids[ln]) * U + c0 + c;
                    if (!(a.dirichlet_c && a.dirichlet_c[dof]))
                    {
                        if constexpr (GHOST)
                            unsafeAtomicAdd(dof < a.n_owned_dofs_c ? a.dst + dof : a.dst_ghost + (dof - a.n_owned_dofs_c),
                                            in[c * cs + (ln / nc) * sxc + ln % nc]);
                        else
                            unsafeAtomicAdd(a.dst + dof, in[c * cs + (ln / nc) * sxc + ln % nc]);
                    }
                }
                __syncthreads();
            }
        }
    }
}

// owner[node] = min over the fine elements that contain it (an integer atomicMin: the same table on every run)
__global__ void transferOwnerKernel(const uint32_t* __restrict__ nodes_f, int64_t n_entries, int N, int32_t* __restrict__ owner)
{
    for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n_entries; i += int64_t(gridDim.x) * blockDim.x)
        atomicMin(owner + nodes_f[i], int32_t(i / N));
}

// ... of a partitioned mesh: only the owned nodes (< n_owned_nodes) enter; owner [owned + ghost nodes], the ghost entries keep the fill
__global__ void transferOwnerOwnedKernel(const uint32_t* __restrict__ nodes_f, int64_t n_entries, int N, int64_t n_owned_nodes,
                                         int32_t* __restrict__ owner)
{
    for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n_entries; i += int64_t(gridDim.x) * blockDim.x)
    {
        const uint32_t node = nodes_f[i];
        if (node < n_owned_nodes)
            atomicMin(owner + node, int32_t(i / N));
    }
}
// count += the owned fine nodes that no local element contains (owner still holds `fill`): rows of P nobody would compute
__global__ void transferCountUnhandledKernel(const int32_t* __restrict__ owner, int64_t n_owned_nodes, int32_t fill,
                                             unsigned long long* __restrict__ count)
{
    unsigned long long mine = 0;
    for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n_owned_nodes; i += int64_t(gridDim.x) * blockDim.x)
        mine += owner[i] == fill;
    if (mine)
        atomicAdd(count, mine);
}

// Validation of a level pair, one thread per fine element: the coarse partner lies in range, no coarse element is named twice
// (with equal element counts: a permutation), and the two elements have bitwise equal vertices.  flag[0] <- the smallest
// 4 * element + offence (1 out of range, 2 named twice, 3 other vertices).  `hit` [n_elems], filled with ~0 by the caller, ends as
// the lowest fine element that names each coarse one: whichever of two claimants comes second sees the other's index, and the
// higher of the two is reported -- the same element on every run, whatever order the threads arrive in
__global__ void transferCheckPairKernel(int64_t n_elems, const int64_t* __restrict__ elem_map, const unsigned long long* __restrict__ verts_f,
                                        const unsigned long long* __restrict__ verts_c, int words, unsigned* __restrict__ hit,
                                        unsigned long long* __restrict__ flag)
{
    for (int64_t e = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; e < n_elems; e += int64_t(gridDim.x) * blockDim.x)
    {
        const int64_t ec = elem_map ? elem_map[e] : e;
        if (ec < 0 || ec >= n_elems)
        {
            atomicMin(flag, static_cast< unsigned long long >(e) * 4u + 1u);
            continue;
        }
        const unsigned other = atomicMin(hit + ec, unsigned(e));
        if (other != ~0u)
            atomicMin(flag, static_cast< unsigned long long >(other > unsigned(e) ? other : unsigned(e)) * 4u + 2u);
        bool same = true;
        for (int k = 0; k < words; ++k)
            same = same && verts_f[e * words + k] == verts_c[ec * words + k];
        if (!same)
            atomicMin(flag, static_cast< unsigned long long >(e) * 4u + 3u);
    }
}
} // namespace l3k::dev
#endif
