// vtk.hpp -- the device kernels of the ParaView export (api_vtk.hip; the file layout is described in include/l3k.h and
// host/vtk_text.cpp): the base64 stream encoder, the interleave of a field group, and the coordinates and sub-cell topology of a mesh.
//
// Encoder.  The text of an array is the base64 of the virtual stream S = header (the uint64 payload size) || payload.  Three stream
// bytes give four text bytes, so text DWORD o depends on stream bytes 3o .. 3o + 2 alone: a lane produces W consecutive text dwords
// (W = 1, 2 or 4: one 4-, 8- or 16-byte store) from the stream dwords that hold its 3W bytes, read as aligned dwords (the payload is
// 8-byte aligned, so stream dword k >= 2 is payload dword k - 2; neighbouring lanes share a dword, which the L1 serves).  No LDS, no
// atomics, no byte stores; lanes stride over the window in whole grids.  A window is a range of text dwords of one array (a pipeline
// chunk): its start is a multiple of 4 text dwords = 12 stream bytes.  The stream's last 1 or 2 left-over bytes and the `=` padding
// are the last text dword of the array, produced by the same code: stream bytes past the end read as 0 and the characters that no
// stream byte reaches become `=`.  Payload bytes in a dword that the payload does not fill are fetched byte by byte, so nothing past
// the payload is read.
#ifndef L3K_DEVICE_VTK_HPP
#define L3K_DEVICE_VTK_HPP

#include "common.hpp"

#include <type_traits>

namespace l3k::dev
{
constexpr int vtk_threads = 256;

struct VtkEncodeArgs
{
    const uint32_t* payload;     // 8-byte aligned
    uint64_t        n_bytes;     // of the payload = the header value
    uint32_t*       text;        // the window's first text dword (aligned to the store width)
    uint64_t        first_dword; // the window: text dwords [first_dword, first_dword + n_dwords) of the array's text
    uint64_t        n_dwords;
};

// the four sextets held in the bytes of v -> their characters of the standard alphabet, all four at once: per byte
// c + 'A' + 6 [c >= 26] - 75 [c >= 52] - 15 [c >= 62] + 3 [c >= 63]; (c + 128 - t) has bit 7 set exactly for c >= t, and no byte
// of the result leaves [43, 122], so the dword arithmetic is the four byte results side by side
__device__ __forceinline__ uint32_t vtkAlphabet(uint32_t v)
{
    const uint32_t m26 = ((v + 0x66666666u) >> 7) & 0x01010101u, m52 = ((v + 0x4c4c4c4cu) >> 7) & 0x01010101u;
    const uint32_t m62 = ((v + 0x42424242u) >> 7) & 0x01010101u, m63 = ((v + 0x41414141u) >> 7) & 0x01010101u;
    return v + 0x41414141u + m26 * 6u - m52 * 75u - m62 * 15u + m63 * 3u;
}
// stream dword k (bytes past the end of the stream read as 0)
__device__ __forceinline__ uint32_t vtkStreamDword(const VtkEncodeArgs& a, uint64_t k)
{
    if (k < 2)
        return uint32_t(k == 0 ? a.n_bytes : a.n_bytes >> 32);
    const uint64_t at = (k - 2) * 4; // payload byte
    if (at + 4 <= a.n_bytes)
        return a.payload[k - 2];
    uint32_t                   v     = 0;
    const unsigned char* const bytes = reinterpret_cast< const unsigned char* >(a.payload);
    for (int b = 0; b < 4; ++b)
        if (at + b < a.n_bytes)
            v |= uint32_t(bytes[at + b]) << (8 * b);
    return v;
}
// text dword o of the array from the stream dwords lo = S[3o / 4] and hi = S[3o / 4 + 1]
__device__ __forceinline__ uint32_t vtkTextDword(uint64_t o, uint32_t lo, uint32_t hi, uint64_t stream_bytes)
{
    const unsigned shift = unsigned(3 * o & 3) * 8;
    const uint32_t three = uint32_t(((uint64_t(hi) << 32) | lo) >> shift); // stream bytes 3o, 3o + 1, 3o + 2 in the low 24 bits
    const uint32_t b0 = three & 0xffu, b1 = (three >> 8) & 0xffu, b2 = (three >> 16) & 0xffu;
    const uint32_t g = (b0 << 16) | (b1 << 8) | b2;
    uint32_t       t = vtkAlphabet((g >> 18) | (((g >> 12) & 63u) << 8) | (((g >> 6) & 63u) << 16) | ((g & 63u) << 24));
    if (3 * o + 2 >= stream_bytes) // the array's last dword: `=` where no stream byte reaches
    {
        t = (t & 0x00ffffffu) | (uint32_t('=') << 24);
        if (3 * o + 1 >= stream_bytes)
            t = (t & 0xff00ffffu) | (uint32_t('=') << 16);
    }
    return t;
}

template < int W >
__global__ __launch_bounds__(vtk_threads) void vtkEncodeKernel(VtkEncodeArgs a)
{
    static_assert(W == 1 || W == 2 || W == 4);
    using store_t = std::conditional_t< W == 1, uint32_t, std::conditional_t< W == 2, uint2, uint4 > >;
    const uint64_t stream_bytes = 8 + a.n_bytes;
    const uint64_t n_items      = (a.n_dwords + W - 1) / W;
    for (uint64_t item = uint64_t(blockIdx.x) * vtk_threads + threadIdx.x; item < n_items; item += uint64_t(gridDim.x) * vtk_threads)
    {
        const uint64_t o0 = a.first_dword + item * W; // (a window starts at a multiple of 4 text dwords: o0 is a multiple of W)
        const uint64_t k0 = 3 * o0 / 4;
        constexpr int  S  = W == 4 ? 3 : W + 1; // the stream dwords that hold the lane's 3 W bytes (W = 4: exactly three)
        uint32_t       s[S];
#pragma unroll
        for (int j = 0; j < S; ++j)
            s[j] = vtkStreamDword(a, k0 + j);
        uint32_t t[W];
#pragma unroll
        for (int q = 0; q < W; ++q)
        {
            uint32_t lo, hi;
            if constexpr (W == 4) // text dword q of the four starts in stream dword 0, 0, 1, 2 of the three
            {
                lo = s[3 * q / 4];
                hi = 3 * q / 4 + 1 < S ? s[3 * q / 4 + 1] : 0u;
            }
            else if constexpr (W == 2)
            {
                const bool second = 3 * (o0 + q) / 4 != k0;
                lo                = second ? s[1] : s[0];
                hi                = second ? s[2] : s[1];
            }
            else
                lo = s[0], hi = s[1];
            t[q] = vtkTextDword(o0 + q, lo, hi, stream_bytes);
        }
        if (item * W + W <= a.n_dwords)
        {
            store_t v;
            if constexpr (W == 1)
                v = t[0];
            else if constexpr (W == 2)
                v = make_uint2(t[0], t[1]);
            else
                v = make_uint4(t[0], t[1], t[2], t[3]);
            reinterpret_cast< store_t* >(a.text)[item] = v;
        }
        else // the window's last lane where its length is no multiple of W
#pragma unroll
            for (int q = 0; q < W; ++q)
                if (item * W + q < a.n_dwords)
                    a.text[item * W + q] = t[q];
    }
}

// out[node][0 .. n_out) <- rows of the SoA field storage: 2 or 3 rows -> 3 components, the third +0.0 for two rows
// (encodeFieldImpl, post/VtkExport.hpp:417-448)
__global__ __launch_bounds__(vtk_threads) void vtkInterleaveKernel(const double* __restrict__ r0, const double* __restrict__ r1,
                                                                   const double* __restrict__ r2, int64_t n_nodes,
                                                                   double* __restrict__ out)
{
    for (int64_t i = int64_t(blockIdx.x) * vtk_threads + threadIdx.x; i < n_nodes; i += int64_t(gridDim.x) * vtk_threads)
    {
        out[3 * i]     = r0[i];
        out[3 * i + 1] = r1[i];
        out[3 * i + 2] = r2 ? r2[i] : 0.;
    }
}

// owner[node] = min over the local elements that contain it, ghost nodes included (an integer atomicMin as transferOwnerKernel's,
// device/transfer.hpp: the same table on every run)
__global__ __launch_bounds__(vtk_threads) void vtkOwnerKernel(const uint32_t* __restrict__ elem_nodes, int64_t n_entries, int N,
                                                              int32_t* __restrict__ owner)
{
    for (int64_t i = int64_t(blockIdx.x) * vtk_threads + threadIdx.x; i < n_entries; i += int64_t(gridDim.x) * vtk_threads)
        atomicMin(owner + elem_nodes[i], int32_t(i / N));
}

// coords[node] = the (bi-, tri-)linear map of the element's vertices at the node's GLL reference position
// (mesh/NodePhysicalLocation.hpp), written by the node's owner = the lowest local element that contains it (transferOwnerKernel's
// table over all local nodes): one writer per node, plain stores.  One thread per (element, local node).
struct VtkCoordArgs
{
    const uint32_t* elem_nodes; // [n_elems][n^dim]
    const double*   elem_verts; // [n_elems][2^dim][3]
    const int32_t*  owner;      // [n_nodes]
    double*         coords;     // [n_nodes][3]
    int64_t         n_entries;  // n_elems * n^dim
    int             dim, n;
    double          half_minus[9], half_plus[9]; // (1 - x_i) / 2 and (1 + x_i) / 2 at the GLL points
};
__global__ __launch_bounds__(vtk_threads) void vtkCoordsKernel(VtkCoordArgs a)
{
    const int n = a.n, N = a.dim == 2 ? n * n : n * n * n, nv = a.dim == 2 ? 4 : 8;
    for (int64_t t = int64_t(blockIdx.x) * vtk_threads + threadIdx.x; t < a.n_entries; t += int64_t(gridDim.x) * vtk_threads)
    {
        const int64_t  e    = t / N;
        const int      ln   = int(t - e * N);
        const uint32_t node = a.elem_nodes[t];
        if (a.owner[node] != int32_t(e))
            continue;
        const int     ix = ln % n, iy = (ln / n) % n, iz = ln / (n * n);
        const double* v  = a.elem_verts + e * nv * 3;
        double        x = 0., y = 0., z = 0.;
        for (int k = 0; k < nv; ++k) // vertex k = i + 2 j + 4 l
        {
            double w = ((k & 1) ? a.half_plus[ix] : a.half_minus[ix]) * ((k & 2) ? a.half_plus[iy] : a.half_minus[iy]);
            if (a.dim == 3)
                w *= (k & 4) ? a.half_plus[iz] : a.half_minus[iz];
            x += w * v[3 * k];
            y += w * v[3 * k + 1];
            z += w * v[3 * k + 2];
        }
        double* out = a.coords + int64_t(node) * 3;
        out[0]      = x;
        out[1]      = y;
        out[2]      = a.dim == 2 ? 0. : z;
    }
}

// connectivity and offsets, one thread per sub-cell (serializeElementSubtopo, post/VtkExport.hpp:252-285): cell c is sub-cell
// (layer, row, col) of element c / p^dim
__global__ __launch_bounds__(vtk_threads) void vtkTopologyKernel(const uint32_t* __restrict__ elem_nodes, int64_t n_cells, int dim, int p,
                                                                 uint32_t* __restrict__ conn, uint32_t* __restrict__ offsets)
{
    const int n = p + 1, per = dim == 2 ? p * p : p * p * p, N = dim == 2 ? n * n : n * n * n;
    for (int64_t c = int64_t(blockIdx.x) * vtk_threads + threadIdx.x; c < n_cells; c += int64_t(gridDim.x) * vtk_threads)
    {
        const int64_t   e     = c / per;
        const int       s     = int(c - e * per);
        const int       col = s % p, row = (s / p) % p, layer = s / (p * p);
        const uint32_t* nodes = elem_nodes + e * N + (layer * n * n + row * n + col);
        const uint4     low   = make_uint4(nodes[0], nodes[1], nodes[n + 1], nodes[n]);
        if (dim == 2)
        {
            reinterpret_cast< uint4* >(conn)[c] = low;
            offsets[c]                          = uint32_t(c + 1) * 4u;
        }
        else
        {
            const uint32_t* up                          = nodes + n * n;
            reinterpret_cast< uint4* >(conn)[2 * c]     = low;
            reinterpret_cast< uint4* >(conn)[2 * c + 1] = make_uint4(up[0], up[1], up[n + 1], up[n]);
            offsets[c]                                  = uint32_t(c + 1) * 8u;
        }
    }
}
} // namespace l3k::dev
#endif
