// api_vtk.hip -- the ParaView export of libl3k.so (include/l3k.h: l3k_vtk_*): the kernels of device/vtk.hpp behind a two-buffer
// pipeline that turns device arrays into base64 text in a file.  The XML text and the argument checks that need no device are
// host/vtk_text.cpp.
#include "objects.hpp"

#include "device/vtk.hpp"
#include "host/vtk_text.hpp"

#include <algorithm>
#include <cerrno>

#include <fcntl.h>
#include <unistd.h>

namespace
{
using l3k::dev::VtkEncodeArgs;
constexpr size_t default_chunk_bytes = size_t(4) << 20; // of text (4, 16, 64 and 256 MiB measured within noise of each other)
constexpr int    default_store_bytes = 16;               // text bytes a lane stores at once

// 4, 8 or 16 text bytes per lane: L3K_VTK_STORE_BYTES (read at every call: tools/bench_vtk.py alternates the widths in one process)
int storeBytes()
{
    const char* env = std::getenv("L3K_VTK_STORE_BYTES");
    const int   v   = env ? std::atoi(env) : 0;
    return v == 4 || v == 8 || v == 16 ? v : default_store_bytes;
}

// text dwords [first, first + count) of the array `uint64 n_bytes || payload` into d_text on s (first: a multiple of 4)
int launchEncode(const l3k_ctx* ctx, const void* d_payload, uint64_t n_bytes, uint64_t first, uint64_t count, char* d_text, hipStream_t s)
{
    if (count == 0)
        return 0;
    const VtkEncodeArgs a{static_cast< const uint32_t* >(d_payload), n_bytes, reinterpret_cast< uint32_t* >(d_text), first, count};
    const int           w      = storeBytes() / 4;
    const uint64_t      items  = (count + w - 1) / w;
    const dim3          grid{stridedGrid(ctx, int64_t((items + l3k::dev::vtk_threads - 1) / l3k::dev::vtk_threads))};
    const dim3          block{l3k::dev::vtk_threads};
    if (w == 1)
        hipLaunchKernelGGL(l3k::dev::vtkEncodeKernel< 1 >, grid, block, 0, s, a);
    else if (w == 2)
        hipLaunchKernelGGL(l3k::dev::vtkEncodeKernel< 2 >, grid, block, 0, s, a);
    else
        hipLaunchKernelGGL(l3k::dev::vtkEncodeKernel< 4 >, grid, block, 0, s, a);
    L3K_HIP(hipGetLastError());
    return 0;
}

// Two device halves and two pinned host halves of `chunk` text bytes, the copy stream and the events that order the reuse of the
// halves (the shape of SubBatchPipe, objects.hpp): chunk k is encoded into device half k & 1 on the context's stream, copied to host
// half k & 1 on the copy stream, and handed to the sink by the host while chunk k + 1 is encoded
struct VtkPipe
{
    char*       dev[2]  = {nullptr, nullptr};
    char*       host[2] = {nullptr, nullptr};
    size_t      chunk   = 0;
    hipStream_t copy    = nullptr;
    hipEvent_t  encoded[2] = {nullptr, nullptr}, copied[2] = {nullptr, nullptr};
    VtkPipe()                          = default;
    VtkPipe(const VtkPipe&)            = delete;
    VtkPipe& operator=(const VtkPipe&) = delete;
    ~VtkPipe()
    {
        for (int k = 0; k < 2; ++k)
        {
            if (dev[k])
                (void)hipFree(dev[k]);
            if (host[k])
                (void)hipHostFree(host[k]);
            if (encoded[k])
                (void)hipEventDestroy(encoded[k]);
            if (copied[k])
                (void)hipEventDestroy(copied[k]);
        }
        if (copy)
            (void)hipStreamDestroy(copy);
    }
    int init(size_t chunk_bytes)
    {
        chunk = chunk_bytes;
        L3K_HIP(hipStreamCreateWithFlags(&copy, hipStreamNonBlocking));
        for (int k = 0; k < 2; ++k)
        {
            L3K_HIP(hipMalloc(reinterpret_cast< void** >(&dev[k]), chunk));
            L3K_HIP(hipHostMalloc(reinterpret_cast< void** >(&host[k]), chunk, hipHostMallocDefault));
            L3K_HIP(hipEventCreateWithFlags(&encoded[k], hipEventDisableTiming));
            L3K_HIP(hipEventCreateWithFlags(&copied[k], hipEventDisableTiming));
        }
        return 0;
    }
};

// one array of a file: its payload on the device and, if it has to be formed first, the launch that forms it (queued on the
// context's stream in front of the array's first chunk: behind every encode of the array before it, which may read the same buffer)
struct VtkArray
{
    const void* d_payload;
    uint64_t    n_bytes;
    int (*prepare)(void* user, int index, hipStream_t s);
    void* user;
    int   index;
};

// The text of the arrays, one after the other, through the pipe into sink(text, bytes) (a non-zero return ends the run).  On any
// error both streams are drained before this returns: nothing queued can touch the halves or the payloads afterwards.
template < typename Sink >
int runEncodePipe(const l3k_ctx* ctx, VtkPipe& p, const VtkArray* arrays, int n_arrays, Sink&& sink)
{
    hipStream_t main = ctx->stream;
    size_t      pending_bytes[2] = {0, 0};
    int64_t     k = 0; // chunks queued
    const auto  drainOne = [&](int64_t chunk) -> int { // the host's share of chunk `chunk`: wait for its copy, hand it on
        const int h = int(chunk & 1);
        L3K_HIP(hipEventSynchronize(p.copied[h]));
        return sink(p.host[h], pending_bytes[h]);
    };
    const auto run = [&]() -> int {
        for (int i = 0; i < n_arrays; ++i)
        {
            const VtkArray& arr = arrays[i];
            if (arr.prepare)
                if (int rc = arr.prepare(arr.user, arr.index, main))
                    return rc;
            const uint64_t text_bytes = l3k::host::vtkEncodedBytes(arr.n_bytes);
            for (uint64_t at = 0; at < text_bytes; at += p.chunk, ++k)
            {
                const int      h = int(k & 1);
                const uint64_t n = text_bytes - at < p.chunk ? text_bytes - at : p.chunk;
                if (k >= 2) // the copy of chunk k - 2 has read this device half (the host has waited for it too, in drainOne)
                    L3K_HIP(hipStreamWaitEvent(main, p.copied[h], 0));
                if (int rc = launchEncode(ctx, arr.d_payload, arr.n_bytes, at / 4, n / 4, p.dev[h], main))
                    return rc;
                L3K_HIP(hipEventRecord(p.encoded[h], main));
                L3K_HIP(hipStreamWaitEvent(p.copy, p.encoded[h], 0));
                L3K_HIP(hipMemcpyAsync(p.host[h], p.dev[h], n, hipMemcpyDeviceToHost, p.copy));
                L3K_HIP(hipEventRecord(p.copied[h], p.copy));
                pending_bytes[h] = size_t(n);
                if (k >= 1) // ... while the device works on chunk k, the host hands on chunk k - 1
                    if (int rc = drainOne(k - 1))
                        return rc;
            }
        }
        return k >= 1 ? drainOne(k - 1) : 0;
    };
    const int rc = run();
    if (rc)
    {
        (void)hipStreamSynchronize(p.copy);
        (void)hipStreamSynchronize(main);
    }
    return rc;
}

bool writeAll(int fd, const char* p, size_t n)
{
    while (n > 0)
    {
        const ssize_t w = write(fd, p, n);
        if (w < 0)
        {
            if (errno == EINTR)
                continue;
            return false;
        }
        p += w;
        n -= size_t(w);
    }
    return true;
}
} // namespace

struct l3k_vtk
{
    l3k_mesh*        mesh = nullptr;
    l3k_vtk_info     info{};
    VtkPipe          pipe;
    std::string      mesh_text; // Position, connectivity, offsets, types: encoded once (m_encoded_coords / m_encoded_topo)
    DevBuf< double > interleaved; // [n_points][3]: the payload of a group of 2 or 3 rows, formed in front of its first chunk
    // the export in flight: what the prepare launches read
    const double* d_fields = nullptr;
    size_t        ld       = 0;
};

namespace
{
struct ExportGroups
{
    l3k_vtk*                  vtk;
    const int*                n_comps;
    std::vector< const int* > rows; // of each group
};
int prepareGroup(void* user, int g, hipStream_t s)
{
    const auto*    eg  = static_cast< const ExportGroups* >(user);
    l3k_vtk*       v   = eg->vtk;
    const int*     r   = eg->rows[size_t(g)];
    const int64_t  n   = v->info.n_points;
    const double*  r2  = eg->n_comps[g] == 3 ? v->d_fields + size_t(r[2]) * v->ld : nullptr;
    hipLaunchKernelGGL(l3k::dev::vtkInterleaveKernel, dim3(stridedGrid(v->mesh->ctx, (n + l3k::dev::vtk_threads - 1) / l3k::dev::vtk_threads)),
                       dim3(l3k::dev::vtk_threads), 0, s, v->d_fields + size_t(r[0]) * v->ld, v->d_fields + size_t(r[1]) * v->ld, r2, n,
                       v->interleaved.ptr);
    L3K_HIP(hipGetLastError());
    return 0;
}

// the four mesh sections on the device, one at a time (each is freed before the next is formed), encoded into vtk->mesh_text
int encodeMeshSections(l3k_vtk* v)
{
    const l3k_mesh* m    = v->mesh;
    const l3k_ctx*  ctx  = m->ctx;
    hipStream_t     s    = ctx->stream;
    const auto&     info = v->info;
    const int       n    = m->order + 1;
    const int64_t   N    = m->dim == 2 ? n * n : n * n * n;
    const auto      grid = [&](int64_t count) { return dim3(stridedGrid(ctx, (count + l3k::dev::vtk_threads - 1) / l3k::dev::vtk_threads)); };
    const dim3      block{l3k::dev::vtk_threads};
    v->mesh_text.reserve(size_t(info.encoded_bytes[0] + info.encoded_bytes[1] + info.encoded_bytes[2] + info.encoded_bytes[3]));
    const auto append = [&](const void* d_payload, uint64_t n_bytes) -> int {
        const VtkArray arr{d_payload, n_bytes, nullptr, nullptr, 0};
        return runEncodePipe(ctx, v->pipe, &arr, 1, [&](const char* text, size_t bytes) {
            v->mesh_text.append(text, bytes);
            return 0;
        });
    };
    {
        // Position: the owner table (an integer atomicMin over all local nodes, ghost nodes included), then one writer per node
        DevBuf< int32_t > owner;
        DevBuf< double >  coords;
        if (int rc = owner.alloc(size_t(info.n_points)))
            return rc;
        if (int rc = coords.alloc(size_t(info.n_points) * 3))
            return rc;
        if (info.n_points > 0)
        {
            L3K_HIP(hipMemsetAsync(owner.ptr, 0x7f, size_t(info.n_points) * sizeof(int32_t), s)); // above every element index
            L3K_HIP(hipMemsetAsync(coords.ptr, 0, size_t(info.n_points) * 3 * sizeof(double), s)); // (nodes of no element: the origin)
        }
        if (m->n_elems > 0)
        {
            hipLaunchKernelGGL(l3k::dev::vtkOwnerKernel, grid(m->n_elems * N), block, 0, s, m->elem_nodes.ptr, m->n_elems * N, int(N),
                               owner.ptr);
            L3K_HIP(hipGetLastError());
            l3k::dev::VtkCoordArgs a{};
            a.elem_nodes = m->elem_nodes.ptr, a.elem_verts = m->elem_verts.ptr, a.owner = owner.ptr, a.coords = coords.ptr;
            a.n_entries = m->n_elems * N, a.dim = m->dim, a.n = n;
            const auto gll = l3k::host::gllNodes(n);
            for (int i = 0; i < n; ++i)
                a.half_minus[i] = (1. - gll[size_t(i)]) / 2., a.half_plus[i] = (1. + gll[size_t(i)]) / 2.;
            hipLaunchKernelGGL(l3k::dev::vtkCoordsKernel, grid(a.n_entries), block, 0, s, a);
            L3K_HIP(hipGetLastError());
        }
        if (int rc = append(coords.ptr, info.raw_bytes[0]))
            return rc;
    }
    {
        DevBuf< uint32_t > conn, offsets;
        if (int rc = conn.alloc(size_t(info.n_conn)))
            return rc;
        if (int rc = offsets.alloc(size_t(info.n_cells)))
            return rc;
        if (info.n_cells > 0)
        {
            hipLaunchKernelGGL(l3k::dev::vtkTopologyKernel, grid(info.n_cells), block, 0, s, m->elem_nodes.ptr, info.n_cells, m->dim, m->order,
                               conn.ptr, offsets.ptr);
            L3K_HIP(hipGetLastError());
        }
        if (int rc = append(conn.ptr, info.raw_bytes[1]))
            return rc;
        if (int rc = append(offsets.ptr, info.raw_bytes[2]))
            return rc;
    }
    {
        DevBuf< uint8_t > types; // (rounded up to whole 8 bytes: the encoder's payload is 8-byte aligned, its length is not)
        if (int rc = types.alloc(size_t(info.n_cells + 7) / 8 * 8))
            return rc;
        if (info.n_cells > 0)
            L3K_HIP(hipMemsetAsync(types.ptr, m->dim == 2 ? 9 : 12, size_t(info.n_cells), s)); // subelCellType, VtkExport.hpp:225-236
        if (int rc = append(types.ptr, info.raw_bytes[3]))
            return rc;
    }
    return 0;
}
} // namespace

extern "C" {

int l3k_vtk_encode(l3k_ctx* ctx, const void* d_payload, uint64_t n_bytes, char* d_text, uint64_t text_capacity)
{
    if (!ctx || !d_text || (n_bytes > 0 && !d_payload))
    {
        setError("l3k_vtk_encode: null argument");
        return -1;
    }
    const uint64_t text_bytes = l3k::host::vtkEncodedBytes(n_bytes);
    if (text_capacity < text_bytes)
    {
        setError("l3k_vtk_encode: %llu payload bytes give %llu text bytes, the buffer holds %llu", (unsigned long long)n_bytes,
                 (unsigned long long)text_bytes, (unsigned long long)text_capacity);
        return -1;
    }
    if (reinterpret_cast< uintptr_t >(d_payload) % 8 != 0 || reinterpret_cast< uintptr_t >(d_text) % 16 != 0)
    {
        setError("l3k_vtk_encode: the payload must be 8-byte aligned and the text 16-byte aligned");
        return -1;
    }
    L3K_HIP(hipSetDevice(ctx->device));
    return launchEncode(ctx, d_payload, n_bytes, 0, text_bytes / 4, d_text, ctx->stream);
}

int l3k_vtk_create(l3k_mesh* mesh, const l3k_vtk_opts* opts, l3k_vtk** out)
{
    if (!mesh || !out)
    {
        setError("l3k_vtk_create: null argument");
        return -1;
    }
    *out = nullptr;
    l3k_vtk_info info{};
    if (l3k_vtk_sizes(mesh->dim, mesh->order, mesh->n_elems, mesh->n_owned_nodes + mesh->n_ghost_nodes, &info))
        return -1;
    L3K_HIP(hipSetDevice(mesh->ctx->device));
    auto v  = std::make_unique< l3k_vtk >();
    v->mesh = mesh;
    // no chunk larger than the largest array's text (Position: no field group has more), a multiple of 16, at least 16
    size_t       chunk   = opts && opts->chunk_bytes ? opts->chunk_bytes : default_chunk_bytes;
    const size_t largest = size_t(std::max(info.encoded_bytes[0], info.encoded_bytes[1]));
    chunk                = std::min(chunk, (largest + 15) / 16 * 16);
    chunk                = std::max< size_t >(chunk / 16 * 16, 16);
    info.chunk_bytes     = chunk;
    info.store_bytes     = storeBytes();
    v->info              = info;
    if (int rc = v->pipe.init(chunk))
        return rc;
    if (int rc = encodeMeshSections(v.get()))
        return rc;
    *out = v.release();
    return 0;
}

int l3k_vtk_info_get(const l3k_vtk* vtk, l3k_vtk_info* out)
{
    if (!vtk || !out)
    {
        setError("l3k_vtk_info_get: null argument");
        return -1;
    }
    *out = vtk->info;
    return 0;
}

int l3k_vtk_destroy(l3k_vtk* vtk)
{
    delete vtk;
    return 0;
}

int l3k_vtk_export(l3k_vtk* vtk, const char* path, int rank, int n_ranks, int n_groups, const char* const* names, const int* n_comps,
                   const int* comp_inds, const double* d_fields, size_t ld, int n_fields)
{
    if (!vtk || !path || !path[0] || (n_groups > 0 && !d_fields))
    {
        setError("l3k_vtk_export: null argument");
        return -1;
    }
    if (const std::string err = l3k::host::vtkCheckGroups(rank, n_ranks, n_groups, names, n_comps, comp_inds, n_fields); !err.empty())
    {
        setError("l3k_vtk_export: %s", err.c_str());
        return -1;
    }
    const auto& info = vtk->info;
    if (n_groups > 0 && ld < size_t(info.n_points))
    {
        setError("l3k_vtk_export: field leading dimension %zu < number of local nodes %lld", ld, (long long)info.n_points);
        return -1;
    }
    if (const std::string err = l3k::host::vtkMakeParentDirs(path); !err.empty())
    {
        setError("l3k_vtk_export: %s", err.c_str());
        return -1;
    }
    L3K_HIP(hipSetDevice(vtk->mesh->ctx->device));
    // the arrays of the field groups: a single row is encoded where it lies, 2 or 3 rows are interleaved first
    ExportGroups            eg{vtk, n_comps, {}};
    std::vector< VtkArray > arrays;
    bool                    interleaves = false;
    for (int g = 0, at = 0; g < n_groups; at += n_comps[g], ++g)
    {
        eg.rows.push_back(comp_inds + at);
        if (n_comps[g] == 1)
            arrays.push_back(VtkArray{d_fields + size_t(comp_inds[at]) * ld, l3k::host::vtkGroupBytes(1, info.n_points), nullptr, nullptr, g});
        else
        {
            arrays.push_back(VtkArray{nullptr, l3k::host::vtkGroupBytes(n_comps[g], info.n_points), prepareGroup, &eg, g});
            interleaves = true;
        }
    }
    if (interleaves && !vtk->interleaved.ptr)
        if (int rc = vtk->interleaved.alloc(size_t(info.n_points) * 3))
            return rc;
    for (auto& a : arrays)
        if (a.prepare)
            a.d_payload = vtk->interleaved.ptr;
    vtk->d_fields = d_fields;
    vtk->ld       = ld;

    const auto writeFile = [](const std::string& name, auto&& body) -> int {
        const int fd = open(name.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
        if (fd < 0)
        {
            setError("l3k_vtk_export: cannot open %s: %s", name.c_str(), std::strerror(errno));
            return -1;
        }
        int rc = body(fd);
        if (close(fd) != 0 && !rc)
        {
            setError("l3k_vtk_export: closing %s failed: %s", name.c_str(), std::strerror(errno));
            rc = -1;
        }
        if (rc)
            (void)unlink(name.c_str()); // no half-written file stays
        return rc;
    };
    const auto put = [](int fd, const char* text, size_t bytes) -> int {
        if (writeAll(fd, text, bytes))
            return 0;
        setError("l3k_vtk_export: write failed: %s", std::strerror(errno));
        return -1;
    };
    const std::string vtu_name = l3k::host::vtkVtuFileName(path, rank);
    int               rc       = writeFile(vtu_name, [&](int fd) -> int {
        const std::string head = l3k::host::vtkVtuHeaderText(info.n_points, info.n_cells, info.encoded_bytes, n_groups, names, n_comps);
        if (int e = put(fd, head.data(), head.size()))
            return e;
        if (int e = put(fd, vtk->mesh_text.data(), vtk->mesh_text.size()))
            return e;
        if (int e = runEncodePipe(vtk->mesh->ctx, vtk->pipe, arrays.data(), int(arrays.size()),
                                  [&](const char* text, size_t bytes) { return put(fd, text, bytes); }))
            return e;
        return put(fd, l3k::host::vtk_vtu_postamble, std::strlen(l3k::host::vtk_vtu_postamble));
    });
    if (!rc && rank == 0)
    {
        const std::string pvtu_name = l3k::host::vtkPvtuFileName(path);
        rc = writeFile(pvtu_name, [&](int fd) -> int {
            const std::string text = l3k::host::vtkPvtuText(path, n_ranks, n_groups, names, n_comps);
            return put(fd, text.data(), text.size());
        });
        if (rc)
            (void)unlink(vtu_name.c_str());
    }
    vtk->d_fields = nullptr;
    return rc;
}

} // extern "C"
