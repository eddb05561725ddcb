// api_pmg.hip -- the p-multigrid preconditioner of libl3k.so (include/l3k.h: l3k_pmg_*): the level pairs with their ownership tables,
// the inter-order transfer launches (device/transfer.hpp), the symmetric V-cycle on the Chebyshev smoothers and the PCG entry point;
// and the standalone transfer of one level pair of a partitioned mesh (l3k_transfer_*), whose hierarchy lives above the ABI.
#include "reduce.hpp"
#include "solver.hpp"

#include "device/launch.hpp"
#include "device/transfer.hpp"

#include <algorithm>

namespace
{
using namespace l3k::red; // cg_threads, cg_blocks, liveRow
using l3k::solver::LinOp;
using l3k::solver::Precond;
constexpr int    max_levels       = 8;            // orders 8 > ... > 1
constexpr size_t transfer_lds_cap = size_t(48) << 10; // bytes of LDS per workgroup: three workgroups per CU

// d = r - A z on the live rows (az holds A z), 0 on the rows the smoother has frozen (minv == 0): 3 reads (r, A z and the mask, which
// is always read), 1 write
__global__ __launch_bounds__(cg_threads) void pmgResidualKernel(double* __restrict__ d, const double* __restrict__ r,
                                                                const double* __restrict__ az, const double* __restrict__ minv, int64_t n)
{
    for (int64_t i = int64_t(blockIdx.x) * cg_threads + threadIdx.x; i < n; i += int64_t(gridDim.x) * cg_threads)
    {
        const double v = __builtin_nontemporal_load(r + i) - __builtin_nontemporal_load(az + i);
        __builtin_nontemporal_store(liveRow(__builtin_nontemporal_load(minv + i)) ? v : 0., d + i);
    }
}
// z += e: 2 reads, 1 write (e is 0 on the frozen rows: the smoother stores it so)
__global__ __launch_bounds__(cg_threads) void pmgAddKernel(double* __restrict__ z, const double* __restrict__ e, int64_t n)
{
    for (int64_t i = int64_t(blockIdx.x) * cg_threads + threadIdx.x; i < n; i += int64_t(gridDim.x) * cg_threads)
        __builtin_nontemporal_store(__builtin_nontemporal_load(z + i) + __builtin_nontemporal_load(e + i), z + i);
}
inline int vecGrid(int64_t n)
{
    const int64_t g = (n + cg_threads - 1) / cg_threads;
    return int(g < 1 ? 1 : (g > cg_blocks ? cg_blocks : g));
}
} // namespace

// a level pair: what the transfers between a fine and a coarse mesh need beyond the meshes
struct TransferPair
{
    const int64_t*     elem_map = nullptr; // the caller's
    DevBuf< int32_t >  owner;              // [fine nodes]
    DevBuf< double >   tab_p, tab_r;       // sweep weights of the prolongation [nc][nf] and of the restriction [nf][nc]
    int                group = 1;          // components per pass
    size_t             lds   = 0;
    // deterministic mode: the fine elements sorted by the colour of their coarse partner; det_ptr[c] .. det_ptr[c + 1] = colour c
    DevBuf< int64_t >      det_elems;
    std::vector< int64_t > det_ptr;
};
// one level of the hierarchy and, from level 1 on, the pair it forms with the level above it (the finer one)
struct PmgLevel
{
    l3k_mf*          mf;
    l3k_cheb*        smoother;
    LinOp            op;
    int64_t          n, ld;
    DevBuf< double > work; // r | z | d | e | w | az (ld apart); level 0 takes r and z from the caller and holds d | e | w | az only
    double *         r, *z, *d, *e, *w, *az;
    TransferPair     pair; // (this level = coarse, the previous one = fine)
};
struct l3k_pmg
{
    l3k_ctx*                ctx;
    std::vector< PmgLevel > levels;
    l3k_pmg_info            info;
};
// l3k_transfer_*: one pair on its own, ghost rows included
struct l3k_transfer
{
    l3k_ctx*          ctx;
    l3k_mesh *        fine, *coarse;
    TransferPair      pair;
    l3k_transfer_info info;
};

namespace
{
// workgroups of a transfer launch over `count` elements
unsigned transferGrid(const l3k_ctx* ctx, int64_t count)
{
    return stridedGrid(ctx, count);
}
l3k::dev::TransferGhostArgs pairArgs(const l3k_mesh* mf, const l3k_mesh* mc, const TransferPair& pair)
{
    l3k::dev::TransferGhostArgs a{};
    a.dim = mf->dim, a.nf = mf->order + 1, a.nc = mc->order + 1, a.U = mf->dofs_per_node, a.group = pair.group;
    a.elem_begin = 0, a.elem_count = mf->n_elems;
    a.elem_list = nullptr, a.elem_map = pair.elem_map;
    a.nodes_f = mf->elem_nodes.ptr, a.nodes_c = mc->elem_nodes.ptr;
    a.dirichlet_f = mf->dirichlet.ptr, a.dirichlet_c = mc->dirichlet.ptr;
    a.owner = pair.owner.ptr;
    a.n_owned_dofs_f = mf->nOwnedDofs(), a.n_owned_dofs_c = mc->nOwnedDofs();
    return a;
}
l3k::dev::TransferArgs pairArgs(const PmgLevel& fine, const PmgLevel& coarse)
{
    return pairArgs(fine.mf->mesh, coarse.mf->mesh, coarse.pair);
}
// x_f <- P x_c or x_f += P x_c; frozen: fine rows to leave alone (nullptr: none)
int launchProlong(l3k_pmg* M, int coarse_level, const double* d_xc, double* d_xf, int add, const double* frozen)
{
    const PmgLevel &fine = M->levels[coarse_level - 1], &coarse = M->levels[coarse_level];
    auto            a = pairArgs(fine, coarse);
    if (a.elem_count == 0)
        return 0;
    a.table = coarse.pair.tab_p.ptr, a.frozen = frozen, a.src = d_xc, a.dst = d_xf, a.add = add;
    return l3k::dev::launchKernel("transferKernel<prolong>", l3k::dev::transferKernel< false >, dim3(transferGrid(M->ctx, a.elem_count)),
                                  dim3(l3k::dev::transfer_threads), coarse.pair.lds, M->ctx->stream, a);
}
// The restriction's launches over the elements of `a` (the destination is zeroed by the caller); deterministic mode: one launch
// per colour of the coarse mesh.  what: "p-multigrid hierarchy" / "transfer" for the message
template < typename Args, typename Launch >
int restrictLaunches(const l3k_ctx* ctx, const TransferPair& pair, Args a, const char* what, Launch&& launch)
{
    if (!ctx->deterministic)
        return launch(a);
    if (pair.det_ptr.empty())
    {
        setError("deterministic mode was enabled after this %s was created: create it with the mode on", what);
        return -1;
    }
    a.elem_list = pair.det_elems.ptr;
    for (size_t c = 0; c + 1 < pair.det_ptr.size(); ++c)
    {
        a.elem_begin = pair.det_ptr[c];
        a.elem_count = pair.det_ptr[c + 1] - pair.det_ptr[c];
        if (a.elem_count > 0)
            if (int rc = launch(a))
                return rc;
    }
    return 0;
}
// r_c <- P^T r_f (r_c zeroed here)
int launchRestrict(l3k_pmg* M, int coarse_level, const double* d_rf, double* d_rc)
{
    const PmgLevel &fine = M->levels[coarse_level - 1], &coarse = M->levels[coarse_level];
    auto            a = pairArgs(fine, coarse);
    L3K_HIP(hipMemsetAsync(d_rc, 0, size_t(coarse.n) * sizeof(double), M->ctx->stream));
    if (a.elem_count == 0)
        return 0;
    a.table = coarse.pair.tab_r.ptr, a.frozen = nullptr, a.src = d_rf, a.dst = d_rc, a.add = 1;
    return restrictLaunches(M->ctx, coarse.pair, a, "p-multigrid hierarchy", [&](const l3k::dev::TransferArgs& r) {
        return l3k::dev::launchKernel("transferKernel<restrict>", l3k::dev::transferKernel< true >, dim3(transferGrid(M->ctx, r.elem_count)),
                                      dim3(l3k::dev::transfer_threads), coarse.pair.lds, M->ctx->stream, r);
    });
}
// The names a pair's messages use: l3k_pmg_create speaks of its levels, l3k_transfer_create of its two meshes
struct PairNames
{
    std::string call, both, fine, coarse; // "l3k_pmg_create", "levels 0 and 1", "level 0", "level 1"
};
// A level pair: validation (one kernel, one readback), ownership table, sweep tables, deterministic plan.  `partitioned` (the
// standalone transfer): the ownership table covers owned and ghost fine nodes and only owned ones enter it; the readback of the
// validation then carries a second word, the number of owned fine nodes that no local element contains, which must be 0
int buildPair(l3k_ctx* ctx, const PairNames& nm, const l3k_mesh* mf, const l3k_mesh* mc, TransferPair& coarse, bool partitioned)
{
    hipStream_t st = ctx->stream;
    if (mf->dim != mc->dim || mf->n_elems != mc->n_elems || mf->dofs_per_node != mc->dofs_per_node)
    {
        setError("%s: %s are not one mesh at two orders: dim %d / %d, %lld / %lld elements, %d / %d dofs per "
                 "node", nm.call.c_str(), nm.both.c_str(), mf->dim, mc->dim, (long long)mf->n_elems, (long long)mc->n_elems,
                 mf->dofs_per_node, mc->dofs_per_node);
        return -1;
    }
    if (!(mc->order < mf->order))
    {
        setError("%s: the orders must decrease strictly from level to level; %s has order %d, %s order %d", nm.call.c_str(),
                 nm.fine.c_str(), mf->order, nm.coarse.c_str(), mc->order);
        return -1;
    }
    if (mf->order > 8 || mf->n_elems >= 0x7f7f7f7f) // (the ownership table holds element indices in 32 bits below its fill value)
    {
        setError("%s: orders up to 8 and fewer than 2^31 - 2^24 elements", nm.call.c_str());
        return -1;
    }
    const int64_t n_elems = mf->n_elems;
    const int     words   = (1 << mf->dim) * 3;
    const int     nf = mf->order + 1, nc = mc->order + 1;
    const int     Nf = l3k::dev::transferPow(nf, mf->dim);
    if (partitioned)
    {
        // ownership of the OWNED fine nodes, ahead of the validation (it reads the fine node table only, not the element map), so
        // that its count of nodes without a handler travels in the validation's readback
        const int64_t n_nodes_f = mf->n_owned_nodes + mf->n_ghost_nodes;
        if (int rc = coarse.owner.alloc(size_t(std::max< int64_t >(n_nodes_f, 1))))
            return rc;
        L3K_HIP(hipMemsetAsync(coarse.owner.ptr, 0x7f, coarse.owner.n * sizeof(int32_t), st));
        if (n_elems > 0)
            hipLaunchKernelGGL(l3k::dev::transferOwnerOwnedKernel, dim3(gridFor(n_elems * Nf)), dim3(256), 0, st, mf->elem_nodes.ptr,
                               n_elems * Nf, Nf, mf->n_owned_nodes, coarse.owner.ptr);
        L3K_HIP(hipGetLastError());
    }
    {
        DevBuf< unsigned >           hit;
        DevBuf< unsigned long long > flag; // [0] the validation's word, [1] (partitioned) owned fine nodes without a handler
        if (int rc = hit.alloc(size_t(std::max< int64_t >(n_elems, 1))))
            return rc;
        if (int rc = flag.alloc(2))
            return rc;
        L3K_HIP(hipMemsetAsync(hit.ptr, 0xff, hit.n * sizeof(unsigned), st));
        L3K_HIP(hipMemsetAsync(flag.ptr, 0xff, sizeof(unsigned long long), st));
        L3K_HIP(hipMemsetAsync(flag.ptr + 1, 0, sizeof(unsigned long long), st));
        if (n_elems > 0)
            hipLaunchKernelGGL(l3k::dev::transferCheckPairKernel, dim3(gridFor(n_elems)), dim3(256), 0, st, n_elems, coarse.elem_map,
                               reinterpret_cast< const unsigned long long* >(mf->elem_verts.ptr),
                               reinterpret_cast< const unsigned long long* >(mc->elem_verts.ptr), words, hit.ptr, flag.ptr);
        L3K_HIP(hipGetLastError());
        if (partitioned && mf->n_owned_nodes > 0)
            hipLaunchKernelGGL(l3k::dev::transferCountUnhandledKernel, dim3(gridFor(mf->n_owned_nodes)), dim3(256), 0, st, coarse.owner.ptr,
                               mf->n_owned_nodes, int32_t(0x7f7f7f7f), flag.ptr + 1);
        L3K_HIP(hipGetLastError());
        unsigned long long f[2] = {0, 0};
        L3K_HIP(hipMemcpyAsync(f, flag.ptr, sizeof f, hipMemcpyDeviceToHost, st)); // (the one readback of the validation)
        L3K_HIP(hipStreamSynchronize(st));
        if (f[0] != ~0ull)
        {
            static const char* const why[] = {"", "is mapped outside the coarse mesh", "is mapped to a coarse element that an earlier one "
                                              "already took (the element map is not a permutation)",
                                              "and its coarse partner have different vertices (elem_verts must be bitwise equal)"};
            setError("%s: %s: fine element %llu %s", nm.call.c_str(), nm.both.c_str(), f[0] / 4, why[f[0] % 4]);
            return -1;
        }
        if (f[1] != 0)
        {
            setError("%s: %llu owned nodes of %s lie in no element of this rank: nobody would compute their rows of P (a node is owned "
                     "by the lowest part that touches it, so a partitioned mesh has none)", nm.call.c_str(), f[1], nm.fine.c_str());
            return -1;
        }
    }
    if (!partitioned)
    {
        // ownership of the fine nodes
        const int64_t n_nodes_f = mf->n_owned_nodes;
        if (int rc = coarse.owner.alloc(size_t(std::max< int64_t >(n_nodes_f, 1))))
            return rc;
        L3K_HIP(hipMemsetAsync(coarse.owner.ptr, 0x7f, coarse.owner.n * sizeof(int32_t), st));
        if (n_elems > 0)
            hipLaunchKernelGGL(l3k::dev::transferOwnerKernel, dim3(gridFor(n_elems * Nf)), dim3(256), 0, st, mf->elem_nodes.ptr, n_elems * Nf,
                               Nf, coarse.owner.ptr);
        L3K_HIP(hipGetLastError());
    }
    // sweep weights: restriction W[jf][ic] = l_ic(x_jf) is the table of l3k_interp_1d, the prolongation takes its transpose
    const auto            tr = l3k::host::interp1d(mc->order, mf->order);
    std::vector< double > tp(tr.size());
    for (int i = 0; i < nf; ++i)
        for (int j = 0; j < nc; ++j)
            tp[size_t(j) * nf + i] = tr[size_t(i) * nc + j];
    if (int rc = coarse.tab_r.upload(tr.data(), tr.size(), st))
        return rc;
    if (int rc = coarse.tab_p.upload(tp.data(), tp.size(), st))
        return rc;
    L3K_HIP(hipStreamSynchronize(st)); // (the staging vectors are locals)
    // components per pass: all of them where the LDS holds them
    coarse.group = mf->dofs_per_node;
    while (coarse.group > 1 && l3k::dev::transferLdsBytes(nf, nc, mf->dim, coarse.group) > transfer_lds_cap)
        --coarse.group;
    coarse.lds = l3k::dev::transferLdsBytes(nf, nc, mf->dim, coarse.group);
    if (ctx->deterministic)
    {
        if (!mc->det_built)
        {
            setError("%s: deterministic mode was enabled after the mesh of %s was created: create the mesh with the mode on",
                     nm.call.c_str(), nm.coarse.c_str());
            return -1;
        }
        std::vector< int64_t > map(static_cast< size_t >(n_elems)), order(static_cast< size_t >(n_elems));
        for (int64_t e = 0; e < n_elems; ++e)
            map[e] = order[e] = e;
        if (coarse.elem_map && n_elems > 0)
        {
            L3K_HIP(hipMemcpyAsync(map.data(), coarse.elem_map, size_t(n_elems) * sizeof(int64_t), hipMemcpyDeviceToHost, st));
            L3K_HIP(hipStreamSynchronize(st));
        }
        const auto& colour = mc->det_colour;
        std::stable_sort(order.begin(), order.end(), [&](int64_t x, int64_t y) { return colour[map[x]] < colour[map[y]]; });
        int n_colours = 0;
        for (int64_t e = 0; e < n_elems; ++e)
            n_colours = std::max(n_colours, int(colour[e]) + 1);
        coarse.det_ptr.assign(size_t(n_colours) + 1, n_elems);
        int64_t i = 0;
        for (int c = 0; c < n_colours; ++c)
        {
            coarse.det_ptr[c] = i;
            while (i < n_elems && colour[map[order[i]]] == c)
                ++i;
        }
        if (int rc = coarse.det_elems.upload(order.data(), order.size(), st))
            return rc;
        L3K_HIP(hipStreamSynchronize(st));
    }
    return 0;
}
int buildPair(l3k_pmg* M, int l)
{
    const auto      level = [](int i) { return "level " + std::to_string(i); };
    const PairNames nm{"l3k_pmg_create", "levels " + std::to_string(l - 1) + " and " + std::to_string(l), level(l - 1), level(l)};
    return buildPair(M->ctx, nm, M->levels[l - 1].mf->mesh, M->levels[l].mf->mesh, M->levels[l].pair, false);
}
int residual(l3k_pmg* M, PmgLevel& L, const double* r, const double* z)
{
    if (int rc = L.op.apply(z, L.az))
        return rc;
    hipLaunchKernelGGL(pmgResidualKernel, dim3(vecGrid(L.n)), dim3(cg_threads), 0, M->ctx->stream, L.d, r, L.az, L.smoother->minv, L.n);
    L3K_HIP(hipGetLastError());
    return 0;
}
// z <- cycle(l, r) (include/l3k.h)
int cycle(l3k_pmg* M, int l, const double* r, double* z)
{
    PmgLevel& L = M->levels[l];
    if (int rc = l3k::solver::chebApply(L.smoother, r, z, L.w, L.az, nullptr)) // pre-smoothing, or the coarse solve
        return rc;
    if (l + 1 == int(M->levels.size()))
        return 0;
    PmgLevel& C = M->levels[l + 1];
    if (int rc = residual(M, L, r, z))
        return rc;
    if (int rc = launchRestrict(M, l + 1, L.d, C.r))
        return rc;
    if (int rc = cycle(M, l + 1, C.r, C.z))
        return rc;
    if (int rc = launchProlong(M, l + 1, C.z, z, 1, L.smoother->minv))
        return rc;
    if (int rc = residual(M, L, r, z))
        return rc;
    if (int rc = l3k::solver::chebApply(L.smoother, L.d, L.e, L.w, L.az, nullptr)) // post-smoothing: the same polynomial
        return rc;
    hipLaunchKernelGGL(pmgAddKernel, dim3(vecGrid(L.n)), dim3(cg_threads), 0, M->ctx->stream, z, L.e, L.n);
    L3K_HIP(hipGetLastError());
    return 0;
}
bool overlap(const double* u, const double* v, int64_t n)
{
    return u < v + n && v < u + n;
}
} // namespace

// the cycle as the preconditioner of the Krylov loops (solver.hpp)
Precond l3k::solver::pmgPrecond(l3k_pmg* M)
{
    PmgLevel& L = M->levels[0];
    return {M, L.mf, L.smoother->minv, L.n, L.ld,
            // z <- M^-1 r, then s[2] <- <r, z> in a pass of its own (2 reads) where the loop asks for it
            [](void* o, const double* r, double* z, double*, double*, double* s) {
                l3k_pmg* M = static_cast< l3k_pmg* >(o);
                if (int rc = cycle(M, 0, r, z))
                    return rc;
                return s ? l3k::solver::dotInto(M->ctx, r, z, M->levels[0].n, s, 2) : 0;
            }};
}
extern "C" {
int l3k_pmg_create(l3k_ctx* ctx, int n_levels, const l3k_pmg_level* levels, l3k_pmg** out)
{
    if (!ctx || !levels || !out)
    {
        setError("l3k_pmg_create: null argument");
        return -1;
    }
    if (n_levels < 2 || n_levels > max_levels)
    {
        setError("l3k_pmg_create: n_levels must lie in 2 .. %d, got %d", max_levels, n_levels);
        return -1;
    }
    for (int l = 0; l < n_levels; ++l)
    {
        const l3k_pmg_level& v = levels[l];
        if (!v.mf || !v.smoother)
        {
            setError("l3k_pmg_create: null argument (level %d needs its operator and its smoother)", l);
            return -1;
        }
        if (v.mf->ctx != ctx)
        {
            setError("l3k_pmg_create: level %d lives on another context", l);
            return -1;
        }
        if (v.mf->mesh->n_ghost_nodes != 0)
        {
            setError("l3k_pmg_create serves single-rank systems; the mesh of level %d has ghost nodes", l);
            return -1;
        }
        if (v.smoother->op.object != v.mf)
        {
            setError("l3k_pmg_create: the smoother of level %d was created for another system", l);
            return -1;
        }
    }
    if (int rc = cgWorkspace(ctx))
        return rc;
    L3K_HIP(hipSetDevice(ctx->device));
    auto M = std::make_unique< l3k_pmg >();
    M->ctx = ctx;
    M->levels.resize(size_t(n_levels));
    M->info          = l3k_pmg_info{};
    M->info.n_levels = n_levels;
    for (int l = 0; l < n_levels; ++l)
    {
        PmgLevel& L = M->levels[l];
        L.mf        = levels[l].mf;
        L.smoother  = levels[l].smoother;
        L.op        = l3k::solver::mfOp(L.mf);
        L.n         = L.op.n;
        L.ld        = (L.n + 3) / 4 * 4;
        L.pair.elem_map = l ? levels[l].d_elem_map : nullptr;
        if (int rc = L.work.alloc(size_t((l ? 6 : 4) * L.ld)))
            return rc;
        L.r = l ? L.work.ptr : nullptr, L.z = l ? L.r + L.ld : nullptr;
        L.d = l ? L.z + L.ld : L.work.ptr, L.e = L.d + L.ld, L.w = L.e + L.ld, L.az = L.w + L.ld;
        if (l)
            if (int rc = buildPair(M.get(), l))
                return rc;
        const int applies_cheb         = L.smoother->info.applies_per_call;
        M->info.order[l]               = L.mf->mesh->order;
        M->info.n_dofs[l]              = L.n;
        M->info.applies_per_cycle[l]   = l + 1 == n_levels ? applies_cheb : 2 * applies_cheb + 2;
    }
    *out = M.release();
    return 0;
}
int l3k_pmg_info_get(const l3k_pmg* M, l3k_pmg_info* out)
{
    if (!M || !out)
    {
        setError("l3k_pmg_info_get: null argument");
        return -1;
    }
    *out = M->info;
    return 0;
}
int l3k_pmg_prolong(l3k_pmg* M, int coarse_level, const double* d_xc, double* d_xf, int add)
{
    if (!M || !d_xc || !d_xf)
    {
        setError("l3k_pmg_prolong: null argument");
        return -1;
    }
    if (coarse_level < 1 || coarse_level >= int(M->levels.size()))
    {
        setError("l3k_pmg_prolong: coarse_level %d outside [1, %d)", coarse_level, int(M->levels.size()));
        return -1;
    }
    return launchProlong(M, coarse_level, d_xc, d_xf, add, nullptr);
}
int l3k_pmg_restrict(l3k_pmg* M, int coarse_level, const double* d_rf, double* d_rc)
{
    if (!M || !d_rf || !d_rc)
    {
        setError("l3k_pmg_restrict: null argument");
        return -1;
    }
    if (coarse_level < 1 || coarse_level >= int(M->levels.size()))
    {
        setError("l3k_pmg_restrict: coarse_level %d outside [1, %d)", coarse_level, int(M->levels.size()));
        return -1;
    }
    return launchRestrict(M, coarse_level, d_rf, d_rc);
}
int l3k_pmg_apply(l3k_pmg* M, const double* d_r, double* d_z)
{
    if (!M || !d_r || !d_z)
    {
        setError("l3k_pmg_apply: null argument");
        return -1;
    }
    if (overlap(d_r, d_z, M->levels[0].n)) // (z is written before r is read for the last time)
    {
        setError("l3k_pmg_apply: r and z overlap");
        return -1;
    }
    return cycle(M, 0, d_r, d_z);
}
int l3k_pmg_destroy(l3k_pmg* M)
{
    delete M;
    return 0;
}
int l3k_pcg_solve_pmg(l3k_mf* mf, const double* d_b, double* d_x, l3k_pmg* M, const l3k_cg_opts* opts, l3k_cg_result* result)
{
    if (!mf || !d_b || !d_x || !M || !result)
    {
        setError("l3k_pcg_solve_pmg: null argument");
        return -1;
    }
    if (mf->mesh->n_ghost_nodes != 0)
    {
        setError("l3k_pcg_solve_pmg serves single-rank systems; this mesh has ghost nodes");
        return -1;
    }
    return l3k::solver::pcgSolvePrecond(l3k::solver::mfOp(mf), "l3k_pcg_solve_pmg", d_b, d_x, l3k::solver::pmgPrecond(M), opts, result);
}
int l3k_pmg_residual(l3k_ctx* ctx, double* d_d, const double* d_r, const double* d_az, const double* d_minv, int64_t n)
{
    if (!ctx || n < 0 || (n > 0 && (!d_d || !d_r || !d_az || !d_minv)))
    {
        setError("l3k_pmg_residual: null argument");
        return -1;
    }
    if (n == 0)
        return 0;
    L3K_HIP(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(pmgResidualKernel, dim3(vecGrid(n)), dim3(cg_threads), 0, ctx->stream, d_d, d_r, d_az, d_minv, n);
    L3K_HIP(hipGetLastError());
    return 0;
}
int l3k_transfer_create(l3k_ctx* ctx, l3k_mesh* mesh_fine, l3k_mesh* mesh_coarse, const int64_t* d_elem_map, l3k_transfer** out)
{
    if (!ctx || !mesh_fine || !mesh_coarse || !out)
    {
        setError("l3k_transfer_create: null argument");
        return -1;
    }
    if (mesh_fine->ctx != ctx || mesh_coarse->ctx != ctx)
    {
        setError("l3k_transfer_create: %s lives on another context", mesh_fine->ctx != ctx ? "the fine mesh" : "the coarse mesh");
        return -1;
    }
    L3K_HIP(hipSetDevice(ctx->device));
    auto T    = std::make_unique< l3k_transfer >();
    T->ctx    = ctx;
    T->fine   = mesh_fine;
    T->coarse = mesh_coarse;
    T->pair.elem_map = d_elem_map;
    const PairNames nm{"l3k_transfer_create", "the fine and the coarse mesh", "the fine mesh", "the coarse mesh"};
    if (int rc = buildPair(ctx, nm, mesh_fine, mesh_coarse, T->pair, true))
        return rc;
    T->info = l3k_transfer_info{mesh_fine->order,
                                mesh_coarse->order,
                                mesh_fine->nOwnedDofs(),
                                mesh_fine->nLocalDofs() - mesh_fine->nOwnedDofs(),
                                mesh_coarse->nOwnedDofs(),
                                mesh_coarse->nLocalDofs() - mesh_coarse->nOwnedDofs()};
    *out    = T.release();
    return 0;
}
int l3k_transfer_info_get(const l3k_transfer* T, l3k_transfer_info* out)
{
    if (!T || !out)
    {
        setError("l3k_transfer_info_get: null argument");
        return -1;
    }
    *out = T->info;
    return 0;
}
int l3k_transfer_prolong(l3k_transfer* T, const double* d_xc, const double* d_xc_ghost, double* d_xf, int add, const double* d_frozen)
{
    if (!T || (T->info.n_owned_dofs_coarse > 0 && !d_xc) || (T->info.n_owned_dofs_fine > 0 && !d_xf))
    {
        setError("l3k_transfer_prolong: null argument");
        return -1;
    }
    if (T->info.n_ghost_dofs_coarse > 0 && !d_xc_ghost)
    {
        setError("l3k_transfer_prolong: the coarse mesh has ghost nodes: d_xc_ghost must hold their rows (l3k_halo_import), got NULL");
        return -1;
    }
    auto a = pairArgs(T->fine, T->coarse, T->pair);
    if (a.elem_count == 0)
        return 0;
    L3K_HIP(hipSetDevice(T->ctx->device));
    a.table = T->pair.tab_p.ptr, a.frozen = d_frozen, a.src = d_xc, a.src_ghost = d_xc_ghost, a.dst = d_xf, a.add = add;
    return l3k::dev::launchKernel("transferKernel<prolong, ghost>", l3k::dev::transferKernel< false, true >,
                                  dim3(transferGrid(T->ctx, a.elem_count)), dim3(l3k::dev::transfer_threads), T->pair.lds, T->ctx->stream, a);
}
int l3k_transfer_restrict(l3k_transfer* T, const double* d_rf, double* d_rc, double* d_rc_ghost)
{
    if (!T || (T->info.n_owned_dofs_fine > 0 && !d_rf) || (T->info.n_owned_dofs_coarse > 0 && !d_rc))
    {
        setError("l3k_transfer_restrict: null argument");
        return -1;
    }
    if (T->info.n_ghost_dofs_coarse > 0 && !d_rc_ghost)
    {
        setError("l3k_transfer_restrict: the coarse mesh has ghost nodes: d_rc_ghost must take their rows (for l3k_halo_export_add), got NULL");
        return -1;
    }
    L3K_HIP(hipSetDevice(T->ctx->device));
    if (T->info.n_owned_dofs_coarse > 0)
        L3K_HIP(hipMemsetAsync(d_rc, 0, size_t(T->info.n_owned_dofs_coarse) * sizeof(double), T->ctx->stream));
    if (T->info.n_ghost_dofs_coarse > 0)
        L3K_HIP(hipMemsetAsync(d_rc_ghost, 0, size_t(T->info.n_ghost_dofs_coarse) * sizeof(double), T->ctx->stream));
    auto a = pairArgs(T->fine, T->coarse, T->pair);
    if (a.elem_count == 0)
        return 0;
    a.table = T->pair.tab_r.ptr, a.frozen = nullptr, a.src = d_rf, a.dst = d_rc, a.dst_ghost = d_rc_ghost, a.add = 1;
    return restrictLaunches(T->ctx, T->pair, a, "transfer", [&](const l3k::dev::TransferGhostArgs& r) {
        return l3k::dev::launchKernel("transferKernel<restrict, ghost>", l3k::dev::transferKernel< true, true >,
                                      dim3(transferGrid(T->ctx, r.elem_count)), dim3(l3k::dev::transfer_threads), T->pair.lds,
                                      T->ctx->stream, r);
    });
}
int l3k_transfer_destroy(l3k_transfer* T)
{
    delete T;
    return 0;
}
} // extern "C"
