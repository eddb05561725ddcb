// quad_assemble.hpp -- local systems of bilinear quadrilaterals (dim = 2): the assembled path's element and side kernels.
//
// Reference: assembleLocalSystem (algsys/AssembleLocalSystem.hpp:77-216, :234-256) on a LocalElementView of a quad and on a
// BoundaryElementView of one of its sides,
//   K[(a,u),(b,v)] = sum_q w_q jac_q sum_eq B_q[eq,(a,u)] B_q[eq,(b,v)],   F[(a,u),r] = sum_q w_q jac_q sum_eq B_q[eq,(a,u)] f_q[eq,r],
//   B_q[eq,(a,u)]  = A0[eq][u] phi_a(q) + sum_s A_{s+1}[eq][u] dphi_a/dx_s(q),        node a = ix + (p+1) iy,
// over the nq^2 Gauss points of the element (geometry of quadGeom, kernel input of quadKernelAt) or over the nq points of one
// side (surface jacobian, outward normal and kernel input of quadSideKernel; the local system of the WHOLE element: derivative
// operators reach every node).  Layouts of l3k_local_assemble / l3k_bnd_local_assemble: K row-major [Nd][Nd], F [n_rhs][Nd],
// Nd = (p+1)^2 U; no mask, no lifting.
//
// Organisation: one workgroup per element (or side), the same body for both point sets.
//   phase 1  one point per thread: the external fields at the point (tensor sum over the nodes), geometry, the user's functor,
//            and the record sqrt(w jac) * { A0, D_0, D_1 [eq][u], f [eq][r] } of the point in LDS, D_d = sum_s A_{s+1} dxi_d/dx_s.
//            The weight goes in as its square root (as in boundary_assemble.hpp): K[i][j] and K[j][i] are then the same sequence
//            of operations.  3 E U + E R doubles per point: 36 + 8 at E = 4, U = 3, R = 2, 28.5 KB at nq = 9.
//   phase 2  the lower triangle of K by tiles of `tile_nodes` row nodes (an x-line of nodes where it fits 32 KB): each thread
//            owns a node pair (a, b <= a) of the tile, loops over the points with the 1-D tables in LDS and keeps the U x U block
//            in registers (the arithmetic is small: ~13 Mflop per element at p = 6, U = 3).  The blocks go to an LDS tile of
//            tile_nodes U rows x Nd columns -- K is never resident as a whole: Nd^2 doubles are 173 KB at p = 6, U = 3 -- and the
//            tile leaves with the lanes along the COLUMN index: its own rows (contiguous runs of up to Nd doubles, the part right
//            of the diagonal mirrored inside the tile) and its mirror image above it (runs of tile_nodes U doubles).  Every entry
//            is written exactly once, zeros included; no atomics: K is bitwise symmetric and bitwise reproducible.
//   phase 3  F, one node per thread.
// Measured: the stores reach 0.05-0.08 of the HBM write roofline, so they are not what limits it as it stands; what
// does was not measured (the pair loop of phase 2 is the likely place).  A domain point with detJ <= 0 raises the degenerate-element
// flag (ElemArgs::workspace[0]; no coefficient workspace: Instance::assemble_ws_doubles = 0).
#ifndef L3K_DEVICE_QUAD_ASSEMBLE_HPP
#define L3K_DEVICE_QUAD_ASSEMBLE_HPP

#include "quad_boundary.hpp"

namespace l3k::dev
{
template < typename K, int P, int NQ, int R >
struct QuadAsmCfg
{
    static constexpr int U = K::params.n_unknowns, E = K::params.n_equations, F = K::params.n_fields;
    static constexpr int N1 = P + 1, NN = N1 * N1, Nd = NN * U;
    static constexpr int CS = 3 * E * U + E * R; // coefficient record of a point
    static constexpr int LD = Nd + 1;            // row pitch of the tile (odd: the mirror image reads it by columns)
    // row nodes per tile: what 32 KB hold, an x-line at the most, one node at the least
    static constexpr int tile_budget = 32 * 1024 / int(sizeof(double)) / LD / U;
    static constexpr int tile_nodes  = tile_budget < 1 ? 1 : (tile_budget > N1 ? N1 : tile_budget);
    static constexpr int TR          = tile_nodes * U;
    // threads: one per node pair of the largest tile, whole waves, 256 at the most
    static constexpr int pairs   = tile_nodes * NN;
    static constexpr int threads = pairs >= 256 ? 256 : ((pairs + 63) / 64) * 64;
    template < bool SIDE >
    static constexpr size_t ldsBytes()
    {
        constexpr int npts = SIDE ? NQ : NQ * NQ;
        return sizeof(double) * (size_t(npts) * CS + 2 * size_t(NQ + 2) * N1 + size_t(F) * NN + 12 + size_t(TR) * LD);
    }
};

// One element (SIDE false) or one side of it (SIDE true; `side` as in quadSide): K into Kout, F into Fout (either may be null).
template < typename K, int P, int NQ, int R, bool SIDE >
__device__ __forceinline__ void quadAsmBody(const K& kern, const uint32_t* __restrict__ en, const double* __restrict__ ev,
                                            const double* __restrict__ tables, const double* __restrict__ fields, size_t ldf, double time,
                                            int side, double* __restrict__ Kout, double* __restrict__ Fout, double* degenerate)
{
    using Cfg = QuadAsmCfg< K, P, NQ, R >;
    constexpr int         U = Cfg::U, E = Cfg::E, F = Cfg::F, N1 = Cfg::N1, NN = Cfg::NN, Nd = Cfg::Nd, CS = Cfg::CS, LD = Cfg::LD;
    constexpr int         TN = Cfg::tile_nodes, NT = Cfg::threads, NPTS = SIDE ? NQ : NQ * NQ, NC = NQ + 2;
    constexpr TableLayout TL{N1, NQ};

    extern __shared__ double lds[];
    double* const coef = lds;                // [NPTS][CS]
    double* const tval = coef + NPTS * CS;   // [NC][N1] phi_i at the nq Gauss points, at -1 and at +1
    double* const tder = tval + NC * N1;     // [NC][N1] phi_i' there
    double* const fld  = tder + NC * N1;     // [F][NN] nodal values of the external fields
    double* const vv   = fld + F * NN;       // [4][3]
    double* const tile = vv + 12;            // [TR][LD]
    const int     tid  = threadIdx.x;

    const QuadSide qs = quadSide(SIDE ? side : 0);
    // columns of tval / tder of point q along x and y
    const auto colX = [&](int q) { return SIDE ? (qs.t == 0 ? q : NQ + qs.upper) : q % NQ; };
    const auto colY = [&](int q) { return SIDE ? (qs.t == 1 ? q : NQ + qs.upper) : q / NQ; };

    if (tid < 12)
        vv[tid] = ev[tid];
    for (int t = tid; t < NC * N1; t += NT)
    {
        const int c = t / N1, i = t - c * N1;
        tval[t] = c < NQ ? tables[TL.offI() + i * NQ + c] : (i == (c == NQ ? 0 : P) ? 1. : 0.);
        tder[t] = c < NQ ? tables[TL.offD() + i * NQ + c] : tables[TL.offE() + (c - NQ) * N1 + i];
    }
    if constexpr (F > 0)
        for (int t = tid; t < NN * F; t += NT)
        {
            const int f = t / NN, i = t - f * NN;
            fld[t]      = fields[en[i] + f * ldf];
        }
    __syncthreads();

    // ---- phase 1: the coefficient record of every point
    const double* const qw = tables + TL.offW();
    const double* const qp = tables + TL.offX();
    for (int q = tid; q < NPTS; q += NT)
    {
        const double* const vx = tval + colX(q) * N1;
        const double* const vy = tval + colY(q) * N1;
        const double* const dx = tder + colX(q) * N1;
        const double* const dy = tder + colY(q) * N1;
        double fv[F > 0 ? F : 1], fd0[F > 0 ? F : 1], fd1[F > 0 ? F : 1];
#pragma unroll
        for (int f = 0; f < F; ++f)
        {
            double v = 0., d0 = 0., d1 = 0.;
            for (int iy = 0; iy < N1; ++iy)
            {
                double s = 0., sd = 0.;
                for (int ix = 0; ix < N1; ++ix)
                {
                    s += vx[ix] * fld[f * NN + iy * N1 + ix];
                    sd += dx[ix] * fld[f * NN + iy * N1 + ix];
                }
                v += vy[iy] * s;
                d0 += vy[iy] * sd;
                d1 += dy[iy] * s;
            }
            fv[f] = v, fd0[f] = d0, fd1[f] = d1;
        }
        double Ji[2][2], xy[2], wgt;
        using Iface = KernelInterface< KernelParams{2, E, U, F, R} >;
        typename Iface::Result res{};
        if constexpr (SIDE)
        {
            double nrm[2];
            wgt = qw[q] * quadSideGeom(vv, qs, qp[q], Ji, xy, nrm);
            typename Iface::BoundaryInput in;
#pragma unroll
            for (int f = 0; f < F; ++f)
            {
                in.field_vals[f] = fv[f];
#pragma unroll
                for (int s = 0; s < 2; ++s)
                    in.field_ders[s][f] = Ji[0][s] * fd0[f] + Ji[1][s] * fd1[f];
            }
            in.point  = SpaceTimePoint{Point3{{xy[0], xy[1], 0.}}, time};
            in.normal = {{nrm[0], nrm[1]}};
            kern(in, res);
        }
        else
        {
            const int    qx = q % NQ, qy = q / NQ;
            const double det = quadGeom(vv, qp[qx], qp[qy], Ji, xy);
            wgt              = qw[qx] * qw[qy] * det;
            if (!(det > 0.))
            {
                *degenerate = 1.; // (Encountered degenerate element, algsys/AssembleLocalSystem.hpp:249)
                wgt         = 0.;
            }
            res = quadKernelAt< K, R >(kern, Ji, xy, time, fv, fd0, fd1);
        }
        const double  sw = sqrt(wgt);
        double* const c  = coef + q * CS;
#pragma unroll
        for (int eq = 0; eq < E; ++eq)
        {
#pragma unroll
            for (int u = 0; u < U; ++u)
            {
                c[(0 * E + eq) * U + u] = sw * res.operators[0](eq, u);
                c[(1 * E + eq) * U + u] = sw * (res.operators[1](eq, u) * Ji[0][0] + res.operators[2](eq, u) * Ji[0][1]);
                c[(2 * E + eq) * U + u] = sw * (res.operators[1](eq, u) * Ji[1][0] + res.operators[2](eq, u) * Ji[1][1]);
            }
#pragma unroll
            for (int r = 0; r < R; ++r)
                c[3 * E * U + eq * R + r] = sw * res.rhs(eq, r);
        }
    }
    __syncthreads();

    // B_q[:, (a, .)] of node a at point q from the point's record
    const auto bAt = [&](int q, int ax, int ay, double (&B)[E][U]) {
        const int    cx = colX(q) * N1 + ax, cy = colY(q) * N1 + ay;
        const double v = tval[cx] * tval[cy], d0 = tder[cx] * tval[cy], d1 = tval[cx] * tder[cy];
        const double* const c = coef + q * CS;
#pragma unroll
        for (int eq = 0; eq < E; ++eq)
#pragma unroll
            for (int u = 0; u < U; ++u)
                B[eq][u] = c[(0 * E + eq) * U + u] * v + c[(1 * E + eq) * U + u] * d0 + c[(2 * E + eq) * U + u] * d1;
    };

    // ---- phase 2: the lower triangle, tile by tile
    if (Kout)
        for (int a0 = 0; a0 < NN; a0 += TN)
        {
            const int tn  = a0 + TN <= NN ? TN : NN - a0; // row nodes of this tile
            const int ncn = a0 + tn;                       // column nodes up to the tile's end
            for (int idx = tid; idx < tn * ncn; idx += NT)
            {
                const int ar = idx / ncn, b = idx - ar * ncn, a = a0 + ar;
                if (b > a)
                    continue;
                const int ax = a % N1, ay = a / N1, bx = b % N1, by = b / N1;
                double    acc[U][U];
#pragma unroll
                for (int u = 0; u < U; ++u)
#pragma unroll
                    for (int v = 0; v < U; ++v)
                        acc[u][v] = 0.;
                for (int q = 0; q < NPTS; ++q)
                {
                    double Ba[E][U], Bb[E][U];
                    bAt(q, ax, ay, Ba);
                    bAt(q, bx, by, Bb);
#pragma unroll
                    for (int u = 0; u < U; ++u)
#pragma unroll
                        for (int v = 0; v < U; ++v)
#pragma unroll
                            for (int eq = 0; eq < E; ++eq)
                                acc[u][v] += Ba[eq][u] * Bb[eq][v];
                }
#pragma unroll
                for (int u = 0; u < U; ++u)
#pragma unroll
                    for (int v = 0; v < U; ++v) // (the diagonal block: one of the two equal sums for both places)
                        tile[(ar * U + u) * LD + b * U + v] = (a == b && v > u) ? acc[v][u] : acc[u][v];
            }
            __syncthreads();
            const int row0 = a0 * U, rows = tn * U, ncols = ncn * U;
            // the tile's own rows, lanes along the columns; right of the diagonal: the mirror position inside the tile
            for (int t = tid; t < rows * ncols; t += NT)
            {
                const int r = t / ncols, c = t - r * ncols, i = row0 + r;
                Kout[int64_t(i) * Nd + c] = c > i ? tile[(c - row0) * LD + i] : tile[r * LD + c];
            }
            // its mirror image: the columns [row0, row0 + rows) of the rows above the tile
            for (int t = tid; t < row0 * rows; t += NT)
            {
                const int j = t / rows, r = t - j * rows;
                Kout[int64_t(j) * Nd + row0 + r] = tile[r * LD + j];
            }
            __syncthreads();
        }

    // ---- phase 3: F[r][(a, u)]
    if (Fout)
        for (int a = tid; a < NN; a += NT)
        {
            double acc[R][U];
#pragma unroll
            for (int r = 0; r < R; ++r)
#pragma unroll
                for (int u = 0; u < U; ++u)
                    acc[r][u] = 0.;
            for (int q = 0; q < NPTS; ++q)
            {
                double Ba[E][U];
                bAt(q, a % N1, a / N1, Ba);
                const double* const f = coef + q * CS + 3 * E * U;
#pragma unroll
                for (int r = 0; r < R; ++r)
#pragma unroll
                    for (int u = 0; u < U; ++u)
#pragma unroll
                        for (int eq = 0; eq < E; ++eq)
                            acc[r][u] += Ba[eq][u] * f[eq * R + r];
            }
#pragma unroll
            for (int r = 0; r < R; ++r)
#pragma unroll
                for (int u = 0; u < U; ++u)
                    Fout[r * Nd + a * U + u] = acc[r][u];
        }
}

// element systems of the elements [elem_begin, elem_begin + elem_count) into the slots elem_begin_out + 0, 1, ...
template < typename K, int P, int NQ, int R >
__global__ __launch_bounds__((QuadAsmCfg< K, P, NQ, R >::threads)) void quadAssembleKernel(const ElemArgs a, const K kern)
{
    constexpr int   NN = QuadAsmCfg< K, P, NQ, R >::NN, Nd = QuadAsmCfg< K, P, NQ, R >::Nd;
    const int64_t   e    = a.elem_begin + blockIdx.x;
    const int64_t   slot = a.elem_begin_out + blockIdx.x;
    quadAsmBody< K, P, NQ, R, false >(kern, a.elem_nodes + e * NN, a.elem_verts + e * 12, a.tables, a.fields, a.ldf, a.time, 0,
                                      a.K ? a.K + slot * int64_t(Nd) * Nd : nullptr, a.F ? a.F + slot * int64_t(R) * Nd : nullptr, a.workspace);
}
// side systems of the sides [face_begin, face_begin + face_count) of the list into the slots 0, 1, ... (the write mode of
// launchSideAssemble; SideAsmArgs::accumulate is refused by the launcher)
template < typename K, int P, int NQ, int R >
__global__ __launch_bounds__((QuadAsmCfg< K, P, NQ, R >::threads)) void quadSideAssembleKernel(const SideAsmArgs a, const K kern)
{
    constexpr int NN = QuadAsmCfg< K, P, NQ, R >::NN, Nd = QuadAsmCfg< K, P, NQ, R >::Nd;
    const int64_t f  = a.face_begin + blockIdx.x;
    const int64_t e  = a.face_elem[f];
    const int64_t slot = blockIdx.x;
    quadAsmBody< K, P, NQ, R, true >(kern, a.elem_nodes + e * NN, a.elem_verts + e * 12, a.tables, a.fields, a.ldf, a.time, a.face_side[f],
                                     a.K ? a.K + slot * int64_t(Nd) * Nd : nullptr, a.F ? a.F + slot * int64_t(R) * Nd : nullptr, nullptr);
}

template < typename K, int P, int NQ, int R >
int launchQuadAssemble(const ElemArgs& a, const void* kparam_blob, hipStream_t stream)
{
    using Cfg = QuadAsmCfg< K, P, NQ, R >;
    if (a.elem_count <= 0 || (!a.K && !a.F))
        return 0;
    if (a.elem_count > int64_t(0x7fffffff) || a.K_tiled || a.checksum)
    {
        setError("quad assembly: %s", a.elem_count > int64_t(0x7fffffff) ? "batch too large for one launch"
                                                                          : "row-major K_e only (no tiled layout, no checksum)");
        return -1;
    }
    return launchKernel("quadAssembleKernel", quadAssembleKernel< K, P, NQ, R >, dim3(static_cast< unsigned >(a.elem_count)),
                        dim3(Cfg::threads), Cfg::template ldsBytes< false >(), stream, a, functorFrom< K >(kparam_blob));
}
template < typename K, int P, int NQ, int R >
int launchQuadSideAssemble(const SideAsmArgs& a, const void* kparam_blob, hipStream_t stream)
{
    using Cfg = QuadAsmCfg< K, P, NQ, R >;
    if (a.face_count <= 0 || (!a.K && !a.F))
        return 0;
    if (a.face_count > int64_t(0x7fffffff) || a.accumulate)
    {
        setError("quad side assembly: %s", a.accumulate ? "no accumulate mode" : "batch too large for one launch");
        return -1;
    }
    return launchKernel("quadSideAssembleKernel", quadSideAssembleKernel< K, P, NQ, R >, dim3(static_cast< unsigned >(a.face_count)),
                        dim3(Cfg::threads), Cfg::template ldsBytes< true >(), stream, a, functorFrom< K >(kparam_blob));
}
// the assembly slot of a quad shape: nullptr where the working set of a workgroup exceeds the LDS (the entry points then refuse
// the shape: "no assembly launcher")
template < typename K, int P, int NQ, int R >
constexpr LaunchFn selectQuadAssemble()
{
    if constexpr (QuadAsmCfg< K, P, NQ, R >::template ldsBytes< false >() <= lds_limit_bytes)
        return &launchQuadAssemble< K, P, NQ, R >;
    else
        return nullptr;
}
template < typename K, int P, int NQ, int R >
constexpr SideAsmFn selectQuadSideAssemble()
{
    if constexpr (QuadAsmCfg< K, P, NQ, R >::template ldsBytes< true >() <= lds_limit_bytes)
        return &launchQuadSideAssemble< K, P, NQ, R >;
    else
        return nullptr;
}
} // namespace l3k::dev
#endif
