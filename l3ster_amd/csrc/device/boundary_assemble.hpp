// boundary_assemble.hpp -- local systems of boundary equation kernels on element sides (the assembled and condensed paths).
//
// Reference: assembleLocalSystem on a BoundaryElementView (algsys/AssembleLocalSystem.hpp:77-216), called from the boundary
// overload of assembleGlobalSystem (algsys/AssembleGlobalSystem.hpp:55-96): the local system of the WHOLE element from the side
// quadrature,
//   K_s[(b,u),(b',u')] = sum_q w_q jac_q sum_eq B_q[eq,(b,u)] B_q[eq,(b',u')],   F_s[(b,u),r] = sum_q w_q jac_q sum_eq B_q[eq,(b,u)] f_q[eq,r],
//   B_q[eq,(b,u)] = A0[eq][u] phi_b(q) + sum_s A_{s+1}[eq][u] dphi_b/dx_s(q)
// with the side quadrature, surface Jacobian, normal and point / time input of faceKernel (boundary.hpp).  Layouts are those of
// l3k_local_assemble: K_s row-major [Nd][Nd], F_s column-major [Nd][n_rhs], Nd = (p+1)^3 U; no Dirichlet lifting.
//
// Two kernels.
//   sideCoefKernel   one workgroup per side, one quadrature point per thread: geometry, the user's functor, and the record
//                    sqrt(w jac) * { A0, D_t1, D_t2, D_n [eq][u], f [eq][r] } of the point in HBM (D_d = sum_s A_{s+1} dxi_d/dx_s).
//                    The weight is folded in as its square root so that K[i][j] and K[j][i] are the SAME sequence of operations.
//   sideMatrixKernel one workgroup per (side, 64 x 64 tile of the lower triangle of K_s): a rank-(nq^2 E) update with a 4 x 4
//                    register block per thread.  The panels B[k][dof] of the tile's rows and columns are built in LDS from the 1-D
//                    tables, 32 (point, equation) pairs at a time: on a side the basis values and tangential derivatives live on
//                    the n^2 side nodes, the normal derivative on every node (phi_k'(+-1) along the normal line), so an entry is
//                    four products.  A chunk whose row or column panel is identically zero (kernels without derivative operators
//                    and nodes off the side) is skipped.  The tile leaves through LDS: rows of 64 consecutive doubles, and the
//                    mirror image of an off-diagonal tile the same way -- K_s is bitwise symmetric (diagonal tiles by the
//                    commutativity of the product) and bitwise reproducible (no atomics).
// Store modes: write (every entry of K_s, zeros included; output slot = position in the launch) and accumulate (K_e += K_s into
// the slot of the side's element).  Accumulating launches take the sides of one `round` only -- the r-th side of every element --
// so no two workgroups of a launch add into the same entries, and the launches of a stream order the sides of an element.
#ifndef L3K_DEVICE_BOUNDARY_ASSEMBLE_HPP
#define L3K_DEVICE_BOUNDARY_ASSEMBLE_HPP

#include "boundary.hpp"

namespace l3k::dev
{
template < typename K, int R >
constexpr int sideCoefDoubles()
{
    return 4 * K::params.n_equations * K::params.n_unknowns + K::params.n_equations * R;
}
template < typename K, int P, int NQ >
constexpr size_t sideCoefLdsDoubles()
{
    constexpr int F = K::params.n_fields, N1 = P + 1;
    return size_t(F) * N1 * N1 * N1 + 2 * size_t(F) * N1 * N1 + 4 * size_t(F) * NQ * NQ + 24;
}

template < typename K, int P, int NQ, int R >
__global__ __launch_bounds__(256) void sideCoefKernel(const SideAsmArgs a, const K kern)
{
    constexpr KernelParams params = K::params;
    constexpr int          U = params.n_unknowns, E = params.n_equations, F = params.n_fields;
    constexpr int          N1 = P + 1, NN = N1 * N1 * N1, N2 = N1 * N1, NQ2 = NQ * NQ, NT = 256;
    constexpr int          CS = sideCoefDoubles< K, R >();
    constexpr TableLayout  TL{N1, NQ};
    using Iface = KernelInterface< KernelParams{params.dimension, E, U, F, R} >;

    extern __shared__ double lds[];
    double* const            xs = lds;               // [F][NN]
    double* const            pv = xs + F * NN;       // [2][F][N2]
    double* const            q  = pv + 2 * F * N2;   // [4][F][NQ2]
    double* const            vs = q + 4 * F * NQ2;   // [8][3]

    const int      tid  = threadIdx.x;
    const int64_t  f    = a.face_begin + blockIdx.x;
    const int64_t  e    = a.face_elem[f];
    const int      side = a.face_side[f];
    const SideAxes sa   = sideAxes(side);
    const double*  qw   = a.tables + TL.offW();
    const double*  qp   = a.tables + TL.offX();

    if (tid < 24)
        vs[tid] = a.elem_verts[e * 24 + tid];
    if constexpr (F > 0)
    {
        // the external fields at the side quadrature points: value, d/dxi_t1, d/dxi_t2, d/dxi_n (as faceKernel)
        const uint32_t* en   = a.elem_nodes + e * NN;
        const double*   tabI = a.tables + TL.offI();
        const double*   tabD = a.tables + TL.offD();
        const double*   tabE = a.tables + TL.offE() + sa.upper * N1;
        const int       str[3] = {1, N1, N2};
        const int       st1 = str[sa.t1], st2 = str[sa.t2], stn = str[sa.n];
        const int       kface = sa.upper ? P : 0;
        for (int t = tid; t < NN * F; t += NT)
        {
            const int fl = t / NN, i = t - fl * NN;
            xs[fl * NN + i] = a.fields[en[i] + fl * a.ldf];
        }
        __syncthreads();
        for (int t = tid; t < F * N2; t += NT)
        {
            const int     op = t / N2, ij = t - op * N2, j = ij / N1, i = ij - j * N1;
            const double* col = xs + op * NN + i * st1 + j * st2;
            double        dn  = 0.;
#pragma unroll
            for (int k = 0; k < N1; ++k)
                dn += tabE[k] * col[k * stn];
            pv[op * N2 + ij]          = col[kface * stn];
            pv[F * N2 + op * N2 + ij] = dn;
        }
        __syncthreads();
        for (int t = tid; t < F * NQ2; t += NT)
        {
            const int     op = t / NQ2, ab = t - op * NQ2, qb = ab / NQ, qa = ab - qb * NQ;
            const double* p0 = pv + op * N2;
            const double* p1 = pv + F * N2 + op * N2;
            double        val = 0., d1 = 0., d2 = 0., dn = 0.;
            for (int j = 0; j < N1; ++j)
            {
                double s0 = 0., s1 = 0., sn = 0.;
#pragma unroll
                for (int i = 0; i < N1; ++i)
                {
                    const double Ia = tabI[i * NQ + qa];
                    s0 += Ia * p0[i + N1 * j];
                    s1 += tabD[i * NQ + qa] * p0[i + N1 * j];
                    sn += Ia * p1[i + N1 * j];
                }
                const double Ib = tabI[j * NQ + qb];
                val += Ib * s0;
                d1 += Ib * s1;
                d2 += tabD[j * NQ + qb] * s0;
                dn += Ib * sn;
            }
            q[(0 * F + op) * NQ2 + ab] = val;
            q[(1 * F + op) * NQ2 + ab] = d1;
            q[(2 * F + op) * NQ2 + ab] = d2;
            q[(3 * F + op) * NQ2 + ab] = dn;
        }
    }
    __syncthreads();

    // planes of q holding the derivative along reference axis 0, 1, 2
    const int pl0 = sa.n == 0 ? 3 : 1, pl1 = sa.n == 1 ? 3 : (sa.n == 0 ? 1 : 2), pl2 = sa.n == 2 ? 3 : 2;
    double*   out = a.coef + size_t(blockIdx.x) * NQ2 * CS;
    for (int qi = tid; qi < NQ2; qi += NT)
    {
        const int    qb = qi / NQ, qa = qi - qb * NQ;
        double       Jm[3][3], Ji[3][3], xyz[3], nrm[3];
        const double jac = sidePointGeom(vs, sa, qp[qa], qp[qb], Jm, Ji, xyz, nrm);
        const double sw  = sqrt(qw[qa] * qw[qb] * jac);
        typename Iface::BoundaryInput in;
#pragma unroll
        for (int fl = 0; fl < F; ++fl)
        {
            const double d0 = q[(pl0 * F + fl) * NQ2 + qi], d1 = q[(pl1 * F + fl) * NQ2 + qi], d2 = q[(pl2 * F + fl) * NQ2 + qi];
            in.field_vals[fl] = q[fl * NQ2 + qi];
#pragma unroll
            for (int s = 0; s < 3; ++s)
                in.field_ders[s][fl] = Ji[0][s] * d0 + Ji[1][s] * d1 + Ji[2][s] * d2;
        }
        in.point  = SpaceTimePoint{Point3{{xyz[0], xyz[1], xyz[2]}}, a.time};
        in.normal = {{nrm[0], nrm[1], nrm[2]}};
        typename Iface::Result res{};
        kern(in, res);
        double* c = out + qi * CS;
#pragma unroll
        for (int eq = 0; eq < E; ++eq)
        {
#pragma unroll
            for (int u = 0; u < U; ++u)
            {
                double Dm[3]; // reference-space operator blocks D_d = sum_s A_{s+1} Ji[d][s]
#pragma unroll
                for (int d = 0; d < 3; ++d)
                    Dm[d] = res.operators[1](eq, u) * Ji[d][0] + res.operators[2](eq, u) * Ji[d][1] + res.operators[3](eq, u) * Ji[d][2];
                // plane order: value, t1, t2, n
                c[(0 * E + eq) * U + u] = sw * res.operators[0](eq, u);
                c[(1 * E + eq) * U + u] = sw * (sa.n == 0 ? Dm[1] : Dm[0]);
                c[(2 * E + eq) * U + u] = sw * (sa.n == 2 ? Dm[1] : Dm[2]);
                c[(3 * E + eq) * U + u] = sw * (sa.n == 0 ? Dm[0] : (sa.n == 1 ? Dm[1] : Dm[2]));
            }
#pragma unroll
            for (int r = 0; r < R; ++r)
                c[4 * E * U + eq * R + r] = sw * res.rhs(eq, r);
        }
    }
}

inline constexpr int side_tile  = 64; // rows / columns of a tile of K_s
inline constexpr int side_chunk = 32; // (quadrature point, equation) pairs per panel chunk

// P, NQ: the shape; U, E, R: of the functor whose coefficient records a.coef holds (CS doubles per point)
template < int P, int NQ, int U, int E, int R >
__global__ __launch_bounds__(256) void sideMatrixKernel(const SideAsmArgs a)
{
    constexpr int         N1 = P + 1, N2 = N1 * N1, NN = N2 * N1, Nd = NN * U, NQ2 = NQ * NQ, KT = NQ2 * E;
    constexpr int         TS = side_tile, KC = side_chunk, NTL = (Nd + TS - 1) / TS, NPAIR = NTL * (NTL + 1) / 2;
    constexpr int         CS = 4 * E * U + E * R, CW = 4 * U + R, LD = TS + 1;
    constexpr TableLayout TL{N1, NQ};
    __shared__ double     tI[N1 * NQ], tD[N1 * NQ], tE[N1];
    __shared__ double     cf[KC * CW];                                       // the chunk's coefficients: [k][4][U] | [k][R]
    __shared__ double     pan[2 * KC * TS > TS * LD ? 2 * KC * TS : TS * LD]; // row panel | column panel [k][dof]; then the tile

    const int     tid   = threadIdx.x;
    const int     per   = a.K ? NPAIR : NTL; // workgroups per side (F only: one per row tile)
    const int64_t fl    = blockIdx.x / per;
    const int     pair  = int(blockIdx.x - fl * per);
    const int64_t f     = a.face_begin + fl;
    if (a.accumulate && a.face_rank[f] != a.round) // (uniform over the workgroup)
        return;
    int ti = pair, tj = 0;
    if (a.K)
    {
        ti = 0;
        while ((ti + 1) * (ti + 2) / 2 <= pair)
            ++ti;
        tj = pair - ti * (ti + 1) / 2;
    }
    const int64_t  slot = a.accumulate ? a.face_elem[f] - a.elem_base : fl;
    const SideAxes sa   = sideAxes(a.face_side[f]);
    const int      kface = sa.upper ? P : 0;
    const double*  cside = a.coef + size_t(fl) * NQ2 * CS;

    for (int t = tid; t < N1 * NQ; t += 256)
    {
        tI[t] = a.tables[TL.offI() + t];
        tD[t] = a.tables[TL.offD() + t];
    }
    if (tid < N1)
        tE[tid] = a.tables[TL.offE() + sa.upper * N1 + tid];

    // this thread's entry of the panels: dof l of the row (which == 0) or column (which == 1) tile, every second k
    const int  l = tid & 63, which = tid >> 7, sub = (tid >> 6) & 1;
    const int  dof   = (which ? tj : ti) * TS + l;
    const bool valid = dof < Nd;
    const int  b = valid ? dof / U : 0, u = valid ? dof - b * U : 0;
    const int  c3[3] = {b % N1, (b / N1) % N1, b / N2};
    const int  ci = sa.n == 0 ? c3[1] : c3[0], cj = sa.n == 2 ? c3[1] : c3[2], ck = sa.n == 0 ? c3[0] : (sa.n == 1 ? c3[1] : c3[2]);
    const bool on_side = ck == kface;
    double* const       Ar = pan;
    double* const       Bc = ti == tj ? pan : pan + KC * TS; // (a diagonal tile multiplies its row panel with itself)
    const int           ty = tid >> 4, tx = tid & 15;
    double              acc[4][4] = {};
    double              facc[R]   = {};
    bool                any       = false;
    __syncthreads();
    const double en = tE[ck];

#pragma unroll 1
    for (int k0 = 0; k0 < KT; k0 += KC)
    {
        const int kc = KT - k0 < KC ? KT - k0 : KC;
        __syncthreads(); // the previous chunk has been consumed
        for (int t = tid; t < kc * CW; t += 256)
        {
            const int k = t / CW, j = t - k * CW, qi = (k0 + k) / E, eq = (k0 + k) - qi * E;
            const double* c = cside + qi * CS;
            cf[t] = j < 4 * U ? c[((j / U) * E + eq) * U + (j % U)] : c[4 * E * U + eq * R + (j - 4 * U)];
        }
        __syncthreads();
        int nz = 0;
        for (int k = sub; k < kc; k += 2)
        {
            const int     qi = (k0 + k) / E, qb = qi / NQ, qa = qi - qb * NQ;
            const double  Ia = tI[ci * NQ + qa], Ib = tI[cj * NQ + qb];
            const double* c  = cf + k * CW + u;
            double        B  = c[3 * U] * (Ia * Ib * en);
            if (on_side)
                B += c[0] * (Ia * Ib) + c[U] * (tD[ci * NQ + qa] * Ib) + c[2 * U] * (Ia * tD[cj * NQ + qb]);
            if (!valid)
                B = 0.;
            nz |= B != 0.;
            pan[(which * KC + k) * TS + l] = B;
        }
        const int row_nz = __syncthreads_or(which == 0 && nz);
        const int col_nz = __syncthreads_or(which == 1 && nz);
        if (a.K && row_nz && (col_nz || ti == tj))
        {
            any = true;
            for (int k = 0; k < kc; ++k)
            {
                double ar[4], bc[4];
#pragma unroll
                for (int r = 0; r < 4; ++r)
                {
                    ar[r] = Ar[k * TS + ty * 4 + r];
                    bc[r] = Bc[k * TS + tx * 4 + r];
                }
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int c = 0; c < 4; ++c)
                        acc[r][c] = fma(ar[r], bc[c], acc[r][c]);
            }
        }
        if (a.F && tj == 0 && tid < TS && row_nz)
            for (int k = 0; k < kc; ++k)
#pragma unroll
                for (int r = 0; r < R; ++r)
                    facc[r] = fma(Ar[k * TS + tid], cf[k * CW + 4 * U + r], facc[r]);
    }
    if (a.F && tj == 0 && tid < TS && ti * TS + tid < Nd)
    {
        double* Fo = a.F + slot * int64_t(R) * Nd + ti * TS + tid;
#pragma unroll
        for (int r = 0; r < R; ++r)
            Fo[int64_t(r) * Nd] = a.accumulate ? Fo[int64_t(r) * Nd] + facc[r] : facc[r];
    }
    if (!a.K || (a.accumulate && !any)) // (uniform: `any` follows the workgroup-wide votes)
        return;
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c)
            pan[(ty * 4 + r) * LD + tx * 4 + c] = acc[r][c];
    __syncthreads();
    double* const Ko   = a.K + slot * int64_t(Nd) * Nd;
    const int     wv   = tid >> 6, lane = tid & 63;
    const int     i0 = ti * TS, j0 = tj * TS;
    for (int rr = wv; rr < TS; rr += 4)
        if (i0 + rr < Nd && j0 + lane < Nd)
        {
            double* o = Ko + int64_t(i0 + rr) * Nd + j0 + lane;
            *o        = a.accumulate ? *o + pan[rr * LD + lane] : pan[rr * LD + lane];
        }
    if (ti != tj) // the mirror image
        for (int cc = wv; cc < TS; cc += 4)
            if (j0 + cc < Nd && i0 + lane < Nd)
            {
                double* o = Ko + int64_t(j0 + cc) * Nd + i0 + lane;
                *o        = a.accumulate ? *o + pan[lane * LD + cc] : pan[lane * LD + cc];
            }
}

template < typename K, int P, int NQ, int R >
int launchSideAssemble(const SideAsmArgs& a, const void* kparam_blob, hipStream_t stream)
{
    if (a.face_count <= 0 || (!a.K && !a.F))
        return 0;
    constexpr int U = K::params.n_unknowns, E = K::params.n_equations, N1 = P + 1, Nd = N1 * N1 * N1 * U;
    constexpr int NTL = (Nd + side_tile - 1) / side_tile, NPAIR = NTL * (NTL + 1) / 2;
    const int64_t grid = a.face_count * (a.K ? NPAIR : NTL);
    if (grid > int64_t(0x7fffffff))
    {
        setError("batch too large: %lld side-matrix tiles in one launch", (long long)grid);
        return -1;
    }
    if (a.round == 0)
    {
        constexpr size_t lds = sizeof(double) * sideCoefLdsDoubles< K, P, NQ >();
        static_assert(lds <= lds_limit_bytes, "side working set exceeds 160 KiB of LDS");
        if (int rc = launchKernel("sideCoefKernel", sideCoefKernel< K, P, NQ, R >, dim3(static_cast< unsigned >(a.face_count)), dim3(256), lds,
                                  stream, a, functorFrom< K >(kparam_blob)))
            return rc;
    }
    return launchKernel("sideMatrixKernel", sideMatrixKernel< P, NQ, U, E, R >, dim3(static_cast< unsigned >(grid)), dim3(256), 0, stream, a);
}
// coefficient doubles per side of launchSideAssemble< K, P, NQ, R >
template < typename K, int NQ, int R >
constexpr size_t sideAssembleWorkspaceDoubles()
{
    return size_t(NQ) * NQ * sideCoefDoubles< K, R >();
}
} // namespace l3k::dev
#endif
