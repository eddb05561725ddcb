// quad_boundary.hpp -- boundary equation kernels, integrals and values at nodes on bilinear quadrilaterals (dim = 2).
//
// The 2-D counterparts of boundary.hpp and integral.hpp.  A quad side is a line: the basis values at a side point are those of
// the p+1 side nodes, the tangential derivative acts along the side, and the normal derivative is one contraction of the
// (p+1)^2 nodal values with phi_k'(+-1).  Side geometry as in mapping/BoundaryIntegralJacobian.hpp and
// mapping/BoundaryNormal.hpp for dim = 2: line jacobian |dx/dxi_t|, outward unit normal from the rotated tangent.
//
// Organisation as in quad.hpp: one wave per side (or element), quadWaves() of them per workgroup, wave-private LDS, no
// workgroup barrier.  Surface work (O(1/ne) of the apply) and post-processing, so written for clarity.  Integrals write one
// set of E partial sums per side / element, reduced in a fixed order here and by reducePartialsKernel (api_post.hip).
#ifndef L3K_DEVICE_QUAD_BOUNDARY_HPP
#define L3K_DEVICE_QUAD_BOUNDARY_HPP

#include "quad.hpp"

namespace l3k::dev
{
// side s of a quad (mesh/ElementTraits.hpp): 0 y- (eta = -1), 1 y+ (eta = +1), 2 x- (xi = -1), 3 x+ (xi = +1)
struct QuadSide
{
    int    n, t;  // normal and tangential reference axis
    int    upper; // side at xi_n = +1
    double nsign; // outward normal = nsign * (t_y, -t_x) / |t|, t = dx/dxi_t
};
__device__ __forceinline__ QuadSide quadSide(int side)
{
    QuadSide s;
    s.upper = side & 1;
    s.n     = side < 2 ? 1 : 0;
    s.t     = 1 - s.n;
    s.nsign = (side == 0 || side == 3) ? 1. : -1.;
    return s;
}

// geometry at the point of side `qs` with tangential reference coordinate c: J^-1, the point, the outward unit normal;
// returns the line jacobian |dx/dxi_t|
__device__ __forceinline__ double quadSideGeom(const double* __restrict__ vs, const QuadSide& qs, double c, double Ji[2][2], double xy[2],
                                               double nrm[2])
{
    const double cn = qs.upper ? 1. : -1.;
    const double xi = qs.n == 0 ? cn : c, eta = qs.n == 1 ? cn : c;
    quadGeom(vs, xi, eta, Ji, xy);
    double tg[2];
#pragma unroll
    for (int s = 0; s < 2; ++s)
    {
        const double c0 = vs[0 * 3 + s], c1 = vs[1 * 3 + s], c2 = vs[2 * 3 + s], c3 = vs[3 * 3 + s];
        tg[s] = qs.t == 0 ? .25 * ((1. - eta) * (c1 - c0) + (1. + eta) * (c3 - c2)) : .25 * ((1. - xi) * (c2 - c0) + (1. + xi) * (c3 - c1));
    }
    const double len = sqrt(tg[0] * tg[0] + tg[1] * tg[1]);
    nrm[0]           = qs.nsign * tg[1] / len;
    nrm[1]           = -qs.nsign * tg[0] / len;
    return len;
}

// fixed-order sum over the lanes of one wave: out[v] = sum_lane vals[v]   (red: NV x quad_wave doubles of the wave's LDS)
template < int NV >
__device__ __forceinline__ void waveReduceStore(const double (&vals)[NV], double* red, double* out, int lane)
{
#pragma unroll
    for (int v = 0; v < NV; ++v)
        red[v * quad_wave + lane] = vals[v];
    stageFence();
    for (int v = lane; v < NV; v += quad_wave)
    {
        double s = 0.;
        for (int l = 0; l < quad_wave; ++l)
            s += red[v * quad_wave + l];
        out[v] = s;
    }
}

// ------------------------------------------------------------------------------------------------ boundary equation kernels
// bytes of LDS per side: nodal values, the side-node values and normal contraction, 3 planes at the side points, the vertices,
// and in RHS_MODE the per-point coefficient record of the diagonal
template < typename K, int P, int NQ, int R, bool RHS_MODE >
constexpr size_t quadSideBytes()
{
    constexpr int U = K::params.n_unknowns, E = K::params.n_equations, NF = U * R + K::params.n_fields, N1 = P + 1;
    return sizeof(double) * (size_t(NF) * (N1 * N1 + 2 * N1 + 3 * NQ) + 12 + (RHS_MODE ? size_t(NQ) * (1 + 3 * E * U) : 0));
}

// RHS_MODE == false: y += alpha * A_b x (Dirichlet dofs read as 0 and skipped in the scatter);
// RHS_MODE == true: rhs += B_b^T W (f_b - B_b g), diag += diag(A_b) where a.diag is set.  R columns in one pass.
template < typename K, int P, int NQ, int R, bool RHS_MODE >
__global__ __launch_bounds__(quad_wave * quadWaves(quadSideBytes< K, P, NQ, R, RHS_MODE >())) void quadSideKernel(const ElemArgs a, const K kern)
{
    constexpr KernelParams params = K::params;
    constexpr int          U = params.n_unknowns, E = params.n_equations, F = params.n_fields, OPS = U * R, NF = OPS + F;
    constexpr int          N1 = P + 1, NN = N1 * N1, NT = quad_wave, CS = 1 + 3 * E * U;
    constexpr size_t       side_doubles = quadSideBytes< K, P, NQ, R, RHS_MODE >() / sizeof(double);
    constexpr TableLayout  TL{N1, NQ};
    using Iface = KernelInterface< KernelParams{2, E, U, F, R} >;

    extern __shared__ double lds[];
    const int     wave = threadIdx.x / NT, lane = threadIdx.x % NT;
    const int64_t sb   = int64_t(blockIdx.x) * (blockDim.x / NT) + wave;
    if (sb >= a.face_count) // (no workgroup barrier below)
        return;
    double* const xs   = lds + size_t(wave) * side_doubles; // [NF][NN] nodal values
    double* const sv   = xs + NF * NN;                      // [NF][N1] values at the side nodes, then the result through them
    double* const sd   = sv + NF * N1;                      // [NF][N1] sum_k phi_k'(+-1) x(i, k), then the result through it
    double* const qv   = sd + NF * N1;                      // [3][NF][NQ] value, d/dxi_t, d/dxi_n at the points, then r0, r_t, r_n
    double* const vv   = qv + 3 * NF * NQ;                  // [4][3]
    double* const coef = vv + 12;                           // [NQ][CS] (RHS_MODE)

    const int64_t   f     = a.face_begin + sb;
    const int64_t   e     = a.face_elem[f];
    const QuadSide  qs    = quadSide(a.face_side[f]);
    const uint32_t* en    = a.elem_nodes + e * NN;
    const double*   tabI  = a.tables + TL.offI();
    const double*   tabD  = a.tables + TL.offD();
    const double*   tabE  = a.tables + TL.offE() + qs.upper * N1; // phi_k'(+-1)
    const double*   qw    = a.tables + TL.offW();
    const double*   qp    = a.tables + TL.offX();
    const int       st    = qs.t == 0 ? 1 : N1, sn = qs.n == 0 ? 1 : N1;
    const int       kface = qs.upper ? P : 0;

    if (lane < 12)
        vv[lane] = a.elem_verts[e * 12 + lane];
    // ---- gather (as quadApplyKernel)
    for (int t = lane; t < NN * U; t += NT)
    {
        const int     i   = t / U;
        const int     u   = t - i * U;
        const int64_t dof = int64_t(en[i]) * a.dofs_per_node + a.field_inds[u];
        const bool    dir = a.dirichlet != nullptr && a.dirichlet[dof] != 0;
#pragma unroll
        for (int r = 0; r < R; ++r)
        {
            double val;
            if constexpr (RHS_MODE)
                val = (dir && a.dirichlet_vals) ? a.dirichlet_vals[dof + a.ldg * r] : 0.;
            else
                val = dir ? 0. : (dof < a.n_owned_dofs ? a.x[dof + a.ldx * r] : a.xg[(dof - a.n_owned_dofs) + a.ldxg * r]);
            xs[(r * U + u) * NN + i] = val;
        }
    }
    if constexpr (F > 0)
        for (int t = lane; t < NN * F; t += NT)
        {
            const int fl = t / NN, i = t - fl * NN;
            xs[(OPS + fl) * NN + i] = a.fields[en[i] + fl * a.ldf];
        }
    stageFence();

    // ---- values at the side nodes and the normal contraction (i along the side)
    for (int t = lane; t < NF * N1; t += NT)
    {
        const int     op  = t / N1, i = t - op * N1;
        const double* col = xs + op * NN + i * st;
        double        dn  = 0.;
#pragma unroll
        for (int k = 0; k < N1; ++k)
            dn += tabE[k] * col[k * sn];
        sv[t] = col[kface * sn];
        sd[t] = dn;
    }
    stageFence();
    // ---- to the side points: value, d/dxi_t, d/dxi_n
    for (int t = lane; t < NF * NQ; t += NT)
    {
        const int op = t / NQ, q = t - op * NQ;
        double    v = 0., dt = 0., dn = 0.;
#pragma unroll
        for (int i = 0; i < N1; ++i)
        {
            v += tabI[i * NQ + q] * sv[op * N1 + i];
            dt += tabD[i * NQ + q] * sv[op * N1 + i];
            dn += tabI[i * NQ + q] * sd[op * N1 + i];
        }
        qv[(0 * NF + op) * NQ + q] = v;
        qv[(1 * NF + op) * NQ + q] = dt;
        qv[(2 * NF + op) * NQ + q] = dn;
    }
    stageFence();

    // planes of qv holding the derivative along reference axis 0 (xi) and 1 (eta)
    const int pl0 = qs.t == 0 ? 1 : 2, pl1 = 3 - pl0;
    // ---- side points, one per lane
    for (int q = lane; q < NQ; q += NT)
    {
        double       Ji[2][2], xy[2], nrm[2];
        const double wgt = qw[q] * quadSideGeom(vv, qs, qp[q], Ji, xy, nrm);
        typename Iface::BoundaryInput in;
#pragma unroll
        for (int fl = 0; fl < F; ++fl)
        {
            const double d0 = qv[(pl0 * NF + OPS + fl) * NQ + q], d1 = qv[(pl1 * NF + OPS + fl) * NQ + q];
            in.field_vals[fl] = qv[(0 * NF + OPS + fl) * NQ + q];
#pragma unroll
            for (int s = 0; s < 2; ++s)
                in.field_ders[s][fl] = Ji[0][s] * d0 + Ji[1][s] * d1;
        }
        in.point  = SpaceTimePoint{Point3{{xy[0], xy[1], 0.}}, a.time};
        in.normal = {{nrm[0], nrm[1]}};
        typename Iface::Result res{};
        kern(in, res);
        // reference-space operator blocks D_d = sum_s A_{s+1} Ji[d][s]
        double Dm[2][E][U];
#pragma unroll
        for (int d = 0; d < 2; ++d)
#pragma unroll
            for (int eq = 0; eq < E; ++eq)
#pragma unroll
                for (int u = 0; u < U; ++u)
                    Dm[d][eq][u] = res.operators[1](eq, u) * Ji[d][0] + res.operators[2](eq, u) * Ji[d][1];
        double r0[OPS], rd[2][OPS];
#pragma unroll
        for (int r = 0; r < R; ++r)
        {
            double tq[E];
#pragma unroll
            for (int eq = 0; eq < E; ++eq)
            {
                double acc = 0.;
#pragma unroll
                for (int u = 0; u < U; ++u)
                {
                    const int o = r * U + u;
                    acc += res.operators[0](eq, u) * qv[(0 * NF + o) * NQ + q] + Dm[0][eq][u] * qv[(pl0 * NF + o) * NQ + q] +
                           Dm[1][eq][u] * qv[(pl1 * NF + o) * NQ + q];
                }
                tq[eq] = RHS_MODE ? wgt * (res.rhs(eq, r) - acc) : wgt * acc;
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
            {
                double a0 = 0., a1 = 0., a2 = 0.;
#pragma unroll
                for (int eq = 0; eq < E; ++eq)
                {
                    a0 += res.operators[0](eq, u) * tq[eq];
                    a1 += Dm[0][eq][u] * tq[eq];
                    a2 += Dm[1][eq][u] * tq[eq];
                }
                r0[r * U + u]    = a0;
                rd[0][r * U + u] = a1;
                rd[1][r * U + u] = a2;
            }
        }
#pragma unroll
        for (int o = 0; o < OPS; ++o)
        {
            qv[(0 * NF + o) * NQ + q]   = r0[o];
            qv[(pl0 * NF + o) * NQ + q] = rd[0][o];
            qv[(pl1 * NF + o) * NQ + q] = rd[1][o];
        }
        if constexpr (RHS_MODE)
        {
            double* c = coef + q * CS;
            c[0]      = wgt;
#pragma unroll
            for (int eq = 0; eq < E; ++eq)
#pragma unroll
                for (int u = 0; u < U; ++u)
                {
                    // plane order: value, t, n
                    c[1 + (0 * E + eq) * U + u] = res.operators[0](eq, u);
                    c[1 + (1 * E + eq) * U + u] = Dm[qs.t][eq][u];
                    c[1 + (2 * E + eq) * U + u] = Dm[qs.n][eq][u];
                }
        }
    }
    stageFence();

    // ---- transposed: back to the side nodes (sv: through their values and tangential derivatives, sd: through phi_k'(+-1))
    for (int t = lane; t < OPS * N1; t += NT)
    {
        const int op = t / N1, i = t - op * N1;
        double    w0 = 0., w1 = 0.;
#pragma unroll
        for (int q = 0; q < NQ; ++q)
        {
            w0 += tabI[i * NQ + q] * qv[(0 * NF + op) * NQ + q] + tabD[i * NQ + q] * qv[(1 * NF + op) * NQ + q];
            w1 += tabI[i * NQ + q] * qv[(2 * NF + op) * NQ + q];
        }
        sv[t] = w0;
        sd[t] = w1;
    }
    stageFence();

    // ---- scatter-add over all (p+1)^2 nodes (the normal derivative couples every node of the element)
    for (int t = lane; t < NN * U; t += NT)
    {
        const int     i    = t / U;
        const int     u    = t - i * U;
        const int     c[2] = {i % N1, i / N1};
        const int     ct = c[qs.t], ck = c[qs.n];
        const int64_t dof  = int64_t(en[i]) * a.dofs_per_node + a.field_inds[u];
        const bool    dir  = !RHS_MODE && a.dirichlet != nullptr && a.dirichlet[dof] != 0;
        if (!dir)
        {
#pragma unroll
            for (int r = 0; r < R; ++r)
            {
                const int    op  = r * U + u;
                const double val = (ck == kface ? sv[op * N1 + ct] : 0.) + tabE[ck] * sd[op * N1 + ct];
                double* dst = dof < a.n_owned_dofs ? a.y + dof + a.ldy * r : a.yg + (dof - a.n_owned_dofs) + a.ldyg * r;
                unsafeAtomicAdd(dst, (RHS_MODE ? 1. : a.alpha) * val);
            }
        }
        if constexpr (RHS_MODE)
            if (a.diag)
            {
                // diag(A_b)[node, u] = sum_q w jac sum_eq (B_q[eq, (node, u)])^2
                double dsum = 0.;
                for (int q = 0; q < NQ; ++q)
                {
                    const double* cf = coef + q * CS;
                    const double  bv = ck == kface ? tabI[ct * NQ + q] : 0.;
                    const double  bt = ck == kface ? tabD[ct * NQ + q] : 0.;
                    const double  bn = tabI[ct * NQ + q] * tabE[ck];
                    double        sq = 0.;
#pragma unroll
                    for (int eq = 0; eq < E; ++eq)
                    {
                        const double B = cf[1 + (0 * E + eq) * U + u] * bv + cf[1 + (1 * E + eq) * U + u] * bt +
                                         cf[1 + (2 * E + eq) * U + u] * bn;
                        sq += B * B;
                    }
                    dsum += cf[0] * sq;
                }
                double* dd = dof < a.n_owned_dofs ? a.diag + dof : a.diag_g + (dof - a.n_owned_dofs);
                unsafeAtomicAdd(dd, dsum);
            }
    }
}

template < typename K, int P, int NQ, int R, bool RHS_MODE >
int launchQuadSide(const ElemArgs& a, const void* kparam_blob, hipStream_t stream)
{
    if (a.face_count <= 0)
        return 0;
    constexpr size_t sb = quadSideBytes< K, P, NQ, R, RHS_MODE >();
    constexpr int    W  = quadWaves(sb);
    static_assert(sb * W <= lds_limit_bytes, "quad side working set exceeds the LDS");
    const unsigned grid = static_cast< unsigned >((a.face_count + W - 1) / W);
    return launchKernel("quadSideKernel", quadSideKernel< K, P, NQ, R, RHS_MODE >, dim3(grid), dim3(quad_wave * W), sb * W, stream, a,
                        functorFrom< K >(kparam_blob));
}

// ------------------------------------------------------------------------------------------------ integrals
// bytes of LDS per element (4 buffers of F x max(p+1, nq)^2: nodal values, sweep temporary, values, d/dxi; d/deta reuses the
// temporary) or per side (nodal values, side-node values and normal contraction); + the vertices and the reduction buffer
template < typename K, int P, int NQ, bool SIDE >
constexpr size_t quadIntegralBytes()
{
    constexpr int FA = K::params.n_fields > 0 ? K::params.n_fields : 1, E = K::params.n_equations, N1 = P + 1, M = cmax(N1, NQ);
    return sizeof(double) * ((SIDE ? size_t(FA) * (N1 * N1 + 2 * N1) : 4 * size_t(FA) * M * M) + 12 + size_t(E) * quad_wave);
}

// the integral (a.square: of the square) of a residual kernel over one element (SIDE false) or one element side per wave;
// writes the E sums of the wave's element / side to a.partial[position in the launch]
template < typename K, int P, int NQ, bool SIDE >
__global__ __launch_bounds__(quad_wave * quadWaves(quadIntegralBytes< K, P, NQ, SIDE >())) void quadIntegralKernel(const ElemArgs a, const K kern)
{
    constexpr KernelParams params = K::params;
    constexpr int          E = params.n_equations, F = params.n_fields, FA = F > 0 ? F : 1;
    constexpr int          N1 = P + 1, NN = N1 * N1, M = cmax(N1, NQ), M2 = M * M, NT = quad_wave;
    constexpr size_t       wave_doubles = quadIntegralBytes< K, P, NQ, SIDE >() / sizeof(double);
    constexpr TableLayout  TL{N1, NQ};
    using Iface = KernelInterface< params >;

    extern __shared__ double lds[];
    const int     wave = threadIdx.x / NT, lane = threadIdx.x % NT;
    const int64_t sb   = int64_t(blockIdx.x) * (blockDim.x / NT) + wave;
    if (sb >= (SIDE ? a.face_count : a.elem_count))
        return;
    double* const xs  = lds + size_t(wave) * wave_doubles;                  // [F][NN] (domain: [F][M2]) nodal values
    double* const vv  = xs + (SIDE ? FA * (NN + 2 * N1) : 4 * FA * M2);     // [4][3]
    double* const red = vv + 12;                                            // [E][NT]

    const int64_t   f    = SIDE ? a.face_begin + sb : 0;
    const int64_t   e    = SIDE ? a.face_elem[f] : a.elem_begin + sb;
    const uint32_t* en   = a.elem_nodes + e * NN;
    const double*   tabI = a.tables + TL.offI();
    const double*   qw   = a.tables + TL.offW();
    const double*   qp   = a.tables + TL.offX();
    if (lane < 12)
        vv[lane] = a.elem_verts[e * 12 + lane];
    for (int t = lane; t < NN * F; t += NT) // FieldAccess::fill, post/FieldAccess.hpp:21-30
    {
        const int fl = t / NN, i = t - fl * NN;
        xs[fl * (SIDE ? NN : M2) + i] = a.fields[en[i] + fl * a.ldf];
    }
    stageFence();

    double acc[E];
#pragma unroll
    for (int i = 0; i < E; ++i)
        acc[i] = 0.;
    if constexpr (SIDE)
    {
        const QuadSide qs    = quadSide(a.face_side[f]);
        const double*  tabD  = a.tables + TL.offD();
        const double*  tabE  = a.tables + TL.offE() + qs.upper * N1;
        const int      st    = qs.t == 0 ? 1 : N1, sn = qs.n == 0 ? 1 : N1;
        const int      kface = qs.upper ? P : 0;
        double* const  sv    = xs + FA * NN; // [F][N1] side-node values
        double* const  sd    = sv + FA * N1; // [F][N1] normal contraction
        for (int t = lane; t < F * N1; t += NT)
        {
            const int     fl  = t / N1, i = t - fl * N1;
            const double* col = xs + fl * NN + i * st;
            double        dn  = 0.;
#pragma unroll
            for (int k = 0; k < N1; ++k)
                dn += tabE[k] * col[k * sn];
            sv[t] = col[kface * sn];
            sd[t] = dn;
        }
        stageFence();
        for (int q = lane; q < NQ; q += NT)
        {
            double       Ji[2][2], xy[2], nrm[2];
            const double wgt = qw[q] * quadSideGeom(vv, qs, qp[q], Ji, xy, nrm);
            typename Iface::BoundaryInput in;
#pragma unroll
            for (int fl = 0; fl < F; ++fl)
            {
                double v = 0., dt = 0., dn = 0.;
#pragma unroll
                for (int i = 0; i < N1; ++i)
                {
                    v += tabI[i * NQ + q] * sv[fl * N1 + i];
                    dt += tabD[i * NQ + q] * sv[fl * N1 + i];
                    dn += tabI[i * NQ + q] * sd[fl * N1 + i];
                }
                const double d0 = qs.t == 0 ? dt : dn, d1 = qs.t == 0 ? dn : dt;
                in.field_vals[fl] = v;
#pragma unroll
                for (int s = 0; s < 2; ++s)
                    in.field_ders[s][fl] = Ji[0][s] * d0 + Ji[1][s] * d1;
            }
            in.point  = SpaceTimePoint{Point3{{xy[0], xy[1], 0.}}, a.time};
            in.normal = {{nrm[0], nrm[1]}};
            typename Iface::Rhs out{};
            kern(in, out);
#pragma unroll
            for (int i = 0; i < E; ++i)
                acc[i] += wgt * (a.square ? out[i] * out[i] : out[i]);
        }
    }
    else
    {
        double* const B1 = xs + FA * M2; // sweep temporary, then d/deta
        double* const V  = B1 + FA * M2; // values at the points
        double* const D0 = V + FA * M2;  // d/dxi at the points
        if constexpr (F > 0)
        {
            const double* tabC = a.tables + TL.offC();
            sweep< 0, N1, NQ, false, false, N1, N1, 1, F, NT >(xs, B1, M2, tabI, lane); // -> (NQ, N1)
            stageFence();
            sweep< 1, N1, NQ, false, false, NQ, N1, 1, F, NT >(B1, V, M2, tabI, lane); // -> (NQ, NQ)
            stageFence();
            sweep< 0, NQ, NQ, false, false, NQ, NQ, 1, F, NT >(V, D0, M2, tabC, lane);
            sweep< 1, NQ, NQ, false, false, NQ, NQ, 1, F, NT >(V, B1, M2, tabC, lane);
            stageFence();
        }
        for (int q = lane; q < NQ * NQ; q += NT)
        {
            const int    qx = q % NQ, qy = q / NQ;
            double       Ji[2][2], xy[2];
            const double wgt = qw[qx] * qw[qy] * quadGeom(vv, qp[qx], qp[qy], Ji, xy);
            typename Iface::DomainInput in;
#pragma unroll
            for (int fl = 0; fl < F; ++fl)
            {
                const double d0 = D0[fl * M2 + q], d1 = B1[fl * M2 + q];
                in.field_vals[fl] = V[fl * M2 + q];
#pragma unroll
                for (int s = 0; s < 2; ++s)
                    in.field_ders[s][fl] = Ji[0][s] * d0 + Ji[1][s] * d1;
            }
            in.point = SpaceTimePoint{Point3{{xy[0], xy[1], 0.}}, a.time};
            typename Iface::Rhs out{};
            kern(in, out);
#pragma unroll
            for (int i = 0; i < E; ++i)
                acc[i] += wgt * (a.square ? out[i] * out[i] : out[i]);
        }
    }
    waveReduceStore< E >(acc, red, a.partial + sb * E, lane);
}

template < typename K, int P, int NQ, bool SIDE >
int launchQuadIntegral(const ElemArgs& a, const void* kparam_blob, hipStream_t stream)
{
    const int64_t count = SIDE ? a.face_count : a.elem_count;
    if (count <= 0)
        return 0;
    constexpr size_t wb = quadIntegralBytes< K, P, NQ, SIDE >();
    constexpr int    W  = quadWaves(wb);
    static_assert(wb * W <= lds_limit_bytes, "quad integral working set exceeds the LDS");
    const unsigned grid = static_cast< unsigned >((count + W - 1) / W);
    return launchKernel("quadIntegralKernel", quadIntegralKernel< K, P, NQ, SIDE >, dim3(grid), dim3(quad_wave * W), wb * W, stream, a,
                        functorFrom< K >(kparam_blob));
}

// ------------------------------------------------------------------------------------------------ values at nodes
// computeValuesAtNodes on quads (as valuesAtNodesKernel): the residual kernel evaluated at the GLL nodes of one element side
// (SIDE) or of one element per wave, field derivatives from the GLL differentiation matrix; equation e accumulates into dof
// field_inds[e] of the node together with a contribution count
template < typename K, int P >
constexpr size_t quadAtNodesBytes()
{
    constexpr int FA = K::params.n_fields > 0 ? K::params.n_fields : 1;
    return sizeof(double) * (size_t(FA) * (P + 1) * (P + 1) + 12);
}

template < typename K, int P, int NQ, bool SIDE >
__global__ __launch_bounds__(quad_wave * quadWaves(quadAtNodesBytes< K, P >())) void quadValuesAtNodesKernel(const ElemArgs a, const K kern)
{
    constexpr KernelParams params = K::params;
    constexpr int          E = params.n_equations, F = params.n_fields, FA = F > 0 ? F : 1;
    constexpr int          N1 = P + 1, NN = N1 * N1, NT = quad_wave;
    constexpr TableLayout  TL{N1, NQ};
    using Iface = KernelInterface< params >;

    extern __shared__ double lds[];
    const int     wave = threadIdx.x / NT, lane = threadIdx.x % NT;
    const int64_t sb   = int64_t(blockIdx.x) * (blockDim.x / NT) + wave;
    if (sb >= (SIDE ? a.face_count : a.elem_count))
        return;
    double* const xs = lds + size_t(wave) * (quadAtNodesBytes< K, P >() / sizeof(double)); // [F][NN]
    double* const vv = xs + FA * NN;                                                         // [4][3]

    const int64_t   f    = SIDE ? a.face_begin + sb : 0;
    const int64_t   e    = SIDE ? a.face_elem[f] : a.elem_begin + sb;
    const QuadSide  qs   = quadSide(SIDE ? a.face_side[f] : 0);
    const uint32_t* en   = a.elem_nodes + e * NN;
    const double*   gll  = a.tables + TL.offG();
    const double*   tabG = a.tables + TL.offDG();
    if (lane < 12)
        vv[lane] = a.elem_verts[e * 12 + lane];
    for (int t = lane; t < NN * F; t += NT)
    {
        const int fl = t / NN, i = t - fl * NN;
        xs[fl * NN + i] = a.fields[en[i] + fl * a.ldf];
    }
    stageFence();
    const int str[2] = {1, N1};
    for (int t = lane; t < (SIDE ? N1 : NN); t += NT)
    {
        int c[2];
        if constexpr (SIDE) // getSideNodeInds: the normal coordinate sits at the side's end
        {
            c[qs.t] = t;
            c[qs.n] = qs.upper ? P : 0;
        }
        else
        {
            c[0] = t % N1, c[1] = t / N1;
        }
        const int i = c[0] + N1 * c[1];
        double    Ji[2][2], xy[2], nrm[2] = {0., 0.};
        if constexpr (SIDE)
            quadSideGeom(vv, qs, gll[c[qs.t]], Ji, xy, nrm);
        else
            quadGeom(vv, gll[c[0]], gll[c[1]], Ji, xy);
        typename Iface::BoundaryInput in;
#pragma unroll
        for (int fl = 0; fl < F; ++fl)
        {
            const double* xf = xs + fl * NN;
            in.field_vals[fl] = xf[i];
            double dr[2]      = {0., 0.};
            for (int d = 0; d < 2; ++d)
                for (int b = 0; b < N1; ++b)
                    dr[d] += tabG[b * N1 + c[d]] * xf[i + (b - c[d]) * str[d]];
#pragma unroll
            for (int s = 0; s < 2; ++s)
                in.field_ders[s][fl] = Ji[0][s] * dr[0] + Ji[1][s] * dr[1];
        }
        in.point  = SpaceTimePoint{Point3{{xy[0], xy[1], 0.}}, a.time};
        in.normal = {{nrm[0], nrm[1]}};
        typename Iface::Rhs out{};
        kern(in, out);
        const int64_t node = en[i];
#pragma unroll
        for (int eq = 0; eq < E; ++eq)
        {
            const int64_t dof = node * a.dofs_per_node + a.field_inds[eq];
            unsafeAtomicAdd(a.node_sum + dof, out[eq]);
            unsafeAtomicAdd(a.node_count + dof, 1.);
        }
    }
}

template < typename K, int P, int NQ, bool SIDE >
int launchQuadValuesAtNodes(const ElemArgs& a, const void* kparam_blob, hipStream_t stream)
{
    const int64_t count = SIDE ? a.face_count : a.elem_count;
    if (count <= 0)
        return 0;
    constexpr size_t wb = quadAtNodesBytes< K, P >();
    constexpr int    W  = quadWaves(wb);
    const unsigned   grid = static_cast< unsigned >((count + W - 1) / W);
    return launchKernel("quadValuesAtNodesKernel", quadValuesAtNodesKernel< K, P, NQ, SIDE >, dim3(grid), dim3(quad_wave * W), wb * W, stream,
                        a, functorFrom< K >(kparam_blob));
}
// side form where a side list is given (a.face_elem set), as launchValuesAtNodesAny
template < typename K, int P, int NQ >
int launchQuadValuesAtNodesAny(const ElemArgs& a, const void* kparam_blob, hipStream_t stream)
{
    return a.face_elem ? launchQuadValuesAtNodes< K, P, NQ, true >(a, kparam_blob, stream)
                       : launchQuadValuesAtNodes< K, P, NQ, false >(a, kparam_blob, stream);
}
} // namespace l3k::dev
#endif
