// quad.hpp -- matrix-free operator apply, diagonal and lifted right-hand side on bilinear quadrilaterals (dim = 2).
//
// The 2-D counterpart of sumfact_apply.hpp / diag.hpp: evalLocalOperatorSumFact on quads (algsys/SumFactorization.hpp:438-467
// sumFactBackQuad, :614-676 evalAtQuadQPs, :758-841 sumFactForwardQuad) fused with the gather / scatter of
// algsys/MatrixFreeSystem.hpp:421-467,494-537, in the collocation-derivative form the hex kernels use: 2 interpolation
// sweeps (I) to the Gauss grid, 2 collocation-derivative sweeps (C) on it, the quadrature-point stage, and the transposed
// sweeps back to the nodes.
//
// Organisation: one wave per element, quadWaves() independent elements per workgroup (no barrier between the waves: a wave's
// LDS instructions execute in issue order, stageFence only keeps the compiler from moving LDS accesses across stages).  Each
// wave owns (U*R + F) x max(p+1, nq)^2 doubles in 4 LDS buffers -- under 1 KB per buffer and operand at nq = 7, so the LDS
// does not bound occupancy (profiles/README.md: 0.06-0.12 of the HBM roofline, lanes idle at low orders).  Quadrature points go one per
// lane (nq^2 <= 64 up to order 7), looping where nq^2 > 64.  x^T A x is not fused here (ElemArgs::energy_done stays unset,
// the library falls back to the dot product); the R columns of an instance go through in one pass.
#ifndef L3K_DEVICE_QUAD_HPP
#define L3K_DEVICE_QUAD_HPP

#include "sumfact_apply.hpp"
#include "sumfact_fast.hpp"

namespace l3k::dev
{
inline constexpr int quad_wave = 64;

// bytes of LDS per element of the apply / rhs kernel: 4 buffers of NF x M^2 doubles + the 4 vertices
template < typename K, int P, int NQ, int R >
constexpr size_t quadApplyElemBytes()
{
    constexpr int M = cmax(P + 1, NQ);
    return sizeof(double) * (4 * size_t(K::params.n_unknowns * R + K::params.n_fields) * M * M + 12);
}
// ... of the diagonal kernel: coefficient array, sweep temporary, element diagonal (U x M^2 each), fields at the points
// (value + 2 derivatives + 1 temporary, F x M^2 each), geometry at the points (J^-1, w detJ, x, y: 7 x M^2), the vertices
template < typename K, int P, int NQ >
constexpr size_t quadDiagElemBytes()
{
    constexpr int M = cmax(P + 1, NQ);
    return sizeof(double) * (size_t(3 * K::params.n_unknowns + 4 * K::params.n_fields + 7) * M * M + 12);
}
// elements (= waves) per workgroup: 4, fewer where that would take more than 64 KB of LDS
constexpr int quadWaves(size_t elem_bytes)
{
    return elem_bytes * 4 <= 65536 ? 4 : (elem_bytes * 2 <= 65536 ? 2 : 1);
}

// Geometry of a bilinear quad (vertices v = i + 2j, z ignored) at (xi, eta): Ji[d][s] = d xi_d / d x_s, position; returns detJ
__device__ __forceinline__ double quadGeom(const double* __restrict__ vs /*[4][3]*/, double xi, double eta, double Ji[2][2], double xy[2])
{
    double Jm[2][2]; // Jm[s][d] = d x_s / d xi_d
#pragma unroll
    for (int s = 0; s < 2; ++s)
    {
        const double c0 = vs[0 * 3 + s], c1 = vs[1 * 3 + s], c2 = vs[2 * 3 + s], c3 = vs[3 * 3 + s];
        Jm[s][0] = .25 * ((1. - eta) * (c1 - c0) + (1. + eta) * (c3 - c2));
        Jm[s][1] = .25 * ((1. - xi) * (c2 - c0) + (1. + xi) * (c3 - c1));
        xy[s]    = .25 * ((1. - xi) * (1. - eta) * c0 + (1. + xi) * (1. - eta) * c1 + (1. - xi) * (1. + eta) * c2 +
                       (1. + xi) * (1. + eta) * c3);
    }
    const double det = Jm[0][0] * Jm[1][1] - Jm[0][1] * Jm[1][0];
    const double id  = 1. / det;
    Ji[0][0]         = Jm[1][1] * id;
    Ji[0][1]         = -Jm[0][1] * id;
    Ji[1][0]         = -Jm[1][0] * id;
    Ji[1][1]         = Jm[0][0] * id;
    return det;
}

// The domain kernel's input at one point (evalAtQuadQPs, algsys/SumFactorization.hpp:614-676): interpolated fields, their
// physical derivatives, the point {x, y, 0} and the time.  fv / fd0 / fd1: field values and reference derivatives.
template < typename K, int RT >
__device__ __forceinline__ auto quadKernelAt(const K& kern, const double (*Ji)[2], const double* xy, double time, const double* fv,
                                             const double* fd0, const double* fd1)
{
    constexpr KernelParams params = K::params;
    using Iface = KernelInterface< KernelParams{2, params.n_equations, params.n_unknowns, params.n_fields, RT} >;
    typename Iface::DomainInput in;
#pragma unroll
    for (int f = 0; f < params.n_fields; ++f)
    {
        in.field_vals[f] = fv[f];
#pragma unroll
        for (int s = 0; s < 2; ++s)
            in.field_ders[s][f] = Ji[0][s] * fd0[f] + Ji[1][s] * fd1[f];
    }
    in.point = SpaceTimePoint{Point3{{xy[0], xy[1], 0.}}, time};
    typename Iface::Result res{};
    kern(in, res);
    return res;
}

// One element per wave: y += alpha * A x (RHS_MODE false) or rhs += B^T W (f - B g) (RHS_MODE true, g = Dirichlet values on
// Dirichlet dofs, 0 elsewhere; nothing skipped in the scatter, as in sumfactApplyKernel).  R columns in one pass.
template < typename K, int P, int NQ, int R, bool RHS_MODE >
__global__ __launch_bounds__(quad_wave * quadWaves(quadApplyElemBytes< K, P, NQ, R >())) void quadApplyKernel(const ElemArgs a, const K kern)
{
    constexpr KernelParams params = K::params;
    constexpr int          U = params.n_unknowns, E = params.n_equations, F = params.n_fields, OPS = U * R, NF = OPS + F;
    constexpr int          N1 = P + 1, NN = N1 * N1, NQP = NQ * NQ, M = cmax(N1, NQ), M2 = M * M, NT = quad_wave;
    constexpr size_t       elem_doubles = quadApplyElemBytes< K, P, NQ, R >() / sizeof(double);
    constexpr TableLayout  TL{N1, NQ};

    extern __shared__ double lds[];
    const int     wave = threadIdx.x / NT, lane = threadIdx.x % NT;
    const int64_t eb   = int64_t(blockIdx.x) * (blockDim.x / NT) + wave;
    if (eb >= a.elem_count) // (no workgroup barrier below: a wave without an element may leave)
        return;
    double* const B0 = lds + size_t(wave) * elem_doubles; // nodal values, then the result at the nodes
    double* const B1 = B0 + NF * M2;                      // sweep temporary
    double* const V  = B1 + NF * M2;                      // values at the points, then r0 and the transposed sweeps
    double* const D0 = V + NF * M2;                       // d/dxi at the points, then rd[0]
    double* const vv = D0 + NF * M2;                      // [4][3]
    double* const D1 = B1;                                // d/deta at the points reuses the interpolation temporary

    const int64_t   e  = a.elem_begin + eb;
    const uint32_t* en = a.elem_nodes + e * NN;
    if (lane < 12)
        vv[lane] = a.elem_verts[e * 12 + lane];

    // ---- gather (gatherSumFact, algsys/MatrixFreeSystem.hpp:421-467), unknown fastest over the lanes
    for (int t = lane; t < NN * U; t += NT)
    {
        const int     i    = t / U;
        const int     u    = t - i * U;
        const int64_t dof  = int64_t(en[i]) * a.dofs_per_node + a.field_inds[u];
        const bool    dir  = a.dirichlet != nullptr && a.dirichlet[dof] != 0;
#pragma unroll
        for (int r = 0; r < R; ++r)
        {
            double val;
            if constexpr (RHS_MODE)
                val = (dir && a.dirichlet_vals) ? a.dirichlet_vals[dof + a.ldg * r] : 0.;
            else
                val = dir ? 0. : (dof < a.n_owned_dofs ? a.x[dof + a.ldx * r] : a.xg[(dof - a.n_owned_dofs) + a.ldxg * r]);
            B0[(r * U + u) * M2 + i] = val;
        }
    }
    if constexpr (F > 0)
        for (int t = lane; t < NN * F; t += NT) // FieldAccess::fill, post/FieldAccess.hpp:21-30
        {
            const int f = t / NN, i = t - f * NN;
            B0[(OPS + f) * M2 + i] = a.fields[en[i] + f * a.ldf];
        }
    stageFence();

    const double* const tabI = a.tables + TL.offI();
    const double* const tabC = a.tables + TL.offC();
    // ---- interpolation to the Gauss points (x, then y), collocation derivatives on the Gauss grid
    sweep< 0, N1, NQ, false, false, N1, N1, 1, NF, NT >(B0, B1, M2, tabI, lane); // -> (NQ, N1)
    stageFence();
    sweep< 1, N1, NQ, false, false, NQ, N1, 1, NF, NT >(B1, V, M2, tabI, lane); // -> (NQ, NQ)
    stageFence();
    sweep< 0, NQ, NQ, false, false, NQ, NQ, 1, NF, NT >(V, D0, M2, tabC, lane);
    sweep< 1, NQ, NQ, false, false, NQ, NQ, 1, NF, NT >(V, D1, M2, tabC, lane);
    stageFence();

    // ---- quadrature points: t = w detJ (A0 v + sum_d D_d dv_d) (or w detJ (f - ...)), r0 = A0^T t, r_d = D_d^T t
    const double* const qw = a.tables + TL.offW();
    const double* const qp = a.tables + TL.offX();
    for (int q = lane; q < NQP; q += NT)
    {
        const int qx = q % NQ, qy = q / NQ;
        double    Ji[2][2], xy[2];
        const double wgt = qw[qx] * qw[qy] * quadGeom(vv, qp[qx], qp[qy], Ji, xy);
        double       fv[F > 0 ? F : 1], fd0[F > 0 ? F : 1], fd1[F > 0 ? F : 1];
#pragma unroll
        for (int f = 0; f < F; ++f)
        {
            fv[f]  = V[(OPS + f) * M2 + q];
            fd0[f] = D0[(OPS + f) * M2 + q];
            fd1[f] = D1[(OPS + f) * M2 + q];
        }
        const auto res = quadKernelAt< K, R >(kern, Ji, xy, a.time, fv, fd0, fd1);
        // D_d = sum_s A_{s+1} Ji[d][s]   (:655-660)
        double Dm[2][E][U];
#pragma unroll
        for (int d = 0; d < 2; ++d)
#pragma unroll
            for (int e_ = 0; e_ < E; ++e_)
#pragma unroll
                for (int u = 0; u < U; ++u)
                    Dm[d][e_][u] = res.operators[1](e_, u) * Ji[d][0] + res.operators[2](e_, u) * Ji[d][1];
#pragma unroll
        for (int r = 0; r < R; ++r)
        {
            double v[U], d0[U], d1[U];
#pragma unroll
            for (int u = 0; u < U; ++u)
            {
                v[u]  = V[(r * U + u) * M2 + q];
                d0[u] = D0[(r * U + u) * M2 + q];
                d1[u] = D1[(r * U + u) * M2 + q];
            }
            double t[E];
#pragma unroll
            for (int e_ = 0; e_ < E; ++e_)
            {
                double acc = 0.;
#pragma unroll
                for (int u = 0; u < U; ++u)
                    acc += res.operators[0](e_, u) * v[u] + Dm[0][e_][u] * d0[u] + Dm[1][e_][u] * d1[u];
                t[e_] = RHS_MODE ? wgt * (res.rhs(e_, r) - acc) : wgt * acc;
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
            {
                double a0 = 0., a1 = 0., a2 = 0.;
#pragma unroll
                for (int e_ = 0; e_ < E; ++e_)
                {
                    a0 += res.operators[0](e_, u) * t[e_];
                    a1 += Dm[0][e_][u] * t[e_];
                    a2 += Dm[1][e_][u] * t[e_];
                }
                V[(r * U + u) * M2 + q]  = a0;
                D0[(r * U + u) * M2 + q] = a1;
                D1[(r * U + u) * M2 + q] = a2;
            }
        }
    }
    stageFence();

    // ---- transposed collocation derivatives accumulate into the value array, transposed interpolation back to the nodes
    sweep< 0, NQ, NQ, true, true, NQ, NQ, 1, OPS, NT >(D0, V, M2, tabC, lane);
    stageFence();
    sweep< 1, NQ, NQ, true, true, NQ, NQ, 1, OPS, NT >(D1, V, M2, tabC, lane);
    stageFence();
    sweep< 1, NQ, N1, true, false, NQ, NQ, 1, OPS, NT >(V, D0, M2, tabI, lane); // -> (NQ, N1)
    stageFence();
    sweep< 0, NQ, N1, true, false, NQ, N1, 1, OPS, NT >(D0, B0, M2, tabI, lane); // -> (N1, N1)
    stageFence();

    // ---- scatter-add (scatterSumFact, algsys/MatrixFreeSystem.hpp:494-537; scatterInit :377-390 in RHS mode)
    for (int t = lane; t < NN * U; t += NT)
    {
        const int     i    = t / U;
        const int     u    = t - i * U;
        const int64_t node = en[i];
        const int64_t dof  = node * a.dofs_per_node + a.field_inds[u];
        const bool    dir  = !RHS_MODE && a.dirichlet != nullptr && a.dirichlet[dof] != 0;
        const bool    excl = !RHS_MODE && a.fuse_beta && node >= a.exclusive_node_begin && node < a.exclusive_node_end;
#pragma unroll
        for (int r = 0; r < R; ++r)
        {
            const double val = (RHS_MODE ? 1. : a.alpha) * B0[(r * U + u) * M2 + i];
            double* dst = dof < a.n_owned_dofs ? a.y + dof + a.ldy * r : a.yg + (dof - a.n_owned_dofs) + a.ldyg * r;
            if (excl) // node of this element only: write alpha*A*x + beta*y (see l3k_mf_scale)
                *dst = (dir ? 0. : val) + (a.beta == 0. ? 0. : a.beta * *dst);
            else if (!dir)
                unsafeAtomicAdd(dst, val);
        }
    }
}

// diag(K_e)[b*U+u] = sum_q w detJ sum_e (B_q[e, b*U+u])^2, expanded as in diag.hpp: with c_0 = A0[e][u], c_d = (sum_s A_s Ji[d][s])[e][u]
// the square is sum_{k<=l} m_kl c_k c_l psi_k psi_l, and each psi_k psi_l is a tensor product of the 1-D tables I*I, I*D, D*D:
// 6 coefficient arrays per element, each contracted with 2 transposed sweeps.  One element per wave, atomics into the diagonal.
template < typename K, int P, int NQ >
__global__ __launch_bounds__(quad_wave * quadWaves(quadDiagElemBytes< K, P, NQ >())) void quadDiagKernel(const ElemArgs a, const K kern)
{
    constexpr KernelParams params = K::params;
    constexpr int          U = params.n_unknowns, E = params.n_equations, F = params.n_fields;
    constexpr int          N1 = P + 1, NN = N1 * N1, NQP = NQ * NQ, M = cmax(N1, NQ), M2 = M * M, NT = quad_wave;
    constexpr size_t       elem_doubles = quadDiagElemBytes< K, P, NQ >() / sizeof(double);
    constexpr TableLayout  TL{N1, NQ};

    extern __shared__ double lds[];
    const int     wave = threadIdx.x / NT, lane = threadIdx.x % NT;
    const int64_t eb   = int64_t(blockIdx.x) * (blockDim.x / NT) + wave;
    if (eb >= a.elem_count)
        return;
    double* const Gb  = lds + size_t(wave) * elem_doubles; // [U][M2] coefficient array of the current (k, l)
    double* const T1  = Gb + U * M2;                        // sweep temporary
    double* const acc = T1 + U * M2;                        // [U][M2] element diagonal at the nodes
    double* const Fv  = acc + U * M2;                       // fields: values, d/dxi, d/deta at the points, + 1 temporary
    double* const geo = Fv + 4 * F * M2;                    // [7][M2]: J^-1 (4), w detJ, x, y at the points
    double* const vv  = geo + 7 * M2;                       // [4][3]

    const int64_t   e  = a.elem_begin + eb;
    const uint32_t* en = a.elem_nodes + e * NN;
    if (lane < 12)
        vv[lane] = a.elem_verts[e * 12 + lane];
    for (int i = lane; i < U * M2; i += NT)
        acc[i] = 0.;
    if constexpr (F > 0)
    {
        double* const Ft = Fv + 3 * F * M2;
        for (int t = lane; t < NN * F; t += NT)
        {
            const int f = t / NN, i = t - f * NN;
            Ft[f * M2 + i] = a.fields[en[i] + f * a.ldf];
        }
        stageFence();
        const double* tabI = a.tables + TL.offI();
        const double* tabC = a.tables + TL.offC();
        sweep< 0, N1, NQ, false, false, N1, N1, 1, F, NT >(Ft, Fv + F * M2, M2, tabI, lane);
        stageFence();
        sweep< 1, N1, NQ, false, false, NQ, N1, 1, F, NT >(Fv + F * M2, Fv, M2, tabI, lane);
        stageFence();
        sweep< 0, NQ, NQ, false, false, NQ, NQ, 1, F, NT >(Fv, Fv + 1 * F * M2, M2, tabC, lane);
        sweep< 1, NQ, NQ, false, false, NQ, NQ, 1, F, NT >(Fv, Fv + 2 * F * M2, M2, tabC, lane);
    }
    stageFence();
    {
        const double* qw = a.tables + TL.offW();
        const double* qp = a.tables + TL.offX();
        for (int q = lane; q < NQP; q += NT)
        {
            const int qx = q % NQ, qy = q / NQ;
            double    Ji[2][2], xy[2];
            const double wgt = qw[qx] * qw[qy] * quadGeom(vv, qp[qx], qp[qy], Ji, xy);
#pragma unroll
            for (int i = 0; i < 4; ++i)
                geo[i * M2 + q] = Ji[i / 2][i % 2];
            geo[4 * M2 + q] = wgt;
            geo[5 * M2 + q] = xy[0];
            geo[6 * M2 + q] = xy[1];
        }
    }
    stageFence();

    const double* tab[3] = {a.tables + TL.offII(), a.tables + TL.offID(), a.tables + TL.offDD()};
    auto pairStep = [&]< int KK, int LL >() {
        for (int q = lane; q < NQP; q += NT)
        {
            double Ji[2][2], fv[F > 0 ? F : 1], fd0[F > 0 ? F : 1], fd1[F > 0 ? F : 1];
#pragma unroll
            for (int i = 0; i < 4; ++i)
                Ji[i / 2][i % 2] = geo[i * M2 + q];
            const double wgt   = geo[4 * M2 + q];
            const double xy[2] = {geo[5 * M2 + q], geo[6 * M2 + q]};
#pragma unroll
            for (int f = 0; f < F; ++f)
            {
                fv[f]  = Fv[f * M2 + q];
                fd0[f] = Fv[(F + f) * M2 + q];
                fd1[f] = Fv[(2 * F + f) * M2 + q];
            }
            const auto res  = quadKernelAt< K, 1 >(kern, Ji, xy, a.time, fv, fd0, fd1);
            auto       coef = [&](int k, int e_, int u) {
                return k == 0 ? res.operators[0](e_, u) : res.operators[1](e_, u) * Ji[k - 1][0] + res.operators[2](e_, u) * Ji[k - 1][1];
            };
#pragma unroll
            for (int u = 0; u < U; ++u)
            {
                double g = 0.;
#pragma unroll
                for (int e_ = 0; e_ < E; ++e_)
                    g += coef(KK, e_, u) * coef(LL, e_, u);
                Gb[u * M2 + q] = (KK == LL ? 1. : 2.) * wgt * g;
            }
        }
        stageFence();
        // psi_k psi_l along one axis: I*I (neither differentiates that axis), I*D (one does), D*D (both)
        constexpr auto sel = [](int axis) { return (KK == axis + 1 ? 1 : 0) + (LL == axis + 1 ? 1 : 0); };
        sweep< 1, NQ, N1, true, false, NQ, NQ, 1, U, NT >(Gb, T1, M2, tab[sel(1)], lane); // -> (NQ, N1)
        stageFence();
        sweep< 0, NQ, N1, true, true, NQ, N1, 1, U, NT >(T1, acc, M2, tab[sel(0)], lane); // += (N1, N1)
        stageFence();
    };
    pairStep.template operator()< 0, 0 >();
    pairStep.template operator()< 0, 1 >();
    pairStep.template operator()< 0, 2 >();
    pairStep.template operator()< 1, 1 >();
    pairStep.template operator()< 1, 2 >();
    pairStep.template operator()< 2, 2 >();

    // scatterInit: add everywhere (Dirichlet rows are overwritten by the finalisation, MatrixFreeSystem.hpp:911-915)
    for (int t = lane; t < NN * U; t += NT)
    {
        const int     i   = t / U;
        const int     u   = t - i * U;
        const int64_t dof = int64_t(en[i]) * a.dofs_per_node + a.field_inds[u];
        double*       dst = dof < a.n_owned_dofs ? a.diag + dof : a.diag_g + (dof - a.n_owned_dofs);
        unsafeAtomicAdd(dst, acc[u * M2 + i]);
    }
}

template < typename K, int P, int NQ, int R, bool RHS_MODE >
int launchQuadElems(const ElemArgs& a, const void* kparam_blob, hipStream_t stream)
{
    if (a.elem_count <= 0)
        return 0;
    constexpr size_t   eb = quadApplyElemBytes< K, P, NQ, R >();
    constexpr int      W  = quadWaves(eb);
    static_assert(eb * W <= lds_limit_bytes, "quad element working set exceeds the LDS");
    const unsigned grid = static_cast< unsigned >((a.elem_count + W - 1) / W);
    return launchKernel("quadApplyKernel", quadApplyKernel< K, P, NQ, R, RHS_MODE >, dim3(grid), dim3(quad_wave * W), eb * W, stream, a,
                        functorFrom< K >(kparam_blob));
}
template < typename K, int P, int NQ, int R >
int launchQuadApply(const ElemArgs& a, const void* kparam_blob, hipStream_t stream)
{
    return launchQuadElems< K, P, NQ, R, false >(a, kparam_blob, stream);
}
// diag + rhs of one element range
template < typename K, int P, int NQ, int R >
int launchQuadDiagRhs(const ElemArgs& a, const void* kparam_blob, hipStream_t stream)
{
    if (a.elem_count <= 0)
        return 0;
    if (int rc = launchQuadElems< K, P, NQ, R, true >(a, kparam_blob, stream))
        return rc;
    if (!a.diag)
        return 0;
    constexpr size_t eb = quadDiagElemBytes< K, P, NQ >();
    constexpr int    W  = quadWaves(eb);
    static_assert(eb * W <= lds_limit_bytes, "quad diagonal working set exceeds the LDS");
    const unsigned grid = static_cast< unsigned >((a.elem_count + W - 1) / W);
    return launchKernel("quadDiagKernel", quadDiagKernel< K, P, NQ >, dim3(grid), dim3(quad_wave * W), eb * W, stream, a,
                        functorFrom< K >(kparam_blob));
}
// the route of an apply through the quad kernel as text (l3k_mf_route)
template < typename K, int P, int NQ, int R >
int describeQuadApply(const ElemArgs& a, char* buf, size_t n)
{
    constexpr size_t eb = quadApplyElemBytes< K, P, NQ, R >();
    constexpr int    W  = quadWaves(eb);
    std::snprintf(buf, n, "quadApplyKernel<p=%d,nq=%d,U=%d,F=%d,R=%d>: one wave per element, %d elements per workgroup, %zu B LDS per element, "
                          "grid %lld%s%s",
                  P, NQ, K::params.n_unknowns, K::params.n_fields, R, W, eb, (long long)((a.elem_count + W - 1) / W),
                  a.dense ? "" : ", non-dense dof layout", a.energy ? "; x^T A x not fused (the caller takes the dot product)" : "");
    return 0;
}
} // namespace l3k::dev
#endif
