// condense.hpp -- static condensation of the element-internal dofs (the reference's CondensationPolicy::ElementBoundary,
// algsys/StaticCondensationManager.hpp:322-350 condenseSystem, :410-470 recoverSolution) on element matrices formed by the
// assembly kernels.
//
// The element system is read in the permuted order [internal dofs ; primary dofs] (both lists ascending in the element-local
// node index, dofs node-major b U + u: mesh/ElementTraits.hpp:37-59), with the R right-hand sides as R extra columns:
//     M = [ K_ii  K_ib  F_i ]
//         [ K_bi  K_bb  F_b ]
// A partial right-looking Cholesky over the Ni U internal pivots, on the upper triangle (logical column >= logical row), turns
// the internal rows into [L^T | W = L^-1 K_ib | h = L^-1 F_i] and the primary rows into [S = K_bb - W^T W | g = F_b - W^T h].
// Recovery runs the same elimination on the internal rows only and then x_i = L^-T (h - W x_b).
//
// Everything happens IN PLACE on the row-major K_e [Nd][Nd] and the column-major F_e [R][Nd] of each element (a logical entry
// (I, J) lives at K_e[perm(I)][perm(J)], or F_e[J - Nd][perm(I)] for the right-hand-side columns): no gathered copy.  Panels of
// NB pivots are two launches each, so that several workgroups share an element (a global barrier between the steps):
//   * condensePanelKernel:  the NB x NB diagonal block factored in LDS (every workgroup of the element redoes it: 1/3 NB^3),
//                           then one thread per later column solves the panel rows for it (L_D^-1, NB values in registers);
//   * condenseUpdateKernel: the rank-NB update of the trailing upper triangle in 64 x 64 tiles, the two NB x 64 panel slabs in
//                           LDS, a 4 x 4 register block per thread on the FP64 FMA pipe.
// A pivot that is not a positive finite number stops the element: its flag is set (error -2, "non-positive pivot in the
// element-internal block") and every later kernel leaves it alone -- its outputs are zeros, nothing of it is scattered.
// Kernels are templated on (P, U) only: instances shared by several functors compile once.
#ifndef L3K_DEVICE_CONDENSE_HPP
#define L3K_DEVICE_CONDENSE_HPP

#include "common.hpp"
#include "launch.hpp"

namespace l3k::dev
{
// k-th internal node (all of ix, iy, iz in 1 .. p-1) of an element with n = p + 1 nodes per direction, ascending
__host__ __device__ constexpr int internalNodeOf(int k, int n)
{
    const int m = n > 2 ? n - 2 : 1;
    return (1 + k % m) + n * (1 + (k / m) % m) + n * n * (1 + k / (m * m));
}
// q-th primary (element-boundary) node, ascending: the layer z = 0, 4 p nodes of each middle layer (the row y = 0, the two
// ends of the rows 0 < y < p, the row y = p), the layer z = p
__host__ __device__ constexpr int primaryNodeOf(int q, int n)
{
    const int p = n - 1, L = n * n;
    if (q < L)
        return q;
    q -= L;
    const int mid = 4 * p;
    if (q < (p - 1) * mid)
    {
        const int iz = 1 + q / mid, t = q % mid;
        int       ix, iy;
        if (t < n)
            ix = t, iy = 0;
        else if (t < n + 2 * (p - 1))
            iy = 1 + (t - n) / 2, ix = ((t - n) % 2) ? p : 0;
        else
            iy = p, ix = t - n - 2 * (p - 1);
        return ix + n * iy + L * iz;
    }
    return L * p + (q - (p - 1) * mid);
}

struct CondenseArgs
{
    double*   K;     // [count][Nd][Nd] row-major element matrices, eliminated in place
    double*   F;     // [count][R][Nd] element right-hand sides, eliminated in place, or nullptr (R = 0)
    double*   Rd;    // [count][Ni U][NB] the factored diagonal blocks of the panels (recovery reads them)
    int*      fail;  // [count] per element: a pivot was not positive
    unsigned* nfail; // elements that failed (one counter)
    int64_t   count;
    int       n_rhs;
    int       recover; // 1: eliminate the internal rows only and solve for x_i; 0: condense
    // condense outputs: S [count][Nbd][Nbd] row-major bitwise symmetric, G [count][R][Nbd] (condense_local), or nullptr; and
    // `mirror`: the Schur block copied to its lower triangle in place (condense_global: the scatter reads whole rows)
    double* S;
    double* G;
    int     mirror;
    // recovery: x [R][ldx] over the local dofs, through the element's node ids
    const uint32_t* elem_nodes;
    int64_t         first;
    int             dpn;
    int             field_inds[max_unknowns];
    double*         x;
    size_t          ldx;
};

template < int P, int U >
struct CondShape
{
    static constexpr int n = P + 1, NN = n * n * n, Ni = (P - 1) * (P - 1) * (P - 1), Np = NN - Ni;
    static constexpr int Nd = NN * U, Nid = Ni * U, Nbd = Np * U;
    static constexpr int NB = 32; // pivots per panel
    // element-local dof of logical index I (internal dofs first, then the primary ones)
    __device__ static int perm(int I)
    {
        if (I < Nid)
            return internalNodeOf(I / U, n) * U + I % U;
        const int q = I - Nid;
        return primaryNodeOf(q / U, n) * U + q % U;
    }
};

// address of the logical entry (I, J), I < Nd, J < Nd + R
template < int P, int U >
__device__ __forceinline__ double* condAt(double* Ke, double* Fe, int I, int J)
{
    using S = CondShape< P, U >;
    const int pi = S::perm(I);
    return J < S::Nd ? Ke + int64_t(pi) * S::Nd + S::perm(J) : Fe + int64_t(J - S::Nd) * S::Nd + pi;
}

// a positive finite double, by its bits (immune to the finite-math flags of the build)
__device__ __forceinline__ bool positiveFinite(double d)
{
    const long long b = __double_as_longlong(d);
    return b > 0 && b < 0x7ff0000000000000LL;
}

// panel [p0, p0 + pn): grid = count x chunks of 256 later columns
template < int P, int U >
__global__ __launch_bounds__(256) void condensePanelKernel(const CondenseArgs a, int p0, int pn, int nchunk)
{
    using S = CondShape< P, U >;
    constexpr int NB = S::NB;
    __shared__ double D[NB][NB + 1];
    const int64_t e   = blockIdx.x / nchunk;
    const int     c   = int(blockIdx.x - e * nchunk);
    const int     tid = threadIdx.x;
    if (a.fail[e])
        return;
    double* Ke = a.K + e * int64_t(S::Nd) * S::Nd;
    double* Fe = a.F ? a.F + e * int64_t(a.n_rhs) * S::Nd : nullptr;
    for (int t = tid; t < pn * pn; t += 256)
    {
        const int i = t / pn, j = t - i * pn;
        if (j >= i)
            D[i][j] = *condAt< P, U >(Ke, Fe, p0 + i, p0 + j);
    }
    // unblocked upper Cholesky of the diagonal block: thread j owns column j
    for (int k = 0; k < pn; ++k)
    {
        __syncthreads();
        const double dkk = D[k][k];
        if (!positiveFinite(dkk)) // (uniform: every thread reads the same value)
        {
            if (tid == 0) // (every workgroup of the element that sees it counts: the counter only needs to be non-zero)
            {
                a.fail[e] = 1;
                atomicAdd(a.nfail, 1u);
            }
            return;
        }
        const double r = sqrt(dkk);
        __syncthreads();
        if (tid >= k && tid < pn)
            D[k][tid] = tid == k ? r : D[k][tid] / r;
        __syncthreads();
        if (tid > k && tid < pn)
            for (int i = k + 1; i <= tid; ++i)
                D[i][tid] -= D[k][i] * D[k][tid];
    }
    __syncthreads();
    if (c == 0)
        for (int t = tid; t < pn * NB; t += 256)
        {
            const int i = t / NB, j = t - i * NB;
            a.Rd[(e * S::Nid + p0 + i) * NB + j] = j >= i && j < pn ? D[i][j] : 0.;
        }
    // the panel rows of the later columns: v <- L_D^-1 v, one column per thread
    const int ncol = S::Nd + (a.F ? a.n_rhs : 0);
    const int J    = p0 + pn + c * 256 + tid;
    if (J >= ncol)
        return;
    double  v[NB];
    double* ptr[NB];
#pragma unroll
    for (int i = 0; i < NB; ++i)
        if (i < pn)
        {
            ptr[i] = condAt< P, U >(Ke, Fe, p0 + i, J);
            v[i]   = *ptr[i];
        }
#pragma unroll
    for (int i = 0; i < NB; ++i)
        if (i < pn)
        {
            double s = v[i];
#pragma unroll
            for (int m = 0; m < i; ++m)
                s -= D[m][i] * v[m];
            v[i]    = s / D[i][i];
            *ptr[i] = v[i];
        }
}

// trailing update after the panel [p0, p0 + pn): M[I][J] -= sum_k M[k][I] M[k][J] for p1 <= I < i_end, J >= I;
// grid = count x nti x ntj tiles of 64 x 64 (tiles wholly below the diagonal return at once)
template < int P, int U >
__global__ __launch_bounds__(256) void condenseUpdateKernel(const CondenseArgs a, int p0, int pn, int i_end, int nti, int ntj)
{
    using S = CondShape< P, U >;
    constexpr int NB = S::NB, T = 64;
    __shared__ double As[NB][T], Bs[NB][T];
    const int64_t per = int64_t(nti) * ntj;
    const int64_t e   = blockIdx.x / per;
    const int     w   = int(blockIdx.x - e * per);
    const int     ti = w / ntj, tj = w - ti * ntj;
    const int     p1 = p0 + pn, I0 = p1 + ti * T, J0 = p1 + tj * T;
    if (J0 + T - 1 < I0 || a.fail[e])
        return;
    double*   Ke   = a.K + e * int64_t(S::Nd) * S::Nd;
    double*   Fe   = a.F ? a.F + e * int64_t(a.n_rhs) * S::Nd : nullptr;
    const int ncol = S::Nd + (a.F ? a.n_rhs : 0);
    const int tid  = threadIdx.x;
    for (int t = tid; t < pn * T; t += 256)
    {
        const int k = t / T, j = t - k * T;
        As[k][j]    = I0 + j < i_end ? *condAt< P, U >(Ke, Fe, p0 + k, I0 + j) : 0.;
        Bs[k][j]    = J0 + j < ncol ? *condAt< P, U >(Ke, Fe, p0 + k, J0 + j) : 0.;
    }
    __syncthreads();
    const int tx = tid & 15, ty = tid >> 4;
    double    acc[4][4] = {};
    for (int k = 0; k < pn; ++k)
    {
        double av[4], bv[4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
        {
            av[i] = As[k][ty + 16 * i];
            bv[i] = Bs[k][tx + 16 * i];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                acc[i][j] += av[i] * bv[j];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
    {
        const int I = I0 + ty + 16 * i;
        if (I >= i_end)
            continue;
#pragma unroll
        for (int j = 0; j < 4; ++j)
        {
            const int J = J0 + tx + 16 * j;
            if (J >= I && J < ncol)
                *condAt< P, U >(Ke, Fe, I, J) -= acc[i][j];
        }
    }
}

// condense_local outputs: row a of S (bitwise symmetric: the upper triangle, mirrored) and entry a of the R columns of G;
// grid = count x Nbd rows.  Without internal nodes S is K_e itself, entry for entry.
template < int P, int U >
__global__ __launch_bounds__(256) void condenseOutputKernel(const CondenseArgs a)
{
    using S = CondShape< P, U >;
    const int64_t e  = blockIdx.x / S::Nbd;
    const int     r  = int(blockIdx.x - e * S::Nbd);
    const bool    ok = !a.fail[e];
    double*       Ke = a.K + e * int64_t(S::Nd) * S::Nd;
    double*       Fe = a.F ? a.F + e * int64_t(a.n_rhs) * S::Nd : nullptr;
    if (a.S)
    {
        double* out = a.S + (e * S::Nbd + r) * int64_t(S::Nbd);
        for (int c = threadIdx.x; c < S::Nbd; c += 256)
        {
            const int lo = S::Nid > 0 && c < r ? c : r, hi = S::Nid > 0 && c < r ? r : c;
            out[c]       = ok ? *condAt< P, U >(Ke, Fe, S::Nid + lo, S::Nid + hi) : 0.;
        }
    }
    if (a.G && Fe)
        for (int k = threadIdx.x; k < a.n_rhs; k += 256)
            a.G[(e * a.n_rhs + k) * S::Nbd + r] = ok ? *condAt< P, U >(Ke, Fe, S::Nid + r, S::Nd + k) : 0.;
}

// the Schur block's upper triangle copied to its lower one, in place, through 32 x 32 LDS tiles; grid = count x nt x nt
template < int P, int U >
__global__ __launch_bounds__(256) void condenseMirrorKernel(const CondenseArgs a, int nt)
{
    using S = CondShape< P, U >;
    constexpr int T = 32;
    __shared__ double tile[T][T + 1];
    const int64_t per = int64_t(nt) * nt;
    const int64_t e   = blockIdx.x / per;
    const int     w   = int(blockIdx.x - e * per);
    const int     ta = w / nt, tb = w - ta * nt;
    if (ta > tb || a.fail[e])
        return;
    double* Ke = a.K + e * int64_t(S::Nd) * S::Nd;
    for (int t = threadIdx.x; t < T * T; t += 256)
    {
        const int i = t / T, j = t - i * T, r = ta * T + i, c = tb * T + j;
        if (r < S::Nbd && c < S::Nbd && c > r)
            tile[i][j] = Ke[int64_t(S::perm(S::Nid + r)) * S::Nd + S::perm(S::Nid + c)];
    }
    __syncthreads();
    for (int t = threadIdx.x; t < T * T; t += 256)
    {
        const int j = t / T, i = t - j * T, r = ta * T + i, c = tb * T + j; // (writes: row c, consecutive columns r)
        if (r < S::Nbd && c < S::Nbd && c > r)
            Ke[int64_t(S::perm(S::Nid + c)) * S::Nd + S::perm(S::Nid + r)] = tile[i][j];
    }
}

// recovery after the elimination of the internal rows: per element and right-hand side, y = h - W x_b (a wave per internal
// row), then x_i = L^-T y by back substitution (the workgroup on one row at a time, fixed summation order: bitwise
// reproducible), written to the element's internal dofs with plain stores (each belongs to this element only)
template < int P, int U >
__global__ __launch_bounds__(256) void condenseRecoverKernel(const CondenseArgs a)
{
    using S = CondShape< P, U >;
    constexpr int NB = S::NB;
    __shared__ double xs[S::Nid > 0 ? S::Nid : 1];
    __shared__ double red[4];
    const int64_t   e = blockIdx.x;
    if (a.fail[e])
        return;
    double*         Ke   = a.K + e * int64_t(S::Nd) * S::Nd;
    double*         Fe   = a.F + e * int64_t(a.n_rhs) * S::Nd;
    const double*   Rde  = a.Rd + e * int64_t(S::Nid) * NB;
    const uint32_t* en   = a.elem_nodes + (a.first + e) * S::NN;
    const int       tid  = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    auto            dofAt = [&](int b) { return int64_t(en[b / U]) * a.dpn + a.field_inds[b % U]; };
    auto            R     = [&](int k, int j) { // L^T entry (k, j), j >= k
        return j / NB == k / NB ? Rde[int64_t(k) * NB + j % NB] : *condAt< P, U >(Ke, Fe, k, j);
    };
    for (int r = 0; r < a.n_rhs; ++r)
    {
        const double* xr = a.x + size_t(r) * a.ldx;
        for (int k = wv; k < S::Nid; k += 4)
        {
            const double* Wk = Ke + int64_t(S::perm(k)) * S::Nd;
            double        s  = 0.;
            for (int j = lane; j < S::Nbd; j += 64)
            {
                const int q = j / U, u = j - q * U, b = primaryNodeOf(q, S::n) * U + u;
                s += Wk[b] * xr[dofAt(b)];
            }
            for (int o = 32; o > 0; o >>= 1)
                s += __shfl_xor(s, o);
            if (lane == 0)
                xs[k] = Fe[int64_t(r) * S::Nd + S::perm(k)] - s;
        }
        for (int k = S::Nid - 1; k >= 0; --k)
        {
            __syncthreads(); // xs[k + 1 ..] final
            double s = 0.;
            for (int j = k + 1 + tid; j < S::Nid; j += 256)
                s += R(k, j) * xs[j];
            for (int o = 32; o > 0; o >>= 1)
                s += __shfl_xor(s, o);
            if (lane == 0)
                red[wv] = s;
            __syncthreads();
            if (tid == 0)
                xs[k] = (xs[k] - (((red[0] + red[1]) + red[2]) + red[3])) / R(k, k);
        }
        __syncthreads();
        double* xw = a.x + size_t(r) * a.ldx;
        for (int k = tid; k < S::Nid; k += 256)
            xw[dofAt(S::perm(k))] = xs[k];
        __syncthreads();
    }
}

// the elimination and its output step for `a.count` element systems on `stream`
template < int P, int U >
int launchCondense(const CondenseArgs& a, hipStream_t stream)
{
    using S = CondShape< P, U >;
    constexpr int NB = S::NB;
    if (a.count == 0)
        return 0;
    const int ncol  = S::Nd + (a.F ? a.n_rhs : 0);
    const int i_end = a.recover ? S::Nid : S::Nd;
    for (int p0 = 0; p0 < S::Nid; p0 += NB)
    {
        const int pn = S::Nid - p0 < NB ? S::Nid - p0 : NB, p1 = p0 + pn;
        const int nchunk = (ncol - p1 + 255) / 256 > 0 ? (ncol - p1 + 255) / 256 : 1;
        if (int rc = launchKernel("condensePanelKernel", condensePanelKernel< P, U >, dim3(unsigned(a.count * nchunk)), dim3(256), 0,
                                  stream, a, p0, pn, nchunk))
            return rc;
        const int nti = (i_end - p1 + 63) / 64, ntj = (ncol - p1 + 63) / 64;
        if (nti > 0 && ntj > 0)
            if (int rc = launchKernel("condenseUpdateKernel", condenseUpdateKernel< P, U >, dim3(unsigned(a.count * nti * ntj)), dim3(256),
                                      0, stream, a, p0, pn, i_end, nti, ntj))
                return rc;
    }
    if (a.recover)
        return S::Nid > 0 ? launchKernel("condenseRecoverKernel", condenseRecoverKernel< P, U >, dim3(unsigned(a.count)), dim3(256), 0,
                                         stream, a)
                          : 0;
    if (a.S || a.G)
        if (int rc = launchKernel("condenseOutputKernel", condenseOutputKernel< P, U >, dim3(unsigned(a.count * S::Nbd)), dim3(256), 0,
                                  stream, a))
            return rc;
    if (a.mirror && S::Nid > 0)
    {
        const int nt = (S::Nbd + 31) / 32;
        if (int rc = launchKernel("condenseMirrorKernel", condenseMirrorKernel< P, U >, dim3(unsigned(a.count * nt * nt)), dim3(256), 0,
                                  stream, a, nt))
            return rc;
    }
    return 0;
}
// the launcher of an instance's shape (Instance::condense), or nullptr (quads)
template < int P, int U >
constexpr CondenseFn selectCondense()
{
    if constexpr (P >= 1 && U >= 1 && U <= max_unknowns)
        return &launchCondense< P, U >;
    else
        return nullptr;
}
} // namespace l3k::dev
#endif
