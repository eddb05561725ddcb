// periodic.hpp -- the per-item work of l3k_periodic_match (api_periodic.hip), one function per kernel: plain one-thread-per-item
// code that also compiles for the host, so that a stand-alone program can walk it over a mesh on the CPU
// (tests/cpp/periodic_walk.cpp).
#ifndef L3K_DEVICE_PERIODIC_HPP
#define L3K_DEVICE_PERIODIC_HPP

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

namespace l3k::periodic
{
inline constexpr int      cell_bits = 21; // per axis: 3 * 21 = 63 bits of key
inline constexpr uint32_t no_match  = 0xffffffffu;

// The uniform grid the destination nodes are binned on: origin one cell below the box of the destination vertices, m cells per axis.
// It is made on the host, in a unit without -ffinite-math-only (host/periodic.hpp: periodicMakeGrid), which refuses a box or a
// tolerance that gives no finite lo, inv_h > 0 and m <= 2^cell_bits.
struct Grid
{
    double  lo[3];
    double  inv_h;
    int64_t m;
};

// element-local node of side node q of `side` (sides as for l3k_bnd_create: the last axis first, low side before high side; the
// side's nodes in the lexicographic order of the remaining axes), as its index per axis
__host__ __device__ inline void sideNodeIndex(int dim, int n1, int side, int q, int ijk[3])
{
    const int axis = dim - 1 - (side >> 1), at = (side & 1) ? n1 - 1 : 0;
    ijk[0] = ijk[1] = ijk[2] = 0;
    int rest = q;
    for (int a = 0; a < dim; ++a)
        if (a == axis)
            ijk[a] = at;
        else
        {
            ijk[a] = rest % n1;
            rest /= n1;
        }
}

// slot t = (listed side, side node): the bi-/tri-linear image of the GLL reference position (mesh/NodePhysicalLocation.hpp), and
// the sort key (node id, slot)
__host__ __device__ inline void sideNodeLocation(int64_t t, int dim, int n1, int ns, const double* verts, const uint8_t* side,
                                                 const uint32_t* ids, const double* gll, double* loc, uint64_t* keys)
{
    const int64_t f  = t / ns;
    const int     q  = int(t - f * ns), nv = 1 << dim;
    int           ijk[3];
    sideNodeIndex(dim, n1, side[f], q, ijk);
    double l[3][2];
    for (int a = 0; a < 3; ++a)
    {
        const double g = a < dim ? gll[ijk[a]] : -1.;
        l[a][0]        = 0.5 * (1. - g);
        l[a][1]        = 0.5 * (1. + g);
    }
    const double* v    = verts + f * nv * 3;
    double        x[3] = {0., 0., 0.};
    for (int c = 0; c < nv; ++c)
    {
        const double w = l[0][c & 1] * l[1][(c >> 1) & 1] * l[2][(c >> 2) & 1];
        x[0] += w * v[c * 3 + 0];
        x[1] += w * v[c * 3 + 1];
        x[2] += w * v[c * 3 + 2];
    }
    loc[t * 3 + 0] = x[0];
    loc[t * 3 + 1] = x[1];
    loc[t * 3 + 2] = dim == 3 ? x[2] : 0.;
    keys[t]        = uint64_t(ids[t]) << 32 | uint64_t(t);
}

__host__ __device__ inline uint32_t startsNewId(int64_t t, const uint64_t* sorted)
{
    return (t == 0 || (sorted[t - 1] >> 32) != (sorted[t] >> 32)) ? 1u : 0u;
}

// the first slot of every run of one node id (the lowest slot: the keys are unique, so the sort leaves no choice) becomes unique
// node incl - 1; the unique nodes are ascending in the node id
__host__ __device__ inline void compactNode(int64_t t, const uint64_t* sorted, const uint32_t* incl, const double* loc, uint32_t* uid,
                                            double* uloc)
{
    if (!(t == 0 || incl[t - 1] != incl[t]))
        return;
    const uint32_t u    = incl[t] - 1u;
    const uint64_t slot = sorted[t] & 0xffffffffull;
    uid[u]              = uint32_t(sorted[t] >> 32);
    uloc[u * 3 + 0]     = loc[slot * 3 + 0];
    uloc[u * 3 + 1]     = loc[slot * 3 + 1];
    uloc[u * 3 + 2]     = loc[slot * 3 + 2];
}

// key of the cell of destination node t, x in the low bits (the grid's origin lies one cell below the lowest vertex: the clamp
// guards rounding only)
__host__ __device__ inline uint64_t cellKey(int64_t t, int dim, const Grid& g, const double* uloc)
{
    uint64_t k = 0;
    for (int a = dim - 1; a >= 0; --a)
    {
        const double  f = floor((uloc[t * 3 + a] - g.lo[a]) * g.inv_h);
        const int64_t c = f < 0. ? 0 : (f > double(g.m - 1) ? g.m - 1 : int64_t(f));
        k               = k << cell_bits | uint64_t(c);
    }
    return k;
}

// unique source node t against the destination nodes of its own and the adjacent cells: the 3^(dim-1) runs of three x-adjacent
// cells, each found by one lower bound among the sorted cell keys.  partner: the id of the nearest qualifying destination node,
// ties to the lowest id, or no_match; n_qualify: how many qualified, saturating at 2.
__host__ __device__ inline void matchNode(int64_t t, int dim, const Grid& g, const double* translation, double tolerance,
                                          const double* sloc, const uint64_t* dkeys, const uint32_t* dvals, const uint32_t* did,
                                          const double* dloc, int64_t n_dst, uint32_t* partner, uint8_t* n_qualify)
{
    const double p[3] = {sloc[t * 3 + 0] + translation[0], sloc[t * 3 + 1] + translation[1],
                         dim == 3 ? sloc[t * 3 + 2] + translation[2] : 0.};
    int64_t      c[3] = {0, 0, 0};
    bool         near = true;
    for (int a = 0; a < dim; ++a)
    {
        const double f = floor((p[a] - g.lo[a]) * g.inv_h);
        if (!(f >= -1. && f <= double(g.m))) // further than a cell from every destination node
            near = false;
        else
            c[a] = int64_t(f);
    }
    uint32_t best_id = no_match;
    double   best_d  = 0.;
    int      count   = 0;
    if (near)
    {
        const int64_t x_lo = c[0] - 1 < 0 ? 0 : c[0] - 1, x_hi = c[0] + 1 > g.m - 1 ? g.m - 1 : c[0] + 1;
        const int     nz = dim == 3 ? 3 : 1;
        for (int iz = 0; iz < nz; ++iz)
            for (int iy = 0; iy < 3; ++iy)
            {
                const int64_t cy = c[1] - 1 + iy, cz = dim == 3 ? c[2] - 1 + iz : 0;
                if (cy < 0 || cy >= g.m || cz < 0 || cz >= g.m || x_lo > x_hi)
                    continue;
                const uint64_t row  = (uint64_t(cz) << cell_bits | uint64_t(cy)) << cell_bits;
                const uint64_t k_lo = row | uint64_t(x_lo), k_hi = row | uint64_t(x_hi);
                int64_t        lo = 0, hi = n_dst; // first slot whose key is not below k_lo
                while (lo < hi)
                {
                    const int64_t mid = lo + (hi - lo) / 2;
                    if (dkeys[mid] < k_lo)
                        lo = mid + 1;
                    else
                        hi = mid;
                }
                for (int64_t s = lo; s < n_dst && dkeys[s] <= k_hi; ++s)
                {
                    const uint32_t u  = dvals[s];
                    const double   dx = p[0] - dloc[u * 3 + 0], dy = p[1] - dloc[u * 3 + 1], dz = p[2] - dloc[u * 3 + 2];
                    const double   d  = sqrt(dx * dx + dy * dy + dz * dz);
                    if (!(d < tolerance)) // strict, as in the reference
                        continue;
                    const uint32_t id = did[u];
                    if (count == 0 || d < best_d || (d == best_d && id < best_id))
                        best_d = d, best_id = id;
                    count = count < 2 ? count + 1 : 2;
                }
            }
    }
    partner[t]   = best_id;
    n_qualify[t] = uint8_t(count);
}
} // namespace l3k::periodic
#endif
