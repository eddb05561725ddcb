// mesh_plan.cpp -- see mesh_plan.hpp
#include "host/mesh_plan.hpp"

#include <algorithm>
#include <cmath>
#include <unordered_map>

namespace l3k::dev
{
void setError(const char* fmt, ...);
}

namespace l3k::host
{
using l3k::dev::setError;

int analyseMesh(const l3k_mesh_desc* d, MeshPlan& out)
{
    const int     dim     = d->dim;
    const int64_t N       = dim == 2 ? int64_t(d->order + 1) * (d->order + 1) : int64_t(d->order + 1) * (d->order + 1) * (d->order + 1);
    const int     nvd     = (1 << dim) * 3; // vertex coordinates per element: [2^dim][3]
    const int64_t n_nodes = d->n_owned_nodes + d->n_ghost_nodes;
    out                   = {};
    // operand shapes must match what the kernels assume: every node id inside [0, n_nodes)
    for (int64_t i = 0; i < d->n_elems * N; ++i)
        if (d->elem_nodes[i] >= static_cast< uint64_t >(n_nodes))
        {
            setError("elem_nodes[%lld] = %u is outside the local node range [0,%lld)", (long long)i, d->elem_nodes[i],
                     (long long)n_nodes);
            return -1;
        }
    // nodes referenced by exactly one element (the element-internal nodes of the reference's numbering,
    // mesh/LocalMeshView.hpp:425-458) can be scattered with plain stores: find the maximal owned tail range
    {
        std::vector< uint8_t > count(static_cast< size_t >(n_nodes), 0);
        for (int64_t i = 0; i < d->n_elems * N; ++i)
            if (count[d->elem_nodes[i]] < 2)
                ++count[d->elem_nodes[i]];
        int64_t b = d->n_owned_nodes;
        while (b > 0 && count[b - 1] == 1) // exactly one: a node no element touches still needs the beta scaling
            --b;
        out.exclusive_begin = b;
        out.exclusive_end   = d->n_owned_nodes;
        // The single-wave kernel decides "exclusive" by the LOCAL position (element-internal or not) instead of testing
        // every node id: shrink the range until it holds no node that sits on an element's shell, and drop it altogether
        // if some element-internal node lies outside it (numberings that do not put the internal nodes last).
        const int n1 = d->order + 1;
        auto      internal = [&](int64_t i) {
            const int ix = int(i % n1), iy = int((i / n1) % n1), iz = int(i / (n1 * n1));
            if (dim == 2)
                return ix > 0 && ix < n1 - 1 && iy > 0 && iy < n1 - 1;
            return ix > 0 && ix < n1 - 1 && iy > 0 && iy < n1 - 1 && iz > 0 && iz < n1 - 1;
        };
        int64_t max_shell = -1, min_internal = n_nodes;
        for (int64_t e = 0; e < d->n_elems; ++e)
            for (int64_t i = 0; i < N; ++i)
            {
                const int64_t id = d->elem_nodes[e * N + i];
                if (internal(i))
                    min_internal = std::min(min_internal, id);
                else if (id < d->n_owned_nodes)
                    max_shell = std::max(max_shell, id);
            }
        out.exclusive_begin = std::max(out.exclusive_begin, max_shell + 1);
        if (d->n_elems == 0 || d->order < 2 || min_internal < out.exclusive_begin)
            out.exclusive_begin = out.exclusive_end; // empty: every node is scattered with atomics
        // scatter slots: local nodes of a typical element (the middle one of the traversal) in ascending id order --
        // rows that are contiguous in y become contiguous slots; internal positions last.  Hexes only: the quad kernel
        // scatters in lexicographic order
        if (dim == 3 && d->n_elems > 0 && n1 <= 8)
        {
            const uint32_t*        ids = d->elem_nodes + (d->n_elems / 2) * N;
            std::vector< int32_t > order(static_cast< size_t >(N));
            for (int64_t i = 0; i < N; ++i)
                order[i] = int32_t(i);
            std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) {
                const bool ix = internal(x), iy = internal(y);
                return ix != iy ? iy : ids[x] < ids[y];
            });
            out.slot_tab.assign(static_cast< size_t >(n1 * n1 * 8), 0);
            for (int64_t s = 0; s < N; ++s)
            {
                const int32_t i                                    = order[s];
                out.slot_tab[(i % (n1 * n1)) * 8 + i / (n1 * n1)] = uint16_t(s);
                out.n_shell += !internal(i);
            }
        }
    }
    // per-element flags: bit 0 = the element touches a Dirichlet dof, bit 1 = its tri-linear map is affine (a
    // parallelepiped: the bilinear and trilinear coefficient vectors of the 8 vertices vanish), so its Jacobian is one
    // matrix -- the element kernel then inverts it once per element instead of once per quadrature point
    std::vector< uint8_t >& flags = out.elem_flags;
    flags.assign(static_cast< size_t >(d->n_elems), 0);
    for (int64_t e = 0; e < d->n_elems; ++e)
    {
        const double* v = d->elem_verts + e * nvd;
        double        scale = 0., dev = 0.;
        if (dim == 2) // bilinear quad: a parallelogram when the coefficient of xi*eta vanishes
        {
            for (int s = 0; s < 2; ++s)
            {
                const double c10 = -v[0 * 3 + s] + v[1 * 3 + s] - v[2 * 3 + s] + v[3 * 3 + s];
                const double c01 = -v[0 * 3 + s] - v[1 * 3 + s] + v[2 * 3 + s] + v[3 * 3 + s];
                const double c11 = v[0 * 3 + s] - v[1 * 3 + s] - v[2 * 3 + s] + v[3 * 3 + s];
                scale            = std::max({scale, std::fabs(c10), std::fabs(c01)});
                dev              = std::max(dev, std::fabs(c11));
            }
            if (dev <= 1e-14 * scale)
                flags[e] |= 2;
            continue;
        }
        for (int s = 0; s < 3; ++s)
        {
            auto c = [&](int sx, int sy, int sz) { // coefficient of xi^sx eta^sy zeta^sz (x 8)
                double acc = 0.;
                for (int k = 0; k < 8; ++k)
                    acc += ((sx && !(k & 1)) ? -1. : 1.) * ((sy && !(k & 2)) ? -1. : 1.) * ((sz && !(k & 4)) ? -1. : 1.) * v[k * 3 + s];
                return acc;
            };
            scale = std::max({scale, std::fabs(c(1, 0, 0)), std::fabs(c(0, 1, 0)), std::fabs(c(0, 0, 1))});
            dev   = std::max({dev, std::fabs(c(1, 1, 0)), std::fabs(c(1, 0, 1)), std::fabs(c(0, 1, 1)), std::fabs(c(1, 1, 1))});
        }
        if (dev <= 1e-14 * scale)
            flags[e] |= 2;
    }
    out.all_affine = d->n_elems > 0;
    for (uint8_t f : flags)
        out.all_affine = out.all_affine && (f & 2);
    if (d->dirichlet)
    {
        for (int64_t e = 0; e < d->n_elems; ++e)
            for (int64_t i = 0; i < N && !(flags[e] & 1); ++i)
                for (int k = 0; k < d->dofs_per_node; ++k)
                    if (d->dirichlet[int64_t(d->elem_nodes[e * N + i]) * d->dofs_per_node + k])
                    {
                        flags[e] |= 1;
                        break;
                    }
        for (int64_t i = 0; i < d->n_owned_nodes * d->dofs_per_node; ++i) // getOwnedDirichletDofs
            if (d->dirichlet[i])
                out.owned_dirichlet_rows.push_back(i);
    }
    return 0;
}

std::vector< uint32_t > cornerNodes(int dim, int order, int64_t n_elems, const uint32_t* elem_nodes)
{
    const int     n1 = order + 1, nv = 1 << dim; // (quads: the 4 corners, v = i + 2j)
    const int64_t N  = dim == 2 ? int64_t(n1) * n1 : int64_t(n1) * n1 * n1;
    int           corner[8];
    for (int v = 0; v < nv; ++v)
        corner[v] = ((v & 1) ? n1 - 1 : 0) + n1 * (((v >> 1) & 1) ? n1 - 1 : 0) + n1 * n1 * (((v >> 2) & 1) ? n1 - 1 : 0);
    std::vector< uint32_t > out(static_cast< size_t >(n_elems) * nv);
    for (int64_t e = 0; e < n_elems; ++e)
        for (int v = 0; v < nv; ++v)
            out[size_t(e) * nv + v] = elem_nodes[e * N + corner[v]];
    return out;
}

int colourItems(int64_t n_items, int64_t n_first, const int64_t* elem_of, const uint32_t* corners, int nv, const char* error_suffix,
                ColourPlan& out)
{
    std::unordered_map< uint32_t, uint64_t > used; // corner node -> colours taken by the items around it
    used.reserve(static_cast< size_t >(n_items) * 2);
    std::vector< uint8_t >& colour = out.colour;
    colour.assign(static_cast< size_t >(n_items), 0);
    int n_colours = 0;
    for (int64_t i = 0; i < n_items; ++i)
    {
        const uint32_t* nodes = corners + size_t(elem_of[i]) * nv;
        uint64_t        taken = 0;
        for (int v = 0; v < nv; ++v)
        {
            const auto it = used.find(nodes[v]);
            if (it != used.end())
                taken |= it->second;
        }
        int c = 0;
        while (c < 64 && ((taken >> c) & 1u))
            ++c;
        if (c == 64)
        {
            setError("deterministic mode: more than 64 colours needed%s", error_suffix);
            return -1;
        }
        colour[i] = uint8_t(c);
        n_colours = std::max(n_colours, c + 1);
        for (int v = 0; v < nv; ++v)
            used[nodes[v]] |= uint64_t(1) << c;
    }
    std::vector< int64_t >& order = out.order;
    order.resize(static_cast< size_t >(n_items));
    for (int64_t i = 0; i < n_items; ++i)
        order[i] = i;
    auto by_colour = [&](int64_t x, int64_t y) { return colour[x] < colour[y]; };
    std::stable_sort(order.begin(), order.begin() + n_first, by_colour);
    std::stable_sort(order.begin() + n_first, order.end(), by_colour);
    for (int cls = 0; cls < 2; ++cls)
    {
        const int64_t b = cls ? n_first : 0, e = cls ? n_items : n_first;
        out.ptr[cls].assign(static_cast< size_t >(n_colours) + 1, e);
        int64_t i = b;
        for (int c = 0; c < n_colours; ++c)
        {
            out.ptr[cls][c] = i;
            while (i < e && colour[order[i]] == c)
                ++i;
        }
    }
    return 0;
}

int checkSides(int dim, int64_t n_elems, int64_t n_faces, const int64_t* face_elem, const uint8_t* face_side)
{
    for (int64_t i = 0; i < n_faces; ++i) // operand shapes must match what the kernel assumes
        if (face_elem[i] < 0 || face_elem[i] >= n_elems || face_side[i] >= 2 * dim)
        {
            setError("side %lld = (element %lld, side %d) is outside the mesh", (long long)i, (long long)face_elem[i],
                     int(face_side[i]));
            return -1;
        }
    return 0;
}

int64_t interiorSidesFirst(int64_t n_interior_elems, int64_t n_faces, const int64_t* face_elem, const uint8_t* face_side,
                           std::vector< int64_t >& fe, std::vector< uint8_t >& fs)
{
    // (they need no ghost data, like the interior elements themselves)
    int64_t n_interior_faces = 0;
    for (int pass = 0; pass < 2; ++pass)
    {
        for (int64_t i = 0; i < n_faces; ++i)
            if ((face_elem[i] >= n_interior_elems) == (pass == 1))
            {
                fe.push_back(face_elem[i]);
                fs.push_back(face_side[i]);
            }
        if (pass == 0)
            n_interior_faces = int64_t(fe.size());
    }
    return n_interior_faces;
}
} // namespace l3k::host
