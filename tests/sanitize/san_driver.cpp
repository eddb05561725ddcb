// Sanitizer leg (the reference's CI runs its test binary under ASan and UBSan, .github/workflows/ci.yml:39-134): the HOST-side product
// code (1-D tables, cube-mesh partitioner, mesh plan, native mesh / results files) and the CPU oracle in one executable built with
// -fsanitize=address,undefined -fno-sanitize-recover=all by tests/test_sanitizers_cpu.py.  No GPU code is involved (GPU AddressSanitizer
// is not available on the pool); every check below is also a functional one, so a wrong answer fails the run as a sanitizer report does.
#include "l3k.h"
#include "host/mesh_plan.hpp"
#include "host/tables.hpp"
#include "oracle.h"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static char last_error[512]; // what the host units refused last (meshPlan() compares the texts)
namespace l3k::dev
{
void setError(const char* fmt, ...) // (registry.cpp pulls in the device headers: the host units only need this)
{
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(last_error, sizeof last_error, fmt, ap);
    va_end(ap);
    std::fprintf(stderr, "%s\n", last_error);
}
} // namespace l3k::dev

#define CHECK(c)                                                                                                       \
    do                                                                                                                 \
    {                                                                                                                  \
        if (!(c))                                                                                                      \
        {                                                                                                              \
            std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #c);                                 \
            std::exit(1);                                                                                              \
        }                                                                                                              \
    } while (0)

static void tables()
{
    for (int p = 1; p <= 8; ++p)
        for (int nq : {p + 1, 2 * p})
        {
            const auto       blk = l3k::host::deviceTableBlock(p, nq);
            CHECK(!blk.empty());
            std::vector< double > I, D, x, w;
            l3k::host::basis1d(p, nq, I, D);
            l3k::host::glRule(nq, x, w);
            double sw = 0.;
            for (double v : w)
                sw += v;
            CHECK(std::fabs(sw - 2.) < 1e-13);
            for (int q = 0; q < nq; ++q) // partition of unity, derivatives sum to zero (tests/MappingTests.cpp)
            {
                double s = 0., d = 0.;
                for (int b = 0; b <= p; ++b)
                {
                    s += I[b * nq + q];
                    d += D[b * nq + q];
                }
                CHECK(std::fabs(s - 1.) < 1e-12 && std::fabs(d) < 1e-10);
            }
        }
}

struct Part
{
    l3k_hostmesh*     hm = nullptr;
    l3k_hostmesh_view v{};
    Part(const int (&ne)[3], int order, const int (&parts)[3], int rank, double perturb)
    {
        CHECK(l3k_cube_partition_create(ne, order, parts, rank, perturb, &hm) == 0);
        CHECK(l3k_hostmesh_view_get(hm, &v) == 0);
    }
    Part(const int (&ne)[2], int order, double perturb) // the quad mesh
    {
        CHECK(l3k_square_mesh_create(ne, order, perturb, &hm) == 0);
        CHECK(l3k_hostmesh_view_get(hm, &v) == 0);
    }
    ~Part() { l3k_hostmesh_destroy(hm); }
    l3k_mesh_desc desc(int dofs_per_node = 1, const uint8_t* dirichlet = nullptr) const
    {
        return {v.dim, v.order, v.n_elems, v.n_interior_elems, v.elem_nodes, v.elem_verts, v.n_owned_nodes, v.n_ghost_nodes, dofs_per_node, dirichlet};
    }
};

static void partitions()
{
    const int cases[][7] = {{3, 2, 2, 2, 2, 1, 1}, {2, 2, 2, 4, 1, 1, 1}, {4, 4, 4, 1, 2, 2, 2}, {5, 3, 2, 3, 2, 3, 1}, {1, 1, 1, 6, 1, 1, 1}};
    for (const auto& c : cases)
    {
        const int ne[3] = {c[0], c[1], c[2]}, parts[3] = {c[4], c[5], c[6]}, order = c[3], n_ranks = parts[0] * parts[1] * parts[2];
        int64_t   owned = 0, elems = 0, n_global = -1;
        for (int r = 0; r < n_ranks; ++r)
        {
            Part P(ne, order, parts, r, 0.1);
            owned += P.v.n_owned_nodes;
            elems += P.v.n_elems;
            n_global = P.v.n_global_nodes;
            const int     N     = (order + 1) * (order + 1) * (order + 1);
            const int64_t n_loc = P.v.n_owned_nodes + P.v.n_ghost_nodes;
            for (int64_t i = 0; i < P.v.n_elems * N; ++i)
                CHECK(P.v.elem_nodes[i] < n_loc);
            for (int k = 0; k < P.v.n_nbrs; ++k)
            {
                CHECK(P.v.nbr_rank[k] >= 0 && P.v.nbr_rank[k] < n_ranks && P.v.nbr_rank[k] != r);
                for (int64_t s = P.v.send_offsets[k]; s < P.v.send_offsets[k + 1]; ++s)
                    CHECK(P.v.send_nodes[s] >= 0 && P.v.send_nodes[s] < P.v.n_owned_nodes);
            }
            if (P.v.n_nbrs)
                CHECK(P.v.ghost_offsets[P.v.n_nbrs] == P.v.n_ghost_nodes);
        }
        CHECK(owned == n_global && elems == int64_t(ne[0]) * ne[1] * ne[2]);
        CHECK(n_global == int64_t(ne[0] * order + 1) * (ne[1] * order + 1) * (ne[2] * order + 1));
    }
    const int ne[3] = {2, 2, 2}, bad_parts[3] = {3, 1, 1}; // more parts than elements along x: an error, not a crash
    l3k_hostmesh* hm = nullptr;
    if (l3k_cube_partition_create(ne, 2, bad_parts, 0, 0., &hm) == 0)
        l3k_hostmesh_destroy(hm);
}

// ---- host/mesh_plan.cpp: every expected value below comes from the shape of the input, none from the code under test
using l3k::host::ColourPlan;
using l3k::host::MeshPlan;

static int analyse(const l3k_mesh_desc& d, MeshPlan& plan)
{
    return l3k::host::analyseMesh(&d, plan);
}
// corner node ids of a lexicographic brick of n[0] x n[1] x n[2] elements (n[2] = 0: quads) on its vertex grid
static std::vector< uint32_t > brickCorners(const int (&n)[3])
{
    const int               dim = n[2] ? 3 : 2, nv = 1 << dim, nz = n[2] ? n[2] : 1;
    std::vector< uint32_t > c;
    for (int k = 0; k < nz; ++k)
        for (int j = 0; j < n[1]; ++j)
            for (int i = 0; i < n[0]; ++i)
                for (int v = 0; v < nv; ++v)
                    c.push_back(uint32_t((i + (v & 1)) + (n[0] + 1) * ((j + ((v >> 1) & 1)) + (n[1] + 1) * (k + (v >> 2)))));
    return c;
}
// the pointer arrays partition each class, every position holds an item of its class and colour, ascending within a colour
static void checkColourPlan(const ColourPlan& p, int64_t n_items, int64_t n_first, int n_colours)
{
    CHECK(int64_t(p.colour.size()) == n_items && int64_t(p.order.size()) == n_items);
    std::vector< int > seen(size_t(n_items), 0);
    for (int cls = 0; cls < 2; ++cls)
    {
        const int64_t lo = cls ? n_first : 0, hi = cls ? n_items : n_first;
        CHECK(int(p.ptr[cls].size()) == n_colours + 1 && p.ptr[cls].front() == lo && p.ptr[cls].back() == hi);
        for (int c = 0; c < n_colours; ++c)
        {
            CHECK(p.ptr[cls][c] <= p.ptr[cls][c + 1]);
            for (int64_t pos = p.ptr[cls][c]; pos < p.ptr[cls][c + 1]; ++pos)
            {
                const int64_t item = p.order[size_t(pos)];
                CHECK(item >= lo && item < hi && p.colour[size_t(item)] == c); // no item crosses the split
                CHECK(pos == p.ptr[cls][c] || p.order[size_t(pos - 1)] < item); // stable within a colour
                ++seen[size_t(item)];
            }
        }
    }
    for (int s : seen)
        CHECK(s == 1);
}
static void colouring()
{
    const int bricks[2][3] = {{3, 3, 2}, {4, 3, 0}};
    for (const auto& n : bricks)
    {
        const int     nv      = n[2] ? 8 : 4, n_colours = nv;
        const int64_t n_items = int64_t(n[0]) * n[1] * (n[2] ? n[2] : 1);
        const auto    corners = brickCorners(n);
        std::vector< int64_t > self(static_cast< size_t >(n_items));
        for (int64_t e = 0; e < n_items; ++e)
            self[size_t(e)] = e;
        for (int64_t n_first : {n_items, n_items / 2, int64_t(0)}) // one class, a split in the middle of the list, the other class
        {
            ColourPlan p;
            CHECK(l3k::host::colourItems(n_items, n_first, self.data(), corners.data(), nv, "", p) == 0);
            for (int64_t e = 0; e < n_items; ++e) // what first-fit yields in lexicographic order
            {
                const int i = int(e % n[0]), j = int((e / n[0]) % n[1]), k = int(e / (n[0] * n[1]));
                CHECK(p.colour[size_t(e)] == (i & 1) + 2 * (j & 1) + 4 * (k & 1));
            }
            checkColourPlan(p, n_items, n_first, n_colours);
        }
    }
    // sides: all six faces of a 2 x 2 x 2 brick, face by face (every element is a corner element and lists three sides)
    const int              two[3]  = {2, 2, 2};
    const auto             corners = brickCorners(two);
    std::vector< int64_t > fe;
    for (int side = 0; side < 6; ++side)
        for (int e = 0; e < 8; ++e)
            if (((e >> (2 - side / 2)) & 1) == (side & 1)) // sides 0 z-, 1 z+, 2 y-, 3 y+, 4 x-, 5 x+
                fe.push_back(e);
    CHECK(fe.size() == 24);
    ColourPlan p;
    CHECK(l3k::host::colourItems(24, 10, fe.data(), corners.data(), 8, " for the boundary sides", p) == 0);
    int n_colours = 0;
    for (uint8_t c : p.colour)
        n_colours = std::max(n_colours, c + 1);
    checkColourPlan(p, 24, 10, n_colours);
    for (size_t a = 0; a < 24; ++a)
        for (size_t b = a + 1; b < 24; ++b)
        {
            bool common = false;
            for (int v = 0; v < 8; ++v)
                for (int w = 0; w < 8; ++w)
                    common = common || corners[size_t(fe[a]) * 8 + v] == corners[size_t(fe[b]) * 8 + w];
            CHECK(!(common && p.colour[a] == p.colour[b])); // (in particular the three sides of one element differ)
        }
    // the cap: one element 65 times needs 65 colours -- refused, each caller with its text
    const std::vector< int64_t > same(65, 0);
    CHECK(l3k::host::colourItems(65, 65, same.data(), corners.data(), 8, " for the boundary sides", p) == -1);
    CHECK(std::strcmp(last_error, "deterministic mode: more than 64 colours needed for the boundary sides") == 0);
    CHECK(l3k::host::colourItems(65, 0, same.data(), corners.data(), 8, "", p) == -1);
    CHECK(std::strcmp(last_error, "deterministic mode: more than 64 colours needed") == 0);
    CHECK(l3k::host::colourItems(64, 64, same.data(), corners.data(), 8, "", p) == 0 && p.colour[63] == 63);
}
static void sideLists()
{
    const int64_t          elem[5] = {3, 1, 4, 0, 3};
    const uint8_t          side[5] = {5, 0, 2, 3, 1};
    std::vector< int64_t > fe;
    std::vector< uint8_t > fs;
    CHECK(l3k::host::interiorSidesFirst(2, 5, elem, side, fe, fs) == 2); // elements 0 and 1 are the interior ones
    CHECK((fe == std::vector< int64_t >{1, 0, 3, 4, 3}) && (fs == std::vector< uint8_t >{0, 3, 5, 2, 1}));
    CHECK(l3k::host::checkSides(3, 5, 5, elem, side) == 0);
    CHECK(l3k::host::checkSides(3, 4, 5, elem, side) == -1); // element 4 of 4
    CHECK(std::strcmp(last_error, "side 2 = (element 4, side 2) is outside the mesh") == 0);
    CHECK(l3k::host::checkSides(2, 5, 5, elem, side) == -1); // side 5 of a quad
    CHECK(std::strcmp(last_error, "side 0 = (element 3, side 5) is outside the mesh") == 0);
    const int64_t neg[1] = {-1};
    CHECK(l3k::host::checkSides(3, 5, 1, neg, side) == -1);
}
static void exclusiveRangeAndSlots()
{
    const int ne[3] = {3, 2, 2}, one[3] = {1, 1, 1};
    for (int p : {1, 2, 3})
    {
        // host/cube_mesh.cpp numbers [owned non-internal | element-internal, contiguous per element | ghosts]: on one rank the
        // internal nodes are the last n_elems (p-1)^3 owned ones, and no other node has a single element
        Part          P(ne, p, one, 0, 0.1);
        const int     n1 = p + 1, N = n1 * n1 * n1, n_int = (p - 1) * (p - 1) * (p - 1);
        const int64_t n  = P.v.n_owned_nodes;
        MeshPlan      plan;
        CHECK(analyse(P.desc(), plan) == 0);
        CHECK(plan.exclusive_end == n && plan.exclusive_begin == n - P.v.n_elems * n_int); // (order 1: empty)
        // the slot table: a permutation of [0, N); the shell of the middle element in ascending node id, then its internal nodes
        const auto internal = [&](int i) {
            const int x = i % n1, y = (i / n1) % n1, z = i / (n1 * n1);
            return x > 0 && x < p && y > 0 && y < p && z > 0 && z < p;
        };
        const uint32_t*    ids = P.v.elem_nodes + (P.v.n_elems / 2) * N;
        std::vector< int > expect(static_cast< size_t >(N));
        for (int i = 0; i < N; ++i)
            expect[size_t(i)] = i;
        std::sort(expect.begin(), expect.end(), [&](int x, int y) { return internal(x) != internal(y) ? internal(y) : ids[x] < ids[y]; });
        CHECK(plan.n_shell == N - n_int && int(plan.slot_tab.size()) == n1 * n1 * 8);
        for (int s = 0; s < N; ++s) // (expect is a permutation of the positions, so the slots read back are one of [0, N))
        {
            const int i = expect[size_t(s)];
            CHECK(plan.slot_tab[size_t(i % (n1 * n1)) * 8 + i / (n1 * n1)] == s && internal(i) == (s >= plan.n_shell));
        }
        if (p == 1)
            continue;
        // an element-internal node swapped with node 0: an internal node outside the tail, no exclusive range
        std::vector< uint32_t > nodes(P.v.elem_nodes, P.v.elem_nodes + P.v.n_elems * N);
        const uint32_t          inner = nodes[size_t(1 + n1 + n1 * n1)]; // local (1, 1, 1) of element 0
        for (auto& id : nodes)
            id = id == 0 ? inner : (id == inner ? 0 : id);
        l3k_mesh_desc d = P.desc();
        d.elem_nodes    = nodes.data();
        CHECK(analyse(d, plan) == 0 && plan.exclusive_begin == plan.exclusive_end);
        // a node id one past the local range, in the last entry: refused before anything is indexed with it
        nodes.back() = uint32_t(P.v.n_owned_nodes);
        char text[128];
        std::snprintf(text, sizeof text, "elem_nodes[%lld] = %u is outside the local node range [0,%lld)", (long long)nodes.size() - 1,
                      nodes.back(), (long long)P.v.n_owned_nodes);
        CHECK(analyse(d, plan) == -1 && std::strcmp(last_error, text) == 0);
    }
    MeshPlan plan; // no table for p + 1 > 8 and none for quads
    Part     P8(one, 8, one, 0, 0.);
    CHECK(analyse(P8.desc(), plan) == 0 && plan.slot_tab.empty() && plan.n_shell == 0);
    CHECK(plan.exclusive_end == 729 && plan.exclusive_begin == 729 - 343);
    const int nq[2] = {4, 3};
    Part      Q(nq, 3, 0.1);
    CHECK(analyse(Q.desc(), plan) == 0 && plan.slot_tab.empty() && plan.n_shell == 0);
    CHECK(plan.exclusive_end == Q.v.n_owned_nodes && plan.exclusive_begin == Q.v.n_owned_nodes - 12 * 4);
}
static void elementFlags()
{
    // (4, 2, 2) elements on the unit cube: every coordinate is a multiple of 1/4, the arithmetic below is exact
    const int ne[3] = {4, 2, 2}, one[3] = {1, 1, 1};
    Part      P(ne, 2, one, 0, 0.);
    MeshPlan  plan;
    CHECK(analyse(P.desc(), plan) == 0 && plan.all_affine && plan.owned_dirichlet_rows.empty());
    for (uint8_t f : plan.elem_flags)
        CHECK(f == 2);
    std::vector< double > verts(P.v.elem_verts, P.v.elem_verts + P.v.n_elems * 24);
    l3k_mesh_desc         d = P.desc();
    d.elem_verts            = verts.data();
    for (size_t i = 0; i < verts.size(); i += 3) // a uniform shear keeps every element a parallelepiped
        verts[i] += 0.25 * verts[i + 1] + 0.5 * verts[i + 2], verts[i + 1] += 0.5 * verts[i + 2];
    CHECK(analyse(d, plan) == 0 && plan.all_affine);
    for (uint8_t f : plan.elem_flags)
        CHECK(f == 2);
    // the vertex (1/4, 1/2, 1/2) moved off its planes: the 8 of 16 elements around it lose the bit, no other
    std::copy(P.v.elem_verts, P.v.elem_verts + P.v.n_elems * 24, verts.begin());
    std::vector< bool > owns(size_t(P.v.n_elems), false);
    for (size_t i = 0; i < verts.size(); i += 3)
        if (verts[i] == 0.25 && verts[i + 1] == 0.5 && verts[i + 2] == 0.5)
        {
            owns[i / 24] = true;
            verts[i] += 0.03, verts[i + 1] += 0.02, verts[i + 2] -= 0.01;
        }
    CHECK(std::count(owns.begin(), owns.end(), true) == 8);
    CHECK(analyse(d, plan) == 0 && !plan.all_affine);
    for (int64_t e = 0; e < P.v.n_elems; ++e)
        CHECK(plan.elem_flags[size_t(e)] == (owns[size_t(e)] ? 0 : 2));
    // quads: the domain's corner (0, 0) belongs to one element; moved, that element is a trapezoid
    const int nq[2] = {4, 2};
    Part      Q(nq, 2, 0.);
    CHECK(analyse(Q.desc(), plan) == 0 && plan.all_affine);
    std::vector< double > qv(Q.v.elem_verts, Q.v.elem_verts + Q.v.n_elems * 12);
    int64_t               trapezoid = -1;
    for (size_t i = 0; i < qv.size(); i += 3)
        if (qv[i] == 0. && qv[i + 1] == 0.)
        {
            CHECK(trapezoid == -1);
            trapezoid = int64_t(i / 12);
            qv[i] -= 0.0625;
        }
    l3k_mesh_desc dq = Q.desc();
    dq.elem_verts    = qv.data();
    CHECK(trapezoid >= 0 && analyse(dq, plan) == 0 && !plan.all_affine);
    for (int64_t e = 0; e < Q.v.n_elems; ++e)
        CHECK(plan.elem_flags[size_t(e)] == (e == trapezoid ? 0 : 2));
    // Dirichlet: the second of two dofs per node on the side y = 0 of the second of two parts (owned and ghost nodes on it);
    // bit 0 = the element has a vertex with y = 0, the rows = the owned part of the mask in ascending order
    const int              parts[3] = {2, 1, 1};
    Part                   R(ne, 2, parts, 1, 0.);
    const int64_t          n_loc = R.v.n_owned_nodes + R.v.n_ghost_nodes;
    std::vector< uint8_t > mask(size_t(n_loc) * 2, 0);
    std::vector< int64_t > rows;
    bool                   ghost_masked = false;
    for (int64_t i = 0; i < n_loc; ++i)
        if (R.v.node_boundary[i] & (1 << 2))
        {
            mask[size_t(i) * 2 + 1] = 1;
            if (i < R.v.n_owned_nodes)
                rows.push_back(i * 2 + 1);
            ghost_masked = ghost_masked || i >= R.v.n_owned_nodes;
        }
    CHECK(!rows.empty() && ghost_masked);
    CHECK(analyse(R.desc(2, mask.data()), plan) == 0 && plan.owned_dirichlet_rows == rows);
    for (int64_t e = 0; e < R.v.n_elems; ++e)
    {
        bool on_side = false;
        for (int v = 0; v < 8; ++v)
            on_side = on_side || R.v.elem_verts[e * 24 + v * 3 + 1] == 0.;
        CHECK(plan.elem_flags[size_t(e)] == (on_side ? 3 : 2));
    }
}
static void meshPlan()
{
    colouring();
    sideLists();
    exclusiveRangeAndSlots();
    elementFlags();
}

// the oracle on a partition: sum-factorised mesh apply == sum over the elements of K_e x_e (local assembly), diag == diag K
static void oracle(int kernel_id, int p)
{
    int dim, E, U, F;
    CHECK(orc_kernel_params(kernel_id, &dim, &E, &U, &F) == 0 && dim == 3);
    const int ne[3] = {2, 1, 2}, parts[3] = {1, 1, 1};
    Part      P(ne, p, parts, 0, 0.15);
    const int N = (p + 1) * (p + 1) * (p + 1), Nd = N * U, nq = orc_n_qps1d(p, 1, 0);
    const int64_t          n = P.v.n_owned_nodes, nd = n * U;
    std::vector< int >     finds(U);
    for (int u = 0; u < U; ++u)
        finds[u] = u;
    std::vector< double > fields(size_t(F > 0 ? F : 1) * n);
    for (size_t i = 0; i < fields.size(); ++i)
        fields[i] = std::sin(0.37 * double(i) + 0.1);
    orc_mesh m{3, p, nq, P.v.n_elems, P.v.elem_nodes, P.v.elem_verts, n, U, finds.data(), nullptr, F ? fields.data() : nullptr};
    std::vector< double > x(nd), y(nd, 0.), yref(nd, 0.), diag(nd, 0.), rhs(nd, 0.), dref(nd, 0.);
    for (int64_t i = 0; i < nd; ++i)
        x[i] = std::cos(0.11 * double(i));
    for (int threads : {1, 3})
    {
        std::fill(y.begin(), y.end(), 0.);
        CHECK(orc_mf_apply(&m, kernel_id, nullptr, 0.25, 1, 1, x.data(), nd, y.data(), nd, 1., 0., 0, P.v.n_elems, 1, 1, nd, threads) == 0);
    }
    CHECK(orc_mf_diag_rhs(&m, kernel_id, nullptr, 0.25, 1, nullptr, 0, diag.data(), rhs.data(), nd, 0, P.v.n_elems, 1, nd, 1) == 0);
    std::vector< double > K(size_t(Nd) * Nd), Fe(Nd), nf(size_t(N) * (F > 0 ? F : 1));
    for (int64_t e = 0; e < P.v.n_elems; ++e)
    {
        const uint32_t* en = P.v.elem_nodes + e * N;
        for (int i = 0; i < N; ++i)
            for (int f = 0; f < F; ++f)
                nf[size_t(i) * F + f] = fields[size_t(f) * n + en[i]];
        CHECK(orc_assemble_local(kernel_id, p, nq, 1, P.v.elem_verts + e * 24, F ? nf.data() : nullptr, nullptr, 0.25, K.data(), Fe.data()) == 0);
        for (int i = 0; i < Nd; ++i)
        {
            double s = 0.;
            for (int j = 0; j < Nd; ++j)
                s += K[size_t(i) * Nd + j] * x[size_t(en[j / U]) * U + j % U];
            yref[size_t(en[i / U]) * U + i % U] += s;
            dref[size_t(en[i / U]) * U + i % U] += K[size_t(i) * Nd + i];
        }
    }
    double err = 0., nrm = 0., derr = 0.;
    for (int64_t i = 0; i < nd; ++i)
    {
        err += (y[i] - yref[i]) * (y[i] - yref[i]);
        nrm += yref[i] * yref[i];
        derr = std::fmax(derr, std::fabs(diag[i] - dref[i]) / (1. + std::fabs(dref[i])));
    }
    CHECK(std::sqrt(err) < 1e-11 * std::sqrt(nrm) && derr < 1e-11);
}

static void files(const char* dir)
{
    // results file: two writers (node ranges), one reader
    const std::string     rp = std::string(dir) + "/san_results.bin";
    const int64_t         n_global = 37, split = 20;
    const size_t          n_fields = 3;
    std::vector< double > a(n_fields * split), b(n_fields * (n_global - split));
    for (size_t f = 0; f < n_fields; ++f)
    {
        for (int64_t i = 0; i < split; ++i)
            a[f * split + i] = double(100 * f + i);
        for (int64_t i = split; i < n_global; ++i)
            b[f * (n_global - split) + (i - split)] = double(100 * f + i);
    }
    CHECK(l3k_results_save(rp.c_str(), "sanitizer run", n_fields, n_global, 0, split, a.data(), split, 1) == 0);
    CHECK(l3k_results_save(rp.c_str(), "sanitizer run", n_fields, n_global, split, n_global - split, b.data(), n_global - split, 0) == 0);
    size_t nf = 0, nn = 0;
    CHECK(l3k_results_info(rp.c_str(), &nf, &nn) == 0 && nf == n_fields && nn == size_t(n_global));
    const int64_t ids[4] = {36, 0, 19, 20};
    double        out[4];
    CHECK(l3k_results_load(rp.c_str(), 2, 4, ids, 0, out) == 0);
    for (int k = 0; k < 4; ++k)
        CHECK(out[k] == double(200 + ids[k]));
    const int64_t bad[1] = {37};
    CHECK(l3k_results_load(rp.c_str(), 0, 1, bad, 0, out) != 0); // out of range: an error, not a read past the end
    std::remove(rp.c_str());

    // mesh file: two parts (order 2: one hex domain of two elements + a boundary domain of quads; an empty part), read back
    const std::string       mp = std::string(dir) + "/san_mesh.bin";
    std::vector< uint64_t > hn(2 * 27), qn(3 * 9), hid = {0, 1}, qid = {2, 3, 4};
    std::vector< double >   hv(2 * 8 * 3), qv(3 * 4 * 3);
    for (size_t i = 0; i < hn.size(); ++i)
        hn[i] = 3 * i + 1;
    for (size_t i = 0; i < qn.size(); ++i)
        qn[i] = 5 * i;
    for (size_t i = 0; i < hv.size(); ++i)
        hv[i] = 0.25 * double(i);
    for (size_t i = 0; i < qv.size(); ++i)
        qv[i] = -0.5 * double(i);
    l3k_meshfile_domain doms[2]{};
    doms[0].id  = 0;
    doms[0].hex = {2, hn.data(), hv.data(), hid.data()};
    doms[1].id   = 7;
    doms[1].quad = {3, qn.data(), qv.data(), qid.data()};
    const uint16_t         bids[1] = {7};
    l3k_meshfile_part_desc d0{2, 2, doms, 11, 40, 1, bids}, d1{2, 0, nullptr, 0, 0, 0, nullptr};
    size_t                 bytes[2];
    CHECK(l3k_meshfile_part_bytes(&d0, &bytes[0]) == 0 && l3k_meshfile_part_bytes(&d1, &bytes[1]) == 0);
    CHECK(l3k_meshfile_save(mp.c_str(), "two parts", 2, bytes, 1, &d1, 0) == 0); // (any order of the ranks' calls)
    CHECK(l3k_meshfile_save(mp.c_str(), "two parts", 2, bytes, 0, &d0, 1) == 0);
    size_t np = 0, pb[2] = {0, 0};
    CHECK(l3k_meshfile_info(mp.c_str(), &np, pb, 2) == 0 && np == 2 && pb[0] == bytes[0] && pb[1] == bytes[1]);
    l3k_meshfile_part* part = nullptr;
    CHECK(l3k_meshfile_load(mp.c_str(), 0, 2, &part) == 0);
    l3k_meshfile_part_desc r{};
    CHECK(l3k_meshfile_part_get(part, &r) == 0);
    CHECK(r.n_domains == 2 && r.nodes_begin == 11 && r.n_owned_nodes == 40 && r.n_boundary_ids == 1 && r.boundary_ids[0] == 7);
    CHECK(r.domains[0].hex.n == 2 && r.domains[1].quad.n == 3);
    CHECK(std::memcmp(r.domains[0].hex.nodes, hn.data(), hn.size() * 8) == 0 && std::memcmp(r.domains[1].quad.verts, qv.data(), qv.size() * 8) == 0);
    CHECK(l3k_meshfile_part_destroy(part) == 0);
    CHECK(l3k_meshfile_load(mp.c_str(), 1, 2, &part) == 0);
    CHECK(l3k_meshfile_part_get(part, &r) == 0 && r.n_domains == 0);
    CHECK(l3k_meshfile_part_destroy(part) == 0);
    CHECK(l3k_meshfile_load(mp.c_str(), 2, 2, &part) != 0); // no such part
    CHECK(l3k_meshfile_load(mp.c_str(), 0, 3, &part) != 0); // the sizes do not parse as an order-3 mesh: refused
    // a truncated file is refused, not read past its end
    {
        FILE* f = std::fopen(mp.c_str(), "rb");
        CHECK(f != nullptr);
        std::vector< char > all(1 << 16);
        const size_t        got = std::fread(all.data(), 1, all.size(), f);
        std::fclose(f);
        const std::string tp = std::string(dir) + "/san_mesh_truncated.bin";
        f                    = std::fopen(tp.c_str(), "wb");
        std::fwrite(all.data(), 1, got - 40, f);
        std::fclose(f);
        CHECK(l3k_meshfile_load(tp.c_str(), 1, 2, &part) != 0 || l3k_meshfile_part_destroy(part) == 0);
        CHECK(l3k_meshfile_load(tp.c_str(), 0, 2, &part) != 0 || l3k_meshfile_part_destroy(part) == 0);
        std::remove(tp.c_str());
    }
    std::remove(mp.c_str());
}

int main(int argc, char** argv)
{
    const char* dir = argc > 1 ? argv[1] : "/tmp";
    tables();
    partitions();
    meshPlan();
    oracle(0, 2);  // Diffusion3D
    oracle(0, 3);
    oracle(1, 2);  // variable coefficient from an external field
    oracle(10, 2); // operators and rhs read the point and the time
    files(dir);
    std::puts("sanitizer driver: ok");
    return 0;
}
