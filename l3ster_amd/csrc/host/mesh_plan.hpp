// mesh_plan.hpp -- what the host works out about a mesh before anything is uploaded: the route the element kernels take, the
// colouring of deterministic mode, the side lists of boundary terms.  Plain C++, no device needed: tests/sanitize/san_driver.cpp
#ifndef L3K_HOST_MESH_PLAN_HPP
#define L3K_HOST_MESH_PLAN_HPP

#include "l3k.h"

#include <cstdint>
#include <vector>

namespace l3k::host
{
struct MeshPlan
{
    // the owned nodes that are internal to the one element that references them: stored, not added to (empty: begin == end)
    int64_t exclusive_begin = 0, exclusive_end = 0;
    // scatter order of the single-wave kernel (l3k_mesh::slot_tab); none for quads, for p + 1 > 8 and without elements
    std::vector< uint16_t > slot_tab;
    int                     n_shell = 0;
    std::vector< uint8_t >  elem_flags; // bit 0 = touches a Dirichlet dof, bit 1 = the (bi / tri)linear map is affine
    bool                    all_affine = false;
    std::vector< int64_t >  owned_dirichlet_rows; // ascending (getOwnedDirichletDofs)
};
// 0, or -1 with the error set: a node id outside the local range
int analyseMesh(const l3k_mesh_desc* d, MeshPlan& out);

// [n_elems][2^dim]: the corner nodes of every element, v = i + 2j (+ 4k)
std::vector< uint32_t > cornerNodes(int dim, int order, int64_t n_elems, const uint32_t* elem_nodes);

struct ColourPlan
{
    std::vector< uint8_t > colour; // [n_items] in the given order
    std::vector< int64_t > order;  // position -> item: each class (items [0, n_first) and the rest) stably sorted by colour
    std::vector< int64_t > ptr[2]; // ptr[cls][c] .. ptr[cls][c + 1] = the positions of colour c of class cls
};
// Greedy first-fit in the given order: item i takes the nodes corners[elem_of[i]][0 .. nv) and the lowest colour that no
// earlier item with one of them has.  0, or -1 with the error set ("... more than 64 colours needed" + error_suffix)
int colourItems(int64_t n_items, int64_t n_first, const int64_t* elem_of, const uint32_t* corners, int nv, const char* error_suffix,
                ColourPlan& out);

// every (element, side) inside a mesh of n_elems elements of dimension dim: 0, or -1 with the error set
int checkSides(int dim, int64_t n_elems, int64_t n_faces, const int64_t* face_elem, const uint8_t* face_side);
// the list with the sides of interior elements (below n_interior_elems) first, else in the given order; returns their number
int64_t interiorSidesFirst(int64_t n_interior_elems, int64_t n_faces, const int64_t* face_elem, const uint8_t* face_side,
                           std::vector< int64_t >& fe, std::vector< uint8_t >& fs);
} // namespace l3k::host
#endif
