// periodic.hpp -- the host-only side of the periodic boundary conditions (include/l3k.h: l3k_periodic_match, l3k_periodic_merge).
// The finiteness checks of l3k_periodic_match and the construction of its grid live in host/periodic.cpp for the reason given in
// host/chebyshev.hpp: the device translation units are built with -ffinite-math-only, which folds std::isfinite.  Not inline,
// operands read from memory.
#ifndef L3K_HOST_PERIODIC_HPP
#define L3K_HOST_PERIODIC_HPP

#include "device/periodic.hpp"

#include <cstddef>
#include <cstdint>
#include <string>

namespace l3k::host
{
bool allFinite(const double* v, size_t n);
// nullptr = fine, else what is wrong with the translation (its first dim entries) or the tolerance
const char* periodicCheckReals(int dim, const double* translation, const double* tolerance);
// The grid the destination nodes are binned on (device/periodic.hpp: Grid) over the box [box_lo, box_hi] that holds them.  The cell
// edge h is at least 2 tolerance, so that a partner lies in the source node's own or an adjacent cell, and coarse enough for
// cell_bits bits per axis with one cell of margin on either side.  Returns "" and the grid, or what is wrong with the box or the
// tolerance: an extent, 2 tolerance, h, 1 / h or lo - h that is not finite, 1 / h == 0, more cells than the key has bits for.
std::string periodicMakeGrid(int dim, const double* box_lo, const double* box_hi, double tolerance, l3k::periodic::Grid* grid);
// What l3k_periodic_match does between its argument checks and its first launch: every vertex of the listed sides' elements is
// finite (their first dim entries), the box of the vertices of the destination sides' elements (the destination nodes are convex
// combinations of them; no destination side: the origin), the grid over it.  Returns "" and the grid, or the refusal.
std::string periodicBoxAndGrid(int dim, const double* elem_verts, int64_t n_src, const int64_t* src_elem, int64_t n_dst,
                               const int64_t* dst_elem, double tolerance, l3k::periodic::Grid* grid);
} // namespace l3k::host
#endif
