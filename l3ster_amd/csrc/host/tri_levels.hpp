// tri_levels.hpp -- the symbolic phase of the triangular preconditioners (include/l3k.h: l3k_tri_create, l3k_tri_levels), host only:
// the active rows of a CSR graph, the level of every row for the lower and for the upper solve, the rows listed level by level,
// and the launch plan.  tests/tri_ref.py restates the levels in numpy; the two must give identical results.
#ifndef L3K_HOST_TRI_LEVELS_HPP
#define L3K_HOST_TRI_LEVELS_HPP

#include <cstddef>
#include <cstdint>
#include <vector>

namespace l3k::host
{
// the most levels one launch of a fused kernel walks: a single workgroup runs no longer than this many dependent steps
constexpr int64_t tri_max_fused_levels = 4096;

struct TriLevels
{
    int64_t                n_levels = 0, max_rows = 0;
    std::vector< int32_t > level;     // [n]: 1 .. n_levels on an active row, 0 on an empty one
    std::vector< int32_t > rows;      // [n_active]: level by level, ascending within a level
    std::vector< int64_t > level_ptr; // [n_levels + 1]: level l (0-based) is rows[level_ptr[l] .. level_ptr[l + 1])
};
// level(i) = 1 + max level(j) over the stored active j < i of row i (upper: j > i, rows walked downwards); no such j: 1.  A row is
// active if it stores an entry; entries in the column of an empty row do not count.  The graph must be valid (checked by the caller)
void triLevels(int64_t n, const int64_t* row_ptr, const int32_t* col_ind, bool upper, TriLevels& out);

// One launch of the plan: the levels [l0, l1).  fused: one workgroup walks them; else l1 = l0 + 1 and a grid walks the level
struct TriLaunch
{
    int64_t l0, l1;
    bool    fused;
};
// consecutive levels of at most fuse_rows rows form one fused launch of at most tri_max_fused_levels levels; every wider level
// is a launch of its own
std::vector< TriLaunch > triPlan(const TriLevels& lv, int64_t fuse_rows);

// 0, or -1 with the error set (prefixed with `who`): an invalid graph, as l3k_csr_create has it
int triCheckGraph(int64_t n, const int64_t* row_ptr, const int32_t* col_ind, const char* who);
// the first active row without a stored diagonal entry, or -1
int64_t triFirstRowWithoutDiagonal(int64_t n, const int64_t* row_ptr, const int32_t* col_ind);
} // namespace l3k::host
#endif
