// tri_levels.cpp -- level scheduling for the sparse triangular solves of l3k_tri and its host-only entry point l3k_tri_levels (the
// reference hands the whole preconditioner to Ifpack2, solve/Ifpack2Preconditioners.hpp:97-101,134-157).
//
// 1. Active rows: the rows that store an entry.  Empty rows and the columns that belong to them stay out.
// 2. Lower solve: rows ascending, level(i) = 1 + max level(j) over the stored active j < i, 1 without one.  Upper solve: the mirror
//    image, rows descending over the stored active j > i.  A row's dependencies lie in strictly earlier levels.
// 3. The rows are listed level by level by a counting sort, which keeps them ascending within a level.
// 4. The launch plan (triPlan) groups consecutive narrow levels into fused launches.
#include "host/tri_levels.hpp"
#include "l3k.h"

#include <algorithm>

namespace l3k::dev
{
void setError(const char* fmt, ...);
}

namespace l3k::host
{
using l3k::dev::setError;

void triLevels(int64_t n, const int64_t* row_ptr, const int32_t* col_ind, bool upper, TriLevels& out)
{
    out.level.assign(size_t(n), 0);
    out.n_levels = out.max_rows = 0;
    int64_t    n_active = 0;
    const auto active   = [&](int64_t i) { return row_ptr[i + 1] > row_ptr[i]; };
    const auto visit    = [&](int64_t i) {
        if (!active(i))
            return;
        ++n_active;
        int32_t deepest = 0;
        for (int64_t e = row_ptr[i]; e < row_ptr[i + 1]; ++e)
        {
            const int64_t j = col_ind[e];
            if ((upper ? j > i : j < i) && active(j))
                deepest = std::max(deepest, out.level[size_t(j)]);
        }
        out.level[size_t(i)] = deepest + 1;
        out.n_levels         = std::max< int64_t >(out.n_levels, deepest + 1);
    };
    if (upper)
        for (int64_t i = n - 1; i >= 0; --i)
            visit(i);
    else
        for (int64_t i = 0; i < n; ++i)
            visit(i);
    out.level_ptr.assign(size_t(out.n_levels) + 1, 0);
    for (int64_t i = 0; i < n; ++i)
        if (out.level[size_t(i)] > 0)
            ++out.level_ptr[size_t(out.level[size_t(i)])];
    for (int64_t l = 0; l < out.n_levels; ++l)
    {
        out.max_rows = std::max(out.max_rows, out.level_ptr[size_t(l) + 1]);
        out.level_ptr[size_t(l) + 1] += out.level_ptr[size_t(l)];
    }
    out.rows.assign(size_t(n_active), 0);
    std::vector< int64_t > next(out.level_ptr.begin(), out.level_ptr.end());
    for (int64_t i = 0; i < n; ++i)
        if (out.level[size_t(i)] > 0)
            out.rows[size_t(next[size_t(out.level[size_t(i)]) - 1]++)] = int32_t(i);
}

std::vector< TriLaunch > triPlan(const TriLevels& lv, int64_t fuse_rows)
{
    std::vector< TriLaunch > plan;
    for (int64_t l = 0; l < lv.n_levels; ++l)
    {
        const bool narrow = lv.level_ptr[size_t(l) + 1] - lv.level_ptr[size_t(l)] <= fuse_rows;
        if (narrow && !plan.empty() && plan.back().fused && plan.back().l1 == l && l - plan.back().l0 < tri_max_fused_levels)
            plan.back().l1 = l + 1;
        else
            plan.push_back({l, l + 1, narrow});
    }
    return plan;
}

int triCheckGraph(int64_t n, const int64_t* row_ptr, const int32_t* col_ind, const char* who)
{
    if (n < 0 || n > INT32_MAX || !row_ptr)
    {
        setError("%s: need 0 <= n < 2^31 and a row_ptr", who);
        return -1;
    }
    if (row_ptr[0] != 0)
    {
        setError("%s: row_ptr[0] is not 0", who);
        return -1;
    }
    for (int64_t i = 0; i < n; ++i)
    {
        if (row_ptr[i + 1] < row_ptr[i])
        {
            setError("%s: row_ptr decreases at row %lld", who, (long long)i);
            return -1;
        }
        if (row_ptr[i + 1] > row_ptr[i] && !col_ind)
        {
            setError("%s: null col_ind for a graph with entries", who);
            return -1;
        }
        for (int64_t e = row_ptr[i]; e < row_ptr[i + 1]; ++e)
            if (col_ind[e] < 0 || col_ind[e] >= n || (e > row_ptr[i] && col_ind[e] <= col_ind[e - 1]))
            {
                setError("%s: the columns of row %lld are not strictly ascending inside [0, n)", who, (long long)i);
                return -1;
            }
    }
    return 0;
}

int64_t triFirstRowWithoutDiagonal(int64_t n, const int64_t* row_ptr, const int32_t* col_ind)
{
    for (int64_t i = 0; i < n; ++i)
        if (row_ptr[i + 1] > row_ptr[i] && !std::binary_search(col_ind + row_ptr[i], col_ind + row_ptr[i + 1], int32_t(i)))
            return i;
    return -1;
}
} // namespace l3k::host

extern "C" int l3k_tri_levels(int64_t n, const int64_t* row_ptr, const int32_t* col_ind, int upper, int32_t* level_out, int64_t* n_levels)
{
    if (!n_levels || (n > 0 && !level_out))
    {
        l3k::dev::setError("l3k_tri_levels: null argument");
        return -1;
    }
    if (int rc = l3k::host::triCheckGraph(n, row_ptr, col_ind, "l3k_tri_levels"))
        return rc;
    l3k::host::TriLevels lv;
    l3k::host::triLevels(n, row_ptr, col_ind, upper != 0, lv);
    std::copy(lv.level.begin(), lv.level.end(), level_out);
    *n_levels = lv.n_levels;
    return 0;
}
