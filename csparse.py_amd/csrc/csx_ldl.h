// What the factorisations on the Cholesky pattern without a pivot search share (csx_ldl.hip, csx_slu.hip, csx_schur.hip): the
// search of a row in a column's ascending row list, the height levels of the elimination tree, and -- for the partial
// elimination of csx_schur.hip -- the LDL' column launches and the pivot statistics of csx_ldl.hip behind declarations.
#pragma once
#include <algorithm>
#include <vector>

#include "csx_internal.h"

namespace csx {

constexpr int LDL_ACC = 512;    // column entries kept in LDS per wave (24 KB a workgroup); longer columns are updated in place in global memory
constexpr int LDL_WAVES = 4;    // waves per workgroup (csx_chol.hip's CH_WAVES)
constexpr int LDL_NONE = 0x7fffffff;
constexpr int32_t LDL_RUN_UNCAPPED = 0x7fffffff;   // ldl_launch_levels: the walker takes a whole run of narrow levels in one launch

__device__ __forceinline__ int32_t ldl_find_row(const int32_t *rows, int32_t len, int32_t r) {
    int32_t lo = 0, hi = len - 1;
    while (lo < hi) {
        const int32_t mid = (lo + hi) >> 1;
        if (rows[mid] < r) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// height levels: a leaf is at level 0, a column one above its highest child (parent[j] > j: one ascending pass)
inline void ldl_levels(int32_t n, const int32_t *parent, std::vector<int32_t> &ptr, std::vector<int32_t> &cols) {
    std::vector<int32_t> level((size_t)n, 0);
    int32_t nlev = 0;
    for (int32_t j = 0; j < n; j++) {
        const int32_t up = parent[j];
        if (up >= 0) level[(size_t)up] = std::max(level[(size_t)up], level[(size_t)j] + 1);
        nlev = std::max(nlev, level[(size_t)j] + 1);
    }
    ptr.assign((size_t)nlev + 1, 0);
    for (int32_t j = 0; j < n; j++) ptr[(size_t)level[(size_t)j] + 1]++;
    for (int32_t l = 0; l < nlev; l++) ptr[(size_t)l + 1] += ptr[(size_t)l];
    cols.resize((size_t)n);
    std::vector<int32_t> next(ptr.begin(), ptr.end() - 1);
    for (int32_t j = 0; j < n; j++) cols[(size_t)next[(size_t)level[(size_t)j]]++] = j;
}

// csx_ldl.hip: the numeric launches of the LDL' columns over the height levels level_ptr_h (host) / level_ptr, level_cols
// (device), queued on the context's stream: a level of more than LDL_WAVES columns is one launch of the wave-per-column kernel,
// a run of narrower levels goes to the one-workgroup walker, at most run_cap levels a launch.  Lx holds C in the slots of L on
// entry; d, flags[3] as ldl_column has them.  The launch counts are added to *level_launches / *run_launches.
void ldl_launch_levels(const std::vector<int32_t> &level_ptr_h, const int32_t *level_cols, const int32_t *level_ptr, const int32_t *Lp,
                       const int32_t *Li, double *Lx, double *d, const int32_t *row_ptr, const int32_t *row_col,
                       const int32_t *row_pos, double tau, int *flags, int32_t run_cap, int64_t *level_launches,
                       int64_t *run_launches);
// csx_ldl.hip: k_ldl_stats over the first n columns, queued; st[5] initialised to {0, 0, ~0, 0, 0} by the caller
void ldl_launch_stats(int32_t n, const int32_t *Lp, const double *Lx, const double *d, unsigned long long *st);

}  // namespace csx
