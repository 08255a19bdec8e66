// What the factorisations on the Cholesky pattern without a pivot search share (csx_ldl.hip, csx_slu.hip): the search of a row
// in a column's ascending row list and the height levels of the elimination tree.
#pragma once
#include <algorithm>
#include <vector>

#include "csx_internal.h"

namespace csx {

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

}  // namespace csx
