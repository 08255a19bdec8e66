// What the factorisations on the Cholesky pattern without a pivot search share (csx_ldl.hip, csx_slu.hip, csx_hqr.hip,
// csx_schur.hip): the search of a row in a column's ascending row list, the height levels of the elimination tree, and the one
// partial-LDL' factor object with its build, run and refactor (csx_ldl.hip), on which csx_ldl_factor (n1 = n: nothing kept) and
// csx_schur_factor (csx_schur.hip) both stand.
#pragma once
#include <algorithm>
#include <vector>

#include "csx_internal.h"

namespace csx {

constexpr int LDL_ACC = 512;    // column entries kept in LDS per wave (24 KB a workgroup); longer columns are updated in place in global memory
constexpr int LDL_WAVES = 4;    // waves per workgroup (csx_chol.hip's CH_WAVES)
constexpr int LDL_NONE = 0x7fffffff;
constexpr int32_t LDL_RUN_UNCAPPED = 0x7fffffff;   // LdlFactor::run_cap: the walker takes a whole run of narrow levels in one launch

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

// The partial LDL' of P A P' = Lp blockdiag(D1, S) Lp': the first n1 columns eliminated, the Schur complement S of the last
// ns = n - n1 left.  n1 == n is the LDL' factor itself: no trailing column, no chunk, an empty S, and Lp's pattern IS the full
// pattern.  Handles of both kinds (K_LDLFACTOR, K_SCHURFACTOR) own one of these.
struct LdlFactor {
    int32_t n = 0, n1 = 0, ns = 0, anz = 0, lnz = 0, head = 0;   // lnz: entries of the full pattern of chol(P A P'); head = its p[n1]
    int32_t run_cap = LDL_RUN_UNCAPPED;     // levels one launch of the walker takes: the entry point's choice
    const char *who = "";                   // "csx_ldl" / "csx_schur": the entry points' prefix in error texts
    DevBuf<int32_t> p0, i0;                 // A's pattern: every A2 of a refactor is checked against it
    const int32_t *Lp = nullptr, *Li = nullptr;   // the full pattern the kernels read: the committed L's own p / i for ns == 0, ...
    DevBuf<int32_t> fp, fi;                 // ... these for ns > 0 (L then holds the interior columns and a unit tail)
    DevBuf<int32_t> rp, rc, rpos;           // row view of the full pattern (chol_symbolic_device)
    DevBuf<int32_t> win;                    // the entry map
    DevBuf<int32_t> level_cols, level_ptr;  // height levels of the first n1 columns: columns by level, ascending inside one
    std::vector<int32_t> level_ptr_h;
    DevBuf<int32_t> ch_col, ch_row0;        // csx_schur.hip: the (column, first row) pairs of the trailing-column kernel
    int64_t chunks = 0;
    csx_handle_t hL = 0, hd = 0, hS = 0;    // the committed Lp, d, S: owned here, lent out by csx_ldl_parts / csx_schur_parts
    DevBuf<double> Lx, dd, Sx;              // scratch of a run: committed only when none of the n1 columns broke down
    DevBuf<int> flags;                      // [0] smallest broken column, [1] perturbed pivots, [2] columns updated in place
    DevBuf<unsigned long long> stats;       // k_ldl_stats
    hipEvent_t ev_a = nullptr, ev_b = nullptr;
    // csx_ldl_info / csx_schur_info, csx_ldl_stats / csx_schur_stats
    int64_t level_launches = 0, run_launches = 0, schur_launches = 0, long_cols = 0;   // long_cols: counted by the kernels of the last run
    int64_t pos = 0, neg = 0, perturbed = 0, breakdown = -1, kernel_us = 0;
    double min_d = 0.0, max_d = 0.0, max_l = 0.0;
    LdlFactor() = default;
    LdlFactor(const LdlFactor &) = delete;
    LdlFactor &operator=(const LdlFactor &) = delete;
    ~LdlFactor() {
        if (hL) (void)csx_free(hL);
        if (hd) (void)csx_free(hd);
        if (hS) (void)csx_free(hS);
        if (ev_a) (void)hipEventDestroy(ev_a);
        if (ev_b) (void)hipEventDestroy(ev_b);
    }
};

// csx_ldl.hip.  ldl_build: the analysis of A under the caller's S (host parent, cp, pinv) for the elimination of the first n1
// columns, and the committed parts allocated.  ldl_run: the factor of the values Ax (A's storage order) into the scratch arrays,
// with the statistics of what was computed; Lp.x, d and S are committed when none of the n1 columns broke down.  *ok: 1
// committed, 0 breakdown (nothing touched).  Synchronises.  ldl_refactor: ldl_run on the values of A2 after the pattern check
// (*ok = -1, CSX_EINVAL: not A's pattern or length); F null (a handle of another kind) is CSX_EINVAL with *ok untouched.
int ldl_build(Csc *A, const int32_t *parent, const int32_t *cp, const int32_t *pinv, int32_t n1, int32_t run_cap, const char *who,
              LdlFactor *F);
int ldl_run(LdlFactor *F, const double *Ax, double tau, int *ok);
int ldl_refactor(LdlFactor *F, csx_handle_t hA2, double tau, int *ok);
int ldl_stats(const LdlFactor *F, double *out);   // min |d|, max |d|, max |l| of the committed factor
// csx_schur.hip: k_schur_cols over F's chunks -- S into F->Sx from the finished first n1 columns in F->Lx / F->dd -- queued on
// the context's stream
void schur_launch_cols(const LdlFactor *F);

}  // namespace csx
