// The level walk: what the factorisations without a pivot search share (csx_ldl.hip with csx_schur.hip, csx_slu.hip, csx_hqr.hip;
// DESIGN.md §22).  Every column sits on a height level of its elimination tree, and the columns of one level are independent.
//   level_schedule   the launches of a run, decided once at build (host only; csx_level_schedule is its C face)
//   k_level<Col>     a level of more than WALK_WAVES columns: one launch, one wave per column
//   k_run<Col>       a run of narrower levels: one workgroup walks it, a barrier per level
//   walk_levels<Col> the stored schedule, launched
//   k_level_batch / k_run_batch / walk_levels_batch   the same for B value sets on one analysis: the member is a grid dimension,
//                    a batch policy says which arguments are a member's (csx_slu_batch.hip,
//                    csx_ldl_batch.hip, csx_hqr_batch.hip); the host side of a batch is csx_valuebatch.h (§39)
//   row_view         the rows of a CSC pattern with their storage positions (host only; csx_row_view is its C face)
//   LevelFactor     what the factor objects keep for it, with walk_init / walk_set_levels (build), walk_begin / walk_end (the frame
//                    of a run) and walk_refactor (new values on the kept pattern)
// Col is the column policy of a factorisation (LdlColumn, SluColumn, HqrColumn): Args, the types of its column function's kernel
// arguments with their const and __restrict__, and column(j, wave, lane, args...), which names the per-wave LDS arrays and
// forwards to the column function.  The kernels take the arguments one by one under exactly those types: passed as one struct,
// or deduced from the call without the qualifiers, the level kernels come out with other register counts than the six kernels
// they replace.
// The column functions themselves, their flag and stat words and what a run commits stay with each factorisation.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "csx_internal.h"

namespace csx {

constexpr int WALK_WAVES = 4;                       // waves per workgroup = columns a walker takes per level (csx_chol.hip's CH_WAVES)
constexpr int WALK_NONE = 0x7fffffff;               // flags[0] of a run in which no column broke down
constexpr int32_t WALK_RUN_LEVELS = 256;            // levels one launch of the walker takes (Schur, LU, QR): a longer run is several launches
constexpr int32_t WALK_RUN_UNCAPPED = 0x7fffffff;   // ... or the whole run in one launch (LDL')

// ---- the scheduler: host only, no device types ------------------------------------------------------------------------------

struct LevelLaunch {
    bool wide;         // k_level on level l0, or k_run over the levels [l0, l1)
    int32_t l0, l1;
};

// The launches over the levels 0 .. nlev - 1 (level_ptr: nlev + 1 offsets into the columns by level), in order.  A level of more
// than `waves` columns is a launch of its own.  A run of narrower levels goes to the walker: a launch ends before the first wide
// level, after run_levels levels, or -- with a work figure per level -- before the level that would take its sum past run_work;
// a level that alone exceeds run_work is still taken, so every launch holds a level.  run_levels >= 1.
inline std::vector<LevelLaunch> level_schedule(const int32_t *level_ptr, int32_t nlev, int32_t waves, int32_t run_levels,
                                               const int64_t *work = nullptr, int64_t run_work = 0) {
    std::vector<LevelLaunch> out;
    auto narrow = [&](int32_t l) { return level_ptr[l + 1] - level_ptr[l] <= waves; };
    for (int32_t l = 0; l < nlev;) {
        if (!narrow(l)) {
            out.push_back({true, l, l + 1});
            l++;
            continue;
        }
        int32_t e = l;
        int64_t sum = 0;
        while (e < nlev && e - l < run_levels && narrow(e)) {
            if (work) {
                if (e > l && sum + work[e] > run_work) break;
                sum += work[e];
            }
            e++;
        }
        out.push_back({false, l, e});
        l = e;
    }
    return out;
}

// height levels: a leaf is at level 0, a column one above its highest child (parent[j] > j: one ascending pass); n = 0: no level
inline void height_levels(int32_t n, const int32_t *parent, std::vector<int32_t> &ptr, std::vector<int32_t> &cols) {
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

// The row view of a CSC pattern (n columns, n rows; p: n + 1 offsets from 0, i: p[n] rows) with its map to storage positions: row r
// holds (rc, rpos) = (column, position in i) of its entries at [rp[r], rp[r + 1]), the columns ascending, or descending; entries
// of one row in one column keep the same direction by position.  A counting sort by row: the columns are met ascending, and a
// row filled from its end holds them descending.  An empty row stays empty.  false (the outputs mean nothing): a row outside
// 0 .. n - 1.  (csx_row_view is its C face; the batches build A's rows ascending for |S|_1 and R's descending for cs_usolve.)
inline bool row_view(int32_t n, const int32_t *p, const int32_t *i, bool descending, std::vector<int32_t> &rp, std::vector<int32_t> &rc,
                     std::vector<int32_t> &rpos) {
    const size_t nz = n > 0 ? (size_t)p[n] : 0;
    rp.assign((size_t)n + 1, 0);
    for (size_t q = 0; q < nz; q++) {
        if (i[q] < 0 || i[q] >= n) return false;
        rp[(size_t)i[q] + 1]++;
    }
    for (int32_t r = 0; r < n; r++) rp[(size_t)r + 1] += rp[(size_t)r];
    rc.resize(nz);
    rpos.resize(nz);
    std::vector<int32_t> next(rp.begin() + (descending ? 1 : 0), rp.end() - (descending ? 0 : 1));
    for (int32_t j = 0; j < n; j++)
        for (int32_t q = p[j]; q < p[j + 1]; q++) {
            int32_t &slot = next[(size_t)i[(size_t)q]];
            const int32_t at = descending ? --slot : slot++;
            rc[(size_t)at] = j;
            rpos[(size_t)at] = q;
        }
    return true;
}

// ---- the device side --------------------------------------------------------------------------------------------------------

// (the stats kernels order magnitudes by abs_bits, csx_internal.h)

template <class... A>
struct ColumnArgs {};
template <class T>
struct AsGiven {   // (a parameter of this type deduces nothing: it is what the policy's list says, qualifiers included)
    using type = T;
};

// one wave per column of a level
template <class Col, class... A>
__global__ __launch_bounds__(64 * WALK_WAVES) void k_level(const int32_t *__restrict__ cols, int32_t count, A... a) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t c = (int64_t)blockIdx.x * WALK_WAVES + w;
    if (c >= count) return;
    Col::column(cols[c], w, lane, a...);
}

// One workgroup walks the levels [l0, l1), each of at most WALK_WAVES columns: wave w takes column w of the level, a barrier
// between levels makes the finished columns visible to the next.  The trip counts are the level pointers, the same for every
// wave, so every wave reaches every barrier.
template <class Col, class... A>
__global__ __launch_bounds__(64 * WALK_WAVES) void k_run(const int32_t *__restrict__ cols, const int32_t *__restrict__ level_ptr,
                                                        int32_t l0, int32_t l1, A... a) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int32_t l = l0; l < l1; l++) {
        const int32_t b = level_ptr[l], cnt = level_ptr[l + 1] - b;
        if (w < cnt) Col::column(cols[b + w], w, lane, a...);
        __syncthreads();
    }
}

// The same two kernels with a member dimension: B value sets on one analysis (one tree, one schedule), independent of each other
// (csx_slu_batch.hip, csx_ldl_batch.hip, csx_hqr_batch.hip).  Col is a BATCH policy: its column(j, member, wave, lane, args...) says which of the
// arguments belong to a member and by what stride they shift -- it offsets those and forwards to a column policy's column(),
// so the column function and its bits are the single factorisation's.  The templates know nothing else of the policy.
// k_level_batch: one wave per (column of the level, member), the member in grid y (at most WALK_BATCH_MAX of them).
template <class Col, class... A>
__global__ __launch_bounds__(64 * WALK_WAVES) void k_level_batch(const int32_t *__restrict__ cols, int32_t count, A... a) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t c = (int64_t)blockIdx.x * WALK_WAVES + w;
    if (c >= count) return;
    Col::column(cols[c], (int32_t)blockIdx.y, w, lane, a...);
}

// k_run_batch: one workgroup per member (grid x) walks the levels [l0, l1) with k_run's barriers
template <class Col, class... A>
__global__ __launch_bounds__(64 * WALK_WAVES) void k_run_batch(const int32_t *__restrict__ cols, const int32_t *__restrict__ level_ptr,
                                                              int32_t l0, int32_t l1, A... a) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int32_t l = l0; l < l1; l++) {
        const int32_t b = level_ptr[l], cnt = level_ptr[l + 1] - b;
        if (w < cnt) Col::column(cols[b + w], (int32_t)blockIdx.x, w, lane, a...);
        __syncthreads();
    }
}

constexpr int32_t WALK_BATCH_MAX = 65535;   // members of one batch: the y extent of a grid

// ---- the host side of a factor ----------------------------------------------------------------------------------------------

// What a factor object keeps for the walk; LdlFactor, SluFactor and HqrFactor derive from it.
struct LevelFactor {
    const char *who = "";                   // the entry points' prefix in error texts: "csx_ldl", "csx_schur", "csx_slu", "csx_hqr"
    int32_t m = 0, n = 0, anz = 0;          // A's shape and entries, and ...
    DevBuf<int32_t> p0, i0;                 // ... its pattern: every A2 of a refactor is checked against it
    DevBuf<int32_t> level_cols, level_ptr;  // height levels of the elimination tree: columns by level, ascending inside one
    std::vector<int32_t> level_ptr_h;
    std::vector<LevelLaunch> schedule;      // the launches of a run, in order
    DevBuf<int> flags;                      // [0] the smallest broken column or WALK_NONE; the rest is the column function's
    DevBuf<unsigned long long> stats;       // the stats kernel's words
    hipEvent_t ev_a = nullptr, ev_b = nullptr;
    int64_t level_launches = 0, run_launches = 0, long_cols = 0;   // of the last run (long_cols: counted by its kernels)
    int64_t breakdown = -1, kernel_us = 0;
    ~LevelFactor() {   // (not copyable: DevBuf members)
        if (ev_a) (void)hipEventDestroy(ev_a);
        if (ev_b) (void)hipEventDestroy(ev_b);
    }
    int64_t levels() const { return (int64_t)level_ptr_h.size() - 1; }
    int64_t launches() const { return level_launches + run_launches; }
};

// build: A's pattern kept, the flag and stat words allocated, the events made
inline int walk_init(LevelFactor *F, const Csc *A, const char *who, size_t nflags, size_t nstats) {
    F->who = who;
    F->m = A->m;
    F->n = A->n;
    F->anz = A->nnz;
    CSX_TRY(rf_keep_pattern(A, F->p0, F->i0));
    CSX_TRY(F->flags.alloc(nflags));
    CSX_TRY(F->stats.alloc(nstats));
    CSX_HIP(hipEventCreate(&F->ev_a));
    CSX_HIP(hipEventCreate(&F->ev_b));
    return CSX_OK;
}

// build: the schedule of F->level_ptr_h (level_schedule's caps), and the levels queued for the device.  cols: the columns by level
// (height_levels), which like F->level_ptr_h must stay alive until the context's stream is synchronised.
inline int walk_set_levels(LevelFactor *F, const std::vector<int32_t> &cols, int32_t run_levels, const int64_t *work = nullptr,
                           int64_t run_work = 0) {
    F->schedule = level_schedule(F->level_ptr_h.data(), (int32_t)F->levels(), WALK_WAVES, run_levels, work, run_work);
    CSX_TRY(upload(F->level_cols, cols));
    CSX_TRY(upload(F->level_ptr, F->level_ptr_h));
    return CSX_OK;
}

// the numeric launches of a run: F's schedule on the context's stream, counted; called as walk_levels<Col>(F, Col::Args(), ...)
template <class Col, class... A>
void walk_levels(LevelFactor *F, ColumnArgs<A...>, typename AsGiven<A>::type... a) {
    hipStream_t s = ctx().stream;
    const std::vector<int32_t> &lp = F->level_ptr_h;
    for (const LevelLaunch &L : F->schedule) {
        if (L.wide) {
            const int32_t cnt = lp[(size_t)L.l0 + 1] - lp[(size_t)L.l0];
            hipLaunchKernelGGL((k_level<Col, A...>), dim3((unsigned)((cnt + WALK_WAVES - 1) / WALK_WAVES)), dim3(64 * WALK_WAVES), 0, s,
                               F->level_cols.get() + lp[(size_t)L.l0], cnt, a...);
            F->level_launches++;
        } else {
            hipLaunchKernelGGL((k_run<Col, A...>), dim3(1), dim3(64 * WALK_WAVES), 0, s, F->level_cols.get(), F->level_ptr.get(), L.l0,
                               L.l1, a...);
            F->run_launches++;
        }
    }
}

// F's stored schedule for `members` value sets (1 .. WALK_BATCH_MAX): one launch per LevelLaunch whatever their number, the
// member in the grid.  F itself is only read: the launches are counted into level_launches / run_launches, the batch's own.
// Called as walk_levels_batch<Col>(F, members, &wide, &runs, Col::Args(), ...).
template <class Col, class... A>
void walk_levels_batch(const LevelFactor *F, int32_t members, int64_t *level_launches, int64_t *run_launches, ColumnArgs<A...>,
                       typename AsGiven<A>::type... a) {
    hipStream_t s = ctx().stream;
    const std::vector<int32_t> &lp = F->level_ptr_h;
    for (const LevelLaunch &L : F->schedule) {
        if (L.wide) {
            const int32_t cnt = lp[(size_t)L.l0 + 1] - lp[(size_t)L.l0];
            hipLaunchKernelGGL((k_level_batch<Col, A...>), dim3((unsigned)((cnt + WALK_WAVES - 1) / WALK_WAVES), (unsigned)members),
                               dim3(64 * WALK_WAVES), 0, s, F->level_cols.get() + lp[(size_t)L.l0], cnt, a...);
            ++*level_launches;
        } else {
            hipLaunchKernelGGL((k_run_batch<Col, A...>), dim3((unsigned)members), dim3(64 * WALK_WAVES), 0, s, F->level_cols.get(),
                               F->level_ptr.get(), L.l0, L.l1, a...);
            ++*run_launches;
        }
    }
}

// The frame of a run.  walk_begin: the flag and stat words set to flags0 / stats0 (host arrays that outlive the run), the launch
// counters to 0, event a.  The factor then queues its scatters, walk_levels and its stats kernel.  walk_end: event b, the words
// read back into hflags / hstats (synchronises), kernel_us, breakdown and *ok = 1 (no column broke down: the factor commits) or 0.
inline int walk_begin(LevelFactor *F, const int *flags0, size_t nflags, const unsigned long long *stats0, size_t nstats) {
    hipStream_t s = ctx().stream;
    F->level_launches = F->run_launches = 0;
    CSX_HIP(hipMemcpyAsync(F->flags, flags0, nflags * sizeof(int), hipMemcpyHostToDevice, s));
    CSX_HIP(hipMemcpyAsync(F->stats, stats0, nstats * sizeof(unsigned long long), hipMemcpyHostToDevice, s));
    CSX_HIP(hipEventRecord(F->ev_a, s));
    return CSX_OK;
}

inline int walk_end(LevelFactor *F, int *hflags, size_t nflags, unsigned long long *hstats, size_t nstats, int *ok) {
    hipStream_t s = ctx().stream;
    (void)hipEventRecord(F->ev_b, s);
    if (hipGetLastError() != hipSuccess ||
        hipMemcpyAsync(hflags, F->flags.get(), nflags * sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipMemcpyAsync(hstats, F->stats.get(), nstats * sizeof(unsigned long long), hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess) {
        set_error("%s: %s", F->who, hipGetErrorString(hipGetLastError()));
        (void)hipStreamSynchronize(s);
        return CSX_ERUNTIME;
    }
    float ms = 0.0f;
    F->kernel_us = hipEventElapsedTime(&ms, F->ev_a, F->ev_b) == hipSuccess ? (int64_t)(1e3 * ms) : 0;
    F->breakdown = hflags[0] == WALK_NONE ? -1 : hflags[0];
    *ok = F->breakdown < 0 ? 1 : 0;
    return CSX_OK;
}

// refactor: run(x2) on the values of A2 after the pattern check (*ok = -1, CSX_EINVAL: not A's pattern or length, nothing changes)
template <class Run>
int walk_refactor(LevelFactor *F, csx_handle_t hA2, int *ok, Run run) {
    *ok = -1;
    const double *x2 = nullptr;
    CSX_TRY(rf_values(hA2, F->m, F->n, F->anz, F->p0, F->i0, F->flags, &x2));
    if (!x2) {
        set_error("%s_refactor: A2 does not have the pattern (or the length) of the factored matrix", F->who);
        return CSX_EINVAL;
    }
    return run(x2);
}

}  // namespace csx
