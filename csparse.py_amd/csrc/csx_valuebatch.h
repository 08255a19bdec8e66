// What a value batch is, whatever its factorisation: B value sets on the analysis of one borrowed LevelFactor (DESIGN.md §39;
// csx_slu_batch.hip, csx_ldl_batch.hip, csx_hqr_batch.hip: §32, §36, §38).
//   ValueBatch       the borrowed factor and its handle, B, the flag (B x 3) and stat (B x nstats) words with their host copies of
//                    the last run, two events, the launch counters; SluBatch, LdlBatch, HqrBatch add their value planes
//   batch_get / batch_members_ok / batch_values / batch_limits   the guards of the entry points, with their texts
//   k_batch_init / k_batch_scatter   the words of a run set; every member's values through one or two entry maps
//   batch_alloc_common, batch_begin .. batch_end   the frame of a run -- walk_begin / walk_end of the single factors for B members.
//                    Between them the factorisation queues its scatter (batch_scatter), walk_levels_batch<its policy> and its
//                    stats kernel, itself: the walk's arguments go one by one under the policy's types (csx_levelwalk.h)
//   batch_norm1, batch_info_lower, batch_stats, batch_member   the bodies the entry points share
//   batch_solve_lower   the solve frame of the two lower factors on csx_batchsolve.h's sweeps and permutation kernel
// The batch policies, the stats and norm kernels, the choice of sweeps and permutations and QR's solve stay with each factorisation.
#pragma once
#include <cstring>
#include <memory>

#include "csx_batchsolve.h"

namespace csx {

struct ValueBatch {
    const char *who;          // the prefix of the error texts: "csx_slu_batch", "csx_ldl_batch", "csx_hqr_batch"
    int nstats, imin;         // stat words of a member; the one that is a minimum: it starts as ~0 and is 0 for n = 0
    LevelFactor *F = nullptr; // borrowed: valid while hF resolves to it (batch_get)
    csx_handle_t hF = 0;
    int32_t B = 0;
    DevBuf<int> flags;                          // per member: [0] the smallest broken column or WALK_NONE; the rest is the column function's
    DevBuf<unsigned long long> stats;           // per member: the stats kernel's words
    std::vector<int> hflags;                    // of the last run
    std::vector<unsigned long long> hstats;
    std::vector<double> htau;                   // the thresholds of a run on their way to the device
    hipEvent_t ev_a = nullptr, ev_b = nullptr;
    int64_t level_launches = 0, run_launches = 0, kernel_us = 0;
    ValueBatch(const char *who_, int nstats_, int imin_) : who(who_), nstats(nstats_), imin(imin_) {}
    ~ValueBatch() {   // (not copyable: DevBuf members)
        if (ev_a) (void)hipEventDestroy(ev_a);
        if (ev_b) (void)hipEventDestroy(ev_b);
    }
};

// ---- the guards ---------------------------------------------------------------------------------------------------------------

// the batch behind h, or null -- with a text when the factor it borrows has been freed.  Batch names its handle kinds (KIND,
// FACTOR_KIND) and its factor under its own type (factor())
template <class Batch>
Batch *batch_get(csx_handle_t h) {
    Batch *b = (Batch *)get(h, Batch::KIND);
    if (!b) return nullptr;
    if (get(b->hF, Batch::FACTOR_KIND) != (void *)b->factor()) {
        set_error("%s: the factor of this batch has been freed", b->who);
        return nullptr;
    }
    return b;
}

inline bool batch_members_ok(const char *who, int64_t B) {
    if (B >= 1 && B <= WALK_BATCH_MAX) return true;
    set_error("%s: B = %lld, a batch holds 1 .. %d members (split a larger family into several batches)", who, (long long)B,
              (int)WALK_BATCH_MAX);
    return false;
}

// the value block behind hV: nnz(A) x B doubles, row-major (entry q of member m at V[q B + m]), or null with a text
inline const double *batch_values(const char *who, csx_handle_t hV, int64_t anz, int32_t B) {
    const double *V = batch_block(hV, anz * B);
    if (!V) set_error("%s: V is not a block of nnz(A) x B = %lld x %d doubles", who, (long long)anz, (int)B);
    return V;
}

// the six constants every batch reports first
inline int batch_limits(int32_t *out) {
    if (!out) return CSX_EINVAL;
    out[0] = WALK_BATCH_MAX;
    out[1] = WALK_WAVES;
    out[2] = SLB_THREADS;
    out[3] = SLB_FETCH;
    out[4] = SLB_RUN_WAVES;
    out[5] = SLB_RUN_FETCH;
    return CSX_OK;
}

// ---- a run ----------------------------------------------------------------------------------------------------------------------

static __global__ __launch_bounds__(256) void k_batch_init(int32_t B, int nstats, int imin, int *flags, unsigned long long *stats) {
    const int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= B) return;
    flags[3 * m] = WALK_NONE;
    flags[3 * m + 1] = flags[3 * m + 2] = 0;
    for (int t = 0; t < nstats; t++) stats[nstats * m + t] = t == imin ? ~0ull : 0ull;
}

// slot q of member blockIdx.y, the n1 slots of the plane X1 first and the n2 of X2 after them: V is nnz x B, row-major (entry
// win[q] of member m at V[win[q] * B + m]; of duplicates the map's entry); a slot no entry lands in is +0.0
static __global__ __launch_bounds__(256) void k_batch_scatter(int64_t n1, int64_t n2, int32_t B, const int32_t *__restrict__ win1,
                                                              const int32_t *__restrict__ win2, const double *__restrict__ V,
                                                              double *__restrict__ X1, double *__restrict__ X2) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n1 + n2) return;
    const int64_t m = blockIdx.y;
    const int32_t a = q < n1 ? win1[q] : win2[q - n1];
    const double v = a >= 0 ? V[(int64_t)a * B + m] : 0.0;
    if (q < n1) X1[m * n1 + q] = v;
    else X2[m * n2 + (q - n1)] = v;
}

// every member's values into its member-major planes, one launch (none without a slot); n2 = 0: one plane
inline void batch_scatter(const ValueBatch *b, const double *V, int64_t n1, const int32_t *win1, double *X1, int64_t n2,
                          const int32_t *win2, double *X2) {
    if (n1 + n2)
        hipLaunchKernelGGL(k_batch_scatter, dim3((unsigned)((n1 + n2 + 255) / 256), (unsigned)b->B), dim3(256), 0, ctx().stream, n1, n2,
                           b->B, win1, win2, V, X1, X2);
}

// what every batch owns beside its value planes
inline int batch_alloc_common(ValueBatch *b, LevelFactor *F, csx_handle_t hF, int32_t B) {
    b->F = F;
    b->hF = hF;
    b->B = B;
    CSX_TRY(b->flags.alloc((size_t)B * 3));
    CSX_TRY(b->stats.alloc((size_t)B * (size_t)b->nstats));
    b->hflags.assign((size_t)B * 3, 0);
    b->hstats.assign((size_t)B * (size_t)b->nstats, 0);
    CSX_HIP(hipEventCreate(&b->ev_a));
    CSX_HIP(hipEventCreate(&b->ev_b));
    return CSX_OK;
}

// The frame of a run.  batch_begin: the thresholds checked before anything is queued (dtau: where the column policy reads them;
// null: the factorisation has none; tau null: all 0), the launch counters to 0, the flag and stat words set, event a.  The
// factorisation then queues its scatter, walk_levels_batch and its stats kernel.  batch_end: event b, the words read back (one
// synchronisation), kernel_us, ok[m] = 1 where no column of member m broke down.
inline int batch_begin(ValueBatch *b, const double *tau, double *dtau) {
    hipStream_t s = ctx().stream;
    const int32_t B = b->B;
    if (dtau) {
        b->htau.assign((size_t)B, 0.0);
        for (int32_t m = 0; tau && m < B; m++) {
            if (!(tau[m] >= 0.0)) {
                set_error("%s: tau[%d] is negative or NaN", b->who, (int)m);
                return CSX_EINVAL;
            }
            b->htau[(size_t)m] = tau[m];
        }
    }
    b->level_launches = b->run_launches = 0;
    if (dtau) CSX_HIP(hipMemcpyAsync(dtau, b->htau.data(), (size_t)B * sizeof(double), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_batch_init, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, s, B, b->nstats, b->imin, b->flags.get(),
                       b->stats.get());
    CSX_HIP(hipEventRecord(b->ev_a, s));
    return CSX_OK;
}

inline int batch_end(ValueBatch *b, int *ok) {
    hipStream_t s = ctx().stream;
    const size_t B = (size_t)b->B, ns = (size_t)b->nstats;
    (void)hipEventRecord(b->ev_b, s);
    if (hipGetLastError() != hipSuccess ||
        hipMemcpyAsync(b->hflags.data(), b->flags.get(), B * 3 * sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipMemcpyAsync(b->hstats.data(), b->stats.get(), B * ns * sizeof(unsigned long long), hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess) {
        set_error("%s: %s", b->who, hipGetErrorString(hipGetLastError()));
        (void)hipStreamSynchronize(s);
        return CSX_ERUNTIME;
    }
    float ms = 0.0f;
    b->kernel_us = hipEventElapsedTime(&ms, b->ev_a, b->ev_b) == hipSuccess ? (int64_t)(1e3 * ms) : 0;
    for (size_t m = 0; m < B; m++) {
        if (b->F->n == 0) b->hstats[ns * m + (size_t)b->imin] = 0;   // (no column ran: the minimum of nothing reads 0)
        ok[m] = b->hflags[3 * m] == WALK_NONE ? 1 : 0;
    }
    return CSX_OK;
}

// ---- the bodies the entry points share ----------------------------------------------------------------------------------------

// out[m] = the norm of member m: B words zeroed, `launch(best)` queues the factorisation's kernel, which takes the maximum over the
// bit patterns of its sums; one download, synchronises
template <class Launch>
int batch_norm1(int32_t B, double *out, Launch launch) {
    hipStream_t s = ctx().stream;
    DevBuf<unsigned long long> d;
    CSX_TRY(d.alloc((size_t)B));
    CSX_HIP(hipMemsetAsync(d, 0, (size_t)B * sizeof(unsigned long long), s));
    launch(d.get());
    CSX_LAUNCH_CHECK();
    static_assert(sizeof(double) == sizeof(unsigned long long), "the sums travel as their bit patterns");
    CSX_HIP(hipMemcpyAsync(out, d.get(), (size_t)B * sizeof(double), hipMemcpyDeviceToHost, s));
    CSX_HIP(hipStreamSynchronize(s));
    return CSX_OK;
}

// the info of a batch of lower factors (LU, LDL'): shared[8], members[5 B] as include/csx.h lays them out
inline void batch_info_lower(const ValueBatch *b, int64_t lnz, int64_t *shared, int64_t *members) {
    shared[0] = b->F->n;
    shared[1] = lnz;
    shared[2] = b->F->levels();
    shared[3] = b->level_launches + b->run_launches;
    shared[4] = b->level_launches;
    shared[5] = b->run_launches;
    shared[6] = b->kernel_us;
    shared[7] = b->B;
    for (int32_t m = 0; m < b->B; m++) {
        const int *f = &b->hflags[(size_t)3 * m];
        const unsigned long long *st = &b->hstats[(size_t)b->nstats * m];
        members[5 * m + 0] = f[1];
        members[5 * m + 1] = f[0] == WALK_NONE ? -1 : f[0];
        members[5 * m + 2] = f[2];
        members[5 * m + 3] = (int64_t)st[0];
        members[5 * m + 4] = (int64_t)st[1];
    }
}

// out[count m ..] = the stat words [first, first + count) of member m, which hold the bit patterns of doubles
inline void batch_stats(const ValueBatch *b, int first, int count, double *out) {
    for (int32_t m = 0; m < b->B; m++)
        std::memcpy(out + (size_t)count * m, &b->hstats[(size_t)b->nstats * m + (size_t)first], (size_t)count * sizeof(double));
}

// member m's piece of a member-major plane (stride len) queued for out; the caller synchronises
inline int batch_member(const double *plane, int32_t m, size_t len, double *out) {
    if (len) CSX_HIP(hipMemcpyAsync(out, plane + (size_t)m * len, len * sizeof(double), hipMemcpyDeviceToHost, ctx().stream));
    return CSX_OK;
}

// The solve frame of a lower factor: X (n x B r behind hX, row-major) into W[p_in[i], :] = X[i, :], `sweeps(W)` queues the
// factorisation's two batch_sweep calls, X[i, :] = W[p_out[i], :] with NaN in the columns of a failed member; synchronises.
// who: the entry point's name in the texts.
template <class Sweeps>
int batch_solve_lower(const ValueBatch *b, const char *who, csx_handle_t hX, int32_t r, const int32_t *p_in, const int32_t *p_out,
                      Sweeps sweeps) {
    const int64_t n = b->F->n, K = (int64_t)b->B * r;
    if (!batch_solve_fits(n, K)) {
        set_error("%s: B r = %lld columns are more than one launch takes", who, (long long)K);
        return CSX_EINVAL;
    }
    double *X = batch_block(hX, n * K);
    if (!X) {
        set_error("%s: X is not a block of n x B r = %lld x %lld doubles", who, (long long)n, (long long)K);
        return CSX_EINVAL;
    }
    if (n == 0) return CSX_OK;
    hipStream_t s = ctx().stream;
    DevBuf<double> W;
    CSX_TRY(W.alloc((size_t)(n * K)));
    const unsigned blocks = (unsigned)((n * K + 255) / 256);
    hipLaunchKernelGGL(k_batch_permute, dim3(blocks), dim3(256), 0, s, n, K, r, p_in, 1, (const int *)nullptr, (const double *)X, W.get());
    CSX_TRY(sweeps(W.get()));
    hipLaunchKernelGGL(k_batch_permute, dim3(blocks), dim3(256), 0, s, n, K, r, p_out, 0, (const int *)b->flags.get(),
                       (const double *)W.get(), X);
    CSX_LAUNCH_CHECK();
    CSX_HIP(hipStreamSynchronize(s));   // W goes out of scope
    return CSX_OK;
}

}  // namespace csx
