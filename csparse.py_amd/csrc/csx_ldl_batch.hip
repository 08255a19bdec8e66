// Many symmetric value sets on the analysis of one L D L' (the definition is the comment of csx_ldl_batch_factor in
// include/csx.h).  An LdlBatch BORROWS an LdlFactor of kind K_LDLFACTOR (nothing kept: ns = 0) -- pattern, row view, entry map,
// height levels, launch schedule, permutation -- and owns B value sets: Lx (B x lnz doubles, member-major: member m's column j is
// the contiguous piece ldl_column expects), dd (B x n), tau (B), flags (B x 3), stats (B x 5).  It never writes the factor's L.x /
// d or its scratch, and keeps its own launch counters.
//   k_ldb_init / k_ldb_scatter   the flag and stat words; every member's values through win (of duplicates the last)
//   LdlBatchColumn   the batch policy of the level walk (csx_levelwalk.h: k_level_batch, k_run_batch): Lx by lnz, d by n, flags by
//                    3, tau read from an array, then LdlColumn::column -- ldl_column itself, the host rule's bits
//   k_ldb_stats      ldl_stats_column per (column, member)
//   k_ldb_norm1      |S_m|_1 by k_norm1_sym's rule
//   the solve        csx_batchsolve.h's sweeps: the rows of L ascending, then the dots of L descending with the division by d
//                    BEFORE each chain -- no pass of its own over X for D
// There is NO scratch-then-commit: a member that breaks down is marked failed (ok[m] = 0, its values mean nothing) where the
// single factor keeps its old values.
#include <cmath>
#include <cstring>

#include "csx_batchsolve.h"
#include "csx_internal.h"
#include "csx_ldl.h"

#pragma clang fp contract(off)

namespace csx {

struct LdlBatch {
    LdlFactor *F = nullptr;   // borrowed: valid while hF resolves to it
    csx_handle_t hF = 0;
    int32_t B = 0;
    DevBuf<double> Lx, dd, tau;
    DevBuf<int> flags;
    DevBuf<unsigned long long> stats;
    std::vector<int> hflags;                    // of the last run
    std::vector<unsigned long long> hstats;
    hipEvent_t ev_a = nullptr, ev_b = nullptr;
    int64_t level_launches = 0, run_launches = 0, kernel_us = 0;
    ~LdlBatch() {
        if (ev_a) (void)hipEventDestroy(ev_a);
        if (ev_b) (void)hipEventDestroy(ev_b);
    }
};

void destroy(LdlBatch *b) { delete b; }

// ---- factor ------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void k_ldb_init(int32_t B, int *flags, unsigned long long *stats) {
    const int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= B) return;
    flags[3 * m] = WALK_NONE;
    flags[3 * m + 1] = flags[3 * m + 2] = 0;
    for (int t = 0; t < 5; t++) stats[5 * m + t] = t == 2 ? ~0ull : 0ull;
}

// slot q of member blockIdx.y: V is nnz x B, row-major (entry win[q] of member m at V[win[q] * B + m]); a fill slot is 0.0
__global__ __launch_bounds__(256) void k_ldb_scatter(int64_t lnz, int32_t B, const int32_t *__restrict__ win,
                                                     const double *__restrict__ V, double *__restrict__ Lx) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= lnz) return;
    const int64_t m = blockIdx.y;
    const int32_t a = win[q];
    Lx[m * lnz + q] = a >= 0 ? V[(int64_t)a * B + m] : 0.0;
}

// The batch policy: the member's own Lx (stride lnz), d (stride n), flags (stride 3) and tau (tau[member]); the rest is shared.
struct LdlBatchColumn {
    using Args = ColumnArgs<const int32_t *__restrict__, const int32_t *__restrict__, double *, double *, const int32_t *__restrict__,
                            const int32_t *__restrict__, const int32_t *__restrict__, const double *__restrict__, int *, int64_t, int64_t>;
    static __device__ __forceinline__ void column(int32_t j, int32_t member, int w, int lane, const int32_t *Lp, const int32_t *Li,
                                                  double *Lx, double *d, const int32_t *row_ptr, const int32_t *row_col,
                                                  const int32_t *row_pos, const double *tau, int *flags, int64_t lnz, int64_t n) {
        LdlColumn::column(j, w, lane, Lp, Li, Lx + member * lnz, d + member * n, row_ptr, row_col, row_pos, tau[member],
                          flags + 3 * (int64_t)member);
    }
};

__global__ __launch_bounds__(256) void k_ldb_stats(int32_t n, int64_t lnz, const int32_t *__restrict__ Lp, const double *__restrict__ Lx,
                                                   const double *__restrict__ d, unsigned long long *st) {
    const int lane = threadIdx.x & 63;
    const int64_t j = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, m = blockIdx.y;
    if (j >= n) return;
    ldl_stats_column(j, lane, Lp, Lx + m * lnz, d + m * (int64_t)n, st + 5 * m);
}

// k_norm1_sym's rule per (row r, member m): first the entries of stored column r with row <= r in storage order, then the entries
// of row r with column > r in the row view's order (ascending (column, storage position)), one sequential rounded sum; the
// maximum over the bit patterns of fabs of the sums, a NaN ranking above inf (an unsigned maximum is the same in any order)
__global__ __launch_bounds__(256) void k_ldb_norm1(int32_t n, int32_t B, const int32_t *__restrict__ cp, const int32_t *__restrict__ ci,
                                                   const int32_t *__restrict__ rp, const int32_t *__restrict__ rc,
                                                   const int32_t *__restrict__ rpos, const double *__restrict__ V,
                                                   unsigned long long *best) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (int64_t)n * B) return;
    const int64_t r = t / B, m = t - r * B;
    double s = 0.0;
    for (int32_t q = cp[r], e = cp[r + 1]; q < e; q++)
        if (ci[q] <= r) s = s + fabs(V[(int64_t)q * B + m]);
    for (int32_t q = rp[r], e = rp[r + 1]; q < e; q++)
        if (rc[q] > r) s = s + fabs(V[(int64_t)rpos[q] * B + m]);
    atomicMax(best + m, (unsigned long long)abs_bits(s));
}

// ---- host -------------------------------------------------------------------------------------------------------------------

// the LDL' factor behind hF, or null with a text: a Schur factor (the same object with columns kept) has no batch
static LdlFactor *ldb_factor(const char *who, csx_handle_t hF) {
    LdlFactor *F = (LdlFactor *)get(hF, K_LDLFACTOR);
    if (F && F->ns == 0) return F;
    if (F || get(hF, K_SCHURFACTOR)) set_error("%s: a Schur factor (columns kept) has no batch; factor with csx_ldl_factor", who);
    else set_error("%s: F is not a factor of csx_ldl_factor (or has been freed)", who);
    return nullptr;
}

static LdlBatch *ldb_get(csx_handle_t h) {
    LdlBatch *b = (LdlBatch *)get(h, K_LDLBATCH);
    if (!b) return nullptr;
    if ((LdlFactor *)get(b->hF, K_LDLFACTOR) != b->F) {
        set_error("csx_ldl_batch: the factor of this batch has been freed");
        return nullptr;
    }
    return b;
}

static bool ldb_members_ok(const char *who, int64_t B) {
    if (B >= 1 && B <= WALK_BATCH_MAX) return true;
    set_error("%s: B = %lld, a batch holds 1 .. %d members (split a larger family into several batches)", who, (long long)B,
              (int)WALK_BATCH_MAX);
    return false;
}

// The row view of A's pattern with its map back to storage positions, from F's kept p0 / i0: row r holds (column, position) of
// its entries in ascending (column, position) -- the order of A's cached row gather, which k_norm1_sym reads.  Built on the first
// csx_ldl_batch_norm1 on F and kept there (A's pattern never changes); synchronises once.
static int ldb_row_view(LdlFactor *F) {
    if (F->a_rows) return CSX_OK;
    const size_t n = (size_t)F->n, nz = (size_t)F->anz;
    std::vector<int32_t> p, i;
    CSX_TRY(download_i32(p, F->p0, n + 1));
    CSX_TRY(download_i32(i, F->i0, nz));
    std::vector<int32_t> rp(n + 1, 0), rc(nz), rpos(nz);
    for (size_t q = 0; q < nz; q++) {
        if (i[q] < 0 || (size_t)i[q] >= n) return CSX_EINVAL;
        rp[(size_t)i[q] + 1]++;
    }
    for (size_t r = 0; r < n; r++) rp[r + 1] += rp[r];
    std::vector<int32_t> next(rp.begin(), rp.end() - 1);
    for (size_t j = 0; j < n; j++)
        for (int32_t q = p[j]; q < p[j + 1]; q++) {
            const int32_t at = next[(size_t)i[(size_t)q]]++;
            rc[(size_t)at] = (int32_t)j;
            rpos[(size_t)at] = q;
        }
    CSX_TRY(upload(F->arp, rp));
    CSX_TRY(upload(F->arc, rc));
    CSX_TRY(upload(F->apos, rpos));
    CSX_HIP(hipStreamSynchronize(ctx().stream));   // (the host lists go out of scope)
    F->a_rows = true;
    return CSX_OK;
}

// every member's factor of V into the batch's arrays; ok[m] = 1 where no column of member m broke down.  One synchronisation.
static int ldb_run(LdlBatch *b, const double *V, const double *tau, int *ok) {
    hipStream_t s = ctx().stream;
    LdlFactor *F = b->F;
    const int32_t n = F->n, B = b->B;
    const int64_t lnz = F->lnz;
    std::vector<double> htau((size_t)B, 0.0);
    for (int32_t m = 0; tau && m < B; m++) {
        if (!(tau[m] >= 0.0)) {
            set_error("csx_ldl_batch: tau[%d] is negative or NaN", (int)m);
            return CSX_EINVAL;
        }
        htau[(size_t)m] = tau[m];
    }
    b->level_launches = b->run_launches = 0;
    CSX_HIP(hipMemcpyAsync(b->tau, htau.data(), (size_t)B * sizeof(double), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_ldb_init, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, s, B, b->flags.get(), b->stats.get());
    CSX_HIP(hipEventRecord(b->ev_a, s));
    if (lnz)
        hipLaunchKernelGGL(k_ldb_scatter, dim3((unsigned)((lnz + 255) / 256), (unsigned)B), dim3(256), 0, s, lnz, B, F->win.get(), V,
                           b->Lx.get());
    walk_levels_batch<LdlBatchColumn>(F, B, &b->level_launches, &b->run_launches, LdlBatchColumn::Args(), F->Lp, F->Li, b->Lx, b->dd,
                                      F->rp, F->rc, F->rpos, b->tau, b->flags, lnz, (int64_t)n);
    if (n > 0)
        hipLaunchKernelGGL(k_ldb_stats, dim3((unsigned)(((int64_t)n + 3) / 4), (unsigned)B), dim3(256), 0, s, n, lnz, F->Lp,
                           b->Lx.get(), b->dd.get(), b->stats.get());
    (void)hipEventRecord(b->ev_b, s);
    if (hipGetLastError() != hipSuccess ||
        hipMemcpyAsync(b->hflags.data(), b->flags.get(), (size_t)B * 3 * sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipMemcpyAsync(b->hstats.data(), b->stats.get(), (size_t)B * 5 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s) !=
            hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess) {
        set_error("csx_ldl_batch: %s", hipGetErrorString(hipGetLastError()));
        (void)hipStreamSynchronize(s);
        return CSX_ERUNTIME;
    }
    float ms = 0.0f;
    b->kernel_us = hipEventElapsedTime(&ms, b->ev_a, b->ev_b) == hipSuccess ? (int64_t)(1e3 * ms) : 0;
    for (int32_t m = 0; m < B; m++) {
        if (n == 0) b->hstats[(size_t)5 * m + 2] = 0;
        ok[m] = b->hflags[(size_t)3 * m] == WALK_NONE ? 1 : 0;
    }
    return CSX_OK;
}

static int ldb_alloc(LdlFactor *F, csx_handle_t hF, int32_t B, std::unique_ptr<LdlBatch> *out) {
    std::unique_ptr<LdlBatch> b(new LdlBatch());
    b->F = F;
    b->hF = hF;
    b->B = B;
    CSX_TRY(b->Lx.alloc((size_t)B * (size_t)F->lnz));
    CSX_TRY(b->dd.alloc((size_t)B * (size_t)F->n));
    CSX_TRY(b->tau.alloc((size_t)B));
    CSX_TRY(b->flags.alloc((size_t)B * 3));
    CSX_TRY(b->stats.alloc((size_t)B * 5));
    b->hflags.assign((size_t)B * 3, 0);
    b->hstats.assign((size_t)B * 5, 0);
    CSX_HIP(hipEventCreate(&b->ev_a));
    CSX_HIP(hipEventCreate(&b->ev_b));
    *out = std::move(b);
    return CSX_OK;
}

}  // namespace csx

using namespace csx;

extern "C" int csx_ldl_batch_limits(int32_t *out) {   // (no device needed)
    if (!out) return CSX_EINVAL;
    out[0] = WALK_BATCH_MAX;
    out[1] = WALK_WAVES;
    out[2] = SLB_THREADS;
    out[3] = SLB_FETCH;
    out[4] = SLB_RUN_WAVES;
    out[5] = SLB_RUN_FETCH;
    return CSX_OK;
}

extern "C" int csx_ldl_batch_factor(csx_handle_t hF, csx_handle_t hV, int32_t B, const double *tau, csx_handle_t *out, int *ok) {
    CSX_TRY(require_ready());
    if (out) *out = 0;
    LdlFactor *F = ldb_factor("csx_ldl_batch_factor", hF);
    if (!F || !out || !ok) return CSX_EINVAL;
    if (!ldb_members_ok("csx_ldl_batch_factor", B)) return CSX_EINVAL;
    const double *V = batch_block(hV, (int64_t)F->anz * B);
    if (!V) {
        set_error("csx_ldl_batch_factor: V is not a block of nnz(A) x B = %lld x %d doubles", (long long)F->anz, (int)B);
        return CSX_EINVAL;
    }
    std::unique_ptr<LdlBatch> b;
    CSX_TRY(ldb_alloc(F, hF, B, &b));
    CSX_TRY(ldb_run(b.get(), V, tau, ok));
    *out = put(K_LDLBATCH, b.release());
    return CSX_OK;
}

extern "C" int csx_ldl_batch_refactor(csx_handle_t h, csx_handle_t hV, const double *tau, int *ok) {
    CSX_TRY(require_ready());
    LdlBatch *b = ldb_get(h);
    if (!b || !ok) return CSX_EINVAL;
    const double *V = batch_block(hV, (int64_t)b->F->anz * b->B);
    if (!V) {
        set_error("csx_ldl_batch_refactor: V is not a block of nnz(A) x B = %lld x %d doubles", (long long)b->F->anz, (int)b->B);
        return CSX_EINVAL;
    }
    return ldb_run(b, V, tau, ok);
}

extern "C" int csx_ldl_batch_norm1(csx_handle_t hF, csx_handle_t hV, int32_t B, double *out) {
    CSX_TRY(require_ready());
    LdlFactor *F = ldb_factor("csx_ldl_batch_norm1", hF);
    if (!F || !out) return CSX_EINVAL;
    if (!ldb_members_ok("csx_ldl_batch_norm1", B)) return CSX_EINVAL;
    const double *V = batch_block(hV, (int64_t)F->anz * B);
    if (!V) {
        set_error("csx_ldl_batch_norm1: V is not a block of nnz(A) x B = %lld x %d doubles", (long long)F->anz, (int)B);
        return CSX_EINVAL;
    }
    CSX_TRY(ldb_row_view(F));
    hipStream_t s = ctx().stream;
    DevBuf<unsigned long long> d;
    CSX_TRY(d.alloc((size_t)B));
    CSX_HIP(hipMemsetAsync(d, 0, (size_t)B * sizeof(unsigned long long), s));
    const int64_t items = (int64_t)F->n * B;
    if (items > 0)
        hipLaunchKernelGGL(k_ldb_norm1, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, s, F->n, B, F->p0.get(), F->i0.get(),
                           F->arp.get(), F->arc.get(), F->apos.get(), V, d.get());
    CSX_LAUNCH_CHECK();
    static_assert(sizeof(double) == sizeof(unsigned long long), "the sums travel as their bit patterns");
    CSX_HIP(hipMemcpyAsync(out, d.get(), (size_t)B * sizeof(double), hipMemcpyDeviceToHost, s));
    CSX_HIP(hipStreamSynchronize(s));
    return CSX_OK;
}

extern "C" int csx_ldl_batch_solve(csx_handle_t h, csx_handle_t hX, int32_t r) {
    CSX_TRY(require_ready());
    LdlBatch *b = ldb_get(h);
    if (!b || r < 1) return CSX_EINVAL;
    const LdlFactor *F = b->F;
    const int64_t n = F->n, K = (int64_t)b->B * r;
    if (!batch_solve_fits(n, K)) {
        set_error("csx_ldl_batch_solve: B r = %lld columns are more than one launch takes", (long long)K);
        return CSX_EINVAL;
    }
    double *X = batch_block(hX, n * K);
    if (!X) {
        set_error("csx_ldl_batch_solve: X is not a block of n x B r = %lld x %lld doubles", (long long)n, (long long)K);
        return CSX_EINVAL;
    }
    if (n == 0) return CSX_OK;
    hipStream_t s = ctx().stream;
    DevBuf<double> W;
    CSX_TRY(W.alloc((size_t)(n * K)));
    const unsigned blocks = (unsigned)((n * K + 255) / 256);
    const BatchPattern P = {F->Lp, F->Li, F->rp.get(), F->rc.get(), F->rpos.get(), n, F->lnz, b->B};
    hipLaunchKernelGGL(k_slb_permute_in, dim3(blocks), dim3(256), 0, s, n, K, F->pinv, X, W.get());
    // cs_lsolve(L), then x / d and cs_ltsolve(L) in one sweep: the division by d_j opens row j's backward chain.  It cannot close
    // row j's forward chain instead: the forward chains of the later rows read x_j undivided (csx_batchsolve.h).
    CSX_TRY(batch_sweep(F, P, true, b->Lx.get(), false, nullptr, r, W.get()));
    CSX_TRY(batch_sweep(F, P, false, b->Lx.get(), false, b->dd.get(), r, W.get()));
    hipLaunchKernelGGL(k_slb_permute_out, dim3(blocks), dim3(256), 0, s, n, K, r, F->pinv, b->flags.get(), W.get(), X);
    CSX_LAUNCH_CHECK();
    CSX_HIP(hipStreamSynchronize(s));   // W goes out of scope
    return CSX_OK;
}

extern "C" int csx_ldl_batch_info(csx_handle_t h, int64_t *shared, int64_t *members) {
    CSX_TRY(require_ready());
    LdlBatch *b = ldb_get(h);
    if (!b || !shared || !members) return CSX_EINVAL;
    shared[0] = b->F->n;
    shared[1] = b->F->lnz;
    shared[2] = b->F->levels();
    shared[3] = b->level_launches + b->run_launches;
    shared[4] = b->level_launches;
    shared[5] = b->run_launches;
    shared[6] = b->kernel_us;
    shared[7] = b->B;
    for (int32_t m = 0; m < b->B; m++) {
        const int *f = &b->hflags[(size_t)3 * m];
        members[5 * m + 0] = f[1];
        members[5 * m + 1] = f[0] == WALK_NONE ? -1 : f[0];
        members[5 * m + 2] = f[2];
        members[5 * m + 3] = (int64_t)b->hstats[(size_t)5 * m + 0];
        members[5 * m + 4] = (int64_t)b->hstats[(size_t)5 * m + 1];
    }
    return CSX_OK;
}

extern "C" int csx_ldl_batch_stats(csx_handle_t h, double *out) {
    CSX_TRY(require_ready());
    LdlBatch *b = ldb_get(h);
    if (!b || !out) return CSX_EINVAL;
    for (int32_t m = 0; m < b->B; m++) std::memcpy(out + 3 * m, &b->hstats[(size_t)5 * m + 2], 3 * sizeof(double));
    return CSX_OK;
}

extern "C" int csx_ldl_batch_member(csx_handle_t h, int32_t m, double *Lx_out, double *d_out) {
    CSX_TRY(require_ready());
    LdlBatch *b = ldb_get(h);
    if (!b || m < 0 || m >= b->B || !Lx_out || !d_out) return CSX_EINVAL;
    hipStream_t s = ctx().stream;
    const size_t lnz = (size_t)b->F->lnz, n = (size_t)b->F->n;
    if (lnz) CSX_HIP(hipMemcpyAsync(Lx_out, b->Lx.get() + (size_t)m * lnz, lnz * sizeof(double), hipMemcpyDeviceToHost, s));
    if (n) CSX_HIP(hipMemcpyAsync(d_out, b->dd.get() + (size_t)m * n, n * sizeof(double), hipMemcpyDeviceToHost, s));
    CSX_HIP(hipStreamSynchronize(s));
    return CSX_OK;
}

extern "C" int csx_ldl_batch_d(csx_handle_t h, double *out) {
    CSX_TRY(require_ready());
    LdlBatch *b = ldb_get(h);
    if (!b || !out) return CSX_EINVAL;
    hipStream_t s = ctx().stream;
    const size_t all = (size_t)b->B * (size_t)b->F->n;
    if (all) CSX_HIP(hipMemcpyAsync(out, b->dd.get(), all * sizeof(double), hipMemcpyDeviceToHost, s));
    CSX_HIP(hipStreamSynchronize(s));
    return CSX_OK;
}
