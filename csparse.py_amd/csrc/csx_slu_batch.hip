// Many value sets on the analysis of one static-pivot L U (the definition is the comment of csx_slu_batch_factor
// in include/csx.h).  An SluBatch BORROWS an SluFactor -- pattern, row view, entry maps, height levels, launch schedule, the
// two permutations -- and owns B value sets: Lx and Ux (B x lnz doubles each, member-major: member m's column j is the
// contiguous piece slu_column expects), flags (B x 3), stats (B x 6), tau (B).  It never writes the factor's L.x / Ut.x or its
// scratch, and keeps its own launch counters.
//   k_slb_init / k_slb_scatter   the flag and stat words; every member's values through winL / winU (of duplicates the last)
//   SluBatchColumn   the batch policy of the level walk (csx_levelwalk.h: k_level_batch, k_run_batch): Lx, Ux by lnz, flags by 3,
//                    tau read from an array, then SluColumn::column -- slu_column itself, the host rule's bits
//   k_slb_stats      slu_stats_column per (column, member)
//   k_slb_norm1      |A_m|_1 by k_norm1's rule
//   batch_sweep      the two sweeps of a solve in the reference's operation order, over F's height levels, and the solve's
//                    permutations: csx_batchsolve.h (k_slb_level, k_slb_run, k_slb_permute_in / _out), shared with the LDL' batch
// There is NO scratch-then-commit: a member that breaks down is marked failed (ok[m] = 0, its values mean nothing) where the
// single factor keeps its old values.  Keeping them would take a second B x lnz pair of arrays.
#include <cmath>
#include <cstring>
#include <limits>

#include "csx_batchsolve.h"
#include "csx_internal.h"
#include "csx_slu.h"

#pragma clang fp contract(off)

namespace csx {

struct SluBatch {
    SluFactor *F = nullptr;   // borrowed: valid while hF resolves to it
    csx_handle_t hF = 0;
    int32_t B = 0;
    DevBuf<double> Lx, Ux, tau;
    DevBuf<int> flags;
    DevBuf<unsigned long long> stats;
    std::vector<int> hflags;                    // of the last run
    std::vector<unsigned long long> hstats;
    hipEvent_t ev_a = nullptr, ev_b = nullptr;
    int64_t level_launches = 0, run_launches = 0, kernel_us = 0;
    ~SluBatch() {
        if (ev_a) (void)hipEventDestroy(ev_a);
        if (ev_b) (void)hipEventDestroy(ev_b);
    }
};

void destroy(SluBatch *b) { delete b; }

// ---- factor ------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void k_slb_init(int32_t B, int *flags, unsigned long long *stats) {
    const int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= B) return;
    flags[3 * m] = WALK_NONE;
    flags[3 * m + 1] = flags[3 * m + 2] = 0;
    for (int t = 0; t < 6; t++) stats[6 * m + t] = t == 2 ? ~0ull : 0ull;
}

// slot q of member blockIdx.y: V is nnz x B, row-major (entry winL[q] of member m at V[winL[q] * B + m])
__global__ __launch_bounds__(256) void k_slb_scatter(int64_t lnz, int32_t B, const int32_t *__restrict__ winL,
                                                     const int32_t *__restrict__ winU, const double *__restrict__ V,
                                                     double *__restrict__ Lx, double *__restrict__ Ux) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= lnz) return;
    const int64_t m = blockIdx.y, at = m * lnz + q;
    const int32_t a = winL[q], b = winU[q];
    Lx[at] = a >= 0 ? V[(int64_t)a * B + m] : 0.0;
    Ux[at] = b >= 0 ? V[(int64_t)b * B + m] : 0.0;
}

// The batch policy: the member's own Lx, Ux (stride lnz), flags (stride 3) and tau (tau[member]); everything else is shared.
struct SluBatchColumn {
    using Args = ColumnArgs<const int32_t *__restrict__, const int32_t *__restrict__, double *, double *, const int32_t *__restrict__,
                            const int32_t *__restrict__, const int32_t *__restrict__, const double *__restrict__, int *, int64_t>;
    static __device__ __forceinline__ void column(int32_t j, int32_t member, int w, int lane, const int32_t *Lp, const int32_t *Li,
                                                  double *Lx, double *Ux, const int32_t *row_ptr, const int32_t *row_col,
                                                  const int32_t *row_pos, const double *tau, int *flags, int64_t lnz) {
        SluColumn::column(j, w, lane, Lp, Li, Lx + member * lnz, Ux + member * lnz, row_ptr, row_col, row_pos, tau[member],
                          flags + 3 * (int64_t)member);
    }
};

__global__ __launch_bounds__(256) void k_slb_stats(int32_t n, int64_t lnz, const int32_t *__restrict__ Lp, const double *__restrict__ Lx,
                                                   const double *__restrict__ Ux, unsigned long long *st) {
    const int lane = threadIdx.x & 63;
    const int64_t j = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, m = blockIdx.y;
    if (j >= n) return;
    slu_stats_column((int32_t)j, lane, Lp, Lx + m * lnz, Ux + m * lnz, st + 6 * m);
}

// k_norm1's rule per member: one sequential sum per column, the maximum over the bit patterns of the sums that are not NaN
__global__ __launch_bounds__(256) void k_slb_norm1(int32_t n, int32_t B, const int32_t *__restrict__ Ap, const double *__restrict__ V,
                                                   unsigned long long *best) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (int64_t)n * B) return;
    const int64_t j = t / B, m = t - j * B;
    double sum = 0.0;
    for (int32_t p = Ap[j]; p < Ap[j + 1]; p++) sum += fabs(V[(int64_t)p * B + m]);
    if (sum == sum) atomicMax(best + m, (unsigned long long)__double_as_longlong(sum));
}

// ---- solve: the two sweeps and the permutations are csx_batchsolve.h's (shared with csx_ldl_batch.hip) -----------------------------

// ---- host -------------------------------------------------------------------------------------------------------------------

static SluBatch *slb_get(csx_handle_t h) {
    SluBatch *b = (SluBatch *)get(h, K_SLUBATCH);
    if (!b) return nullptr;
    if ((SluFactor *)get(b->hF, K_SLUFACTOR) != b->F) {
        set_error("csx_slu_batch: the factor of this batch has been freed");
        return nullptr;
    }
    return b;
}

static bool slb_members_ok(const char *who, int64_t B) {
    if (B >= 1 && B <= WALK_BATCH_MAX) return true;
    set_error("%s: B = %lld, a batch holds 1 .. %d members (split a larger family into several batches)", who, (long long)B,
              (int)WALK_BATCH_MAX);
    return false;
}

// every member's factor of V into the batch's arrays; ok[m] = 1 where no column of member m broke down.  One synchronisation.
static int slb_run(SluBatch *b, const double *V, const double *tau, int *ok) {
    hipStream_t s = ctx().stream;
    SluFactor *F = b->F;
    Csc *L = csc(F->hL);
    if (!L) return CSX_EINVAL;
    const int32_t n = F->n, B = b->B;
    const int64_t lnz = F->lnz;
    std::vector<double> htau((size_t)B, 0.0);
    for (int32_t m = 0; tau && m < B; m++) {
        if (!(tau[m] >= 0.0)) {
            set_error("csx_slu_batch: tau[%d] is negative or NaN", (int)m);
            return CSX_EINVAL;
        }
        htau[(size_t)m] = tau[m];
    }
    b->level_launches = b->run_launches = 0;
    CSX_HIP(hipMemcpyAsync(b->tau, htau.data(), (size_t)B * sizeof(double), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_slb_init, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, s, B, b->flags.get(), b->stats.get());
    CSX_HIP(hipEventRecord(b->ev_a, s));
    if (lnz)
        hipLaunchKernelGGL(k_slb_scatter, dim3((unsigned)((lnz + 255) / 256), (unsigned)B), dim3(256), 0, s, lnz, B, F->winL.get(),
                           F->winU.get(), V, b->Lx.get(), b->Ux.get());
    walk_levels_batch<SluBatchColumn>(F, B, &b->level_launches, &b->run_launches, SluBatchColumn::Args(), L->p, L->i, b->Lx, b->Ux,
                                      F->rp, F->rc, F->rpos, b->tau, b->flags, lnz);
    if (n > 0)
        hipLaunchKernelGGL(k_slb_stats, dim3((unsigned)(((int64_t)n + 3) / 4), (unsigned)B), dim3(256), 0, s, n, lnz, L->p,
                           b->Lx.get(), b->Ux.get(), b->stats.get());
    (void)hipEventRecord(b->ev_b, s);
    if (hipGetLastError() != hipSuccess ||
        hipMemcpyAsync(b->hflags.data(), b->flags.get(), (size_t)B * 3 * sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipMemcpyAsync(b->hstats.data(), b->stats.get(), (size_t)B * 6 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s) !=
            hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess) {
        set_error("csx_slu_batch: %s", hipGetErrorString(hipGetLastError()));
        (void)hipStreamSynchronize(s);
        return CSX_ERUNTIME;
    }
    float ms = 0.0f;
    b->kernel_us = hipEventElapsedTime(&ms, b->ev_a, b->ev_b) == hipSuccess ? (int64_t)(1e3 * ms) : 0;
    for (int32_t m = 0; m < B; m++) {
        if (n == 0) b->hstats[(size_t)6 * m + 2] = 0;
        ok[m] = b->hflags[(size_t)3 * m] == WALK_NONE ? 1 : 0;
    }
    return CSX_OK;
}

static int slb_sweep(SluBatch *b, bool rows, const double *val, bool div, int32_t r, double *X) {
    const SluFactor *F = b->F;
    const Csc *L = csc(F->hL);
    if (!L) return CSX_EINVAL;
    const BatchPattern P = {L->p, L->i, F->rp.get(), F->rc.get(), F->rpos.get(), F->n, F->lnz, b->B};
    return batch_sweep(F, P, rows, val, div, nullptr, r, X);
}

static int slb_alloc(SluFactor *F, csx_handle_t hF, int32_t B, std::unique_ptr<SluBatch> *out) {
    std::unique_ptr<SluBatch> b(new SluBatch());
    b->F = F;
    b->hF = hF;
    b->B = B;
    const size_t all = (size_t)B * (size_t)F->lnz;
    CSX_TRY(b->Lx.alloc(all));
    CSX_TRY(b->Ux.alloc(all));
    CSX_TRY(b->tau.alloc((size_t)B));
    CSX_TRY(b->flags.alloc((size_t)B * 3));
    CSX_TRY(b->stats.alloc((size_t)B * 6));
    b->hflags.assign((size_t)B * 3, 0);
    b->hstats.assign((size_t)B * 6, 0);
    CSX_HIP(hipEventCreate(&b->ev_a));
    CSX_HIP(hipEventCreate(&b->ev_b));
    *out = std::move(b);
    return CSX_OK;
}

}  // namespace csx

using namespace csx;

extern "C" int csx_slu_batch_limits(int32_t *out) {   // (no device needed)
    if (!out) return CSX_EINVAL;
    out[0] = WALK_BATCH_MAX;
    out[1] = WALK_WAVES;
    out[2] = SLB_THREADS;
    out[3] = SLB_FETCH;
    out[4] = SLB_RUN_WAVES;
    out[5] = SLB_RUN_FETCH;
    return CSX_OK;
}

extern "C" int csx_slu_batch_factor(csx_handle_t hF, csx_handle_t hV, int32_t B, const double *tau, csx_handle_t *out, int *ok) {
    CSX_TRY(require_ready());
    SluFactor *F = (SluFactor *)get(hF, K_SLUFACTOR);
    if (!F || !out || !ok) return CSX_EINVAL;
    *out = 0;
    if (!slb_members_ok("csx_slu_batch_factor", B)) return CSX_EINVAL;
    const double *V = batch_block(hV, (int64_t)F->anz * B);
    if (!V) {
        set_error("csx_slu_batch_factor: V is not a block of nnz(A) x B = %lld x %d doubles", (long long)F->anz, (int)B);
        return CSX_EINVAL;
    }
    std::unique_ptr<SluBatch> b;
    CSX_TRY(slb_alloc(F, hF, B, &b));
    CSX_TRY(slb_run(b.get(), V, tau, ok));
    *out = put(K_SLUBATCH, b.release());
    return CSX_OK;
}

extern "C" int csx_slu_batch_refactor(csx_handle_t h, csx_handle_t hV, const double *tau, int *ok) {
    CSX_TRY(require_ready());
    SluBatch *b = slb_get(h);
    if (!b || !ok) return CSX_EINVAL;
    const double *V = batch_block(hV, (int64_t)b->F->anz * b->B);
    if (!V) {
        set_error("csx_slu_batch_refactor: V is not a block of nnz(A) x B = %lld x %d doubles", (long long)b->F->anz, (int)b->B);
        return CSX_EINVAL;
    }
    return slb_run(b, V, tau, ok);
}

extern "C" int csx_slu_batch_norm1(csx_handle_t hF, csx_handle_t hV, int32_t B, double *out) {
    CSX_TRY(require_ready());
    SluFactor *F = (SluFactor *)get(hF, K_SLUFACTOR);
    if (!F || !out) return CSX_EINVAL;
    if (!slb_members_ok("csx_slu_batch_norm1", B)) return CSX_EINVAL;
    const double *V = batch_block(hV, (int64_t)F->anz * B);
    if (!V) {
        set_error("csx_slu_batch_norm1: V is not a block of nnz(A) x B = %lld x %d doubles", (long long)F->anz, (int)B);
        return CSX_EINVAL;
    }
    hipStream_t s = ctx().stream;
    DevBuf<unsigned long long> d;
    CSX_TRY(d.alloc((size_t)B));
    CSX_HIP(hipMemsetAsync(d, 0, (size_t)B * sizeof(unsigned long long), s));
    const int64_t items = (int64_t)F->n * B;
    if (items > 0)
        hipLaunchKernelGGL(k_slb_norm1, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, s, F->n, B, F->p0.get(), V, d.get());
    CSX_LAUNCH_CHECK();
    static_assert(sizeof(double) == sizeof(unsigned long long), "the sums travel as their bit patterns");
    CSX_HIP(hipMemcpyAsync(out, d.get(), (size_t)B * sizeof(double), hipMemcpyDeviceToHost, s));
    CSX_HIP(hipStreamSynchronize(s));
    return CSX_OK;
}

extern "C" int csx_slu_batch_solve(csx_handle_t h, csx_handle_t hX, int32_t r, int trans) {
    CSX_TRY(require_ready());
    SluBatch *b = slb_get(h);
    if (!b || r < 1) return CSX_EINVAL;
    const SluFactor *F = b->F;
    const int64_t n = F->n, K = (int64_t)b->B * r;
    if (!batch_solve_fits(n, K)) {
        set_error("csx_slu_batch_solve: B r = %lld columns are more than one launch takes", (long long)K);
        return CSX_EINVAL;
    }
    double *X = batch_block(hX, n * K);
    if (!X) {
        set_error("csx_slu_batch_solve: X is not a block of n x B r = %lld x %lld doubles", (long long)n, (long long)K);
        return CSX_EINVAL;
    }
    if (n == 0) return CSX_OK;
    hipStream_t s = ctx().stream;
    DevBuf<double> W;
    CSX_TRY(W.alloc((size_t)(n * K)));
    const unsigned blocks = (unsigned)((n * K + 255) / 256);
    const int32_t *p_in = trans ? F->pinv : F->comb, *p_out = trans ? F->comb : F->pinv;
    hipLaunchKernelGGL(k_slb_permute_in, dim3(blocks), dim3(256), 0, s, n, K, p_in, X, W.get());
    // A x = b: cs_lsolve(L), cs_ltsolve(Ut);  A' x = b: cs_lsolve(Ut), cs_ltsolve(L)
    CSX_TRY(slb_sweep(b, true, trans ? b->Ux.get() : b->Lx.get(), trans != 0, r, W.get()));
    CSX_TRY(slb_sweep(b, false, trans ? b->Lx.get() : b->Ux.get(), trans == 0, r, W.get()));
    hipLaunchKernelGGL(k_slb_permute_out, dim3(blocks), dim3(256), 0, s, n, K, r, p_out, b->flags.get(), W.get(), X);
    CSX_LAUNCH_CHECK();
    CSX_HIP(hipStreamSynchronize(s));   // W goes out of scope
    return CSX_OK;
}

extern "C" int csx_slu_batch_info(csx_handle_t h, int64_t *shared, int64_t *members) {
    CSX_TRY(require_ready());
    SluBatch *b = slb_get(h);
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
        members[5 * m + 3] = (int64_t)b->hstats[(size_t)6 * m + 0];
        members[5 * m + 4] = (int64_t)b->hstats[(size_t)6 * m + 1];
    }
    return CSX_OK;
}

extern "C" int csx_slu_batch_stats(csx_handle_t h, double *out) {
    CSX_TRY(require_ready());
    SluBatch *b = slb_get(h);
    if (!b || !out) return CSX_EINVAL;
    for (int32_t m = 0; m < b->B; m++) std::memcpy(out + 4 * m, &b->hstats[(size_t)6 * m + 2], 4 * sizeof(double));
    return CSX_OK;
}

extern "C" int csx_slu_batch_member(csx_handle_t h, int32_t m, double *Lx_out, double *Utx_out) {
    CSX_TRY(require_ready());
    SluBatch *b = slb_get(h);
    if (!b || m < 0 || m >= b->B || !Lx_out || !Utx_out) return CSX_EINVAL;
    hipStream_t s = ctx().stream;
    const size_t lnz = (size_t)b->F->lnz;
    if (lnz) {
        CSX_HIP(hipMemcpyAsync(Lx_out, b->Lx.get() + (size_t)m * lnz, lnz * sizeof(double), hipMemcpyDeviceToHost, s));
        CSX_HIP(hipMemcpyAsync(Utx_out, b->Ux.get() + (size_t)m * lnz, lnz * sizeof(double), hipMemcpyDeviceToHost, s));
    }
    CSX_HIP(hipStreamSynchronize(s));
    return CSX_OK;
}
