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
//   k_slb_level / k_slb_run <rows or dots>   the two sweeps of a solve in the reference's operation order, over F's height
//                    levels: a wide level is one launch of a thread per (row, member, right-hand side), a run of narrow levels
//                    one launch of a workgroup per member with a wave per (row, right-hand side) -- F's schedule, so
//                    len(schedule) launches a sweep for any B
//   k_slb_permute_in / k_slb_permute_out   the solve's permutations; the second fills a failed member's columns with NaN
// There is NO scratch-then-commit: a member that breaks down is marked failed (ok[m] = 0, its values mean nothing) where the
// single factor keeps its old values.  Keeping them would take a second B x lnz pair of arrays.
#include <cmath>
#include <cstring>
#include <limits>

#include "csx_internal.h"
#include "csx_slu.h"

#pragma clang fp contract(off)

namespace csx {

constexpr int SLB_THREADS = 256;   // threads of a workgroup of the solve kernels: the (row, column) pairs a wide level's workgroup takes
constexpr int SLB_FETCH = 4;       // terms of a chain that a thread of a wide level fetches together, then applies one after the other
constexpr int SLB_RUN_WAVES = 16;  // waves of a walker's workgroup: (row, right-hand side) pairs it takes at a time, a wave each
constexpr int SLB_RUN_FETCH = 64;  // terms of a chain that a walker's wave fetches together, a lane each

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

// ---- solve: the two sweeps ----------------------------------------------------------------------------------------------------
// X is n x K row-major, K = B r; column c belongs to member c / r.  val: the member-major values of the factor the sweep reads
// (stride lnz); div: divide by the diagonal val[Lp[j]] (Ut) or not (unit L).

// x_j = ((x_j - v1 x_k1) - v2 x_k2) - ... over row j's entries off the diagonal in the row view (k ascending), then / d_j
__device__ __forceinline__ void slb_row(int32_t j, int64_t c, int64_t K, const int32_t *__restrict__ Lp,
                                        const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ row_col,
                                        const int32_t *__restrict__ row_pos, const double *__restrict__ v, bool div, double *X) {
    double s = X[(int64_t)j * K + c];
    const int32_t qe = row_ptr[j + 1] - 1;   // the row view ends with the diagonal
    for (int32_t q0 = row_ptr[j]; q0 < qe; q0 += SLB_FETCH) {
        double a_[SLB_FETCH], x_[SLB_FETCH];
#pragma unroll
        for (int u = 0; u < SLB_FETCH; u++) {
            const int32_t q = q0 + u < qe ? q0 + u : q0;
            a_[u] = v[row_pos[q]];
            x_[u] = X[(int64_t)row_col[q] * K + c];
        }
#pragma unroll
        for (int u = 0; u < SLB_FETCH; u++)
            if (q0 + u < qe) {
                const double t = a_[u] * x_[u];
                s = s - t;
            }
    }
    if (div) s = s / v[Lp[j]];
    X[(int64_t)j * K + c] = s;
}

// x_j = ((x_j - v1 x_i1) - v2 x_i2) - ... over column j's stored entries below the diagonal in storage order, then / d_j
__device__ __forceinline__ void slb_dot(int32_t j, int64_t c, int64_t K, const int32_t *__restrict__ Lp, const int32_t *__restrict__ Li,
                                        const double *__restrict__ v, bool div, double *X) {
    double s = X[(int64_t)j * K + c];
    const int32_t pe = Lp[j + 1];
    for (int32_t p0 = Lp[j] + 1; p0 < pe; p0 += SLB_FETCH) {
        double a_[SLB_FETCH], x_[SLB_FETCH];
#pragma unroll
        for (int u = 0; u < SLB_FETCH; u++) {
            const int32_t p = p0 + u < pe ? p0 + u : p0;
            a_[u] = v[p];
            x_[u] = X[(int64_t)Li[p] * K + c];
        }
#pragma unroll
        for (int u = 0; u < SLB_FETCH; u++)
            if (p0 + u < pe) {
                const double t = a_[u] * x_[u];
                s = s - t;
            }
    }
    if (div) s = s / v[Lp[j]];
    X[(int64_t)j * K + c] = s;
}

// a wide level: one thread per (row of the level, column of X), the columns fastest
template <bool ROWS>
__global__ __launch_bounds__(SLB_THREADS) void k_slb_level(const int32_t *__restrict__ cols, int32_t count, int64_t K, int32_t r,
                                                           int64_t lnz, const int32_t *__restrict__ Lp, const int32_t *__restrict__ Li,
                                                           const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ row_col,
                                                           const int32_t *__restrict__ row_pos, const double *__restrict__ val, int div,
                                                           double *X) {
    const int64_t t = (int64_t)blockIdx.x * SLB_THREADS + threadIdx.x;
    if (t >= (int64_t)count * K) return;
    const int64_t i = t / K, c = t - i * K;
    const double *v = val + (c / r) * lnz;
    if (ROWS) slb_row(cols[i], c, K, Lp, row_ptr, row_col, row_pos, v, div != 0, X);
    else slb_dot(cols[i], c, K, Lp, Li, v, div != 0, X);
}

// One WAVE's (row, column of X) of a narrow level, where a chain is long (the top of a nested-dissection tree) and there are few
// of them: the 64 lanes fetch 64 terms of the chain together and each forms one product -- a product is rounded on its own,
// whoever forms it -- then the products are applied one after the other in the chain's order, every lane keeping the same sum.
template <bool ROWS>
__device__ __forceinline__ void slb_wave_chain(int32_t j, int64_t c, int64_t K, int lane, const int32_t *__restrict__ Lp,
                                               const int32_t *__restrict__ Li, const int32_t *__restrict__ row_ptr,
                                               const int32_t *__restrict__ row_col, const int32_t *__restrict__ row_pos,
                                               const double *__restrict__ v, bool div, double *X) {
    const int32_t q0 = __builtin_amdgcn_readfirstlane(ROWS ? row_ptr[j] : Lp[j] + 1);
    const int32_t qe = __builtin_amdgcn_readfirstlane(ROWS ? row_ptr[j + 1] - 1 : Lp[j + 1]);
    double s = X[(int64_t)j * K + c];
    for (int32_t b = q0; b < qe; b += 64) {
        const int32_t q = b + lane;
        double t = 0.0;
        if (q < qe) {
            const double a = ROWS ? v[row_pos[q]] : v[q];
            const int32_t k = ROWS ? row_col[q] : Li[q];
            t = a * X[(int64_t)k * K + c];
        }
        const int32_t terms = qe - b < 64 ? qe - b : 64;
        for (int32_t u = 0; u < terms; u++) {
            const double tu = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(t), u),
                                               __builtin_amdgcn_readlane(__double2loint(t), u));
            s = s - tu;
        }
    }
    if (div) s = s / v[Lp[j]];
    if (lane == 0) X[(int64_t)j * K + c] = s;
}

// a run of narrow levels: the workgroup of member blockIdx.x walks [l0, l1) -- ascending for the rows, descending for the dots --
// with a barrier per level; its SLB_RUN_WAVES waves take the (row of the level, right-hand side) pairs one each at a time
// (slb_wave_chain).  The trip counts are the level pointers and r, the same for every wave, so every wave reaches every barrier.
template <bool ROWS>
__global__ __launch_bounds__(64 * SLB_RUN_WAVES) void k_slb_run(const int32_t *__restrict__ cols, const int32_t *__restrict__ level_ptr,
                                                         int32_t l0, int32_t l1, int64_t K, int32_t r, int64_t lnz,
                                                         const int32_t *__restrict__ Lp, const int32_t *__restrict__ Li,
                                                         const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ row_col,
                                                         const int32_t *__restrict__ row_pos, const double *__restrict__ val, int div,
                                                         double *X) {
    const int64_t m = blockIdx.x;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const double *v = val + m * lnz;
    for (int32_t s = 0; s < l1 - l0; s++) {
        const int32_t l = ROWS ? l0 + s : l1 - 1 - s;
        const int32_t b = level_ptr[l], cnt = level_ptr[l + 1] - b;
        for (int32_t t = w; t < cnt * r; t += SLB_RUN_WAVES) {
            const int32_t i = t / r;
            const int32_t j = __builtin_amdgcn_readfirstlane(cols[b + i]);
            slb_wave_chain<ROWS>(j, m * r + (t - i * r), K, lane, Lp, Li, row_ptr, row_col, row_pos, v, div != 0, X);
        }
        __syncthreads();
    }
}

// W[p[i], :] = X[i, :] (p null: the identity)
__global__ __launch_bounds__(256) void k_slb_permute_in(int64_t n, int64_t K, const int32_t *__restrict__ p, const double *__restrict__ X,
                                                        double *__restrict__ W) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * K) return;
    const int64_t i = t / K, c = t - i * K;
    W[(p ? (int64_t)p[i] : i) * K + c] = X[t];
}

// X[i, :] = W[p[i], :], NaN in the columns of a member that broke down
__global__ __launch_bounds__(256) void k_slb_permute_out(int64_t n, int64_t K, int32_t r, const int32_t *__restrict__ p,
                                                         const int *__restrict__ flags, const double *__restrict__ W,
                                                         double *__restrict__ X) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * K) return;
    const int64_t i = t / K, c = t - i * K;
    const bool ok = flags[3 * (c / r)] == WALK_NONE;
    X[t] = ok ? W[(p ? (int64_t)p[i] : i) * K + c] : __longlong_as_double(0x7ff8000000000000ll);
}

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

// the device block of at least `need` doubles behind a vector handle, or null
static double *slb_block(csx_handle_t h, int64_t need) {
    Vec *v = vec(h);
    return v && v->d && v->len >= need ? (double *)v->d : nullptr;
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
    hipStream_t s = ctx().stream;
    const SluFactor *F = b->F;
    const Csc *L = csc(F->hL);
    const std::vector<int32_t> &lp = F->level_ptr_h;
    const int64_t K = (int64_t)b->B * r, lnz = F->lnz;
    const size_t nl = F->schedule.size();
    for (size_t t = 0; t < nl; t++) {
        const LevelLaunch &Ln = F->schedule[rows ? t : nl - 1 - t];
        if (Ln.wide) {
            const int32_t cnt = lp[(size_t)Ln.l0 + 1] - lp[(size_t)Ln.l0];
            const unsigned blocks = (unsigned)(((int64_t)cnt * K + SLB_THREADS - 1) / SLB_THREADS);
            const int32_t *cols = F->level_cols.get() + lp[(size_t)Ln.l0];
            if (rows)
                hipLaunchKernelGGL(k_slb_level<true>, dim3(blocks), dim3(SLB_THREADS), 0, s, cols, cnt, K, r, lnz, L->p, L->i,
                                   F->rp.get(), F->rc.get(), F->rpos.get(), val, div ? 1 : 0, X);
            else
                hipLaunchKernelGGL(k_slb_level<false>, dim3(blocks), dim3(SLB_THREADS), 0, s, cols, cnt, K, r, lnz, L->p, L->i,
                                   F->rp.get(), F->rc.get(), F->rpos.get(), val, div ? 1 : 0, X);
        } else if (rows) {
            hipLaunchKernelGGL(k_slb_run<true>, dim3((unsigned)b->B), dim3(64 * SLB_RUN_WAVES), 0, s, F->level_cols.get(), F->level_ptr.get(),
                               Ln.l0, Ln.l1, K, r, lnz, L->p, L->i, F->rp.get(), F->rc.get(), F->rpos.get(), val, div ? 1 : 0, X);
        } else {
            hipLaunchKernelGGL(k_slb_run<false>, dim3((unsigned)b->B), dim3(64 * SLB_RUN_WAVES), 0, s, F->level_cols.get(), F->level_ptr.get(),
                               Ln.l0, Ln.l1, K, r, lnz, L->p, L->i, F->rp.get(), F->rc.get(), F->rpos.get(), val, div ? 1 : 0, X);
        }
    }
    CSX_LAUNCH_CHECK();
    return CSX_OK;
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
    const double *V = slb_block(hV, (int64_t)F->anz * B);
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
    const double *V = slb_block(hV, (int64_t)b->F->anz * b->B);
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
    const double *V = slb_block(hV, (int64_t)F->anz * B);
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
    if (K > 0x7fffffffll / WALK_WAVES || n * K > 0x7fffffffll * SLB_THREADS) {   // (a walker counts rows x r in 32 bits)
        set_error("csx_slu_batch_solve: B r = %lld columns are more than one launch takes", (long long)K);
        return CSX_EINVAL;
    }
    double *X = slb_block(hX, n * K);
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
