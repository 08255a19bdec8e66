// Many value sets on the analysis of one static-pivot L U (the definition is the comment of csx_slu_batch_factor
// in include/csx.h).  An SluBatch BORROWS an SluFactor -- pattern, row view, entry maps, height levels, launch schedule, the
// two permutations -- and owns B value sets: Lx and Ux (B x lnz doubles each, member-major: member m's column j is the
// contiguous piece slu_column expects), flags (B x 3), stats (B x 6), tau (B).  It never writes the factor's L.x / Ut.x or its
// scratch, and keeps its own launch counters.  What a batch of any factorisation is -- the object's common part, the guards, the
// frame of a run (the flag and stat words set, every member's values through winL / winU, of duplicates the last), the solve
// frame -- is csx_valuebatch.h; this file holds what is the L U's:
//   SluBatchColumn  the batch policy of the level walk (csx_levelwalk.h: k_level_batch, k_run_batch): Lx, Ux by lnz, flags by 3,
//                    tau read from an array, then SluColumn::column -- slu_column itself, the host rule's bits
//   k_slb_stats      slu_stats_column per (column, member)
//   k_slb_norm1      |A_m|_1 by k_norm1's rule
//   the solve        which permutations and which planes: csx_batchsolve.h's sweeps (k_slb_level, k_slb_run) in the reference's
//                    operation order over F's height levels, the rows and the dots without a division before the chain
// There is NO scratch-then-commit: a member that breaks down is marked failed (ok[m] = 0, its values mean nothing) where the
// single factor keeps its old values.  Keeping them would take a second B x lnz pair of arrays.
#include <cmath>

#include "csx_internal.h"
#include "csx_slu.h"
#include "csx_valuebatch.h"

#pragma clang fp contract(off)

namespace csx {

struct SluBatch : ValueBatch {
    static constexpr Kind KIND = K_SLUBATCH, FACTOR_KIND = K_SLUFACTOR;
    DevBuf<double> Lx, Ux, tau;
    SluBatch() : ValueBatch("csx_slu_batch", 6, 2) {}   // slu_stats_column's six words, min |d| the third
    SluFactor *factor() const { return static_cast<SluFactor *>(F); }
};

void destroy(SluBatch *b) { delete b; }

// ---- factor ------------------------------------------------------------------------------------------------------------------

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

// ---- host -------------------------------------------------------------------------------------------------------------------

// every member's factor of V into the batch's arrays; ok[m] = 1 where no column of member m broke down.  One synchronisation.
static int slb_run(SluBatch *b, const double *V, const double *tau, int *ok) {
    hipStream_t s = ctx().stream;
    SluFactor *F = b->factor();
    Csc *L = csc(F->hL);
    if (!L) return CSX_EINVAL;
    const int32_t n = F->n, B = b->B;
    const int64_t lnz = F->lnz;
    CSX_TRY(batch_begin(b, tau, b->tau.get()));
    batch_scatter(b, V, lnz, F->winL.get(), b->Lx.get(), lnz, F->winU.get(), b->Ux.get());
    walk_levels_batch<SluBatchColumn>(F, B, &b->level_launches, &b->run_launches, SluBatchColumn::Args(), L->p, L->i, b->Lx, b->Ux,
                                      F->rp, F->rc, F->rpos, b->tau, b->flags, lnz);
    if (n > 0)
        hipLaunchKernelGGL(k_slb_stats, dim3((unsigned)(((int64_t)n + 3) / 4), (unsigned)B), dim3(256), 0, s, n, lnz, L->p,
                           b->Lx.get(), b->Ux.get(), b->stats.get());
    return batch_end(b, ok);
}

}  // namespace csx

using namespace csx;

extern "C" int csx_slu_batch_limits(int32_t *out) { return batch_limits(out); }   // (no device needed)

extern "C" int csx_slu_batch_factor(csx_handle_t hF, csx_handle_t hV, int32_t B, const double *tau, csx_handle_t *out, int *ok) {
    CSX_TRY(require_ready());
    SluFactor *F = (SluFactor *)get(hF, K_SLUFACTOR);
    if (!F || !out || !ok) return CSX_EINVAL;
    *out = 0;
    if (!batch_members_ok("csx_slu_batch_factor", B)) return CSX_EINVAL;
    const double *V = batch_values("csx_slu_batch_factor", hV, F->anz, B);
    if (!V) return CSX_EINVAL;
    std::unique_ptr<SluBatch> b(new SluBatch());
    CSX_TRY(b->Lx.alloc((size_t)B * (size_t)F->lnz));
    CSX_TRY(b->Ux.alloc((size_t)B * (size_t)F->lnz));
    CSX_TRY(b->tau.alloc((size_t)B));
    CSX_TRY(batch_alloc_common(b.get(), F, hF, B));
    CSX_TRY(slb_run(b.get(), V, tau, ok));
    *out = put(K_SLUBATCH, b.release());
    return CSX_OK;
}

extern "C" int csx_slu_batch_refactor(csx_handle_t h, csx_handle_t hV, const double *tau, int *ok) {
    CSX_TRY(require_ready());
    SluBatch *b = batch_get<SluBatch>(h);
    if (!b || !ok) return CSX_EINVAL;
    const double *V = batch_values("csx_slu_batch_refactor", hV, b->F->anz, b->B);
    return V ? slb_run(b, V, tau, ok) : CSX_EINVAL;
}

extern "C" int csx_slu_batch_norm1(csx_handle_t hF, csx_handle_t hV, int32_t B, double *out) {
    CSX_TRY(require_ready());
    SluFactor *F = (SluFactor *)get(hF, K_SLUFACTOR);
    if (!F || !out) return CSX_EINVAL;
    if (!batch_members_ok("csx_slu_batch_norm1", B)) return CSX_EINVAL;
    const double *V = batch_values("csx_slu_batch_norm1", hV, F->anz, B);
    if (!V) return CSX_EINVAL;
    return batch_norm1(B, out, [&](unsigned long long *best) {
        const int64_t items = (int64_t)F->n * B;
        if (items > 0)
            hipLaunchKernelGGL(k_slb_norm1, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, ctx().stream, F->n, B, F->p0.get(), V,
                               best);
    });
}

extern "C" int csx_slu_batch_solve(csx_handle_t h, csx_handle_t hX, int32_t r, int trans) {
    CSX_TRY(require_ready());
    SluBatch *b = batch_get<SluBatch>(h);
    if (!b || r < 1) return CSX_EINVAL;
    const SluFactor *F = b->factor();
    const Csc *L = csc(F->hL);
    if (!L) return CSX_EINVAL;
    const BatchPattern P = {L->p, L->i, F->rp.get(), F->rc.get(), F->rpos.get(), F->n, F->lnz, b->B};
    const int32_t *p_in = trans ? F->pinv : F->comb, *p_out = trans ? F->comb : F->pinv;
    // A x = b: cs_lsolve(L), cs_ltsolve(Ut);  A' x = b: cs_lsolve(Ut), cs_ltsolve(L)
    return batch_solve_lower(b, "csx_slu_batch_solve", hX, r, p_in, p_out, [&](double *W) {
        CSX_TRY(batch_sweep<true>(F, P, trans ? b->Ux.get() : b->Lx.get(), trans != 0, nullptr, r, W));
        return batch_sweep<false>(F, P, trans ? b->Lx.get() : b->Ux.get(), trans == 0, nullptr, r, W);
    });
}

extern "C" int csx_slu_batch_info(csx_handle_t h, int64_t *shared, int64_t *members) {
    CSX_TRY(require_ready());
    SluBatch *b = batch_get<SluBatch>(h);
    if (!b || !shared || !members) return CSX_EINVAL;
    batch_info_lower(b, b->factor()->lnz, shared, members);
    return CSX_OK;
}

extern "C" int csx_slu_batch_stats(csx_handle_t h, double *out) {
    CSX_TRY(require_ready());
    SluBatch *b = batch_get<SluBatch>(h);
    if (!b || !out) return CSX_EINVAL;
    batch_stats(b, 2, 4, out);
    return CSX_OK;
}

extern "C" int csx_slu_batch_member(csx_handle_t h, int32_t m, double *Lx_out, double *Utx_out) {
    CSX_TRY(require_ready());
    SluBatch *b = batch_get<SluBatch>(h);
    if (!b || m < 0 || m >= b->B || !Lx_out || !Utx_out) return CSX_EINVAL;
    const size_t lnz = (size_t)b->factor()->lnz;
    CSX_TRY(batch_member(b->Lx, m, lnz, Lx_out));
    CSX_TRY(batch_member(b->Ux, m, lnz, Utx_out));
    CSX_HIP(hipStreamSynchronize(ctx().stream));
    return CSX_OK;
}
