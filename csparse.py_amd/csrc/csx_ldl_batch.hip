// Many symmetric value sets on the analysis of one L D L' (the definition is the comment of csx_ldl_batch_factor in
// include/csx.h).  An LdlBatch BORROWS an LdlFactor of kind K_LDLFACTOR (nothing kept: ns = 0) -- pattern, row view, entry map,
// height levels, launch schedule, permutation -- and owns B value sets: Lx (B x lnz doubles, member-major: member m's column j is
// the contiguous piece ldl_column expects), dd (B x n), tau (B), flags (B x 3), stats (B x 5).  It never writes the factor's L.x /
// d or its scratch, and keeps its own launch counters.  What a batch of any factorisation is -- the object's common part, the
// guards, the frame of a run (the flag and stat words set, every member's values through win, of duplicates the last), the solve
// frame -- is csx_valuebatch.h; this file holds what is the L D L''s:
//   LdlBatchColumn  the batch policy of the level walk (csx_levelwalk.h: k_level_batch, k_run_batch): Lx by lnz, d by n, flags by
//                    3, tau read from an array, then LdlColumn::column -- ldl_column itself, the host rule's bits
//   k_ldb_stats      ldl_stats_column per (column, member)
//   k_ldb_norm1      |S_m|_1 by k_norm1_sym's rule, over the row view of A's pattern (row_view of csx_levelwalk.h, kept in F)
//   the solve        csx_batchsolve.h's sweeps: the rows of L ascending, then the dots of L descending with the division by d
//                    BEFORE each chain -- no pass of its own over X for D
// There is NO scratch-then-commit: a member that breaks down is marked failed (ok[m] = 0, its values mean nothing) where the
// single factor keeps its old values.
#include <cmath>

#include "csx_internal.h"
#include "csx_ldl.h"
#include "csx_valuebatch.h"

#pragma clang fp contract(off)

namespace csx {

struct LdlBatch : ValueBatch {
    static constexpr Kind KIND = K_LDLBATCH, FACTOR_KIND = K_LDLFACTOR;
    DevBuf<double> Lx, dd, tau;
    LdlBatch() : ValueBatch("csx_ldl_batch", 5, 2) {}   // ldl_stats_column's five words, min |d| the third
    LdlFactor *factor() const { return static_cast<LdlFactor *>(F); }
};

void destroy(LdlBatch *b) { delete b; }

// ---- factor ------------------------------------------------------------------------------------------------------------------

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

// The row view of A's pattern with its map back to storage positions, from F's kept p0 / i0: row r holds (column, position) of
// its entries in ascending (column, position) -- the order of A's cached row gather, which k_norm1_sym reads.  Built on the first
// csx_ldl_batch_norm1 on F and kept there (A's pattern never changes); synchronises once.
static int ldb_row_view(LdlFactor *F) {
    if (F->a_rows) return CSX_OK;
    std::vector<int32_t> p, i, rp, rc, rpos;
    CSX_TRY(download_i32(p, F->p0, (size_t)F->n + 1));
    CSX_TRY(download_i32(i, F->i0, (size_t)F->anz));
    if ((F->n > 0 ? p[(size_t)F->n] : 0) != F->anz || !row_view(F->n, p.data(), i.data(), false, rp, rc, rpos)) return CSX_EINVAL;
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
    LdlFactor *F = b->factor();
    const int32_t n = F->n, B = b->B;
    const int64_t lnz = F->lnz;
    CSX_TRY(batch_begin(b, tau, b->tau.get()));
    batch_scatter(b, V, lnz, F->win.get(), b->Lx.get(), 0, nullptr, nullptr);
    walk_levels_batch<LdlBatchColumn>(F, B, &b->level_launches, &b->run_launches, LdlBatchColumn::Args(), F->Lp, F->Li, b->Lx, b->dd,
                                      F->rp, F->rc, F->rpos, b->tau, b->flags, lnz, (int64_t)n);
    if (n > 0)
        hipLaunchKernelGGL(k_ldb_stats, dim3((unsigned)(((int64_t)n + 3) / 4), (unsigned)B), dim3(256), 0, s, n, lnz, F->Lp,
                           b->Lx.get(), b->dd.get(), b->stats.get());
    return batch_end(b, ok);
}

}  // namespace csx

using namespace csx;

extern "C" int csx_ldl_batch_limits(int32_t *out) { return batch_limits(out); }   // (no device needed)

extern "C" int csx_ldl_batch_factor(csx_handle_t hF, csx_handle_t hV, int32_t B, const double *tau, csx_handle_t *out, int *ok) {
    CSX_TRY(require_ready());
    if (out) *out = 0;
    LdlFactor *F = ldb_factor("csx_ldl_batch_factor", hF);
    if (!F || !out || !ok) return CSX_EINVAL;
    if (!batch_members_ok("csx_ldl_batch_factor", B)) return CSX_EINVAL;
    const double *V = batch_values("csx_ldl_batch_factor", hV, F->anz, B);
    if (!V) return CSX_EINVAL;
    std::unique_ptr<LdlBatch> b(new LdlBatch());
    CSX_TRY(b->Lx.alloc((size_t)B * (size_t)F->lnz));
    CSX_TRY(b->dd.alloc((size_t)B * (size_t)F->n));
    CSX_TRY(b->tau.alloc((size_t)B));
    CSX_TRY(batch_alloc_common(b.get(), F, hF, B));
    CSX_TRY(ldb_run(b.get(), V, tau, ok));
    *out = put(K_LDLBATCH, b.release());
    return CSX_OK;
}

extern "C" int csx_ldl_batch_refactor(csx_handle_t h, csx_handle_t hV, const double *tau, int *ok) {
    CSX_TRY(require_ready());
    LdlBatch *b = batch_get<LdlBatch>(h);
    if (!b || !ok) return CSX_EINVAL;
    const double *V = batch_values("csx_ldl_batch_refactor", hV, b->F->anz, b->B);
    return V ? ldb_run(b, V, tau, ok) : CSX_EINVAL;
}

extern "C" int csx_ldl_batch_norm1(csx_handle_t hF, csx_handle_t hV, int32_t B, double *out) {
    CSX_TRY(require_ready());
    LdlFactor *F = ldb_factor("csx_ldl_batch_norm1", hF);
    if (!F || !out) return CSX_EINVAL;
    if (!batch_members_ok("csx_ldl_batch_norm1", B)) return CSX_EINVAL;
    const double *V = batch_values("csx_ldl_batch_norm1", hV, F->anz, B);
    if (!V) return CSX_EINVAL;
    CSX_TRY(ldb_row_view(F));
    return batch_norm1(B, out, [&](unsigned long long *best) {
        const int64_t items = (int64_t)F->n * B;
        if (items > 0)
            hipLaunchKernelGGL(k_ldb_norm1, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, ctx().stream, F->n, B, F->p0.get(),
                               F->i0.get(), F->arp.get(), F->arc.get(), F->apos.get(), V, best);
    });
}

extern "C" int csx_ldl_batch_solve(csx_handle_t h, csx_handle_t hX, int32_t r) {
    CSX_TRY(require_ready());
    LdlBatch *b = batch_get<LdlBatch>(h);
    if (!b || r < 1) return CSX_EINVAL;
    const LdlFactor *F = b->factor();
    const BatchPattern P = {F->Lp, F->Li, F->rp.get(), F->rc.get(), F->rpos.get(), F->n, F->lnz, b->B};
    // cs_lsolve(L), then x / d and cs_ltsolve(L) in one sweep: the division by d_j opens row j's backward chain.  It cannot close
    // row j's forward chain instead: the forward chains of the later rows read x_j undivided (csx_batchsolve.h).
    return batch_solve_lower(b, "csx_ldl_batch_solve", hX, r, F->pinv, F->pinv, [&](double *W) {
        CSX_TRY(batch_sweep<true>(F, P, b->Lx.get(), false, nullptr, r, W));
        return batch_sweep<false, true>(F, P, b->Lx.get(), false, b->dd.get(), r, W);
    });
}

extern "C" int csx_ldl_batch_info(csx_handle_t h, int64_t *shared, int64_t *members) {
    CSX_TRY(require_ready());
    LdlBatch *b = batch_get<LdlBatch>(h);
    if (!b || !shared || !members) return CSX_EINVAL;
    batch_info_lower(b, b->factor()->lnz, shared, members);
    return CSX_OK;
}

extern "C" int csx_ldl_batch_stats(csx_handle_t h, double *out) {
    CSX_TRY(require_ready());
    LdlBatch *b = batch_get<LdlBatch>(h);
    if (!b || !out) return CSX_EINVAL;
    batch_stats(b, 2, 3, out);
    return CSX_OK;
}

extern "C" int csx_ldl_batch_member(csx_handle_t h, int32_t m, double *Lx_out, double *d_out) {
    CSX_TRY(require_ready());
    LdlBatch *b = batch_get<LdlBatch>(h);
    if (!b || m < 0 || m >= b->B || !Lx_out || !d_out) return CSX_EINVAL;
    CSX_TRY(batch_member(b->Lx, m, (size_t)b->factor()->lnz, Lx_out));
    CSX_TRY(batch_member(b->dd, m, (size_t)b->F->n, d_out));
    CSX_HIP(hipStreamSynchronize(ctx().stream));
    return CSX_OK;
}

extern "C" int csx_ldl_batch_d(csx_handle_t h, double *out) {
    CSX_TRY(require_ready());
    LdlBatch *b = batch_get<LdlBatch>(h);
    if (!b || !out) return CSX_EINVAL;
    CSX_TRY(batch_member(b->dd, 0, (size_t)b->B * (size_t)b->F->n, out));   // all members' pivots: one piece
    CSX_HIP(hipStreamSynchronize(ctx().stream));
    return CSX_OK;
}

