// Partial LDL' with the Schur complement of a kept index set (the definition is the comment of csx_schur_factor
// in include/csx.h).  The permutation numbers the n1 interior indices first and the ns kept ones last; the symbolic analysis,
// the entry map and the scatter are csx_chol's on the FULL pattern Lf of chol(P A P'), whose row view is what the trailing
// columns need.  The factor object, its build, run, commit and refactor are csx_ldl.hip's (LdlFactor, ldl_build, ldl_run,
// ldl_refactor: csx_ldl.h), the interior columns' launches the level walk's (csx_levelwalk.h) with the walker cut at
// WALK_RUN_LEVELS -- the LDL' factor is this one at n1 = n; what is here is what only ns > 0 needs:
//   k_schur_cols    the trailing columns, one wide level: one wave per (column j, chunk of at most LDL_ACC consecutive rows of
//                   j .. n - 1), the chunk's sums in wave-private LDS indexed by row - chunk start
// with its chunk list and the entry points.
// Every sum is updated in ascending k by one wave, one update after the other: Lp.x, d and S are byte-equal to csx_schur_host.
#include <algorithm>
#include <vector>

#include "csx_internal.h"
#include "csx_ldl.h"

#pragma clang fp contract(off)

namespace csx {

// Wave c takes rows [row0, min(row0 + LDL_ACC, n)) of column j = ch_col[c] of the permuted matrix, j >= n1.  Lx: the scratch
// values on the full pattern -- C in the slots of the trailing columns, the finished L in the interior ones; d: the interior
// pivots.  The row view of row j lists its columns k ascending and ends with the diagonal; the first k >= n1 ends the updates.
__global__ __launch_bounds__(64 * WALK_WAVES) void k_schur_cols(const int32_t *__restrict__ ch_col, const int32_t *__restrict__ ch_row0,
                                                              int64_t count, int32_t n, int32_t n1, const int32_t *__restrict__ Lp,
                                                              const int32_t *__restrict__ Li, const double *__restrict__ Lx,
                                                              const double *__restrict__ d, const int32_t *__restrict__ row_ptr,
                                                              const int32_t *__restrict__ row_col,
                                                              const int32_t *__restrict__ row_pos, double *__restrict__ S) {
    __shared__ double s_acc[WALK_WAVES][LDL_ACC];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t c = (int64_t)blockIdx.x * WALK_WAVES + w;
    if (c >= count) return;
    double *acc = s_acc[w];
    const int32_t j = ch_col[c], r0 = ch_row0[c];
    const int32_t rows = min(LDL_ACC, n - r0), r1 = r0 + rows;
    for (int32_t t = lane; t < rows; t += 64) acc[t] = 0.0;
    __builtin_amdgcn_wave_barrier();
    for (int32_t p = Lp[j] + lane; p < Lp[j + 1]; p += 64) {   // C(:, j): distinct rows
        const int32_t r = Li[p];
        if (r >= r0 && r < r1) acc[r - r0] = Lx[p];
    }
    __builtin_amdgcn_wave_barrier();
    // the updates (csx_colupdate.h): weight L(j,k) d[k], kept columns k >= n1 refused, sums in the LDS chunk at row - r0 or skipped
    column_updates<1>(
        j, Lp, Li, row_ptr, row_col, row_pos, lane,
        [&](int32_t k, int32_t pos, double (&w)[1]) {
            if (k >= n1) return false;   // k ascending: nothing but trailing columns from here on
            w[0] = Lx[pos] * d[k];
            return true;
        },
        [&](int32_t p, double (&v)[1]) { v[0] = Lx[p]; },
        [&](int32_t row, const double (&a)[1]) {
            if (row >= r0 && row < r1) acc[row - r0] = acc[row - r0] - a[0];
        });
    __builtin_amdgcn_wave_barrier();
    const int64_t ns = n - n1, cj = j - n1;
    for (int32_t t = lane; t < rows; t += 64) {
        const int64_t cr = r0 + t - n1;
        const double v = acc[t];
        S[cr * ns + cj] = v;
        S[cj * ns + cr] = v;
    }
}

void schur_launch_cols(const LdlFactor *F) {
    hipLaunchKernelGGL(k_schur_cols, dim3((unsigned)((F->chunks + WALK_WAVES - 1) / WALK_WAVES)), dim3(64 * WALK_WAVES), 0, ctx().stream,
                       F->ch_col.get(), F->ch_row0.get(), F->chunks, F->n, F->n1, F->Lp, F->Li, F->Lx.get(), F->dd.get(), F->rp.get(),
                       F->rc.get(), F->rpos.get(), F->Sx.get());
}

// the chunk list of k_schur_cols: every trailing column j cut into runs of at most LDL_ACC rows of j .. n - 1.  Synchronises.
static int schur_chunks(LdlFactor *F) {
    std::vector<int32_t> ch_col, ch_row0;
    for (int32_t j = F->n1; j < F->n; j++)
        for (int32_t r0 = j; r0 < F->n; r0 += LDL_ACC) {
            ch_col.push_back(j);
            ch_row0.push_back(r0);
        }
    F->chunks = (int64_t)ch_col.size();
    CSX_TRY(upload(F->ch_col, ch_col));
    CSX_TRY(upload(F->ch_row0, ch_row0));
    CSX_HIP(hipStreamSynchronize(ctx().stream));   // (the two lists have landed)
    return CSX_OK;
}

}  // namespace csx

using namespace csx;

extern "C" int csx_schur_factor(csx_handle_t hA, const int32_t *parent, const int32_t *cp, const int32_t *pinv, int32_t n1, double tau,
                                csx_handle_t *out, int *ok) {
    CSX_TRY(require_ready());
    Csc *A = csc(hA);
    if (!A || !out || !ok || !A->x || A->m != A->n || !cp || (A->n > 0 && !parent) || !(tau >= 0.0)) return CSX_EINVAL;
    if (n1 < 0 || n1 > A->n || (int64_t)(A->n - n1) * (A->n - n1) >= ((int64_t)1 << 31)) return CSX_EINVAL;
    *out = 0;
    *ok = 0;
    std::unique_ptr<LdlFactor> F(new LdlFactor());
    CSX_TRY(ldl_build(A, parent, cp, pinv, n1, WALK_RUN_LEVELS, "csx_schur", F.get()));
    CSX_TRY(schur_chunks(F.get()));
    CSX_TRY(ldl_run(F.get(), A->x, tau, ok));
    if (*ok) *out = put(K_SCHURFACTOR, F.release());
    return CSX_OK;
}

extern "C" int csx_schur_refactor(csx_handle_t h, csx_handle_t hA2, double tau, int *ok) {
    CSX_TRY(require_ready());
    return ldl_refactor((LdlFactor *)get(h, K_SCHURFACTOR), hA2, tau, ok);
}

extern "C" int csx_schur_parts(csx_handle_t h, csx_handle_t *L, csx_handle_t *d, csx_handle_t *S) {
    CSX_TRY(require_ready());
    LdlFactor *F = (LdlFactor *)get(h, K_SCHURFACTOR);
    if (!F || !L || !d || !S) return CSX_EINVAL;
    *L = F->hL;
    *d = F->hd;
    *S = F->hS;
    return CSX_OK;
}

extern "C" int csx_schur_info(csx_handle_t h, int64_t *info) {
    CSX_TRY(require_ready());
    LdlFactor *F = (LdlFactor *)get(h, K_SCHURFACTOR);
    if (!F || !info) return CSX_EINVAL;
    info[0] = F->n;
    info[1] = F->n1;
    info[2] = F->ns;
    info[3] = (int64_t)F->head + F->ns;
    info[4] = F->levels();
    info[5] = F->launches() + F->schur_launches;
    info[6] = F->level_launches;
    info[7] = F->run_launches;
    info[8] = F->schur_launches;
    info[9] = F->chunks;
    info[10] = F->pos;
    info[11] = F->neg;
    info[12] = F->perturbed;
    info[13] = F->breakdown;
    info[14] = F->kernel_us;
    info[15] = F->long_cols;
    info[16] = LDL_ACC;
    return CSX_OK;
}

extern "C" int csx_schur_stats(csx_handle_t h, double *out) {
    CSX_TRY(require_ready());
    return ldl_stats((const LdlFactor *)get(h, K_SCHURFACTOR), out);
}
