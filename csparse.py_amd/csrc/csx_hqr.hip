// Sparse Householder QR of a matrix in one connected piece (the definition is the comment of csx_hqr_factor in
// include/csx.h).  Householder QR searches for no pivot: the patterns of V and R follow from cs_sqr's analysis and the column
// elimination tree before a value is read (csx_hqr_symbolic_host), and column k reads only V(:,c) and beta[c] of its descendants
// c.  So the columns of one height level of the tree are independent, as in csx_ldl.hip and csx_slu.hip.
//   hqr_column    one wave's column, behind the policy HqrColumn of the level walk (csx_levelwalk.h: k_level, k_run, the
//                 schedule with the walker cut at WALK_RUN_LEVELS levels or HQR_RUN_WORK slot updates a launch)
//   k_hqr_stats   min / max |r_kk| and the number of exact zeros on R's diagonal
// Both, with the factor object, are in csx_hqr.h, which csx_hqr_batch.hip (many value sets on one analysis) shares.
// Every row a reflection of column k touches is a slot of R(:,k) or of V(:,k): the column's own slots are its accumulators, in
// wave-private LDS up to HQR_ACC slots and in place in the scratch arrays beyond.  A reflection's dot product is 64 strided
// partial sums and a butterfly, a fixed order: V.x, R.x and beta are byte-equal to csx_hqr_host, the same on every run.
// A factor or refactor runs into scratch arrays and is committed only when no diagonal of R came out non-finite.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "csx_hqr.h"

#pragma clang fp contract(off)

namespace csx {

// hqr_stats_column (csx_hqr.h) for one value set
__global__ __launch_bounds__(256) void k_hqr_stats(int32_t n, const int32_t *__restrict__ Rp, const double *__restrict__ Rx,
                                                   unsigned long long *st) {
    hqr_stats_column((int64_t)blockIdx.x * blockDim.x + threadIdx.x, threadIdx.x & 63, n, Rp, Rx, st);
}

void destroy(HqrFactor *F) { delete F; }

// The factor of the values Ax (A's storage order) into the scratch arrays, with the statistics of what was computed; commits
// into V.x / R.x / beta when no column broke down.  *ok: 1 committed, 0 breakdown (the factor untouched).  Synchronises.
static int hqr_run(HqrFactor *F, const double *Ax, int *ok) {
    hipStream_t s = ctx().stream;
    Csc *V = csc(F->hV), *R = csc(F->hR);
    if (!V || !R || !V->x || !R->x || V->nnz != F->vnz || R->nnz != F->rnz) return CSX_EINVAL;
    const int32_t n = F->n;
    const int hinit[2] = {WALK_NONE, 0};
    const unsigned long long sinit[3] = {~0ull, 0ull, 0ull};
    CSX_TRY(walk_begin(F, hinit, 2, sinit, 3));
    CSX_TRY(chol_scatter(F->vnz, F->winV, Ax, F->Vx));
    CSX_TRY(chol_scatter(F->rnz, F->winR, Ax, F->Rx));
    walk_levels<HqrColumn>(F, HqrColumn::Args(), V->p, V->i, F->Vx, R->p, R->i, F->Rx, F->bx, F->sp, F->srow, F->sdst, F->flags);
    if (n > 0)
        hipLaunchKernelGGL(k_hqr_stats, dim3((unsigned)(((int64_t)n + 255) / 256)), dim3(256), 0, s, n, R->p, F->Rx.get(),
                           F->stats.get());
    int hflags[2] = {WALK_NONE, 0};
    unsigned long long hst[3] = {0, 0, 0};
    CSX_TRY(walk_end(F, hflags, 2, hst, 3, ok));
    F->long_cols = hflags[1];
    if (!*ok) return CSX_OK;
    if (n == 0) hst[0] = 0;
    std::memcpy(&F->min_r, &hst[0], 8);
    std::memcpy(&F->max_r, &hst[1], 8);
    F->zeros = (int64_t)hst[2];
    if (F->vnz) CSX_HIP(hipMemcpyAsync(V->x, F->Vx.get(), (size_t)F->vnz * sizeof(double), hipMemcpyDeviceToDevice, s));
    if (F->rnz) CSX_HIP(hipMemcpyAsync(R->x, F->Rx.get(), (size_t)F->rnz * sizeof(double), hipMemcpyDeviceToDevice, s));
    if (n) CSX_HIP(hipMemcpyAsync(F->beta.get(), F->bx.get(), (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, s));
    for (Csc *M : {V, R}) {   // (copies of the old values; V's reflection levels are pattern only and stay)
        M->rows.reset();
        M->tiled.reset();
    }
    CSX_HIP(hipStreamSynchronize(s));
    return CSX_OK;
}

static int hqr_build(Csc *A, const int32_t *q, const int32_t *parent, const int32_t *pinv, const int32_t *leftmost, int32_t m2,
                     HqrFactor *F) {
    hipStream_t s = ctx().stream;
    const int32_t m = A->m, n = A->n;
    F->m2 = m2;
    if (!A->trusted) CSX_TRY(csc_validate(A));
    std::vector<int32_t> ap, ai, vp, vi, rp, ri;
    CSX_TRY(download_i32(ap, A->p, (size_t)n + 1));
    CSX_TRY(download_i32(ai, A->i, (size_t)A->nnz));
    if (hqr_symbolic(m, n, m2, ap.data(), ai.data(), q, parent, pinv, leftmost, vp, vi, rp, ri) != CSX_OK) {
        set_error("csx_hqr_factor: the symbolic analysis is not this matrix's");
        return CSX_EINVAL;
    }
    F->vnz = vp[(size_t)n];
    F->rnz = rp[(size_t)n];
    // the entry maps (of duplicates the last stored) and the sorted view of every column's slots
    std::vector<int32_t> winV((size_t)F->vnz, -1), winR((size_t)F->rnz, -1), where((size_t)m2, -1);
    std::vector<int32_t> sp((size_t)n + 1, 0), srow((size_t)F->vnz + (size_t)F->rnz - (size_t)n), sdst(srow.size());
    std::vector<std::pair<int32_t, int32_t>> tmp;
    for (int32_t k = 0; k < n; k++) {
        const int32_t rb = rp[(size_t)k], nr = rp[(size_t)k + 1] - rb - 1, vb = vp[(size_t)k], nv = vp[(size_t)k + 1] - vb;
        for (int32_t t = 0; t < nr; t++) where[(size_t)ri[(size_t)(rb + t)]] = t;          // columns c < k: R's slots
        for (int32_t j = 0; j < nv; j++) where[(size_t)vi[(size_t)(vb + j)]] = nr + j;     // rows >= k: V's slots
        const int32_t col = q ? q[k] : k;
        for (int32_t p = ap[(size_t)col]; p < ap[(size_t)col + 1]; p++) {
            const int32_t slot = where[(size_t)pinv[ai[(size_t)p]]];   // (hqr_symbolic has seen that the row has one)
            if (slot < nr) winR[(size_t)(rb + slot)] = p;
            else winV[(size_t)(vb + slot - nr)] = p;
        }
        const int32_t sb = rb - k + vb;
        sp[(size_t)k] = sb;
        tmp.clear();
        for (int32_t t = 0; t < nr; t++) tmp.emplace_back(ri[(size_t)(rb + t)], t);
        for (int32_t j = 0; j < nv; j++) tmp.emplace_back(vi[(size_t)(vb + j)], nr + j);
        std::sort(tmp.begin(), tmp.end());
        for (size_t t = 0; t < tmp.size(); t++) {
            srow[(size_t)sb + t] = tmp[t].first;
            sdst[(size_t)sb + t] = tmp[t].second;
        }
    }
    sp[(size_t)n] = F->rnz - n + F->vnz;
    CSX_TRY(walk_init(F, A, "csx_hqr", 2, 3));
    std::vector<int32_t> cols;
    height_levels(n, parent, F->level_ptr_h, cols);
    // the work of a level the walker may take: the slot updates of its longest column, every reflection's entries summed
    std::vector<int64_t> work((size_t)F->levels(), 0);
    for (int32_t l = 0; l < F->levels(); l++) {
        const int32_t b = F->level_ptr_h[(size_t)l], e = F->level_ptr_h[(size_t)l + 1];
        if (e - b > WALK_WAVES) continue;   // (a wide level: a launch of its own whatever it costs)
        for (int32_t t = b; t < e; t++) {
            const int32_t k = cols[(size_t)t];
            int64_t w = 0;
            for (int32_t u = rp[(size_t)k]; u < rp[(size_t)k + 1] - 1; u++) w += vp[(size_t)ri[(size_t)u] + 1] - vp[(size_t)ri[(size_t)u]];
            work[(size_t)l] = std::max(work[(size_t)l], w);
        }
    }
    CSX_TRY(walk_set_levels(F, cols, WALK_RUN_LEVELS, work.data(), HQR_RUN_WORK));
    CSX_TRY(upload(F->sp, sp));
    CSX_TRY(upload(F->srow, srow));
    CSX_TRY(upload(F->sdst, sdst));
    CSX_TRY(upload(F->winV, winV));
    CSX_TRY(upload(F->winR, winR));
    if (q) CSX_TRY(upload(F->perm_q, q, (size_t)n));   // the permutations of a batched solve (csx_hqr_batch.hip); they land
    CSX_TRY(upload(F->perm_p, pinv, (size_t)m));       // ... before the synchronisation below
    std::unique_ptr<Csc> V, R;
    {
        DevBuf<int32_t> dvp, dvi, drp, dri;
        CSX_TRY(upload(dvp, vp));
        CSX_TRY(upload(dvi, vi));
        CSX_TRY(upload(drp, rp));
        CSX_TRY(upload(dri, ri));
        CSX_TRY(csc_copy_pattern(m2, n, F->vnz, dvp.get(), dvi.get(), true, &V));
        CSX_TRY(csc_copy_pattern(n, n, F->rnz, drp.get(), dri.get(), true, &R));   // nothing of R lies below row n
        CSX_HIP(hipStreamSynchronize(s));   // (the host vectors and the staging buffers have landed)
    }
    CSX_TRY(F->beta.alloc((size_t)std::max(n, 1)));
    CSX_TRY(F->bx.alloc((size_t)std::max(n, 1)));
    CSX_TRY(F->Vx.alloc((size_t)F->vnz));
    CSX_TRY(F->Rx.alloc((size_t)F->rnz));
    std::unique_ptr<Vec> B(new Vec());
    B->len = n;
    B->d = F->beta.get();
    B->owns = false;
    F->hV = put(K_CSC, V.release());
    F->hR = put(K_CSC, R.release());
    F->hB = put(K_VEC, B.release());
    return CSX_OK;
}

}  // namespace csx

using namespace csx;

extern "C" int csx_hqr_factor(csx_handle_t hA, const int32_t *q, const int32_t *parent, const int32_t *pinv, const int32_t *leftmost,
                              int32_t m2, csx_handle_t *out, int *ok) {
    CSX_TRY(require_ready());
    Csc *A = csc(hA);
    if (!A || !out || !ok || !A->x || A->m < A->n || m2 < A->m || (A->n > 0 && !parent) || (A->m > 0 && (!pinv || !leftmost)))
        return CSX_EINVAL;
    *out = 0;
    *ok = 0;
    std::unique_ptr<HqrFactor> F(new HqrFactor());
    CSX_TRY(hqr_build(A, q, parent, pinv, leftmost, m2, F.get()));
    CSX_TRY(hqr_run(F.get(), A->x, ok));
    if (*ok) *out = put(K_HQRFACTOR, F.release());
    return CSX_OK;
}

extern "C" int csx_hqr_refactor(csx_handle_t h, csx_handle_t hA2, int *ok) {
    CSX_TRY(require_ready());
    HqrFactor *F = (HqrFactor *)get(h, K_HQRFACTOR);
    if (!F || !ok) return CSX_EINVAL;
    return walk_refactor(F, hA2, ok, [&](const double *x2) { return hqr_run(F, x2, ok); });
}

extern "C" int csx_hqr_parts(csx_handle_t h, csx_handle_t *V, csx_handle_t *R, csx_handle_t *beta) {
    CSX_TRY(require_ready());
    HqrFactor *F = (HqrFactor *)get(h, K_HQRFACTOR);
    if (!F || !V || !R || !beta) return CSX_EINVAL;
    *V = F->hV;
    *R = F->hR;
    *beta = F->hB;
    return CSX_OK;
}

extern "C" int csx_hqr_info(csx_handle_t h, int64_t *info) {
    CSX_TRY(require_ready());
    HqrFactor *F = (HqrFactor *)get(h, K_HQRFACTOR);
    if (!F || !info) return CSX_EINVAL;
    info[0] = F->m;
    info[1] = F->n;
    info[2] = F->m2;
    info[3] = F->vnz;
    info[4] = F->rnz;
    info[5] = F->levels();
    info[6] = F->launches();
    info[7] = F->level_launches;
    info[8] = F->run_launches;
    info[9] = F->long_cols;
    info[10] = F->zeros;
    info[11] = F->breakdown;
    info[12] = F->kernel_us;
    info[13] = HQR_ACC;
    info[14] = WALK_RUN_LEVELS;
    return CSX_OK;
}

extern "C" int csx_hqr_stats(csx_handle_t h, double *out) {
    CSX_TRY(require_ready());
    HqrFactor *F = (HqrFactor *)get(h, K_HQRFACTOR);
    if (!F || !out) return CSX_EINVAL;
    out[0] = F->min_r;
    out[1] = F->max_r;
    return CSX_OK;
}

extern "C" int csx_hqr_window(int32_t *entries, int32_t *run_levels) {   // (no device needed)
    if (!entries || !run_levels) return CSX_EINVAL;
    *entries = HQR_ACC;
    *run_levels = WALK_RUN_LEVELS;
    return CSX_OK;
}
