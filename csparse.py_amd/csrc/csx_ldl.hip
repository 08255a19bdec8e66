// LDL' with static 1x1 pivots for symmetric indefinite matrices (the definition is the comment of
// csx_ldl_factor in include/csx.h).  L D L' = C = upper(P A P') on the pattern of the Cholesky factor: without a pivot search
// the pattern of L is cs_chol's, so the symbolic step (chol_symbolic_device), the entry map (chol_entry_map) and the scatter
// (chol_scatter) are csx_chol's own; the numeric kernels here are the left-looking column of chol_column with d[k] carried
// beside L(j,k), no square root, and the pivot rule (perturbation below tau, breakdown at 0 or a non-finite pivot).
//   ldl_column    one wave's column, behind the policy LdlColumn of the level walk (csx_ldl.h; csx_levelwalk.h: k_level, k_run, the
//                 schedule)
//   k_ldl_stats   inertia, min / max |d|, max |l| off the diagonal in one pass (ldl_stats_column, csx_ldl.h)
//   k_block_div_rows  X[i, :] /= d[i], the D step of a solve
// Every sum is updated in ascending k by one wave, one update after the other: L.x and d are byte-equal to csx_ldl_host.
// A factor or refactor runs into scratch arrays and is committed only when no column broke down.
// The host side is the partial elimination of the first n1 columns (LdlFactor, ldl_build, ldl_run, ldl_refactor: csx_ldl.h):
// csx_ldl_factor is n1 = n with the walker uncapped, csx_schur_factor (csx_schur.hip) its own n1 with the walker cut; the
// trailing columns are csx_schur.hip's kernel behind schur_launch_cols.  csx_level_schedule, the walk's scheduler on host
// arrays, and csx_row_view, its row-view builder (csx_levelwalk.h), are exported here.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "csx_internal.h"
#include "csx_ldl.h"

#pragma clang fp contract(off)

namespace csx {

// ldl_column, its policy LdlColumn and one column of the statistics: csx_ldl.h (shared with csx_ldl_batch.hip)

// One wave per column: ldl_stats_column (csx_ldl.h) into the five words st
__global__ __launch_bounds__(256) void k_ldl_stats(int32_t n, const int32_t *__restrict__ Lp, const double *__restrict__ Lx,
                                                   const double *__restrict__ d, unsigned long long *st) {
    const int lane = threadIdx.x & 63;
    const int64_t j = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (j >= n) return;
    ldl_stats_column(j, lane, Lp, Lx, d, st);
}

// X[i, c] = X[i, c] / d[i] over a row-major rows x nrhs block; PAIR: two columns per thread through 16-byte accesses
// (nrhs even and X 16-byte aligned: a pair never straddles a row)
template <bool PAIR>
__global__ __launch_bounds__(256) void k_block_div_rows(double *__restrict__ X, const double *__restrict__ d, int64_t rows,
                                                        int32_t nrhs) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t total = rows * nrhs;
    if (PAIR) {
        double2 *X2 = reinterpret_cast<double2 *>(X);
        for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; 2 * e < total; e += stride) {
            const double di = d[(2 * e) / nrhs];
            double2 v = X2[e];
            v.x = v.x / di;
            v.y = v.y / di;
            X2[e] = v;
        }
    } else {
        for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) X[e] = X[e] / d[e / nrhs];
    }
}

void destroy(LdlFactor *F) { delete F; }

int ldl_run(LdlFactor *F, const double *Ax, double tau, int *ok) {
    hipStream_t s = ctx().stream;
    Csc *L = csc(F->hL);
    Vec *dv = vec(F->hd), *Sv = vec(F->hS);
    const int64_t ns = F->ns;
    if (!L || !dv || !Sv || !L->x || L->nnz != F->head + ns || dv->len != F->n1 || Sv->len != ns * ns) return CSX_EINVAL;
    const int32_t n1 = F->n1;
    F->schur_launches = 0;
    const int hinit[3] = {WALK_NONE, 0, 0};
    const unsigned long long sinit[5] = {0ull, 0ull, ~0ull, 0ull, 0ull};
    CSX_TRY(walk_begin(F, hinit, 3, sinit, 5));
    CSX_TRY(chol_scatter(F->lnz, F->win, Ax, F->Lx));
    walk_levels<LdlColumn>(F, LdlColumn::Args(), F->Lp, F->Li, F->Lx, F->dd, F->rp, F->rc, F->rpos, tau, F->flags);
    if (F->chunks > 0) {
        schur_launch_cols(F);
        F->schur_launches = 1;
    }
    if (n1 > 0)
        hipLaunchKernelGGL(k_ldl_stats, dim3((unsigned)(((int64_t)n1 + 3) / 4)), dim3(256), 0, s, n1, F->Lp, F->Lx.get(), F->dd.get(),
                           F->stats.get());
    int hflags[3] = {WALK_NONE, 0, 0};
    unsigned long long hst[5] = {0, 0, 0, 0, 0};
    CSX_TRY(walk_end(F, hflags, 3, hst, 5, ok));
    F->perturbed = hflags[1];
    F->long_cols = hflags[2];
    if (!*ok) return CSX_OK;
    F->pos = (int64_t)hst[0];
    F->neg = (int64_t)hst[1];
    if (n1 == 0) hst[2] = 0;
    std::memcpy(&F->min_d, &hst[2], 8);
    std::memcpy(&F->max_d, &hst[3], 8);
    std::memcpy(&F->max_l, &hst[4], 8);
    // (the ns unit values behind L->x[head) were written by ldl_build and never change)
    if (F->head) CSX_HIP(hipMemcpyAsync(L->x, F->Lx.get(), (size_t)F->head * sizeof(double), hipMemcpyDeviceToDevice, s));
    if (n1) CSX_HIP(hipMemcpyAsync(dv->d, F->dd.get(), (size_t)n1 * sizeof(double), hipMemcpyDeviceToDevice, s));
    if (ns) CSX_HIP(hipMemcpyAsync(Sv->d, F->Sx.get(), (size_t)(ns * ns) * sizeof(double), hipMemcpyDeviceToDevice, s));
    L->rows.reset();    // (copies of the old values)
    L->tiled.reset();
    CSX_HIP(hipStreamSynchronize(s));
    return CSX_OK;
}

int ldl_build(Csc *A, const int32_t *parent, const int32_t *cp, const int32_t *pinv, int32_t n1, int32_t run_levels, const char *who,
              LdlFactor *F) {
    hipStream_t s = ctx().stream;
    const int32_t n = A->n, ns = n - n1;
    F->n1 = n1;
    F->ns = ns;
    F->lnz = cp[n];
    if (cp[0] != 0 || F->lnz < n) return CSX_EINVAL;
    for (int32_t j = 0; j < n; j++)
        if (cp[j + 1] <= cp[j]) return CSX_EINVAL;
    F->head = cp[n1];
    if (!A->trusted) CSX_TRY(csc_validate(A));
    CSX_TRY(walk_init(F, A, who, 3, 5));
    const int64_t lpnz = (int64_t)F->head + ns;
    std::unique_ptr<Csc> L(new Csc());
    L->m = L->n = n;
    L->nnz = (int32_t)lpnz;
    CSX_TRY(dalloc(&L->x, (size_t)lpnz));
    std::vector<int32_t> cols, lp, tail;   // (host lists of the copies queued below: alive until the stream is synchronised)
    const std::vector<double> ones((size_t)ns, 1.0);
    if (n == 0) {
        CSX_TRY(dalloc(&L->p, 1));
        CSX_HIP(hipMemsetAsync(L->p, 0, sizeof(int32_t), s));
        CSX_TRY(dalloc(&L->i, 0));
        F->Lp = L->p;
        F->Li = L->i;
        F->level_ptr_h.assign(1, 0);
    } else {
        int32_t *fp = nullptr, *fi = nullptr;
        const int st = chol_symbolic_device(A, parent, cp, pinv, &fp, &fi, &F->rp, &F->rc, &F->rpos, nullptr);   // (checks S and pinv)
        if (ns == 0) {   // Lp's pattern is the full pattern
            L->p = fp;
            L->i = fi;
        } else {
            F->fp = DevBuf<int32_t>(fp);
            F->fi = DevBuf<int32_t>(fi);
        }
        CSX_TRY(st);
        F->Lp = fp;
        F->Li = fi;
        // the height levels of the first n1 columns: the tree cut at n1 (a parent among the kept columns is no parent); a column's
        // level depends on its children alone, so the cut leaves the levels below it as they are, and at n1 == n it cuts nothing
        std::vector<int32_t> cut((size_t)n1);
        for (int32_t j = 0; j < n1; j++) cut[(size_t)j] = parent[j] < n1 ? parent[j] : -1;
        height_levels(n1, cut.data(), F->level_ptr_h, cols);
        CSX_TRY(walk_set_levels(F, cols, run_levels));
        CSX_TRY(F->win.alloc((size_t)F->lnz));
        if (pinv) {   // (kept: csx_ldl_batch_solve permutes with it)
            CSX_TRY(upload(F->perm_p, pinv, (size_t)n));
            F->pinv = F->perm_p;
        }
        CSX_TRY(chol_entry_map(A, F->pinv, fp, fi, F->lnz, F->win, F->flags));
        if (ns) {   // Lp: the interior columns of the full pattern, then one unit diagonal entry per kept column
            lp.resize((size_t)n + 1);
            tail.resize((size_t)ns);
            for (int32_t j = 0; j <= n; j++) lp[(size_t)j] = j <= n1 ? cp[j] : F->head + (j - n1);
            for (int32_t t = 0; t < ns; t++) tail[(size_t)t] = n1 + t;
            CSX_TRY(dalloc(&L->p, (size_t)n + 1));
            CSX_TRY(dalloc(&L->i, (size_t)lpnz));
            CSX_HIP(hipMemcpyAsync(L->p, lp.data(), ((size_t)n + 1) * sizeof(int32_t), hipMemcpyHostToDevice, s));
            if (F->head) CSX_HIP(hipMemcpyAsync(L->i, fi, (size_t)F->head * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
            CSX_HIP(hipMemcpyAsync(L->i + F->head, tail.data(), (size_t)ns * sizeof(int32_t), hipMemcpyHostToDevice, s));
            CSX_HIP(hipMemcpyAsync(L->x + F->head, ones.data(), (size_t)ns * sizeof(double), hipMemcpyHostToDevice, s));
        }
        int bad = 0;
        CSX_HIP(hipMemcpyAsync(&bad, F->flags.get(), sizeof(int), hipMemcpyDeviceToHost, s));
        CSX_HIP(hipStreamSynchronize(s));   // (every host list above has landed too)
        if (bad) {
            set_error("%s_factor: an upper entry of A has no slot in L (S is not A's)", who);
            return CSX_EINVAL;
        }
    }
    CSX_TRY(F->Lx.alloc((size_t)F->lnz));
    CSX_TRY(F->dd.alloc((size_t)n1));
    CSX_TRY(F->Sx.alloc((size_t)ns * (size_t)ns));
    std::unique_ptr<Vec> dv(new Vec()), Sv(new Vec());
    dv->len = n1;
    CSX_TRY(dmalloc(&dv->d, (size_t)n1 * sizeof(double)));
    Sv->len = (int64_t)ns * ns;
    CSX_TRY(dmalloc(&Sv->d, (size_t)ns * (size_t)ns * sizeof(double)));
    F->hL = put(K_CSC, L.release());
    F->hd = put(K_VEC, dv.release());
    F->hS = put(K_VEC, Sv.release());
    return CSX_OK;
}

int ldl_refactor(LdlFactor *F, csx_handle_t hA2, double tau, int *ok) {
    if (!F || !ok || !(tau >= 0.0)) return CSX_EINVAL;
    return walk_refactor(F, hA2, ok, [&](const double *x2) { return ldl_run(F, x2, tau, ok); });
}

int ldl_stats(const LdlFactor *F, double *out) {
    if (!F || !out) return CSX_EINVAL;
    out[0] = F->min_d;
    out[1] = F->max_d;
    out[2] = F->max_l;
    return CSX_OK;
}

}  // namespace csx

using namespace csx;

extern "C" int csx_ldl_factor(csx_handle_t hA, const int32_t *parent, const int32_t *cp, const int32_t *pinv, double tau,
                              csx_handle_t *out, int *ok) {
    CSX_TRY(require_ready());
    Csc *A = csc(hA);
    if (!A || !out || !ok || !A->x || A->m != A->n || !cp || (A->n > 0 && !parent) || !(tau >= 0.0)) return CSX_EINVAL;
    *out = 0;
    *ok = 0;
    std::unique_ptr<LdlFactor> F(new LdlFactor());
    CSX_TRY(ldl_build(A, parent, cp, pinv, A->n, WALK_RUN_UNCAPPED, "csx_ldl", F.get()));   // nothing kept
    CSX_TRY(ldl_run(F.get(), A->x, tau, ok));
    if (*ok) *out = put(K_LDLFACTOR, F.release());
    return CSX_OK;
}

extern "C" int csx_ldl_refactor(csx_handle_t h, csx_handle_t hA2, double tau, int *ok) {
    CSX_TRY(require_ready());
    return ldl_refactor((LdlFactor *)get(h, K_LDLFACTOR), hA2, tau, ok);
}

extern "C" int csx_ldl_parts(csx_handle_t h, csx_handle_t *L, csx_handle_t *d) {
    CSX_TRY(require_ready());
    LdlFactor *F = (LdlFactor *)get(h, K_LDLFACTOR);
    if (!F || !L || !d) return CSX_EINVAL;
    *L = F->hL;
    *d = F->hd;
    return CSX_OK;
}

extern "C" int csx_ldl_info(csx_handle_t h, int64_t *info) {
    CSX_TRY(require_ready());
    LdlFactor *F = (LdlFactor *)get(h, K_LDLFACTOR);
    if (!F || !info) return CSX_EINVAL;
    info[0] = F->n;
    info[1] = F->lnz;
    info[2] = F->levels();
    info[3] = F->launches();
    info[4] = F->pos;
    info[5] = F->neg;
    info[6] = F->perturbed;
    info[7] = F->breakdown;
    info[8] = F->kernel_us;
    info[9] = F->level_launches;
    info[10] = F->run_launches;
    info[11] = F->long_cols;
    info[12] = LDL_ACC;
    return CSX_OK;
}

extern "C" int csx_ldl_window(int32_t *entries) {   // (no device needed)
    if (!entries) return CSX_EINVAL;
    *entries = LDL_ACC;
    return CSX_OK;
}

extern "C" int csx_level_schedule(int32_t nlev, const int32_t *level_ptr, int32_t waves, int32_t run_levels, const int64_t *work,
                                  int64_t run_work, int32_t *launches, int32_t *count) {   // (no device needed)
    if (nlev < 0 || !level_ptr || waves < 1 || run_levels < 1 || !count || (nlev > 0 && !launches)) return CSX_EINVAL;
    for (int32_t l = 0; l < nlev; l++)
        if (level_ptr[l + 1] < level_ptr[l]) return CSX_EINVAL;
    const std::vector<LevelLaunch> S = level_schedule(level_ptr, nlev, waves, run_levels, work, run_work);
    for (size_t t = 0; t < S.size(); t++) {
        launches[3 * t] = S[t].wide ? 1 : 0;
        launches[3 * t + 1] = S[t].l0;
        launches[3 * t + 2] = S[t].l1;
    }
    *count = (int32_t)S.size();
    return CSX_OK;
}

extern "C" int csx_row_view(int32_t n, const int32_t *p, const int32_t *i, int descending, int32_t *rp, int32_t *rc,
                            int32_t *rpos) {   // (no device needed)
    if (n < 0 || !p || !rp || p[0] != 0) return CSX_EINVAL;
    for (int32_t j = 0; j < n; j++)
        if (p[j + 1] < p[j]) return CSX_EINVAL;
    if (p[n] > 0 && (!i || !rc || !rpos)) return CSX_EINVAL;
    std::vector<int32_t> hp, hc, hpos;
    if (!row_view(n, p, i, descending != 0, hp, hc, hpos)) return CSX_EINVAL;
    std::copy(hp.begin(), hp.end(), rp);
    std::copy(hc.begin(), hc.end(), rc);
    std::copy(hpos.begin(), hpos.end(), rpos);
    return CSX_OK;
}

extern "C" int csx_ldl_stats(csx_handle_t h, double *out) {
    CSX_TRY(require_ready());
    return ldl_stats((const LdlFactor *)get(h, K_LDLFACTOR), out);
}

extern "C" int csx_block_div_rows(csx_handle_t hX, csx_handle_t hd, int64_t rows, int32_t nrhs) {
    CSX_TRY(require_ready());
    Vec *X = vec(hX), *d = vec(hd);
    if (!X || !d || rows < 0 || nrhs < 1 || d->len < rows || X->len / nrhs < rows) return CSX_EINVAL;
    const int64_t total = rows * nrhs;
    if (total == 0) return CSX_OK;
    const bool pair = nrhs % 2 == 0 && ((uintptr_t)X->d & 15) == 0;
    const int64_t items = pair ? total / 2 : total;
    const int64_t most = (int64_t)std::max(ctx().cus, 1) * 16;
    const unsigned blocks = (unsigned)std::min<int64_t>((items + 255) / 256, most);
    if (pair) hipLaunchKernelGGL(k_block_div_rows<true>, dim3(blocks), dim3(256), 0, ctx().stream, (double *)X->d, (const double *)d->d, rows, nrhs);
    else hipLaunchKernelGGL(k_block_div_rows<false>, dim3(blocks), dim3(256), 0, ctx().stream, (double *)X->d, (const double *)d->d, rows, nrhs);
    CSX_LAUNCH_CHECK();
    return CSX_OK;
}
