// L U with static pivots for general unsymmetric matrices in one connected piece (the definition is the comment
// of csx_slu_factor in include/csx.h).  L U = C = P A(prow, :) P' on the Cholesky pattern of the pattern of A1 + A1', A1 =
// A(prow, :): a matching has put a zero-free diagonal in place, the symmetric order is the caller's, and there is no pivot
// search, so the pattern is known before the values are.  L (unit lower, the 1.0 stored) and Ut (column k = row k of U, the pivot
// first) are two value arrays on that one pattern; the numeric kernel is ldl_column (csx_ldl.hip) with a second accumulator.
//   k_slu_sym_rows / k_slu_sym_ptr / k_slu_sym_fill   the pattern whose upper triangle is that of A1 + A1', for the symbolic step
//   k_slu_entry_map   slot of L and slot of Ut of every entry of A (of duplicates the last)
//   slu_column    one wave's column, behind the policy SluColumn of the level walk (csx_slu.h; csx_levelwalk.h: k_level, k_run,
//                 the schedule with the walker cut at WALK_RUN_LEVELS levels a launch)
//   k_slu_stats   min / max |d|, max |l|, max |u| off the diagonal, pivot signs in one pass
// Every sum is updated in ascending k by one wave, one update after the other: L.x and Ut.x are byte-equal to csx_slu_host.
// A factor or refactor runs into scratch arrays and is committed only when no column broke down.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "csx_internal.h"
#include "csx_slu.h"

#pragma clang fp contract(off)

namespace csx {

// ---- analysis ------------------------------------------------------------------------------------------------------------------

// rows of A1 = A(prow, :): row i of A is row prinv[i] of A1; the entry order inside a column stays, so A's values are A1's
__global__ __launch_bounds__(256) void k_slu_sym_rows(int64_t nnz, const int32_t *__restrict__ Ai, const int32_t *__restrict__ prinv,
                                                      int32_t *__restrict__ out) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q < nnz) out[q] = prinv[Ai[q]];
}

__global__ __launch_bounds__(256) void k_slu_sym_ptr(int32_t n, const int32_t *__restrict__ Ap, const int32_t *__restrict__ Tp,
                                                     int32_t *__restrict__ Mp) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c <= n) Mp[c] = Ap[c] + Tp[c];
}

// column c of M = column c of A1, then column c of A1': its entries above the diagonal are those of A1 + A1' (the symbolic step
// reads nothing else; duplicates start no second walk)
__global__ __launch_bounds__(256) void k_slu_sym_fill(int32_t n, const int32_t *__restrict__ Ap, const int32_t *__restrict__ Ai,
                                                      const int32_t *__restrict__ Tp, const int32_t *__restrict__ Ti,
                                                      int32_t *__restrict__ Mi) {
    const int lane = threadIdx.x & 63;
    const int64_t c = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (c >= n) return;
    const int32_t a = Ap[c], la = Ap[c + 1] - a, b = Tp[c], lb = Tp[c + 1] - b;
    int32_t *out = Mi + a + b;
    for (int32_t t = lane; t < la; t += 64) out[t] = Ai[a + t];
    for (int32_t t = lane; t < lb; t += 64) out[la + t] = Ti[b + t];
}

// Entry q of A at (i, j) is C(i2, j2), i2 = pinv[prinv[i]], j2 = pinv[j]: on or below the diagonal it is the start of L(i2, j2),
// on or above it the start of U(i2, j2) = Ut(j2, i2).  Of duplicates the last wins (cs_lu's scatter, k_chol_winner).
__global__ __launch_bounds__(256) void k_slu_entry_map(int32_t n, const int32_t *__restrict__ Ap, const int32_t *__restrict__ Ai,
                                                       const int32_t *__restrict__ prinv, const int32_t *__restrict__ pinv,
                                                       const int32_t *__restrict__ Lp, const int32_t *__restrict__ Li,
                                                       int32_t *winL, int32_t *winU, int *bad) {
    const int lane = threadIdx.x & 63;
    const int64_t j = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (j >= n) return;
    const int32_t j2 = pinv ? pinv[j] : (int32_t)j;
    for (int32_t p = Ap[j] + lane; p < Ap[j + 1]; p += 64) {
        const int32_t i1 = prinv ? prinv[Ai[p]] : Ai[p];
        const int32_t i2 = pinv ? pinv[i1] : i1;
        const int32_t c = min(i2, j2), r = max(i2, j2);
        const int32_t b = Lp[c], len = Lp[c + 1] - b;
        const int32_t t = find_row(Li + b, len, r);
        if (Li[b + t] != r) {
            *bad = 1;   // the symbolic pattern does not contain this entry
            continue;
        }
        if (i2 >= j2) atomicMax(&winL[b + t], p);
        if (i2 <= j2) atomicMax(&winU[b + t], p);
    }
}

// slu_column, its policy SluColumn and the factor object: csx_slu.h (shared with csx_slu_batch.hip)

// one wave per column (slu_stats_column)
__global__ __launch_bounds__(256) void k_slu_stats(int32_t n, const int32_t *__restrict__ Lp, const double *__restrict__ Lx,
                                                   const double *__restrict__ Ux, unsigned long long *st) {
    const int lane = threadIdx.x & 63;
    const int64_t j = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (j >= n) return;
    slu_stats_column((int32_t)j, lane, Lp, Lx, Ux, st);
}

void destroy(SluFactor *F) { delete F; }

static inline unsigned slu_blocks(int64_t items) { return (unsigned)((items + 255) / 256); }

// The factor of the values Ax (A's storage order) into the scratch arrays, with the statistics of what was computed; commits
// into L.x / Ut.x when no column broke down.  *ok: 1 committed, 0 breakdown (L, Ut untouched).  Synchronises.
static int slu_run(SluFactor *F, const double *Ax, double tau, int *ok) {
    hipStream_t s = ctx().stream;
    Csc *L = csc(F->hL), *U = csc(F->hU);
    if (!L || !U || !L->x || !U->x || L->nnz != F->lnz || U->nnz != F->lnz) return CSX_EINVAL;
    const int32_t n = F->n;
    const int hinit[3] = {WALK_NONE, 0, 0};
    const unsigned long long sinit[6] = {0ull, 0ull, ~0ull, 0ull, 0ull, 0ull};
    CSX_TRY(walk_begin(F, hinit, 3, sinit, 6));
    CSX_TRY(chol_scatter(F->lnz, F->winL, Ax, F->Lx));
    CSX_TRY(chol_scatter(F->lnz, F->winU, Ax, F->Ux));
    walk_levels<SluColumn>(F, SluColumn::Args(), L->p, L->i, F->Lx, F->Ux, F->rp, F->rc, F->rpos, tau, F->flags);
    if (n > 0)
        hipLaunchKernelGGL(k_slu_stats, dim3((unsigned)(((int64_t)n + 3) / 4)), dim3(256), 0, s, n, L->p, F->Lx.get(), F->Ux.get(),
                           F->stats.get());
    int hflags[3] = {WALK_NONE, 0, 0};
    unsigned long long hst[6] = {0, 0, 0, 0, 0, 0};
    CSX_TRY(walk_end(F, hflags, 3, hst, 6, ok));
    F->perturbed = hflags[1];
    F->long_cols = hflags[2];
    if (!*ok) return CSX_OK;
    F->pos = (int64_t)hst[0];
    F->neg = (int64_t)hst[1];
    if (n == 0) hst[2] = 0;
    std::memcpy(&F->min_d, &hst[2], 8);
    std::memcpy(&F->max_d, &hst[3], 8);
    std::memcpy(&F->max_l, &hst[4], 8);
    std::memcpy(&F->max_u, &hst[5], 8);
    if (F->lnz) {
        CSX_HIP(hipMemcpyAsync(L->x, F->Lx.get(), (size_t)F->lnz * sizeof(double), hipMemcpyDeviceToDevice, s));
        CSX_HIP(hipMemcpyAsync(U->x, F->Ux.get(), (size_t)F->lnz * sizeof(double), hipMemcpyDeviceToDevice, s));
    }
    for (Csc *M : {L, U}) {   // (copies of the old values)
        M->rows.reset();
        M->tiled.reset();
    }
    CSX_HIP(hipStreamSynchronize(s));
    return CSX_OK;
}

// M (pattern only): column c = column c of A1 followed by column c of A1', A1 = A(prow, :); a1i: A1's row indices (A's when
// prinv is null)
static int slu_symmetrised(const Csc *A, const int32_t *prinv, DevBuf<int32_t> &a1i, Csc *M) {
    hipStream_t s = ctx().stream;
    const int32_t n = A->n, anz = A->nnz;
    const int32_t *rows = A->i;
    if (prinv) {
        CSX_TRY(a1i.alloc((size_t)anz));
        if (anz) hipLaunchKernelGGL(k_slu_sym_rows, dim3(slu_blocks(anz)), dim3(256), 0, s, (int64_t)anz, A->i, prinv, a1i.get());
        CSX_LAUNCH_CHECK();
        rows = a1i.get();
    }
    Csc A1, T;
    A1.owns = false;
    A1.m = A1.n = n;
    A1.nnz = anz;
    A1.p = A->p;
    A1.i = const_cast<int32_t *>(rows);
    CSX_TRY(transpose_device(&A1, false, &T));
    M->m = M->n = n;
    M->nnz = 2 * anz;
    CSX_TRY(dalloc(&M->p, (size_t)n + 1));
    CSX_TRY(dalloc(&M->i, (size_t)M->nnz));
    hipLaunchKernelGGL(k_slu_sym_ptr, dim3(slu_blocks((int64_t)n + 1)), dim3(256), 0, s, n, A->p, T.p, M->p);
    hipLaunchKernelGGL(k_slu_sym_fill, dim3((unsigned)(((int64_t)n + 3) / 4)), dim3(256), 0, s, n, A->p, rows, T.p, T.i, M->i);
    CSX_LAUNCH_CHECK();
    CSX_HIP(hipStreamSynchronize(s));   // T goes out of scope
    return CSX_OK;
}

static int slu_build(Csc *A, const int32_t *parent, const int32_t *cp, const int32_t *prow, const int32_t *pinv, SluFactor *F) {
    hipStream_t s = ctx().stream;
    const int32_t n = A->n;
    F->lnz = cp[n];
    if (cp[0] != 0 || F->lnz < n || A->nnz > 0x3fffffff) return CSX_EINVAL;
    std::vector<int32_t> prinv;
    if (prow) {   // must be a permutation of 0..n-1
        prinv.assign((size_t)n, -1);
        for (int32_t k = 0; k < n; k++) {
            if (prow[k] < 0 || prow[k] >= n || prinv[(size_t)prow[k]] >= 0) {
                set_error("csx_slu_factor: prow is not a permutation");
                return CSX_EINVAL;
            }
            prinv[(size_t)prow[k]] = k;
        }
    }
    if (!A->trusted) CSX_TRY(csc_validate(A));
    CSX_TRY(walk_init(F, A, "csx_slu", 3, 6));
    std::unique_ptr<Csc> L(new Csc());
    L->m = L->n = n;
    L->nnz = F->lnz;
    if (n == 0) {
        CSX_TRY(dalloc(&L->p, 1));
        CSX_HIP(hipMemsetAsync(L->p, 0, sizeof(int32_t), s));
        CSX_TRY(dalloc(&L->i, 0));
        F->level_ptr_h.assign(1, 0);
    } else {
        DevBuf<int32_t> d_prinv, a1i;
        DevBuf<int32_t> &d_pinv = F->perm_p;
        std::vector<int32_t> comb;   // (alive until the synchronisation below)
        if (prow) {
            CSX_TRY(upload(d_prinv, prinv));
            comb.resize((size_t)n);
            for (int32_t k = 0; k < n; k++) comb[(size_t)k] = pinv ? pinv[prinv[(size_t)k]] : prinv[(size_t)k];
            CSX_TRY(upload(F->perm_c, comb));
        }
        Csc M;
        CSX_TRY(slu_symmetrised(A, prow ? d_prinv.get() : nullptr, a1i, &M));
        CSX_TRY(chol_symbolic_device(&M, parent, cp, pinv, &L->p, &L->i, &F->rp, &F->rc, &F->rpos, nullptr));   // (checks S and pinv)
        std::vector<int32_t> cols;
        height_levels(n, parent, F->level_ptr_h, cols);
        CSX_TRY(walk_set_levels(F, cols, WALK_RUN_LEVELS));
        CSX_TRY(F->winL.alloc((size_t)F->lnz));
        CSX_TRY(F->winU.alloc((size_t)F->lnz));
        if (pinv) CSX_TRY(upload(d_pinv, pinv, (size_t)n));
        CSX_HIP(hipMemsetAsync(F->winL, 0xff, (size_t)F->lnz * sizeof(int32_t), s));
        CSX_HIP(hipMemsetAsync(F->winU, 0xff, (size_t)F->lnz * sizeof(int32_t), s));
        CSX_HIP(hipMemsetAsync(F->flags, 0, sizeof(int), s));
        hipLaunchKernelGGL(k_slu_entry_map, dim3((unsigned)(((int64_t)n + 3) / 4)), dim3(256), 0, s, n, A->p, A->i,
                           prow ? d_prinv.get() : nullptr, pinv ? d_pinv.get() : nullptr, L->p, L->i, F->winL.get(), F->winU.get(),
                           F->flags.get());
        CSX_LAUNCH_CHECK();
        int bad = 0;
        CSX_HIP(hipMemcpyAsync(&bad, F->flags.get(), sizeof(int), hipMemcpyDeviceToHost, s));
        CSX_HIP(hipStreamSynchronize(s));   // (cols, level_ptr_h and the permutations have landed too)
        if (bad) {
            set_error("csx_slu_factor: an entry of A has no slot in the pattern (S is not A's)");
            return CSX_EINVAL;
        }
        F->pinv = pinv ? F->perm_p.get() : nullptr;
        F->comb = prow ? F->perm_c.get() : F->pinv;
    }
    CSX_TRY(dalloc(&L->x, (size_t)F->lnz));
    CSX_TRY(F->utx.alloc((size_t)F->lnz));
    CSX_TRY(F->Lx.alloc((size_t)F->lnz));
    CSX_TRY(F->Ux.alloc((size_t)F->lnz));
    std::unique_ptr<Csc> U(new Csc());
    U->owns = false;   // L's pattern, the factor's values
    U->m = U->n = n;
    U->nnz = F->lnz;
    U->p = L->p;
    U->i = L->i;
    U->x = F->utx.get();
    F->hL = put(K_CSC, L.release());
    F->hU = put(K_CSC, U.release());
    return CSX_OK;
}

}  // namespace csx

using namespace csx;

extern "C" int csx_slu_factor(csx_handle_t hA, const int32_t *parent, const int32_t *cp, const int32_t *prow, const int32_t *pinv,
                              double tau, csx_handle_t *out, int *ok) {
    CSX_TRY(require_ready());
    Csc *A = csc(hA);
    if (!A || !out || !ok || !A->x || A->m != A->n || !cp || (A->n > 0 && !parent) || !(tau >= 0.0)) return CSX_EINVAL;
    *out = 0;
    *ok = 0;
    std::unique_ptr<SluFactor> F(new SluFactor());
    CSX_TRY(slu_build(A, parent, cp, prow, pinv, F.get()));
    CSX_TRY(slu_run(F.get(), A->x, tau, ok));
    if (*ok) *out = put(K_SLUFACTOR, F.release());
    return CSX_OK;
}

extern "C" int csx_slu_refactor(csx_handle_t h, csx_handle_t hA2, double tau, int *ok) {
    CSX_TRY(require_ready());
    SluFactor *F = (SluFactor *)get(h, K_SLUFACTOR);
    if (!F || !ok || !(tau >= 0.0)) return CSX_EINVAL;
    return walk_refactor(F, hA2, ok, [&](const double *x2) { return slu_run(F, x2, tau, ok); });
}

extern "C" int csx_slu_parts(csx_handle_t h, csx_handle_t *L, csx_handle_t *Ut) {
    CSX_TRY(require_ready());
    SluFactor *F = (SluFactor *)get(h, K_SLUFACTOR);
    if (!F || !L || !Ut) return CSX_EINVAL;
    *L = F->hL;
    *Ut = F->hU;
    return CSX_OK;
}

extern "C" int csx_slu_info(csx_handle_t h, int64_t *info) {
    CSX_TRY(require_ready());
    SluFactor *F = (SluFactor *)get(h, K_SLUFACTOR);
    if (!F || !info) return CSX_EINVAL;
    info[0] = F->n;
    info[1] = F->lnz;
    info[2] = F->levels();
    info[3] = F->launches();
    info[4] = F->level_launches;
    info[5] = F->run_launches;
    info[6] = F->perturbed;
    info[7] = F->breakdown;
    info[8] = F->kernel_us;
    info[9] = F->long_cols;
    info[10] = SLU_ACC;
    info[11] = WALK_RUN_LEVELS;
    info[12] = F->pos;
    info[13] = F->neg;
    return CSX_OK;
}

extern "C" int csx_slu_window(int32_t *entries, int32_t *run_levels) {   // (no device needed)
    if (!entries || !run_levels) return CSX_EINVAL;
    *entries = SLU_ACC;
    *run_levels = WALK_RUN_LEVELS;
    return CSX_OK;
}

extern "C" int csx_slu_stats(csx_handle_t h, double *out) {
    CSX_TRY(require_ready());
    SluFactor *F = (SluFactor *)get(h, K_SLUFACTOR);
    if (!F || !out) return CSX_EINVAL;
    out[0] = F->min_d;
    out[1] = F->max_d;
    out[2] = F->max_l;
    out[3] = F->max_u;
    return CSX_OK;
}
