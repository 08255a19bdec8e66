// Partial LDL' with the Schur complement of a kept index set (the definition is the comment of csx_schur_factor
// in include/csx.h).  The permutation numbers the n1 interior indices first and the ns kept ones last; the symbolic analysis,
// the entry map and the scatter are csx_chol's on the FULL pattern Lf of chol(P A P'), whose row view is what the trailing
// columns need.  The first n1 columns are csx_ldl's own launches (ldl_launch_levels) over the height levels of the interior:
// a column's level depends on its children alone, so cutting the tree at n1 leaves those levels as they are.
//   k_schur_cols    the trailing columns, one wide level: one wave per (column j, chunk of at most LDL_ACC consecutive rows of
//                   j .. n - 1), the chunk's sums in wave-private LDS indexed by row - chunk start
//   k_schur_commit  Lp.x from the scratch L: the interior columns, then 1.0 for every trailing column
// Every sum is updated in ascending k by one wave, one update after the other: Lp.x, d and S are byte-equal to csx_schur_host.
// A factor or refactor runs into scratch arrays and is committed only when no interior column broke down.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "csx_internal.h"
#include "csx_ldl.h"

#pragma clang fp contract(off)

namespace csx {

constexpr int32_t SCHUR_RUN_LEVELS = 256;   // levels one launch of the walker takes (csx_slu.hip's SLU_RUN_LEVELS)

// Wave c takes rows [row0, min(row0 + LDL_ACC, n)) of column j = ch_col[c] of the permuted matrix, j >= n1.  Lx: the scratch
// values on the full pattern -- C in the slots of the trailing columns, the finished L in the interior ones; d: the interior
// pivots.  The row view of row j lists its columns k ascending and ends with the diagonal; the first k >= n1 ends the updates.
__global__ __launch_bounds__(64 * LDL_WAVES) void k_schur_cols(const int32_t *__restrict__ ch_col, const int32_t *__restrict__ ch_row0,
                                                              int64_t count, int32_t n, int32_t n1, const int32_t *__restrict__ Lp,
                                                              const int32_t *__restrict__ Li, const double *__restrict__ Lx,
                                                              const double *__restrict__ d, const int32_t *__restrict__ row_ptr,
                                                              const int32_t *__restrict__ row_col,
                                                              const int32_t *__restrict__ row_pos, double *__restrict__ S) {
    __shared__ double s_acc[LDL_WAVES][LDL_ACC];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t c = (int64_t)blockIdx.x * LDL_WAVES + w;
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
    const int32_t qe = row_ptr[j + 1] - 1;
    // Updates are applied in order, but fetched eight at a time (ldl_column): lane u reads the descriptor of update u --
    // position of L(j,k), end of column k, w = L(j,k) d[k] -- and the heads of the eight columns are requested together.
    constexpr int UQ = 8;
    for (int32_t q0 = row_ptr[j]; q0 < qe; q0 += UQ) {
        int32_t posq = 0, kendq = 0, kq = LDL_NONE;
        double wq = 0.0;
        if (lane < UQ && q0 + lane < qe) {
            kq = row_col[q0 + lane];
            if (kq < n1) {
                posq = row_pos[q0 + lane];
                kendq = Lp[kq + 1];
                wq = Lx[posq] * d[kq];
            }
        }
        if (__builtin_amdgcn_readlane(kq, 0) >= n1) break;       // k ascending: nothing but trailing columns from here on
        int32_t pos_[UQ], kend_[UQ], r_[UQ];
        double w_[UQ], v_[UQ];
#pragma unroll
        for (int u = 0; u < UQ; u++) {
            pos_[u] = __builtin_amdgcn_readlane(posq, u);
            kend_[u] = __builtin_amdgcn_readlane(kendq, u);      // 0 for an absent update or a trailing column: nothing below
            w_[u] = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(wq), u),
                                     __builtin_amdgcn_readlane(__double2loint(wq), u));
        }
#pragma unroll
        for (int u = 0; u < UQ; u++) {
            const int32_t p = pos_[u] + lane;
            const int32_t pp = p < kend_[u] ? p : pos_[u];        // a valid address either way
            r_[u] = Li[pp];
            v_[u] = Lx[pp];
        }
#pragma unroll
        for (int u = 0; u < UQ; u++) {
            if (pos_[u] + lane < kend_[u] && r_[u] >= r0 && r_[u] < r1) {
                const double v = v_[u] * w_[u];
                acc[r_[u] - r0] = acc[r_[u] - r0] - v;
            }
            for (int32_t p = pos_[u] + 64 + lane; p < kend_[u]; p += 64) {   // columns longer than one wave
                const int32_t r = Li[p];
                if (r >= r0 && r < r1) {
                    const double v = Lx[p] * w_[u];
                    acc[r - r0] = acc[r - r0] - v;
                }
            }
            __builtin_amdgcn_wave_barrier();   // one update after the other: they may hit the same rows
        }
    }
    __builtin_amdgcn_wave_barrier();
    const int64_t ns = n - n1, cj = j - n1;
    for (int32_t t = lane; t < rows; t += 64) {
        const int64_t cr = r0 + t - n1;
        const double v = acc[t];
        S[cr * ns + cj] = v;
        S[cj * ns + cr] = v;
    }
}

__global__ __launch_bounds__(256) void k_schur_commit(int64_t total, int64_t head, const double *__restrict__ Lx, double *__restrict__ out) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q < total) out[q] = q < head ? Lx[q] : 1.0;
}

struct SchurFactor {
    int32_t n = 0, n1 = 0, ns = 0, anz = 0, lnz = 0, head = 0;   // lnz: entries of the full pattern; head = Lf.p[n1]
    DevBuf<int32_t> p0, i0;                 // A's pattern: every A2 of a refactor is checked against it
    DevBuf<int32_t> fp, fi;                 // the full pattern Lf
    DevBuf<int32_t> rp, rc, rpos;           // its row view (chol_symbolic_device)
    DevBuf<int32_t> win;                    // the entry map
    DevBuf<int32_t> level_cols, level_ptr;  // height levels of the interior columns
    std::vector<int32_t> level_ptr_h;
    DevBuf<int32_t> ch_col, ch_row0;        // the (column, first row) pairs of k_schur_cols
    int64_t chunks = 0;
    csx_handle_t hL = 0, hd = 0, hS = 0;    // the committed Lp, d, S: owned here, lent out by csx_schur_parts
    DevBuf<double> Lx, dd, Sx;              // scratch of a run: committed only when no interior column broke down
    DevBuf<int> flags;                      // ldl_column's
    DevBuf<unsigned long long> stats;       // k_ldl_stats
    hipEvent_t ev_a = nullptr, ev_b = nullptr;
    int64_t level_launches = 0, run_launches = 0, schur_launches = 0, long_cols = 0;
    int64_t pos = 0, neg = 0, perturbed = 0, breakdown = -1, kernel_us = 0;
    double min_d = 0.0, max_d = 0.0, max_l = 0.0;
    SchurFactor() = default;
    SchurFactor(const SchurFactor &) = delete;
    SchurFactor &operator=(const SchurFactor &) = delete;
    ~SchurFactor() {
        if (hL) (void)csx_free(hL);
        if (hd) (void)csx_free(hd);
        if (hS) (void)csx_free(hS);
        if (ev_a) (void)hipEventDestroy(ev_a);
        if (ev_b) (void)hipEventDestroy(ev_b);
    }
};

void destroy(SchurFactor *F) { delete F; }

// The partial factor of the values Ax (A's storage order) into the scratch arrays; commits Lp.x, d and S when no interior column
// broke down.  *ok: 1 committed, 0 breakdown (nothing touched).  Synchronises.
static int schur_run(SchurFactor *F, const double *Ax, double tau, int *ok) {
    hipStream_t s = ctx().stream;
    Csc *L = csc(F->hL);
    Vec *dv = vec(F->hd), *Sv = vec(F->hS);
    const int64_t ns = F->ns, lpnz = (int64_t)F->head + ns;
    if (!L || !dv || !Sv || !L->x || L->nnz != lpnz || dv->len != F->n1 || Sv->len != ns * ns) return CSX_EINVAL;
    const int32_t n = F->n, n1 = F->n1;
    F->level_launches = F->run_launches = F->schur_launches = 0;
    const int hinit[3] = {LDL_NONE, 0, 0};
    const unsigned long long sinit[5] = {0ull, 0ull, ~0ull, 0ull, 0ull};
    CSX_HIP(hipMemcpyAsync(F->flags, hinit, sizeof hinit, hipMemcpyHostToDevice, s));
    CSX_HIP(hipMemcpyAsync(F->stats, sinit, sizeof sinit, hipMemcpyHostToDevice, s));
    CSX_HIP(hipEventRecord(F->ev_a, s));
    CSX_TRY(chol_scatter(F->lnz, F->win, Ax, F->Lx));
    ldl_launch_levels(F->level_ptr_h, F->level_cols.get(), F->level_ptr.get(), F->fp.get(), F->fi.get(), F->Lx.get(), F->dd.get(),
                      F->rp.get(), F->rc.get(), F->rpos.get(), tau, F->flags.get(), SCHUR_RUN_LEVELS, &F->level_launches,
                      &F->run_launches);
    if (F->chunks > 0) {
        hipLaunchKernelGGL(k_schur_cols, dim3((unsigned)((F->chunks + LDL_WAVES - 1) / LDL_WAVES)), dim3(64 * LDL_WAVES), 0, s,
                           F->ch_col.get(), F->ch_row0.get(), F->chunks, n, n1, F->fp.get(), F->fi.get(), F->Lx.get(), F->dd.get(),
                           F->rp.get(), F->rc.get(), F->rpos.get(), F->Sx.get());
        F->schur_launches = 1;
    }
    ldl_launch_stats(n1, F->fp.get(), F->Lx.get(), F->dd.get(), F->stats.get());
    (void)hipEventRecord(F->ev_b, s);
    int hflags[3] = {LDL_NONE, 0, 0};
    unsigned long long hst[5] = {0, 0, 0, 0, 0};
    if (hipGetLastError() != hipSuccess || hipMemcpyAsync(hflags, F->flags.get(), sizeof hflags, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipMemcpyAsync(hst, F->stats.get(), sizeof hst, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess) {
        set_error("csx_schur: %s", hipGetErrorString(hipGetLastError()));
        (void)hipStreamSynchronize(s);
        return CSX_ERUNTIME;
    }
    float ms = 0.0f;
    F->kernel_us = hipEventElapsedTime(&ms, F->ev_a, F->ev_b) == hipSuccess ? (int64_t)(1e3 * ms) : 0;
    F->perturbed = hflags[1];
    F->long_cols = hflags[2];
    F->breakdown = hflags[0] == LDL_NONE ? -1 : hflags[0];
    *ok = F->breakdown < 0 ? 1 : 0;
    if (!*ok) return CSX_OK;
    F->pos = (int64_t)hst[0];
    F->neg = (int64_t)hst[1];
    if (n1 == 0) hst[2] = 0;
    std::memcpy(&F->min_d, &hst[2], 8);
    std::memcpy(&F->max_d, &hst[3], 8);
    std::memcpy(&F->max_l, &hst[4], 8);
    if (lpnz) {
        hipLaunchKernelGGL(k_schur_commit, dim3((unsigned)((lpnz + 255) / 256)), dim3(256), 0, s, lpnz, (int64_t)F->head,
                           (const double *)F->Lx.get(), L->x);
        CSX_LAUNCH_CHECK();
    }
    if (n1) CSX_HIP(hipMemcpyAsync(dv->d, F->dd.get(), (size_t)n1 * sizeof(double), hipMemcpyDeviceToDevice, s));
    if (ns) CSX_HIP(hipMemcpyAsync(Sv->d, F->Sx.get(), (size_t)(ns * ns) * sizeof(double), hipMemcpyDeviceToDevice, s));
    L->rows.reset();    // (copies of the old values)
    L->tiled.reset();
    CSX_HIP(hipStreamSynchronize(s));
    return CSX_OK;
}

static int schur_build(Csc *A, const int32_t *parent, const int32_t *cp, const int32_t *pinv, int32_t n1, SchurFactor *F) {
    hipStream_t s = ctx().stream;
    const int32_t n = A->n, ns = n - n1;
    F->n = n;
    F->n1 = n1;
    F->ns = ns;
    F->anz = A->nnz;
    F->lnz = cp[n];
    if (cp[0] != 0 || F->lnz < n) return CSX_EINVAL;
    for (int32_t j = 0; j < n; j++)
        if (cp[j + 1] <= cp[j]) return CSX_EINVAL;
    F->head = cp[n1];
    if (!A->trusted) CSX_TRY(csc_validate(A));
    CSX_TRY(rf_keep_pattern(A, F->p0, F->i0));
    CSX_TRY(F->flags.alloc(3));
    CSX_TRY(F->stats.alloc(5));
    CSX_HIP(hipEventCreate(&F->ev_a));
    CSX_HIP(hipEventCreate(&F->ev_b));
    const int64_t lpnz = (int64_t)F->head + ns;
    std::unique_ptr<Csc> L(new Csc());
    L->m = L->n = n;
    L->nnz = (int32_t)lpnz;
    std::vector<int32_t> ch_col, ch_row0;
    if (n == 0) {
        CSX_TRY(dalloc(&L->p, 1));
        CSX_HIP(hipMemsetAsync(L->p, 0, sizeof(int32_t), s));
        CSX_TRY(dalloc(&L->i, 0));
        F->level_ptr_h.assign(1, 0);
    } else {
        int32_t *fp = nullptr, *fi = nullptr;
        const int st = chol_symbolic_device(A, parent, cp, pinv, &fp, &fi, &F->rp, &F->rc, &F->rpos, nullptr);   // (checks S and pinv)
        F->fp = DevBuf<int32_t>(fp);
        F->fi = DevBuf<int32_t>(fi);
        CSX_TRY(st);
        // the height levels of the interior: the tree cut at n1 (a parent among the kept columns is no parent)
        std::vector<int32_t> cut((size_t)n1), cols;
        for (int32_t j = 0; j < n1; j++) cut[(size_t)j] = parent[j] < n1 ? parent[j] : -1;
        ldl_levels(n1, cut.data(), F->level_ptr_h, cols);
        CSX_TRY(upload(F->level_cols, cols));
        CSX_TRY(upload(F->level_ptr, F->level_ptr_h));
        for (int32_t j = n1; j < n; j++)
            for (int32_t r0 = j; r0 < n; r0 += LDL_ACC) {
                ch_col.push_back(j);
                ch_row0.push_back(r0);
            }
        F->chunks = (int64_t)ch_col.size();
        CSX_TRY(upload(F->ch_col, ch_col));
        CSX_TRY(upload(F->ch_row0, ch_row0));
        CSX_TRY(F->win.alloc((size_t)F->lnz));
        DevBuf<int32_t> d_pinv;
        if (pinv) CSX_TRY(upload(d_pinv, pinv, (size_t)n));
        CSX_TRY(chol_entry_map(A, pinv ? d_pinv.get() : nullptr, F->fp, F->fi, F->lnz, F->win, F->flags));
        // Lp: the interior columns of Lf, then one diagonal entry per kept column
        std::vector<int32_t> lp((size_t)n + 1), tail((size_t)ns);
        for (int32_t j = 0; j <= n; j++) lp[(size_t)j] = j <= n1 ? cp[j] : F->head + (j - n1);
        for (int32_t t = 0; t < ns; t++) tail[(size_t)t] = n1 + t;
        CSX_TRY(dalloc(&L->p, (size_t)n + 1));
        CSX_TRY(dalloc(&L->i, (size_t)lpnz));
        CSX_HIP(hipMemcpyAsync(L->p, lp.data(), ((size_t)n + 1) * sizeof(int32_t), hipMemcpyHostToDevice, s));
        if (F->head) CSX_HIP(hipMemcpyAsync(L->i, F->fi.get(), (size_t)F->head * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
        if (ns) CSX_HIP(hipMemcpyAsync(L->i + F->head, tail.data(), (size_t)ns * sizeof(int32_t), hipMemcpyHostToDevice, s));
        int bad = 0;
        CSX_HIP(hipMemcpyAsync(&bad, F->flags.get(), sizeof(int), hipMemcpyDeviceToHost, s));
        CSX_HIP(hipStreamSynchronize(s));   // (every host vector above has landed too)
        if (bad) {
            set_error("csx_schur_factor: an upper entry of A has no slot in L (S is not A's)");
            return CSX_EINVAL;
        }
    }
    CSX_TRY(dalloc(&L->x, (size_t)lpnz));
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
    std::unique_ptr<SchurFactor> F(new SchurFactor());
    CSX_TRY(schur_build(A, parent, cp, pinv, n1, F.get()));
    CSX_TRY(schur_run(F.get(), A->x, tau, ok));
    if (*ok) *out = put(K_SCHURFACTOR, F.release());
    return CSX_OK;
}

extern "C" int csx_schur_refactor(csx_handle_t h, csx_handle_t hA2, double tau, int *ok) {
    CSX_TRY(require_ready());
    SchurFactor *F = (SchurFactor *)get(h, K_SCHURFACTOR);
    if (!F || !ok || !(tau >= 0.0)) return CSX_EINVAL;
    *ok = -1;
    const double *x2 = nullptr;
    CSX_TRY(rf_values(hA2, F->n, F->n, F->anz, F->p0, F->i0, F->flags, &x2));
    if (!x2) {
        set_error("csx_schur_refactor: A2 does not have the pattern (or the length) of the factored matrix");
        return CSX_EINVAL;   // nothing changes
    }
    return schur_run(F, x2, tau, ok);
}

extern "C" int csx_schur_parts(csx_handle_t h, csx_handle_t *L, csx_handle_t *d, csx_handle_t *S) {
    CSX_TRY(require_ready());
    SchurFactor *F = (SchurFactor *)get(h, K_SCHURFACTOR);
    if (!F || !L || !d || !S) return CSX_EINVAL;
    *L = F->hL;
    *d = F->hd;
    *S = F->hS;
    return CSX_OK;
}

extern "C" int csx_schur_info(csx_handle_t h, int64_t *info) {
    CSX_TRY(require_ready());
    SchurFactor *F = (SchurFactor *)get(h, K_SCHURFACTOR);
    if (!F || !info) return CSX_EINVAL;
    info[0] = F->n;
    info[1] = F->n1;
    info[2] = F->ns;
    info[3] = (int64_t)F->head + F->ns;
    info[4] = (int64_t)F->level_ptr_h.size() - 1;
    info[5] = F->level_launches + F->run_launches + F->schur_launches;
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
    SchurFactor *F = (SchurFactor *)get(h, K_SCHURFACTOR);
    if (!F || !out) return CSX_EINVAL;
    out[0] = F->min_d;
    out[1] = F->max_d;
    out[2] = F->max_l;
    return CSX_OK;
}
