// The one partial-LDL' factor object with its build, run and refactor (csx_ldl.hip), on which csx_ldl_factor (n1 = n: nothing
// kept) and csx_schur_factor (csx_schur.hip) both stand.  The level walk under it is csx_levelwalk.h's.  With it what csx_ldl.hip
// (one factorisation) and csx_ldl_batch.hip (many value sets on one analysis) share: the column function with its
// level-walk policy and one column of the statistics.
#pragma once
#include "csx_colupdate.h"
#include "csx_levelwalk.h"

#pragma clang fp contract(off)

namespace csx {

constexpr int LDL_ACC = 512;    // column entries kept in LDS per wave (24 KB a workgroup); longer columns are updated in place in global memory

// ---- one column -----------------------------------------------------------------------------------------------------------------
// Column j of L and d[j].  On entry Lx[Lp[j] ..] holds C(:, j) in the slots of L (0.0 in fill slots), and every column k < j
// with L(j,k) in the pattern is finished (L(:,k) and d[k] final).  acc_v / acc_r: wave-private LDS (LDL_ACC entries).
// flags[0]: the smallest broken column (atomicMin), flags[1]: perturbed pivots, flags[2]: columns that took the in-place path
// (integer atomicAdd both).
__device__ __forceinline__ void ldl_column(int32_t j, const int32_t *__restrict__ Lp, const int32_t *__restrict__ Li, double *Lx,
                                           double *d, const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ row_col,
                                           const int32_t *__restrict__ row_pos, double tau, double *acc_v, int32_t *acc_r,
                                           int lane, int *flags) {
    const int32_t base = Lp[j], len = Lp[j + 1] - base;
    const bool in_lds = len <= LDL_ACC;
    if (in_lds) {
        for (int32_t t = lane; t < len; t += 64) {
            acc_v[t] = Lx[base + t];
            acc_r[t] = Li[base + t];
        }
    }
    __builtin_amdgcn_wave_barrier();
    // the updates (csx_colupdate.h): weight L(j,k) d[k], one plane Lx, the sums in the LDS window or in place in Lx
    column_updates<1>(
        j, Lp, Li, row_ptr, row_col, row_pos, lane,
        [&](int32_t k, int32_t pos, double (&w)[1]) {
            w[0] = Lx[pos] * d[k];
            return true;
        },
        [&](int32_t p, double (&v)[1]) { v[0] = Lx[p]; },
        [&](int32_t row, const double (&a)[1]) {
            if (in_lds) {
                const int32_t t = find_row(acc_r, len, row);
                acc_v[t] = acc_v[t] - a[0];
            } else {
                const int32_t t = base + find_row(Li + base, len, row);
                Lx[t] = Lx[t] - a[0];
            }
        });
    double dj = in_lds ? acc_v[0] : Lx[base];
    const bool small = tau > 0.0 && fabs(dj) < tau;
    if (small) dj = copysign(tau, dj);
    if (lane == 0) {
        if (small) atomicAdd(flags + 1, 1);
        if (!in_lds) atomicAdd(flags + 2, 1);
        if (dj == 0.0 || !isfinite(dj)) atomicMin(flags, j);
        d[j] = dj;
    }
    __builtin_amdgcn_wave_barrier();
    for (int32_t t = lane; t < len; t += 64) {
        const double v = in_lds ? acc_v[t] : Lx[base + t];
        Lx[base + t] = t == 0 ? 1.0 : v / dj;
    }
    __builtin_amdgcn_wave_barrier();
}

// the level walk's policy (csx_levelwalk.h): ldl_column behind k_level / k_run, with the kernels' argument types and LDS arrays
struct LdlColumn {
    using Args = ColumnArgs<const int32_t *__restrict__, const int32_t *__restrict__, double *, double *, const int32_t *__restrict__,
                            const int32_t *__restrict__, const int32_t *__restrict__, double, int *>;
    static __device__ __forceinline__ void column(int32_t j, int w, int lane, const int32_t *Lp, const int32_t *Li, double *Lx,
                                                  double *d, const int32_t *row_ptr, const int32_t *row_col, const int32_t *row_pos,
                                                  double tau, int *flags) {
        __shared__ double acc_v[WALK_WAVES][LDL_ACC];
        __shared__ int32_t acc_r[WALK_WAVES][LDL_ACC];
        ldl_column(j, Lp, Li, Lx, d, row_ptr, row_col, row_pos, tau, acc_v[w], acc_r[w], lane, flags);
    }
};

// One wave's column of the statistics: st[0] positive pivots, st[1] negative pivots (integer adds), st[2] min |d|, st[3] max |d|,
// st[4] max |l| off the diagonal -- extrema of the bit patterns of fabs taken as unsigned integers (csx_residual.hip's rule: a NaN
// ranks above inf).  The body of k_ldl_stats (csx_ldl.hip), shared with csx_ldl_batch.hip's kernel per (column, member).
__device__ __forceinline__ void ldl_stats_column(int64_t j, int lane, const int32_t *__restrict__ Lp, const double *__restrict__ Lx,
                                                 const double *__restrict__ d, unsigned long long *st) {
    uint64_t lmax = 0;
    for (int32_t p = Lp[j] + 1 + lane; p < Lp[j + 1]; p += 64) {
        const uint64_t v = abs_bits(Lx[p]);
        lmax = v > lmax ? v : lmax;
    }
    for (int off = 1; off < 64; off <<= 1) {
        const uint64_t v = (uint64_t)__shfl_xor((unsigned long long)lmax, off);
        lmax = v > lmax ? v : lmax;
    }
    if (lane == 0) {
        const double dj = d[j];
        if (dj > 0.0) atomicAdd(st + 0, 1ull);
        if (dj < 0.0) atomicAdd(st + 1, 1ull);
        atomicMin(st + 2, (unsigned long long)abs_bits(dj));
        atomicMax(st + 3, (unsigned long long)abs_bits(dj));
        if (lmax) atomicMax(st + 4, (unsigned long long)lmax);
    }
}

// ---- the factor object ---------------------------------------------------------------------------------------------------------
// The partial LDL' of P A P' = Lp blockdiag(D1, S) Lp': the first n1 columns eliminated, the Schur complement S of the last
// ns = n - n1 left.  n1 == n is the LDL' factor itself: no trailing column, no chunk, an empty S, and Lp's pattern IS the full
// pattern.  Handles of both kinds (K_LDLFACTOR, K_SCHURFACTOR) own one of these.
struct LdlFactor : LevelFactor {            // (the levels are those of the first n1 columns)
    int32_t n1 = 0, ns = 0, lnz = 0, head = 0;   // lnz: entries of the full pattern of chol(P A P'); head = its p[n1]
    const int32_t *Lp = nullptr, *Li = nullptr;   // the full pattern the kernels read: the committed L's own p / i for ns == 0, ...
    DevBuf<int32_t> fp, fi;                 // ... these for ns > 0 (L then holds the interior columns and a unit tail)
    DevBuf<int32_t> rp, rc, rpos;           // row view of the full pattern (chol_symbolic_device)
    DevBuf<int32_t> win;                    // the entry map
    DevBuf<int32_t> perm_p;                 // a solve's permutation pinv on the device, only when the caller gave one (then the
    const int32_t *pinv = nullptr;          // ... pointer is set), for csx_ldl_batch_solve
    DevBuf<int32_t> arp, arc, apos;         // the row view of A's own pattern (p0 / i0) with its storage positions, made by the first
    bool a_rows = false;                    // ... csx_ldl_batch_norm1 (csx_ldl_batch.hip)
    DevBuf<int32_t> ch_col, ch_row0;        // csx_schur.hip: the (column, first row) pairs of the trailing-column kernel
    int64_t chunks = 0;
    csx_handle_t hL = 0, hd = 0, hS = 0;    // the committed Lp, d, S: owned here, lent out by csx_ldl_parts / csx_schur_parts
    DevBuf<double> Lx, dd, Sx;              // scratch of a run: committed only when none of the n1 columns broke down
    // flags: [1] perturbed pivots, [2] columns updated in place; stats: k_ldl_stats' five words
    // csx_ldl_info / csx_schur_info, csx_ldl_stats / csx_schur_stats
    int64_t schur_launches = 0, pos = 0, neg = 0, perturbed = 0;
    double min_d = 0.0, max_d = 0.0, max_l = 0.0;
    ~LdlFactor() {
        if (hL) (void)csx_free(hL);
        if (hd) (void)csx_free(hd);
        if (hS) (void)csx_free(hS);
    }
};

// csx_ldl.hip.  ldl_build: the analysis of A under the caller's S (host parent, cp, pinv) for the elimination of the first n1
// columns, the walker taking at most run_levels levels a launch, and the committed parts allocated.  ldl_run: the factor of the
// values Ax (A's storage order) into the scratch arrays, with the statistics of what was computed; Lp.x, d and S are committed
// when none of the n1 columns broke down.  *ok: 1 committed, 0 breakdown (nothing touched).  Synchronises.  ldl_refactor: ldl_run on the values of A2 after the pattern check
// (*ok = -1, CSX_EINVAL: not A's pattern or length); F null (a handle of another kind) is CSX_EINVAL with *ok untouched.
int ldl_build(Csc *A, const int32_t *parent, const int32_t *cp, const int32_t *pinv, int32_t n1, int32_t run_levels, const char *who,
              LdlFactor *F);
int ldl_run(LdlFactor *F, const double *Ax, double tau, int *ok);
int ldl_refactor(LdlFactor *F, csx_handle_t hA2, double tau, int *ok);
int ldl_stats(const LdlFactor *F, double *out);   // min |d|, max |d|, max |l| of the committed factor
// csx_schur.hip: k_schur_cols over F's chunks -- S into F->Sx from the finished first n1 columns in F->Lx / F->dd -- queued on
// the context's stream
void schur_launch_cols(const LdlFactor *F);

}  // namespace csx
