// What csx_slu.hip (one factorisation) and csx_slu_batch.hip (many value sets on one analysis) share of the static-pivot L U
// (DESIGN.md §23, §32): the column function with its level-walk policy, one column of the statistics, and the factor object.
#pragma once
#include "csx_colupdate.h"
#include "csx_levelwalk.h"

#pragma clang fp contract(off)

namespace csx {

constexpr int SLU_ACC = 512;   // column entries kept in LDS per wave (8 + 8 + 4 bytes each: 40 KB a workgroup); longer columns are updated in place

// ---- one column -----------------------------------------------------------------------------------------------------------------
// Column j of L and of Ut.  On entry Lx[Lp[j] ..] holds C(:, j) and Ux[Lp[j] ..] holds C(j, :) in the slots of the pattern (0.0 in
// fill and one-sided slots), and every column k < j with (j,k) in the pattern is finished.  acc_l / acc_u / acc_r: wave-private
// LDS (SLU_ACC entries).  flags[0]: the smallest broken column (atomicMin), flags[1]: perturbed pivots, flags[2]: columns that
// took the in-place path (integer atomicAdd both).
__device__ __forceinline__ void slu_column(int32_t j, const int32_t *__restrict__ Lp, const int32_t *__restrict__ Li, double *Lx,
                                           double *Ux, const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ row_col,
                                           const int32_t *__restrict__ row_pos, double tau, double *acc_l, double *acc_u,
                                           int32_t *acc_r, int lane, int *flags) {
    const int32_t base = Lp[j], len = Lp[j + 1] - base;
    const bool in_lds = len <= SLU_ACC;
    if (in_lds) {
        for (int32_t t = lane; t < len; t += 64) {
            acc_l[t] = Lx[base + t];
            acc_u[t] = Ux[base + t];
            acc_r[t] = Li[base + t];
        }
    }
    __builtin_amdgcn_wave_barrier();
    // The window by its address space.  With two plain double * the captured acc_u and Ux are two loads of one shape from the
    // closure, the compiler merges the tails of the two branches of `sub` below into one subtraction through a pointer chosen
    // between LDS and global memory, and the second plane's sums go through flat loads and stores.  Pointers
    // of different address spaces cannot be merged.  This rests on how the compiler orders its passes: after a compiler
    // upgrade, compare the LU kernels' ds_* / flat_* counts with profiles/column_updates_isa.txt again.
    typedef __attribute__((address_space(3))) double lds_double;
    lds_double *const lds_l = (lds_double *)acc_l, *const lds_u = (lds_double *)acc_u;
    // the updates (csx_colupdate.h): weights Ut(j,k) for plane Lx and L(j,k) for plane Ux, sums in the window or in place, one search
    column_updates<2>(
        j, Lp, Li, row_ptr, row_col, row_pos, lane,
        [&](int32_t, int32_t pos, double (&w)[2]) {
            w[0] = Ux[pos];
            w[1] = Lx[pos];
            return true;
        },
        [&](int32_t p, double (&v)[2]) {
            v[0] = Lx[p];
            v[1] = Ux[p];
        },
        [&](int32_t row, const double (&a)[2]) {
            if (in_lds) {
                const int32_t t = find_row(acc_r, len, row);
                lds_l[t] = lds_l[t] - a[0];
                lds_u[t] = lds_u[t] - a[1];
            } else {
                const int32_t t = base + find_row(Li + base, len, row);
                Lx[t] = Lx[t] - a[0];
                Ux[t] = Ux[t] - a[1];
            }
        });
    double dj = in_lds ? acc_u[0] : Ux[base];
    const bool small = tau > 0.0 && fabs(dj) < tau;
    if (small) dj = copysign(tau, dj);
    if (lane == 0) {
        if (small) atomicAdd(flags + 1, 1);
        if (!in_lds) atomicAdd(flags + 2, 1);
        if (dj == 0.0 || !isfinite(dj)) atomicMin(flags, j);
    }
    __builtin_amdgcn_wave_barrier();
    for (int32_t t = lane; t < len; t += 64) {
        const double vl = in_lds ? acc_l[t] : Lx[base + t];
        const double vu = in_lds ? acc_u[t] : Ux[base + t];
        Lx[base + t] = t == 0 ? 1.0 : vl / dj;
        Ux[base + t] = t == 0 ? dj : vu;
    }
    __builtin_amdgcn_wave_barrier();
}

// the level walk's policy (csx_levelwalk.h): slu_column behind k_level / k_run, with the kernels' argument types and LDS arrays
struct SluColumn {
    using Args = ColumnArgs<const int32_t *__restrict__, const int32_t *__restrict__, double *, double *, const int32_t *__restrict__,
                            const int32_t *__restrict__, const int32_t *__restrict__, double, int *>;
    static __device__ __forceinline__ void column(int32_t j, int w, int lane, const int32_t *Lp, const int32_t *Li, double *Lx,
                                                  double *Ux, const int32_t *row_ptr, const int32_t *row_col,
                                                  const int32_t *row_pos, double tau, int *flags) {
        __shared__ double acc_l[WALK_WAVES][SLU_ACC];
        __shared__ double acc_u[WALK_WAVES][SLU_ACC];
        __shared__ int32_t acc_r[WALK_WAVES][SLU_ACC];
        slu_column(j, Lp, Li, Lx, Ux, row_ptr, row_col, row_pos, tau, acc_l[w], acc_u[w], acc_r[w], lane, flags);
    }
};

// One wave's column of the statistics: st[0] positive pivots, st[1] negative pivots (integer adds), st[2] min |d|, st[3] max |d|,
// st[4] max |l|, st[5] max |u| off the diagonal -- extrema of the bit patterns of fabs taken as unsigned integers (k_ldl_stats' rule)
__device__ __forceinline__ void slu_stats_column(int32_t j, int lane, const int32_t *__restrict__ Lp, const double *__restrict__ Lx,
                                                 const double *__restrict__ Ux, unsigned long long *st) {
    uint64_t lmax = 0, umax = 0;
    for (int32_t p = Lp[j] + 1 + lane; p < Lp[j + 1]; p += 64) {
        const uint64_t a = abs_bits(Lx[p]), b = abs_bits(Ux[p]);
        lmax = a > lmax ? a : lmax;
        umax = b > umax ? b : umax;
    }
    for (int off = 1; off < 64; off <<= 1) {
        const uint64_t a = (uint64_t)__shfl_xor((unsigned long long)lmax, off);
        const uint64_t b = (uint64_t)__shfl_xor((unsigned long long)umax, off);
        lmax = a > lmax ? a : lmax;
        umax = b > umax ? b : umax;
    }
    if (lane == 0) {
        const double dj = Ux[Lp[j]];
        if (dj > 0.0) atomicAdd(st + 0, 1ull);
        if (dj < 0.0) atomicAdd(st + 1, 1ull);
        atomicMin(st + 2, (unsigned long long)abs_bits(dj));
        atomicMax(st + 3, (unsigned long long)abs_bits(dj));
        if (lmax) atomicMax(st + 4, (unsigned long long)lmax);
        if (umax) atomicMax(st + 5, (unsigned long long)umax);
    }
}

struct SluFactor : LevelFactor {
    int32_t lnz = 0;
    DevBuf<int32_t> rp, rc, rpos;           // row view of the pattern (chol_symbolic_device)
    DevBuf<int32_t> winL, winU;             // the two entry maps
    DevBuf<int32_t> perm_p, perm_c;         // a solve's permutations on the device: pinv, and comb = pinv o prow^-1; each only when
    const int32_t *pinv = nullptr, *comb = nullptr;   // ... it is not the identity (then the pointer is set), for csx_slu_batch_solve
    csx_handle_t hL = 0, hU = 0;            // the committed factor: owned here, lent out by csx_slu_parts; Ut borrows L's p and i
    DevBuf<double> utx;                     // Ut's values (Ut itself owns nothing)
    DevBuf<double> Lx, Ux;                  // scratch of a run: committed only when no column broke down
    // flags: [1] perturbed pivots, [2] columns updated in place; stats: k_slu_stats' six words
    // csx_slu_info / csx_slu_stats
    int64_t pos = 0, neg = 0, perturbed = 0;
    double min_d = 0.0, max_d = 0.0, max_l = 0.0, max_u = 0.0;
    ~SluFactor() {
        if (hU) (void)csx_free(hU);
        if (hL) (void)csx_free(hL);
    }
};

}  // namespace csx
