// What csx_hqr.hip (one Householder QR) and csx_hqr_batch.hip (many value sets on one analysis)
// share: the column function with its level-walk policy, the statistics of a column of R, and the factor object.
#pragma once
#include <cmath>

#include "csx_internal.h"
#include "csx_colupdate.h"
#include "csx_levelwalk.h"

#pragma clang fp contract(off)

namespace csx {

constexpr int HQR_ACC = 512;   // slots of a column kept in LDS per wave (8 + 4 + 4 bytes each: 32 KB a workgroup); a longer column is updated in place
constexpr int64_t HQR_RUN_WORK = 1 << 24;   // slot updates one launch of the walker takes at most (its levels' longest columns
                                            // summed), so that no launch of one workgroup holds the device for long

// what one lane wrote, every lane of the wave may read
__device__ __forceinline__ void hqr_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// part[l] + part[l ^ s] for s = 32 .. 1: addition is commutative, so every lane ends with the bytes the fixed tree
// part[l] = part[l] + part[l + s], l < s, leaves in part[0]
__device__ __forceinline__ double hqr_butterfly(double part) {
    for (int s = 32; s >= 1; s >>= 1) part = part + __shfl_xor(part, s);
    return part;
}

// ---- one column -----------------------------------------------------------------------------------------------------------------
// Column k of R and of V.  On entry Rx[Rp[k] ..] and Vx[Vp[k] ..] hold A(:, q[k]) in the column's slots (+0.0 elsewhere) and every
// descendant of k is finished (its V.x, beta in Vx, beta).  The slots in their natural order -- R's entries before the diagonal,
// then V's -- are the accumulators; Srow[Sp[k] ..] lists their rows ascending and Sdst the natural slot of each (R.i and V.i are
// not sorted).  acc / srow / sdst: wave-private LDS (HQR_ACC entries).  flags[0]: the smallest column with a non-finite diagonal
// (atomicMin), flags[1]: columns that took the in-place path (integer atomicAdd).
__device__ __forceinline__ void hqr_column(int32_t k, const int32_t *__restrict__ Vp, const int32_t *__restrict__ Vi, double *Vx,
                                           const int32_t *__restrict__ Rp, const int32_t *__restrict__ Ri, double *Rx, double *beta,
                                           const int32_t *__restrict__ Sp, const int32_t *__restrict__ Srow,
                                           const int32_t *__restrict__ Sdst, double *acc, int32_t *srow, int32_t *sdst, int lane,
                                           int *flags) {
    const int32_t rb = Rp[k], nr = Rp[k + 1] - rb - 1;   // reflections to apply = entries of R(:,k) before the diagonal
    const int32_t vb = Vp[k], nv = Vp[k + 1] - vb;
    const int32_t sb = Sp[k], len = nr + nv;
    const bool in_lds = len <= HQR_ACC;
    const int32_t *rows = in_lds ? srow : Srow + sb;
    const int32_t *dst = in_lds ? sdst : Sdst + sb;
    if (in_lds) {
        for (int32_t t = lane; t < len; t += 64) {
            acc[t] = t < nr ? Rx[rb + t] : Vx[vb + (t - nr)];
            srow[t] = Srow[sb + t];
            sdst[t] = Sdst[sb + t];
        }
    }
    hqr_wave_sync();
    // the accumulator of natural slot s
    auto at = [&](int32_t s) -> double * { return in_lds ? acc + s : (s < nr ? Rx + rb + s : Vx + vb + (s - nr)); };
    auto slot_of = [&](int32_t row) -> int32_t { return dst[find_row(rows, len, row)]; };
    // Reflections are applied in order, but fetched eight at a time (as csx_colupdate.h fetches a column's updates): lane u reads
    // the descriptor of reflection t0 + u -- c, the bounds of V(:,c), beta[c], all final -- and the first 64 entries of the eight
    // columns are requested together and their slots found before the first of them is applied; what is left per reflection is
    // LDS traffic and the butterfly.  The order of the arithmetic is untouched.
    constexpr int UQ = 8;
    for (int32_t t0 = 0; t0 < nr; t0 += UQ) {
        int32_t cbq = 0, ceq = 0;
        double bq = 0.0;
        if (lane < UQ && t0 + lane < nr) {
            const int32_t cq = Ri[rb + t0 + lane];
            cbq = Vp[cq];
            ceq = Vp[cq + 1];
            bq = beta[cq];
        }
        int32_t cb_[UQ], ce_[UQ], s_[UQ];
        double b_[UQ], v_[UQ];
#pragma unroll
        for (int u = 0; u < UQ; u++) {
            cb_[u] = __builtin_amdgcn_readlane(cbq, u);
            ce_[u] = __builtin_amdgcn_readlane(ceq, u);      // 0 for an absent reflection: no entries
            b_[u] = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(bq), u),
                                     __builtin_amdgcn_readlane(__double2loint(bq), u));
        }
#pragma unroll
        for (int u = 0; u < UQ; u++) {
            const int32_t p = cb_[u] + lane;
            const int32_t pp = p < ce_[u] ? p : cb_[u];      // a valid address either way
            s_[u] = Vi[pp];
            v_[u] = Vx[pp];
        }
#pragma unroll
        for (int u = 0; u < UQ; u++) s_[u] = slot_of(s_[u]);  // (rows and their slots do not change while the column is reduced)
#pragma unroll
        for (int u = 0; u < UQ; u++) {
            if (t0 + u >= nr) break;
            const int32_t cb = cb_[u], ce = ce_[u];
            const bool head = cb + lane < ce;
            double part = 0.0;
            if (head) part = part + v_[u] * *at(s_[u]);
            for (int32_t p = cb + 64 + lane; p < ce; p += 64) part = part + Vx[p] * *at(slot_of(Vi[p]));
            const double tau = hqr_butterfly(part) * b_[u];
            if (head) {
                double *a = at(s_[u]);
                *a = *a - v_[u] * tau;
            }
            for (int32_t p = cb + 64 + lane; p < ce; p += 64) {
                double *a = at(slot_of(Vi[p]));
                *a = *a - Vx[p] * tau;
            }
            hqr_wave_sync();   // one reflection after the other: they touch the same rows
            if (in_lds && lane == 0) Rx[rb + t0 + u] = acc[t0 + u];   // R(c,k): row c is slot t, and no later reflection touches it
        }
    }
    // V(:,k) = what is left below the diagonal; tail2 over everything after the head
    double part = 0.0;
    for (int32_t j = 1 + lane; j < nv; j += 64) {
        const double v = *at(nr + j);
        if (in_lds) Vx[vb + j] = v;
        part = part + v * v;
    }
    const double tail2 = hqr_butterfly(part);
    const double head = *at(nr);
    double s, b, v0;   // cs_house, statement for statement as csx_qr_host
    if (tail2 == 0.0) {
        s = fabs(head);
        b = head <= 0.0 ? 2.0 : 0.0;
        v0 = 1.0;
    } else {
        s = __dsqrt_rn(head * head + tail2);
        v0 = head <= 0.0 ? head - s : -tail2 / (head + s);
        b = -1.0 / (s * v0);
    }
    hqr_wave_sync();       // every lane has read the head before it is replaced
    if (lane == 0) {
        Vx[vb] = v0;
        Rx[rb + nr] = s;
        beta[k] = b;
        if (!isfinite(s)) atomicMin(flags, k);
        if (!in_lds) atomicAdd(flags + 1, 1);
    }
    hqr_wave_sync();
}

// the level walk's policy (csx_levelwalk.h): hqr_column behind k_level / k_run, with the kernels' argument types and LDS arrays
struct HqrColumn {
    using Args = ColumnArgs<const int32_t *__restrict__, const int32_t *__restrict__, double *, const int32_t *__restrict__,
                            const int32_t *__restrict__, double *, double *, const int32_t *__restrict__, const int32_t *__restrict__,
                            const int32_t *__restrict__, int *>;
    static __device__ __forceinline__ void column(int32_t k, int w, int lane, const int32_t *Vp, const int32_t *Vi, double *Vx,
                                                  const int32_t *Rp, const int32_t *Ri, double *Rx, double *beta, const int32_t *Sp,
                                                  const int32_t *Srow, const int32_t *Sdst, int *flags) {
        __shared__ double acc[WALK_WAVES][HQR_ACC];
        __shared__ int32_t row[WALK_WAVES][HQR_ACC];
        __shared__ int32_t dst[WALK_WAVES][HQR_ACC];
        hqr_column(k, Vp, Vi, Vx, Rp, Ri, Rx, beta, Sp, Srow, Sdst, acc[w], row[w], dst[w], lane, flags);
    }
};

// One lane per column: st[0] min |r_kk|, st[1] max |r_kk| -- extrema of the bit patterns of fabs taken as unsigned integers
// (k_ldl_stats' rule) -- st[2] the number of exact zeros (integer adds); a wave reduces before its lane 0 touches st.  The body of
// k_hqr_stats (csx_hqr.hip), shared with csx_hqr_batch.hip's kernel per (column, member).
__device__ __forceinline__ void hqr_stats_column(int64_t k, int lane, int32_t n, const int32_t *__restrict__ Rp,
                                                 const double *__restrict__ Rx, unsigned long long *st) {
    unsigned long long lo = ~0ull, hi = 0ull, zeros = 0ull;
    if (k < n) {
        const double d = Rx[Rp[k + 1] - 1];
        lo = hi = (unsigned long long)__double_as_longlong(fabs(d));
        zeros = d == 0.0 ? 1ull : 0ull;
    }
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned long long a = __shfl_xor(lo, off), b = __shfl_xor(hi, off), z = __shfl_xor(zeros, off);
        lo = a < lo ? a : lo;
        hi = b > hi ? b : hi;
        zeros += z;
    }
    if (lane == 0 && lo != ~0ull) {
        atomicMin(st + 0, lo);
        atomicMax(st + 1, hi);
        if (zeros) atomicAdd(st + 2, zeros);
    }
}

struct HqrFactor : LevelFactor {            // (the levels are those of the column elimination tree)
    int32_t m2 = 0, vnz = 0, rnz = 0;
    DevBuf<int32_t> sp, srow, sdst;         // per column the rows of its slots ascending, and the natural slot of each
    DevBuf<int32_t> winV, winR;             // entry maps: the entry of A that lands in a slot of V / of R (-1: none)
    csx_handle_t hV = 0, hR = 0, hB = 0;    // the committed factor: owned here, lent out by csx_hqr_parts
    DevBuf<double> beta;                    // the committed beta (hB's vector borrows it)
    DevBuf<double> Vx, Rx, bx;              // scratch of a run: committed only when no column broke down
    DevBuf<int32_t> perm_q, perm_p;         // the solve's permutations on the device (q: n entries, empty for the identity; pinv: m),
                                            // ... for csx_hqr_batch_solve
    DevBuf<int32_t> rrp, rrc, rrpos;        // the row view of R's pattern with its storage positions (row i: columns descending, so
    bool r_rows = false;                    // ... the diagonal last), made by the first csx_hqr_batch_solve (csx_hqr_batch.hip)
    // flags: [1] columns updated in place; stats: k_hqr_stats' three words
    int64_t zeros = 0;
    double min_r = 0.0, max_r = 0.0;
    ~HqrFactor() {
        if (hB) (void)csx_free(hB);
        if (hR) (void)csx_free(hR);
        if (hV) (void)csx_free(hV);
    }
};

}  // namespace csx
