// The update loop of a left-looking column: what chol_column (csx_chol.hip), ldl_column (csx_ldl.hip), slu_column (csx_slu.h) and
// k_schur_cols (csx_schur.hip) share between their prologue and their epilogue, and the row search of a sorted
// column.  One wave owns column j.  The row view of row j (row_ptr, row_col, row_pos: chol_symbolic_device) lists the columns
// k < j with (j,k) in the pattern, ascending, each with the position of (j,k) in column k, and ends with the diagonal.
//
// The contract of column_updates<NV>, NV value planes on the one pattern Lp / Li:
//   * Updates are applied in ascending k, one after the other, with a wave barrier after each: they may hit the same rows.
//   * They are fetched eight at a time.  Lane u reads the descriptor of update u -- position of (j,k), end of column k, the NV
//     weights -- which is one dependent round trip for eight updates instead of one each; the descriptors are broadcast with
//     readlane and the heads of the eight source columns (64 entries each, every plane) are requested together before any is
//     consumed.  The lanes past a column's end load its first entry instead: a valid address either way, and never used.
//     What a source column has beyond 64 entries follows in a strided tail.
//   * Every product is value x weight in plane i, formed here with contraction off whatever the includer's state, so it is
//     rounded on its own, and handed to the policy for the subtraction.  The pragma covers this body only: a policy's
//     lambdas are compiled under the CALLER's contraction state.  Their subtraction cannot fuse with a product formed here,
//     but arithmetic of their own can (the weight L(j,k) d[k] next to a sum, say): a caller that computes there keeps
//     contraction off in its file, as csx_ldl.hip, csx_slu.h and csx_schur.hip do; chol_column's lambdas only load and subtract.
//   * weights(k, pos, w) -> bool fills w[0 .. NV) for the update by column k whose entry (j,k) is at pos, or refuses it: a
//     refused descriptor gets "end of column 0", so nothing of it is applied, and a batch whose FIRST descriptor is refused
//     ends the loop (k ascends: k_schur_cols stops at the first kept column).  A policy that always returns true costs nothing:
//     the test folds away.  One that refuses costs a lane flag and a readlane a fetch; what it wrote to w is never used.
//   * load(p, v) reads v[0 .. NV), the planes' values at position p of the pattern.
//   * sub(row, a) subtracts the products a[0 .. NV) from the column's sums at `row`, wherever the caller keeps them.
// The three are lambdas of the caller.  Inlined, they leave every kernel's memory and f64 instructions as they were with the
// loop written out (profiles/column_updates_isa.txt) -- on one condition: a `sub` that chooses between an LDS window and global
// memory for MORE than one plane names its LDS pointers by their address space (slu_column says why).
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

namespace csx {

// the slot of row r among rows[0 .. len), ascending and holding r (len >= 1)
__device__ __forceinline__ int32_t find_row(const int32_t *rows, int32_t len, int32_t r) {
    int32_t lo = 0, hi = len - 1;
    while (lo < hi) {
        const int32_t mid = (lo + hi) >> 1;
        if (rows[mid] < r) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

template <int NV, class Weights, class Load, class Sub>
__device__ __forceinline__ void column_updates(int32_t j, const int32_t *__restrict__ Lp, const int32_t *__restrict__ Li,
                                               const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ row_col,
                                               const int32_t *__restrict__ row_pos, int lane, Weights weights, Load load, Sub sub) {
#pragma clang fp contract(off)
    constexpr int UQ = 8;
    const int32_t qe = row_ptr[j + 1] - 1;   // the row view ends with the diagonal
    for (int32_t q0 = row_ptr[j]; q0 < qe; q0 += UQ) {
        int32_t posq = 0, kendq = 0;
        int takenq = 1;
        double wq[NV];
#pragma unroll
        for (int i = 0; i < NV; i++) wq[i] = 0.0;
        if (lane < UQ && q0 + lane < qe) {
            const int32_t kq = row_col[q0 + lane], pq = row_pos[q0 + lane];
            const int32_t kend = Lp[kq + 1];   // (asked for before the weights, beside them: one round trip for both)
            takenq = weights(kq, pq, wq) ? 1 : 0;
            if (takenq) {
                posq = pq;
                kendq = kend;
            }
        }
        if (!__builtin_amdgcn_readlane(takenq, 0)) break;
        int32_t pos_[UQ], kend_[UQ], r_[UQ];
        double w_[UQ][NV], v_[UQ][NV];
#pragma unroll
        for (int u = 0; u < UQ; u++) {
            pos_[u] = __builtin_amdgcn_readlane(posq, u);
            kend_[u] = __builtin_amdgcn_readlane(kendq, u);   // 0 for an absent or refused update: nothing below
#pragma unroll
            for (int i = 0; i < NV; i++)
                w_[u][i] = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(wq[i]), u),
                                            __builtin_amdgcn_readlane(__double2loint(wq[i]), u));
        }
#pragma unroll
        for (int u = 0; u < UQ; u++) {
            const int32_t p = pos_[u] + lane;
            const int32_t pp = p < kend_[u] ? p : pos_[u];     // a valid address either way
            r_[u] = Li[pp];
            load(pp, v_[u]);
        }
#pragma unroll
        for (int u = 0; u < UQ; u++) {
            if (pos_[u] + lane < kend_[u]) {
                double a[NV];
#pragma unroll
                for (int i = 0; i < NV; i++) a[i] = v_[u][i] * w_[u][i];
                sub(r_[u], a);
            }
            for (int32_t p = pos_[u] + 64 + lane; p < kend_[u]; p += 64) {   // columns longer than one wave
                double v[NV], a[NV];
                load(p, v);
#pragma unroll
                for (int i = 0; i < NV; i++) a[i] = v[i] * w_[u][i];
                sub(Li[p], a);
            }
            __builtin_amdgcn_wave_barrier();   // one update after the other: they may hit the same rows
        }
    }
}

}  // namespace csx
