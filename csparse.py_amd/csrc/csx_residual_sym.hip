// csx_residual_sym_block: R = B - S X for row-major blocks of nrhs columns, with the componentwise backward error
//     omega[c] = max_i |r[i, c]| / (|S| |X| + |B|)[i, c]   and   rnorm[c] = max_i |r[i, c]|
// of every column, in ONE pass, where S is the symmetric matrix csx_chol sees in A: the stored entries of A with
// row <= column, mirrored; the strictly lower entries of A are never read as values.  csx_norm1_sym: |S|_1.
//
// Value rule (the same on the host, csx_residual_sym_host): for output row i and column c the terms (a, j) come in two
// phases, each in one fixed order --
//     phase 1: the entries q of stored column i of A, in storage order, with A.i[q] <= i:      (A.x[q], A.i[q])
//     phase 2: the entries of row i in A's cached row gather, in the gather's order (ascending (column, storage
//              position)), with column > i:                                                     (value, column)
// and then csx_residual_block's rule, unchanged:
//     r = B[i, c];    t = a X[j, c] (rounded);      r = r - t (rounded)
//     d = |B[i, c]|;  u = |a| |X[j, c]| (rounded);  d = d + u (rounded)
//     ratio = 0 when |r| == 0 and d == 0, else |r| / d;  maxima over the bit patterns; no floating-point atomics.
// An entry that fails its phase's test is skipped, never added as a zero (the sign of a zero sum, see csx_rowblock.h).
// A strictly upper entry (r, c) is used twice (row c in phase 1, row r in phase 2), a diagonal entry once.  For a fully
// stored symmetric matrix with sorted columns every row's terms are exactly those of csx_residual_block(trans = 0).
//
// Kernel: k_residual_block's shape (csx_residual.hip; csx_rowblock.h) with two (ptr, idx, val) triples and
// the entry loop run once per phase; the phase's test is folded into the in-range test, and a skipped entry reads X at the row
// itself (in range, and one line for all of them).
//
// Algorithmic bytes per call: 24 nnz + 8 (n + 1) + 8 n nrhs + 16 n nrhs (+ 16 nrhs); 8 n nrhs less without R.
#include <cstring>

#include "csx_rowblock.h"

namespace csx {

// cp / ci / cx: A's columns as stored; rp / ri / rx: A's row gather
struct SymArrays {
    const int32_t *cp, *ci;
    const double *cx;
    const int32_t *rp, *ri;
    const double *rx;
};

#pragma clang fp contract(off)
// The entries [b, e) of one phase into the two accumulators of row r.  UPPER: phase 2 (keep j > r), else phase 1
// (keep j <= r).
template <int V, int U, bool UPPER>
__device__ __forceinline__ void sym_phase(int32_t b, int32_t e, int32_t r, const int32_t *__restrict__ idx,
                                          const double *__restrict__ val, const double *__restrict__ Xc, int32_t nrhs,
                                          typename Cols<V>::T &acc, typename Cols<V>::T &den) {
    typedef typename Cols<V>::T T;
    for (int32_t q = b; q < e; q += U) {
        int32_t j[U];
        double v[U];
        bool keep[U];
        T xv[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const bool in = q + u < e;
            const int32_t jj = in ? idx[q + u] : r;
            keep[u] = in && (UPPER ? jj > r : jj <= r);
            j[u] = keep[u] ? jj : r;   // a skipped entry reads X[r, c]: in range, and not used
            v[u] = in ? val[q + u] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < U; u++) xv[u] = Cols<V>::load(Xc + (int64_t)j[u] * nrhs);
#pragma unroll
        for (int u = 0; u < U; u++)
            if (keep[u]) {   // skipped, not added as 0 (csx_rowblock.h)
                const T t = v[u] * xv[u];
                acc = acc - t;
                const T w = fabs(v[u]) * Cols<V>::abs(xv[u]);
                den = den + w;
            }
    }
}

// part: [gridDim.x][2][nrhs] bit patterns: the workgroup's maxima of ratio, then of |r|, per column.
// B and R are not __restrict__: they may be one block (in place); a lane reads B[r, c] before it writes R[r, c] and no
// other lane touches that entry.
template <int G, int V, int U, bool STORE>
__global__ __launch_bounds__(256) void k_residual_sym(int32_t rows, int32_t nrhs, const int32_t *__restrict__ cp,
                                                      const int32_t *__restrict__ ci, const double *__restrict__ cx,
                                                      const int32_t *__restrict__ rp, const int32_t *__restrict__ ri,
                                                      const double *__restrict__ rx, const double *__restrict__ X,
                                                      const double *B, double *R, uint64_t *__restrict__ part) {
    typedef typename Cols<V>::T T;
    constexpr int GROUPS = 256 / G;
    __shared__ uint64_t red[4][G * V][2];
    const int sub = threadIdx.x & (G - 1);
    const int gid = G == 64 ? __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) : (int)(threadIdx.x / G);
    const int wave = threadIdx.x >> 6;
    const int32_t r0 = (int32_t)blockIdx.x * ROWBLOCK_TILE;   // rows <= INT32_MAX, and r0 < rows
    const int32_t r1 = rows - r0 > ROWBLOCK_TILE ? r0 + ROWBLOCK_TILE : rows;
    for (int32_t c0 = 0; c0 < nrhs; c0 += G * V) {
        const int32_t c = c0 + sub * V;
        uint64_t wmax[V], rmax[V];
#pragma unroll
        for (int k = 0; k < V; k++) wmax[k] = rmax[k] = 0;
        if (c < nrhs) {
            const double *Xc = X + c;
            for (int64_t rr = (int64_t)r0 + gid; rr < r1; rr += GROUPS) {
                const int32_t r = (int32_t)rr;
                T acc = Cols<V>::load(B + (int64_t)r * nrhs + c);
                T den = Cols<V>::abs(acc);
                sym_phase<V, U, false>(cp[r], cp[r + 1], r, ci, cx, Xc, nrhs, acc, den);
                sym_phase<V, U, true>(rp[r], rp[r + 1], r, ri, rx, Xc, nrhs, acc, den);
                if (STORE) Cols<V>::store(R + (int64_t)r * nrhs + c, acc);
#pragma unroll
                for (int k = 0; k < V; k++) {
                    const double ar = fabs(Cols<V>::at(acc, k)), d = Cols<V>::at(den, k);
                    const double ratio = (ar == 0.0 && d == 0.0) ? 0.0 : ar / d;
                    wmax[k] = umax64(wmax[k], abs_bits(ratio));
                    rmax[k] = umax64(rmax[k], abs_bits(ar));
                }
            }
        }
        // the groups of a wave hold different rows of the same columns
#pragma unroll
        for (int off = G; off < 64; off <<= 1)
#pragma unroll
            for (int k = 0; k < V; k++) {
                wmax[k] = umax64(wmax[k], (uint64_t)__shfl_xor((unsigned long long)wmax[k], off));
                rmax[k] = umax64(rmax[k], (uint64_t)__shfl_xor((unsigned long long)rmax[k], off));
            }
        if ((threadIdx.x & 63) < G) {
#pragma unroll
            for (int k = 0; k < V; k++) {
                red[wave][sub * V + k][0] = wmax[k];
                red[wave][sub * V + k][1] = rmax[k];
            }
        }
        __syncthreads();
        if (threadIdx.x < G * V && c0 + (int32_t)threadIdx.x < nrhs) {
            uint64_t w = red[0][threadIdx.x][0], a = red[0][threadIdx.x][1];
#pragma unroll
            for (int s = 1; s < 4; s++) {
                w = umax64(w, red[s][threadIdx.x][0]);
                a = umax64(a, red[s][threadIdx.x][1]);
            }
            uint64_t *out = part + (int64_t)blockIdx.x * 2 * nrhs + c0 + threadIdx.x;
            out[0] = w;
            out[nrhs] = a;
        }
        __syncthreads();
    }
}

// part[bx] = max over the rows [256 bx, 256 bx + 256) of the bit pattern of sum |a| over the row's terms, in the value
// rule's order (sequential, rounded): a lane per row
__global__ __launch_bounds__(256) void k_norm1_sym(int32_t rows, const int32_t *__restrict__ cp, const int32_t *__restrict__ ci,
                                                   const double *__restrict__ cx, const int32_t *__restrict__ rp,
                                                   const int32_t *__restrict__ ri, const double *__restrict__ rx,
                                                   uint64_t *__restrict__ part) {
    __shared__ uint64_t red[4];
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    uint64_t m = 0;
    if (r < rows) {
        double s = 0.0;
        for (int32_t q = cp[r], e = cp[r + 1]; q < e; q++)
            if (ci[q] <= r) s = s + fabs(cx[q]);
        for (int32_t q = rp[r], e = rp[r + 1]; q < e; q++)
            if (ri[q] > r) s = s + fabs(rx[q]);
        m = abs_bits(s);
    }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) m = umax64(m, (uint64_t)__shfl_xor((unsigned long long)m, off));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = umax64(umax64(red[0], red[1]), umax64(red[2], red[3]));
}
#pragma clang fp contract(fast)

// A's columns and its row gather (built on demand); zero: the row pointers of a matrix without entries
static int sym_arrays(Csc *A, DevBuf<int32_t> &zero, SymArrays *out) {
    if (A->nnz == 0) {   // no row gather to build: every row is empty
        CSX_TRY(empty_row_ptr(zero, A->n));
        *out = SymArrays{A->p, A->i, A->x, zero, nullptr, nullptr};
        return CSX_OK;
    }
    CSX_TRY(build_row_gather(A));
    const Gather *g = A->rows.get();
    *out = SymArrays{A->p, A->i, A->x, g->ptr, g->idx, g->val};
    return CSX_OK;
}

}  // namespace csx

using namespace csx;

extern "C" int csx_residual_sym_block(csx_handle_t hA, csx_handle_t hX, csx_handle_t hB, csx_handle_t hR, int32_t nrhs,
                                      double *omega, double *rnorm) {
    CSX_TRY(require_ready());
    Csc *A = csc(hA);
    Vec *X = vec(hX), *B = vec(hB), *R = hR ? vec(hR) : nullptr;
    if (!A || !X || !B || (hR && !R) || !A->x || nrhs < 1 || A->m != A->n) return CSX_EINVAL;
    const int32_t n = A->n;
    const int64_t len = (int64_t)n * nrhs;
    if (!residual_blocks_ok(X, len, B, R, len)) return CSX_EINVAL;
    if (n == 0) return residual_maxima(nullptr, 0, nrhs, omega, rnorm);
    CSX_TRY(csc_validate(A));   // a wrapped matrix: its indices address X and the rows (checked once, remembered)
    DevBuf<int32_t> zero;
    SymArrays a;
    CSX_TRY(sym_arrays(A, zero, &a));
    const double *xd = (const double *)X->d, *bd = (const double *)B->d;
    double *rd = R ? (double *)R->d : nullptr;
    const int64_t blocks = ((int64_t)n + ROWBLOCK_TILE - 1) / ROWBLOCK_TILE;
    DevBuf<uint64_t> part;
    CSX_TRY(part.alloc((size_t)blocks * 2 * nrhs));
    rowblock_launch(nrhs, aligned16(xd, bd, rd), [&](auto sh) {
        if (rd) hipLaunchKernelGGL((k_residual_sym<sh.G, sh.V, sh.U, true>), dim3((unsigned)blocks), dim3(256), 0, ctx().stream, n,
                                   nrhs, a.cp, a.ci, a.cx, a.rp, a.ri, a.rx, xd, bd, rd, part.get());
        else hipLaunchKernelGGL((k_residual_sym<sh.G, sh.V, sh.U, false>), dim3((unsigned)blocks), dim3(256), 0, ctx().stream, n,
                                nrhs, a.cp, a.ci, a.cx, a.rp, a.ri, a.rx, xd, bd, rd, part.get());
    });
    CSX_LAUNCH_CHECK();
    return residual_maxima(part, blocks, nrhs, omega, rnorm);
}

extern "C" int csx_norm1_sym(csx_handle_t hA, double *out) {
    CSX_TRY(require_ready());
    Csc *A = csc(hA);
    if (!A || !out || !A->x || A->m != A->n) return CSX_EINVAL;
    *out = 0.0;
    if (A->n == 0) return CSX_OK;
    CSX_TRY(csc_validate(A));
    DevBuf<int32_t> zero;
    SymArrays a;
    CSX_TRY(sym_arrays(A, zero, &a));
    const int64_t blocks = ((int64_t)A->n + 255) / 256;
    DevBuf<uint64_t> part;
    CSX_TRY(part.alloc((size_t)blocks));
    hipLaunchKernelGGL(k_norm1_sym, dim3((unsigned)blocks), dim3(256), 0, ctx().stream, A->n, a.cp, a.ci, a.cx, a.rp, a.ri, a.rx,
                       part.get());
    CSX_LAUNCH_CHECK();
    uint64_t h = 0;
    CSX_TRY(max_partials_host(part, blocks, 1, &h));
    std::memcpy(out, &h, sizeof(double));
    return CSX_OK;
}
