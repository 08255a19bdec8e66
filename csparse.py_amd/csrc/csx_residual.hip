// csx_residual_block: R = B - op(A) X for row-major blocks of nrhs columns, with the componentwise backward error
//     omega[c] = max_i |r[i, c]| / (|op(A)| |X| + |B|)[i, c]   and   rnorm[c] = max_i |r[i, c]|
// of every column, in ONE pass over the matrix.  csx_block_add_cols / csx_block_select_cols: the two
// streaming kernels of the refinement loop built on it.
//
// Value rule (the same on the host, csx_residual_host): for output row i and column c the row's terms (a_q, j_q) are
// taken in one fixed order -- trans == 0: A's cached row gather, ascending (column, storage position); trans != 0:
// the storage order of column i of A, whose stored columns ARE the rows of A' (no plan, no transpose) --
//     r = B[i, c];    t = a_q X[j_q, c] (rounded);      r = r - t (rounded)
//     d = |B[i, c]|;  u = |a_q| |X[j_q, c]| (rounded);  d = d + u (rounded)
//     ratio = 0 when |r| == 0 and d == 0, else |r| / d  (IEEE division; NaN and inf propagate)
// The maxima are taken over the bit patterns of the non-negative doubles as unsigned 64-bit integers: exact, NaN above
// inf, independent of the order.  No floating-point atomics: a workgroup reduces its rows (wave shuffles, then LDS)
// into one partial per column, a second kernel reduces the partials.
//
// Kernel: the row-block shape (csx_rowblock.h) on one (ptr, idx, val) gather: two accumulators per column;
// division and reduction at the row's end.  The loop over the column passes (nrhs > G V) is the outer one here, so that a
// lane carries the maxima of ONE pass.
//
// Algorithmic bytes per call: 12 nnz + 4 (rows + 1) + 8 cols nrhs + 16 rows nrhs (+ 16 nrhs); 8 rows nrhs less
// without R.
#include <cstring>
#include <utility>

#include "csx_rowblock.h"

namespace csx {

#pragma clang fp contract(off)
// part: [gridDim.x][2][nrhs] bit patterns: the workgroup's maxima of ratio, then of |r|, per column.
// B and R are not __restrict__: they may be one block (in place); a lane reads B[r, c] before it writes R[r, c] and no
// other lane touches that entry.
template <int G, int V, int U, bool STORE>
__global__ __launch_bounds__(256) void k_residual_block(int32_t rows, int32_t nrhs, const int32_t *__restrict__ ptr,
                                                        const int32_t *__restrict__ idx, const double *__restrict__ val,
                                                        const double *__restrict__ X, const double *B, double *R,
                                                        uint64_t *__restrict__ part) {
    typedef typename Cols<V>::T T;
    constexpr int GROUPS = 256 / G;
    __shared__ uint64_t red[4][G * V][2];
    const int sub = threadIdx.x & (G - 1);
    const int gid = G == 64 ? __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) : (int)(threadIdx.x / G);
    const int wave = threadIdx.x >> 6;
    const int64_t r0 = (int64_t)blockIdx.x * ROWBLOCK_TILE;
    const int64_t r1 = r0 + ROWBLOCK_TILE < rows ? r0 + ROWBLOCK_TILE : rows;
    for (int32_t c0 = 0; c0 < nrhs; c0 += G * V) {
        const int32_t c = c0 + sub * V;
        uint64_t wmax[V], rmax[V];
#pragma unroll
        for (int k = 0; k < V; k++) wmax[k] = rmax[k] = 0;
        if (c < nrhs) {
            for (int64_t r = r0 + gid; r < r1; r += GROUPS) {
                const int32_t b = ptr[r], e = ptr[r + 1];
                T acc = Cols<V>::load(B + r * nrhs + c);
                T den = Cols<V>::abs(acc);
                for (int32_t q = b; q < e; q += U) {
                    int32_t j[U];
                    double v[U];
                    T xv[U];
#pragma unroll
                    for (int u = 0; u < U; u++) {
                        const bool in = q + u < e;
                        j[u] = in ? idx[q + u] : 0;
                        v[u] = in ? val[q + u] : 0.0;
                    }
#pragma unroll
                    for (int u = 0; u < U; u++) xv[u] = Cols<V>::load(X + (int64_t)j[u] * nrhs + c);
#pragma unroll
                    for (int u = 0; u < U; u++)
                        if (q + u < e) {   // skipped, not added as 0 (csx_rowblock.h)
                            const T t = v[u] * xv[u];
                            acc = acc - t;
                            const T w = fabs(v[u]) * Cols<V>::abs(xv[u]);
                            den = den + w;
                        }
                }
                if (STORE) Cols<V>::store(R + r * nrhs + c, acc);
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
#pragma clang fp contract(fast)

// out[bx][j] = max over the rows [256 bx, 256 bx + 256) of in[row][j], for `width` columns: a lane per column, the
// rows dealt to the 4 waves
__global__ __launch_bounds__(256) void k_max_partials(int64_t count, int32_t width, const uint64_t *__restrict__ in,
                                                      uint64_t *__restrict__ out) {
    __shared__ uint64_t red[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int32_t j = (int32_t)blockIdx.y * 64 + lane;
    const int64_t b0 = (int64_t)blockIdx.x * 256;
    const int64_t b1 = b0 + 256 < count ? b0 + 256 : count;
    uint64_t m = 0;
    if (j < width)
        for (int64_t b = b0 + wave; b < b1; b += 4) m = umax64(m, in[b * width + j]);
    red[wave][lane] = m;
    __syncthreads();
    if (wave == 0 && j < width)
        out[(int64_t)blockIdx.x * width + j] = umax64(umax64(red[0][lane], red[1][lane]), umax64(red[2][lane], red[3][lane]));
}

// out[i, c] = mask[c] ? X[i, c] + D[i, c] : X[i, c]
__global__ __launch_bounds__(256) void k_block_add_cols(int64_t total, int32_t nrhs, const int32_t *__restrict__ mask,
                                                        const double *X, const double *D, double *out) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += stride) {
        const double x = X[t];
        out[t] = mask[t % nrhs] ? x + D[t] : x;
    }
}

// dst[i, c] = src[i, c] where mask[c]
__global__ __launch_bounds__(256) void k_block_select_cols(int64_t total, int32_t nrhs, const int32_t *__restrict__ mask,
                                                           const double *__restrict__ src, double *__restrict__ dst) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += stride)
        if (mask[t % nrhs]) dst[t] = src[t];
}

// h[0 .. width) = the maxima over the `count` rows of part (count x width bit patterns, left as they are); synchronises
int max_partials_host(const uint64_t *part, int64_t count, int32_t width, uint64_t *h) {
    hipStream_t s = ctx().stream;
    DevBuf<uint64_t> pa, pb;
    const uint64_t *in = part;
    if (count > 1) {
        CSX_TRY(pa.alloc((size_t)((count + 255) / 256) * width));
        CSX_TRY(pb.alloc((size_t)((count + 65535) / 65536) * width));
    }
    uint64_t *out = pa, *spare = pb;
    while (count > 1) {
        const int64_t next = (count + 255) / 256;
        hipLaunchKernelGGL(k_max_partials, dim3((unsigned)next, (unsigned)((width + 63) / 64)), dim3(256), 0, s, count, width,
                           in, out);
        CSX_LAUNCH_CHECK();
        in = out;
        std::swap(out, spare);
        count = next;
    }
    CSX_HIP(hipMemcpyAsync(h, in, (size_t)width * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    CSX_HIP(hipStreamSynchronize(s));
    return CSX_OK;
}

int residual_maxima(const uint64_t *part, int64_t blocks, int32_t nrhs, double *omega, double *rnorm) {
    if (!omega && !rnorm) return CSX_OK;
    std::vector<uint64_t> h(2 * (size_t)nrhs, 0);   // the bit pattern of 0.0
    if (blocks > 0) CSX_TRY(max_partials_host(part, blocks, 2 * nrhs, h.data()));
    static_assert(sizeof(double) == sizeof(uint64_t), "bit patterns of doubles");
    if (omega) std::memcpy(omega, h.data(), (size_t)nrhs * sizeof(double));
    if (rnorm) std::memcpy(rnorm, h.data() + nrhs, (size_t)nrhs * sizeof(double));
    return CSX_OK;
}

int empty_row_ptr(DevBuf<int32_t> &zero, int32_t rows) {
    CSX_TRY(zero.alloc((size_t)rows + 1));
    CSX_HIP(hipMemsetAsync(zero.get(), 0, ((size_t)rows + 1) * sizeof(int32_t), ctx().stream));
    return CSX_OK;
}

// the residual of `rows` gathered rows and the maxima of every column (host arrays, either may be null)
static int run_residual(int32_t rows, int32_t nrhs, const int32_t *ptr, const int32_t *idx, const double *val, const double *X,
                        const double *B, double *R, double *omega, double *rnorm) {
    const int64_t blocks = ((int64_t)rows + ROWBLOCK_TILE - 1) / ROWBLOCK_TILE;
    DevBuf<uint64_t> pa;
    CSX_TRY(pa.alloc((size_t)blocks * 2 * nrhs));
    rowblock_launch(nrhs, aligned16(X, B, R), [&](auto sh) {
        if (R) hipLaunchKernelGGL((k_residual_block<sh.G, sh.V, sh.U, true>), dim3((unsigned)blocks), dim3(256), 0, ctx().stream,
                                  rows, nrhs, ptr, idx, val, X, B, R, pa.get());
        else hipLaunchKernelGGL((k_residual_block<sh.G, sh.V, sh.U, false>), dim3((unsigned)blocks), dim3(256), 0, ctx().stream,
                                rows, nrhs, ptr, idx, val, X, B, R, pa.get());
    });
    CSX_LAUNCH_CHECK();
    return residual_maxima(pa, blocks, nrhs, omega, rnorm);
}

static int upload_mask(DevBuf<int32_t> &d, const int32_t *mask, int32_t nrhs) {
    CSX_TRY(upload(d, mask, (size_t)nrhs));
    CSX_HIP(hipStreamSynchronize(ctx().stream));   // the caller's array is pageable: it may change after the call
    return CSX_OK;
}

static unsigned stream_blocks(int64_t total) {
    const int64_t want = (total + 255) / 256, cap = (int64_t)ctx().cus * 16;
    return (unsigned)(want < cap ? want : cap);
}

}  // namespace csx

using namespace csx;

extern "C" int csx_residual_block(csx_handle_t hA, csx_handle_t hX, csx_handle_t hB, csx_handle_t hR, int32_t nrhs, int trans,
                                  double *omega, double *rnorm) {
    CSX_TRY(require_ready());
    Csc *A = csc(hA);
    Vec *X = vec(hX), *B = vec(hB), *R = hR ? vec(hR) : nullptr;
    if (!A || !X || !B || (hR && !R) || !A->x || nrhs < 1) return CSX_EINVAL;
    const int32_t rows = trans ? A->n : A->m, cols = trans ? A->m : A->n;
    const int64_t xlen = (int64_t)cols * nrhs, blen = (int64_t)rows * nrhs;
    if (!residual_blocks_ok(X, xlen, B, R, blen)) return CSX_EINVAL;
    if (rows == 0) return residual_maxima(nullptr, 0, nrhs, omega, rnorm);
    CSX_TRY(csc_validate(A));   // a wrapped matrix: its indices address X and the rows (checked once, remembered)
    const double *xd = (const double *)X->d, *bd = (const double *)B->d;
    double *rd = R ? (double *)R->d : nullptr;
    if (trans) return run_residual(rows, nrhs, A->p, A->i, A->x, xd, bd, rd, omega, rnorm);
    if (A->nnz == 0 || cols == 0) {   // no row gather to build: every row is empty
        DevBuf<int32_t> zero;
        CSX_TRY(empty_row_ptr(zero, rows));
        return run_residual(rows, nrhs, zero, nullptr, nullptr, xd, bd, rd, omega, rnorm);
    }
    CSX_TRY(build_row_gather(A));
    const Gather *g = A->rows.get();
    return run_residual(rows, nrhs, g->ptr, g->idx, g->val, xd, bd, rd, omega, rnorm);
}

extern "C" int csx_block_add_cols(csx_handle_t hX, csx_handle_t hD, csx_handle_t hout, int64_t rows, int32_t nrhs,
                                  const int32_t *mask) {
    CSX_TRY(require_ready());
    Vec *X = vec(hX), *D = vec(hD), *O = vec(hout);
    if (!X || !D || !O || !mask || rows < 0 || nrhs < 1) return CSX_EINVAL;
    const int64_t total = rows * nrhs;
    if (X->len < total || D->len < total || O->len < total) return CSX_EINVAL;
    // out may be X or D themselves (element-wise), not a shifted view of either
    if (O->d != X->d && ranges_overlap(O->d, total, X->d, total)) return CSX_EINVAL;
    if (O->d != D->d && ranges_overlap(O->d, total, D->d, total)) return CSX_EINVAL;
    if (total == 0) return CSX_OK;
    DevBuf<int32_t> dm;
    CSX_TRY(upload_mask(dm, mask, nrhs));
    hipLaunchKernelGGL(k_block_add_cols, dim3(stream_blocks(total)), dim3(256), 0, ctx().stream, total, nrhs, dm.get(),
                       (const double *)X->d, (const double *)D->d, (double *)O->d);
    CSX_LAUNCH_CHECK();
    return CSX_OK;
}

extern "C" int csx_block_select_cols(csx_handle_t hsrc, csx_handle_t hdst, int64_t rows, int32_t nrhs, const int32_t *mask) {
    CSX_TRY(require_ready());
    Vec *S = vec(hsrc), *D = vec(hdst);
    if (!S || !D || !mask || rows < 0 || nrhs < 1) return CSX_EINVAL;
    const int64_t total = rows * nrhs;
    if (S->len < total || D->len < total) return CSX_EINVAL;
    if (ranges_overlap(S->d, total, D->d, total)) return CSX_EINVAL;
    if (total == 0) return CSX_OK;
    DevBuf<int32_t> dm;
    CSX_TRY(upload_mask(dm, mask, nrhs));
    hipLaunchKernelGGL(k_block_select_cols, dim3(stream_blocks(total)), dim3(256), 0, ctx().stream, total, nrhs, dm.get(),
                       (const double *)S->d, (double *)D->d);
    CSX_LAUNCH_CHECK();
    return CSX_OK;
}
