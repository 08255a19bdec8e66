// csx_pattern_outer: out[q] = alpha * sum over c of U[i_q, c] V[j_q, c] for every stored entry q of A -- the outer product of two
// row-major blocks sampled on A's pattern, which is the gradient of a solve with respect to A's entries (DESIGN.md §31;
// include/csx.h has the value rule, csx_pattern_outer_host.cpp its host form).
//
// Kernel.  The work is balanced by ENTRIES: a workgroup takes PO_CHUNK consecutive entries whatever columns they lie in, so one
// column of a million entries and a million columns of one entry are the same launch.
//   phase 1, per wave (its PO_WAVE_CHUNK entries): the columns of its first and last entry by a 64-ary search of A.p -- every
//     lane probes one pointer, a ballot counts those not above the entry: 4 rounds for 5M columns -- then every lane finds the
//     column of its own 4 entries by bisection BETWEEN those two (no step at all inside one long column), the four searches in
//     lock step so that their loads are in flight together.  (row, column) go to LDS.
//   phase 2: a group of W lanes per entry, lane l on the columns l, l + W, ... of the block rows: a row gather is one contiguous
//     8 nrhs-byte segment read by adjacent lanes.  A group takes consecutive entries, PO_FLIGHT per step: their U rows (and the
//     mirrored V rows in sym mode) are all requested before the first product.  The rows of the entries' own column, V[j, :] and
//     in sym mode U[j, :], are shared by the entries of a column: while a step stays inside one column they are read once and
//     kept in registers (up to PO_KEPT passes, nrhs <= PO_KEPT PO_LANES).  The partials are combined by the rule's butterfly
//     through lane exchanges inside the group; the results of a wave's entries go through LDS so that adjacent lanes store
//     adjacent doubles.
// No atomics, no scratch memory; LDS holds the indices and the results of a chunk (16 KiB).
//
// Algorithmic bytes per call: 12 nnz + 4 (n + 1) + 8 (m + n) nrhs.
#include "csx_internal.h"
#include "csx_pattern_outer.h"

namespace csx {

static_assert(PO_CHUNK == 4 * PO_WAVE_CHUNK && PO_WAVE_CHUNK == 4 * WAVE, "a workgroup is 4 waves, a lane searches 4 entries");

// the largest j in [0, n) with p[j] <= q, for 0 <= q < p[n]; the same q in every lane of the wave
__device__ __forceinline__ int32_t po_column_of(const int32_t *__restrict__ p, int32_t n, int32_t q, int lane) {
    int32_t lo = 0, hi = n;   // p[lo] <= q < p[hi]
    while (hi - lo > 1) {
        const int32_t step = (hi - lo + 63) >> 6;
        const int64_t at = (int64_t)lo + (int64_t)(lane + 1) * step;
        const bool le = at < hi && p[at] <= q;
        const int32_t cnt = __popcll(__ballot(le));   // p ascends: the lanes that hold are the first cnt
        const int64_t nhi = (int64_t)lo + (int64_t)(cnt + 1) * step;
        lo += cnt * step;
        hi = nhi < hi ? (int32_t)nhi : hi;
    }
    return lo;
}

#pragma clang fp contract(off)
// P: the passes (columns l, l + W, ... of a lane) a lane can keep of the column's own rows V[j, :] (and U[j, :] in sym mode) in
// registers, 0: none.  A group takes CONSECUTIVE entries, which mostly share their column: while the PO_FLIGHT entries of a step
// do, the column's rows are read once for all of them and kept for the next step; a step that spans columns reads every
// entry's rows.  Both ways take the same values in the same order.
template <int W, bool SYM, int P>
__global__ __launch_bounds__(256) void k_pattern_outer(int32_t n, int32_t nnz, int32_t nrhs, const int32_t *__restrict__ Ap,
                                                       const int32_t *__restrict__ Ai, const double *__restrict__ U,
                                                       const double *__restrict__ V, double alpha, double *__restrict__ out) {
    constexpr int G = WAVE / W;                 // groups of a wave
    constexpr int PER = PO_WAVE_CHUNK / G;      // consecutive entries of a group
    static_assert(PER % PO_FLIGHT == 0, "a group's entries are whole steps");
    __shared__ int32_t s_row[PO_CHUNK], s_col[PO_CHUNK];
    __shared__ double s_out[PO_CHUNK];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t w0 = (int64_t)blockIdx.x * PO_CHUNK + wave * PO_WAVE_CHUNK;   // the wave's entries: [w0, w1)
    const int64_t w1 = w0 + PO_WAVE_CHUNK < nnz ? w0 + PO_WAVE_CHUNK : nnz;
    int32_t *row = s_row + wave * PO_WAVE_CHUNK, *col = s_col + wave * PO_WAVE_CHUNK;
    double *res = s_out + wave * PO_WAVE_CHUNK;
    if (w0 < w1) {
        const int32_t jlo = po_column_of(Ap, n, (int32_t)w0, lane), jhi = po_column_of(Ap, n, (int32_t)(w1 - 1), lane);
        int32_t a[4], b[4], q[4];
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const int64_t e = w0 + lane + 64 * t;
            q[t] = (int32_t)(e < w1 ? e : w1 - 1);
            a[t] = jlo, b[t] = jhi;   // the column lies in [a, b]
        }
        for (int32_t span = jhi - jlo; span > 0; span >>= 1) {
            int32_t mid[4], pm[4];
#pragma unroll
            for (int t = 0; t < 4; t++) {
                mid[t] = (int32_t)(((int64_t)a[t] + b[t] + 1) >> 1);
                pm[t] = Ap[mid[t]];
            }
#pragma unroll
            for (int t = 0; t < 4; t++) {
                if (pm[t] <= q[t]) a[t] = mid[t];
                else b[t] = mid[t] - 1;
            }
        }
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const int e = lane + 64 * t;
            if (w0 + e < w1) {
                row[e] = Ai[w0 + e];
                col[e] = a[t];
            }
        }
    }
    __syncthreads();   // (a wave reads only what it wrote: the barriers order its own LDS traffic)
    const int32_t cnt = w0 < w1 ? (int32_t)(w1 - w0) : 0;
    const int sub = lane & (W - 1), g = lane / W;
    int32_t kept = -1;                       // the column whose rows vrow / urow hold
    double vrow[P > 0 ? P : 1], urow[P > 0 ? P : 1];
    for (int32_t e0 = g * PER; e0 < (g + 1) * PER && e0 < cnt; e0 += PO_FLIGHT) {
        int32_t r[PO_FLIGHT], j[PO_FLIGHT];
        bool in[PO_FLIGHT], live[PO_FLIGHT], two[PO_FLIGHT];
        double s[PO_FLIGHT];
        bool same = P > 0;
#pragma unroll
        for (int u = 0; u < PO_FLIGHT; u++) {
            in[u] = e0 + u < cnt;
            r[u] = in[u] ? row[e0 + u] : 0;
            j[u] = in[u] ? col[e0 + u] : 0;
            live[u] = in[u] && !(SYM && r[u] > j[u]);
            two[u] = SYM && r[u] < j[u];
            s[u] = 0.0;
            same = same && (!in[u] || j[u] == j[0]);
        }
        if (P > 0 && same) {
            if (kept != j[0]) {
                kept = j[0];
#pragma unroll
                for (int pp = 0; pp < P; pp++) {
                    const int32_t c = sub + pp * W;
                    vrow[pp] = c < nrhs ? V[(int64_t)kept * nrhs + c] : 0.0;
                    if (SYM) urow[pp] = c < nrhs ? U[(int64_t)kept * nrhs + c] : 0.0;
                }
            }
#pragma unroll
            for (int pp = 0; pp < P; pp++) {
                const int32_t c = sub + pp * W;
                if (c < nrhs) {
                    double uv[PO_FLIGHT], v2[PO_FLIGHT];
#pragma unroll
                    for (int u = 0; u < PO_FLIGHT; u++) {
                        uv[u] = live[u] ? U[(int64_t)r[u] * nrhs + c] : 0.0;
                        if (SYM) v2[u] = live[u] && two[u] ? V[(int64_t)r[u] * nrhs + c] : 0.0;
                    }
#pragma unroll
                    for (int u = 0; u < PO_FLIGHT; u++) {
                        const double t = uv[u] * vrow[pp];
                        s[u] = pp == 0 ? t : s[u] + t;
                        if (SYM && two[u]) {
                            const double t2 = urow[pp] * v2[u];
                            s[u] = s[u] + t2;
                        }
                    }
                }
            }
        } else {
            for (int32_t c = sub; c < nrhs; c += W) {
                double uv[PO_FLIGHT], vv[PO_FLIGHT], u2[PO_FLIGHT], v2[PO_FLIGHT];
#pragma unroll
                for (int u = 0; u < PO_FLIGHT; u++) {
                    uv[u] = live[u] ? U[(int64_t)r[u] * nrhs + c] : 0.0;
                    vv[u] = live[u] ? V[(int64_t)j[u] * nrhs + c] : 0.0;
                    if (SYM) {
                        u2[u] = live[u] && two[u] ? U[(int64_t)j[u] * nrhs + c] : 0.0;
                        v2[u] = live[u] && two[u] ? V[(int64_t)r[u] * nrhs + c] : 0.0;
                    }
                }
#pragma unroll
                for (int u = 0; u < PO_FLIGHT; u++) {
                    const double t = uv[u] * vv[u];
                    s[u] = c == sub ? t : s[u] + t;
                    if (SYM && two[u]) {
                        const double t2 = u2[u] * v2[u];
                        s[u] = s[u] + t2;
                    }
                }
            }
        }
#pragma unroll
        for (int u = 0; u < PO_FLIGHT; u++) {
#pragma unroll
            for (int d = W / 2; d >= 1; d >>= 1) s[u] = s[u] + __shfl_xor(s[u], d, W);   // lane l < d: s[l] + s[l + d]
            if (sub == 0 && in[u]) res[e0 + u] = live[u] ? alpha * s[u] : 0.0;
        }
    }
    __syncthreads();
    // the wave's results leave together: adjacent lanes store adjacent doubles
#pragma unroll
    for (int t = 0; t < 4; t++) {
        const int e = lane + 64 * t;
        if (e < cnt) out[w0 + e] = res[e];
    }
}
#pragma clang fp contract(fast)

template <bool SYM>
static void launch_outer(unsigned blocks, int32_t n, int32_t nnz, int32_t nrhs, const int32_t *Ap, const int32_t *Ai,
                         const double *U, const double *V, double alpha, double *out) {
#define CSX_PO(W, P) \
    hipLaunchKernelGGL((k_pattern_outer<W, SYM, P>), dim3(blocks), dim3(256), 0, ctx().stream, n, nnz, nrhs, Ap, Ai, U, V, alpha, out)
    const int32_t passes = (nrhs + PO_LANES - 1) / PO_LANES;
    switch (po_width(nrhs)) {
        case 1: CSX_PO(1, 1); break;
        case 2: CSX_PO(2, 1); break;
        case 4: CSX_PO(4, 1); break;
        case 8: CSX_PO(8, 1); break;
        default:
            if (passes <= 1) CSX_PO(16, 1);
            else if (passes <= 2) CSX_PO(16, 2);
            else if (passes <= 4) CSX_PO(16, 4);
            else if (passes <= PO_KEPT) CSX_PO(16, PO_KEPT);
            else CSX_PO(16, 0);
            break;
    }
#undef CSX_PO
}

}  // namespace csx

using namespace csx;

extern "C" int csx_pattern_outer(csx_handle_t hA, csx_handle_t hU, csx_handle_t hV, int32_t nrhs, int mode, double alpha,
                                 csx_handle_t hout) {
    CSX_TRY(require_ready());
    Csc *A = csc(hA);
    Vec *U = vec(hU), *V = vec(hV), *O = vec(hout);
    if (!A || !U || !V || !O || nrhs < 1 || (mode != 0 && mode != 1) || (mode == 1 && A->m != A->n)) return CSX_EINVAL;
    const int64_t ulen = (int64_t)A->m * nrhs, vlen = (int64_t)A->n * nrhs;
    if (U->len < ulen || V->len < vlen || O->len < A->nnz) return CSX_EINVAL;
    if (ranges_overlap(O->d, A->nnz, U->d, ulen) || ranges_overlap(O->d, A->nnz, V->d, vlen)) return CSX_EINVAL;
    if (A->m == 0 || A->n == 0 || A->nnz == 0) return CSX_OK;
    CSX_TRY(csc_validate(A));   // a wrapped matrix: its indices address the rows of U (checked once, remembered)
    const unsigned blocks = (unsigned)(((int64_t)A->nnz + PO_CHUNK - 1) / PO_CHUNK);
    if (mode) launch_outer<true>(blocks, A->n, A->nnz, nrhs, A->p, A->i, (const double *)U->d, (const double *)V->d, alpha,
                                 (double *)O->d);
    else launch_outer<false>(blocks, A->n, A->nnz, nrhs, A->p, A->i, (const double *)U->d, (const double *)V->d, alpha,
                             (double *)O->d);
    CSX_LAUNCH_CHECK();
    return CSX_OK;
}
