// The three block kernels of eigsh() in which the columns of a block MIX: csx_bgs_gram (V_i' W), csx_bgs_update
// (W - sum V_i H_i) and csx_bgs_combine (sum V_i S_i).  Blocks are row-major: the basis is ONE vector of consecutive rows x b
// blocks, W and U are rows x q, 1 <= b, q <= BGS_MAXW.  The kernels of §28 (csx_gmres.hip) keep every column its own system and
// cannot form these sums.
//
// Value rule (the same on the host, csx_bgs_host): §28's, unchanged.  Products are rounded, then added (fp contract off).  A sum
// over the rows is the ORDERED SUM: leaves of GS_CHUNK consecutive rows added in ascending order from +0.0, inner nodes of GS_FAN
// consecutive children added in ascending order from +0.0.  The tree depends on rows alone -- not on b, q, nv, the thread tile,
// the launch or the CU count.  The sums over (i, a) of update and combine run in ascending (i, a), one rounded operation per
// product.  No floating-point atomics.
//
// A row of an n x 8 block is 64 bytes, so no lane walks rows in memory: a workgroup copies a block's row tile -- BGS_TILE doubles,
// rows that are consecutive in memory -- into LDS with coalesced loads (16 bytes per lane where the tile starts on 16) and the
// lanes take their operands from there.
//   gram:    a workgroup owns a leaf; per row tile it stages W once and the tiles of a GROUP of BGS_GROUP basis blocks.  A lane
//            owns a T x T tile of the (a, c) outputs of one basis block (T = 1, 2, 4: the smallest at which the group's outputs
//            fit 256 lanes), so its T T row-ascending chains run side by side on 2 T LDS reads per row.  The lanes of a wave
//            read consecutive doubles of W's row (no bank conflict) and one or a few broadcast addresses of V's.
//   update / combine: a workgroup owns a row tile of W / U in registers: a lane holds BGS_OUT rows of ONE column (lanes dealt
//            column-fastest: a pass of the lanes reads and writes consecutive memory), so a coefficient read serves its four
//            chains.  It walks the basis blocks: V_i's tile (rows padded to an odd count of doubles in LDS: lanes on different
//            rows read distinct banks) and the b x q coefficients H_i go through LDS.
//
// Algorithmic bytes, with B = 8 rows b (one basis block) and Q = 8 rows q:
//   gram     nv B + ceil(nv / BGS_GROUP) Q read, plus the leaf sums: 8 nv b q rows / GS_CHUNK written and read again
//   update   nv B + 2 Q  (every V_i and W read once, W written once)
//   combine  nv B + Q    (every V_i read once, U written once)
#include <cstring>
#include <vector>

#include "csx_gs.h"
#include "csx_internal.h"

namespace csx {

typedef double f64x2b __attribute__((ext_vector_type(2)));

constexpr int BGS_OUT = 4;   // outputs of a lane in update / combine: rows of its one column

// dst[0 .. count) (LDS) = (+-)src[0 .. count) (global, consecutive), by all 256 lanes
__device__ __forceinline__ void bgs_fill(double *dst, const double *__restrict__ src, int32_t count, bool negate) {
    const int32_t t = threadIdx.x;
    if ((reinterpret_cast<uintptr_t>(src) & 15) == 0) {
        const int32_t pairs = count >> 1;
        for (int32_t p = t; p < pairs; p += 256) {
            f64x2b v = *reinterpret_cast<const f64x2b *>(src + 2 * p);
            if (negate) v = -v;
            *reinterpret_cast<f64x2b *>(dst + 2 * p) = v;
        }
        if ((count & 1) && t == 0) dst[count - 1] = negate ? -src[count - 1] : src[count - 1];
    } else {
        for (int32_t p = t; p < count; p += 256) dst[p] = negate ? -src[p] : src[p];
    }
}

// rows of a block's tile in LDS
__host__ __device__ __forceinline__ int32_t bgs_tile_rows(int32_t b, int32_t q) {
    const int32_t w = b > q ? b : q, rt = BGS_TILE / w;
    return rt < GS_CHUNK ? rt : GS_CHUNK;
}

// rows of a row tile of update / combine: a lane owns BGS_OUT rows of one column, the 256 lanes cover 256 / q rows a pass
__host__ __device__ __forceinline__ int32_t bgs_apply_rows(int32_t b, int32_t q) {
    const int32_t rt = bgs_tile_rows(b, q), most = BGS_OUT * (256 / q);
    return rt < most ? rt : most;
}

#pragma clang fp contract(off)
// part[((g nch + leaf) b + a) q + c] = the leaf's sum over its rows, ascending from +0.0, of V_g[r, a] * (+-W[r, c]), for the ng
// basis blocks from Vb on.  ng ceil(b / T) ceil(q / T) <= 256.
template <int T>
__global__ __launch_bounds__(256) void k_bgs_gram(int64_t rows, int32_t b, int32_t q, int64_t nch, int32_t ng,
                                                  const double *__restrict__ Vb, int64_t stride, const double *__restrict__ W,
                                                  int negate, double *__restrict__ part) {
    __shared__ __attribute__((aligned(16))) double Wl[BGS_TILE];
    __shared__ __attribute__((aligned(16))) double Vl[BGS_GROUP][BGS_TILE];
    const int32_t na = (b + T - 1) / T, nc = (q + T - 1) / T, per = na * nc, rt = bgs_tile_rows(b, q);
    const int32_t tile = threadIdx.x;
    const bool active = tile < ng * per;
    const int32_t g = active ? tile / per : 0, rem = active ? tile - g * per : 0;
    const int32_t a0 = (rem / nc) * T, c0 = (rem % nc) * T;
    int32_t ai[T], cj[T];
#pragma unroll
    for (int i = 0; i < T; i++) {
        ai[i] = a0 + i < b ? a0 + i : b - 1;     // a lane past the edge reads the edge and stores nothing
        cj[i] = c0 + i < q ? c0 + i : q - 1;
    }
    for (int64_t leaf = blockIdx.x; leaf < nch; leaf += gridDim.x) {
        const int64_t r0 = leaf * GS_CHUNK;
        const int32_t nleaf = (int32_t)(r0 + GS_CHUNK < rows ? GS_CHUNK : rows - r0);
        double acc[T][T];
#pragma unroll
        for (int i = 0; i < T; i++)
#pragma unroll
            for (int j = 0; j < T; j++) acc[i][j] = 0.0;
        for (int32_t s0 = 0; s0 < nleaf; s0 += rt) {
            const int32_t n = nleaf - s0 < rt ? nleaf - s0 : rt;
            __syncthreads();                                 // the tile before this one has been read
            bgs_fill(Wl, W + (r0 + s0) * q, n * q, negate != 0);
            for (int32_t h = 0; h < ng; h++) bgs_fill(Vl[h], Vb + h * stride + (r0 + s0) * b, n * b, false);
            __syncthreads();
            if (active) {
                const double *vrow = Vl[g], *wrow = Wl;
                for (int32_t r = 0; r < n; r++, vrow += b, wrow += q) {
                    double v[T], w[T];
#pragma unroll
                    for (int i = 0; i < T; i++) {
                        v[i] = vrow[ai[i]];
                        w[i] = wrow[cj[i]];
                    }
#pragma unroll
                    for (int i = 0; i < T; i++)
#pragma unroll
                        for (int j = 0; j < T; j++) {
                            const double p = v[i] * w[j];
                            acc[i][j] = acc[i][j] + p;
                        }
                }
            }
        }
        if (active) {
            double *out = part + ((int64_t)g * nch + leaf) * b * q;
#pragma unroll
            for (int i = 0; i < T; i++)
#pragma unroll
                for (int j = 0; j < T; j++)
                    if (a0 + i < b && c0 + j < q) out[(a0 + i) * q + c0 + j] = acc[i][j];
        }
    }
}

// out[(g cout + j) bq + t] = in[(g cin + FAN j) bq + t] + ... over the node's children in ascending order, from +0.0
__global__ __launch_bounds__(256) void k_bgs_level(int64_t cin, int64_t cout, int32_t bq, int32_t ng, const double *__restrict__ in,
                                                   double *__restrict__ out) {
    const int64_t total = (int64_t)ng * cout * bq, step = (int64_t)gridDim.x * 256;
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += step) {
        const int64_t node = t / bq, e = t - node * bq, g = node / cout, j = node - g * cout;
        const int64_t i0 = j * GS_FAN, i1 = i0 + GS_FAN < cin ? i0 + GS_FAN : cin;
        double s = 0.0;
        for (int64_t i = i0; i < i1; i++) s = s + in[(g * cin + i) * bq + e];
        out[t] = s;
    }
}


// COMBINE == 0:  X[r, c] <- X[r, c] - coef[0, 0, c] V_0[r, 0] - coef[0, 1, c] V_0[r, 1] - ..., ascending in (i, a)
// COMBINE == 1:  X[r, c] = coef[0, 0, c] V_0[r, 0] + ...: the first product as it is, then one rounded addition per further
//                product; +0.0 for nv == 0
template <int COMBINE>
__global__ __launch_bounds__(256) void k_bgs_apply(int64_t rows, int32_t b, int32_t q, int32_t nv, const double *__restrict__ Vb,
                                                   int64_t stride, double *X, const double *__restrict__ coef) {
    __shared__ __attribute__((aligned(16))) double Vl[BGS_TILE + GS_CHUNK];
    __shared__ __attribute__((aligned(16))) double Hl[BGS_MAXW * BGS_MAXW];
    const int32_t rt = bgs_apply_rows(b, q), rp = 256 / q, ldv = b | 1, bq = b * q;
    const int64_t ntiles = (rows + rt - 1) / rt;
    const int32_t rg = (int32_t)threadIdx.x / q, c = (int32_t)threadIdx.x - rg * q;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t t0 = tile * rt;
        const int32_t n = (int32_t)(t0 + rt < rows ? rt : rows - t0);
        double x[BGS_OUT];
        int32_t vo[BGS_OUT];
        bool live[BGS_OUT];
#pragma unroll
        for (int k = 0; k < BGS_OUT; k++) {
            const int32_t r = rg + k * rp;
            live[k] = rg < rp && r < n;
            vo[k] = live[k] ? r * ldv : 0;               // a lane past the tile reads its first row and stores nothing
            x[k] = (!COMBINE && live[k]) ? X[(t0 + r) * q + c] : 0.0;
        }
        for (int32_t i = 0; i < nv; i++) {
            const double *Vi = Vb + i * stride + t0 * b;
            __syncthreads();                             // the basis block before this one has been read
            for (int32_t p = threadIdx.x; p < n * b; p += 256) {
                const int32_t r = p / b;
                Vl[r * ldv + (p - r * b)] = Vi[p];
            }
            bgs_fill(Hl, coef + (int64_t)i * bq, bq, false);
            __syncthreads();
            for (int32_t a = 0; a < b; a++) {
                const double h = Hl[a * q + c];
#pragma unroll
                for (int k = 0; k < BGS_OUT; k++) {
                    const double p = h * Vl[vo[k] + a];
                    if (COMBINE) x[k] = (i == 0 && a == 0) ? p : x[k] + p;
                    else x[k] = x[k] - p;
                }
            }
        }
#pragma unroll
        for (int k = 0; k < BGS_OUT; k++)
            if (live[k]) X[(t0 + rg + k * rp) * q + c] = x[k];
    }
}
#pragma clang fp contract(fast)

static_assert(BGS_TILE >= BGS_MAXW && BGS_TILE >= GS_CHUNK, "a tile holds whole rows, and a whole leaf at width 1 .. 4");
static_assert(BGS_GROUP * ((BGS_MAXW + 3) / 4) * ((BGS_MAXW + 3) / 4) <= 256, "a group's 4 x 4 thread tiles fit 256 lanes");

namespace {

constexpr int64_t BGS_MAX_ROWS = (int64_t)1 << 40;

// one call's view of the work vector
struct BgsWork {
    double *coef = nullptr, *out = nullptr, *partA = nullptr, *partB = nullptr;
    int64_t nch = 1;
};

// the arguments every entry point shares.  The work vector lies apart from the basis and from the block; a block that a call
// writes (update, combine) lies apart from the basis.
int bgs_open(Vec *B, int32_t nv, int32_t b, Vec *X, int32_t q, Vec *work, int64_t rows, bool written, BgsWork &w) {
    if (!B || !X || !work || nv < 0 || b < 1 || b > BGS_MAXW || q < 1 || q > BGS_MAXW || rows < 0 || rows > BGS_MAX_ROWS)
        return CSX_EINVAL;
    const int64_t vblock = rows * b, xblock = rows * q;
    if (nv > 0 && B->len / nv < vblock) return CSX_EINVAL;
    if (X->len < xblock) return CSX_EINVAL;
    const int64_t need = bgs_work_len(rows, b, q, nv);
    if (work->len < need) return CSX_EINVAL;
    if (ranges_overlap(work->d, need, X->d, xblock) || ranges_overlap(work->d, need, B->d, vblock * nv)) return CSX_EINVAL;
    if (written && ranges_overlap(B->d, vblock * nv, X->d, xblock)) return CSX_EINVAL;
    w.nch = gs_chunks(rows);
    const int64_t bq = (int64_t)b * q;
    w.coef = (double *)work->d;
    w.out = w.coef + bq * nv;
    w.partA = w.out + bq * nv;
    w.partB = w.partA + BGS_GROUP * w.nch * bq;
    return CSX_OK;
}

// the coefficients to the work vector; the host array is pageable, so the call waits for the copy
int bgs_stage(const BgsWork &w, const double *coef, int64_t count) {
    if (!count) return CSX_OK;
    CSX_HIP(hipMemcpyAsync(w.coef, coef, (size_t)count * sizeof(double), hipMemcpyHostToDevice, ctx().stream));
    CSX_HIP(hipStreamSynchronize(ctx().stream));
    return CSX_OK;
}

unsigned bgs_blocks(int64_t items, int per_cu) {
    const int64_t cap = (int64_t)ctx().cus * per_cu;
    return (unsigned)(items < cap ? (items > 0 ? items : 1) : cap);
}

int bgs_apply(int combine, csx_handle_t hV, int32_t nv, int32_t b, csx_handle_t hX, int32_t q, csx_handle_t hwork, int64_t rows,
              const double *coef) {
    CSX_TRY(require_ready());
    Vec *B = vec(hV), *X = vec(hX), *work = vec(hwork);
    BgsWork w;
    CSX_TRY(bgs_open(B, nv, b, X, q, work, rows, true, w));
    if (!coef) return CSX_EINVAL;
    if (rows == 0 || (nv == 0 && !combine)) return CSX_OK;
    CSX_TRY(bgs_stage(w, coef, (int64_t)nv * b * q));
    const int64_t ntiles = (rows + bgs_apply_rows(b, q) - 1) / bgs_apply_rows(b, q);
    const unsigned blocks = bgs_blocks(ntiles, 8);
    if (combine)
        hipLaunchKernelGGL(k_bgs_apply<1>, dim3(blocks), dim3(256), 0, ctx().stream, rows, b, q, nv, (const double *)B->d, rows * b,
                           (double *)X->d, (const double *)w.coef);
    else
        hipLaunchKernelGGL(k_bgs_apply<0>, dim3(blocks), dim3(256), 0, ctx().stream, rows, b, q, nv, (const double *)B->d, rows * b,
                           (double *)X->d, (const double *)w.coef);
    CSX_LAUNCH_CHECK();
    return CSX_OK;
}

}  // namespace
}  // namespace csx

using namespace csx;

extern "C" int csx_bgs_gram(csx_handle_t hV, int32_t nv, int32_t b, csx_handle_t hW, int32_t q, csx_handle_t hwork, int64_t rows,
                            int negate, double *out) {
    CSX_TRY(require_ready());
    Vec *B = vec(hV), *W = vec(hW), *work = vec(hwork);
    BgsWork w;
    CSX_TRY(bgs_open(B, nv, b, W, q, work, rows, false, w));
    if (!out) return CSX_EINVAL;
    const int64_t bq = (int64_t)b * q, total = bq * nv;
    if (nv == 0) return CSX_OK;
    if (rows == 0) {
        for (int64_t t = 0; t < total; t++) out[t] = 0.0;
        return CSX_OK;
    }
    const double *Vd = (const double *)B->d, *Wd = (const double *)W->d;
    const int64_t stride = rows * b;
    const unsigned blocks = bgs_blocks(w.nch, 4);
    hipStream_t s = ctx().stream;
    for (int32_t g0 = 0; g0 < nv; g0 += BGS_GROUP) {
        const int32_t ng = nv - g0 < BGS_GROUP ? nv - g0 : BGS_GROUP;
        double *sums = w.out + g0 * bq;
        double *part = w.nch == 1 ? sums : w.partA;
        const double *Vg = Vd + g0 * stride;
        // the smallest thread tile at which the group's outputs fit the 256 lanes: it changes no sum
        if ((int64_t)ng * bq <= 256)
            hipLaunchKernelGGL(k_bgs_gram<1>, dim3(blocks), dim3(256), 0, s, rows, b, q, w.nch, ng, Vg, stride, Wd, negate, part);
        else if ((int64_t)ng * ((b + 1) / 2) * ((q + 1) / 2) <= 256)
            hipLaunchKernelGGL(k_bgs_gram<2>, dim3(blocks), dim3(256), 0, s, rows, b, q, w.nch, ng, Vg, stride, Wd, negate, part);
        else
            hipLaunchKernelGGL(k_bgs_gram<4>, dim3(blocks), dim3(256), 0, s, rows, b, q, w.nch, ng, Vg, stride, Wd, negate, part);
        CSX_LAUNCH_CHECK();
        int64_t count = w.nch;
        const double *in = w.partA;
        while (count > 1) {
            const int64_t next = (count + GS_FAN - 1) / GS_FAN;
            double *to = next == 1 ? sums : (in == w.partA ? w.partB : w.partA);
            hipLaunchKernelGGL(k_bgs_level, dim3(bgs_blocks((ng * next * bq + 255) / 256, 8)), dim3(256), 0, s, count, next,
                               (int32_t)bq, ng, in, to);
            CSX_LAUNCH_CHECK();
            in = to;
            count = next;
        }
    }
    CSX_HIP(hipMemcpyAsync(out, w.out, (size_t)total * sizeof(double), hipMemcpyDeviceToHost, s));
    CSX_HIP(hipStreamSynchronize(s));
    return CSX_OK;
}

extern "C" int csx_bgs_update(csx_handle_t hV, int32_t nv, int32_t b, csx_handle_t hW, int32_t q, csx_handle_t hwork, int64_t rows,
                              const double *H) {
    return bgs_apply(0, hV, nv, b, hW, q, hwork, rows, H);
}

extern "C" int csx_bgs_combine(csx_handle_t hV, int32_t nv, int32_t b, csx_handle_t hU, int32_t q, csx_handle_t hwork, int64_t rows,
                               const double *S) {
    return bgs_apply(1, hV, nv, b, hU, q, hwork, rows, S);
}
