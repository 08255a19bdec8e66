// The four block kernels of restarted GMRES: csx_gs_project, csx_gs_update, csx_gs_scale, csx_gs_combine.
// Blocks are row-major rows x nrhs; every column is its own system; the basis is ONE vector of consecutive blocks.  A column
// with mask[c] == 0 is never written and its values have no effect on any other.
//
// Value rule (the same on the host, csx_gs_host): products are rounded, then added (fp contract off).  A sum over the rows of a
// column is the ORDERED SUM: leaves are GS_CHUNK consecutive rows added in ascending order from +0.0; an inner node is GS_FAN
// consecutive children added in ascending order from +0.0; levels repeat until one value is left.  The tree depends on rows
// alone -- not on nrhs, the column, the number of basis vectors, the mask or the launch.  No floating-point atomics: the
// leaf kernels store one partial per (leaf, column), k_gs_level sums FAN partials per destination, once per level.
//
// Work items are (leaf, column) pairs, dealt to the lanes column-fastest: at nrhs >= 64 a wave reads 512 consecutive bytes of a
// row; narrower blocks put several leaves into a wave, which changes no sum.  Even nrhs on 16-byte-aligned blocks: a lane takes
// two columns through 16-byte loads (V = 2).  Grids are capped at 8 workgroups per CU with a stride loop over the items.
//
// Algorithmic bytes, N = 8 rows nrhs (one block), over the live columns:
//   project  (nv + ceil(nv / GS_GROUP)) N read: every V_i once, W once per register group of GS_GROUP basis vectors
//   update   (nv + 2) N: every V_i and W read once, W written once; the squared norm of the new W comes out of the same pass
//   scale    2 N;   combine  (len + 1) N with len the column's own length
// plus the partial sums: 8 nrhs rows / GS_CHUNK doubles per sum written and read again (1 / 256 of a block).
#include <cstring>
#include <vector>

#include "csx_gs.h"
#include "csx_internal.h"

namespace csx {

typedef double f64x2g __attribute__((ext_vector_type(2)));

template <int V>
struct GCols;
template <>
struct GCols<1> {
    typedef double T;
    static __device__ __forceinline__ T load(const double *p) { return *p; }
    static __device__ __forceinline__ T zero() { return 0.0; }
    static __device__ __forceinline__ double at(T v, int) { return v; }
    static __device__ __forceinline__ T pick(bool a, bool, T x, T y) { return a ? x : y; }
};
template <>
struct GCols<2> {
    typedef f64x2g T;
    static __device__ __forceinline__ T load(const double *p) { return *reinterpret_cast<const f64x2g *>(p); }
    static __device__ __forceinline__ T zero() {
        T z;
        z.x = 0.0;
        z.y = 0.0;
        return z;
    }
    static __device__ __forceinline__ double at(T v, int k) { return k ? v.y : v.x; }
    static __device__ __forceinline__ T pick(bool a, bool b, T x, T y) {
        T r;
        r.x = a ? x.x : y.x;
        r.y = b ? x.y : y.y;
        return r;
    }
};

// p[0 .. V) = v on the live columns: one 16-byte store when both are
template <int V>
__device__ __forceinline__ void gs_store(double *p, typename GCols<V>::T v, const bool *live) {
    if (V == 2 && live[0] && live[1]) {
        *reinterpret_cast<typename GCols<V>::T *>(p) = v;
        return;
    }
#pragma unroll
    for (int q = 0; q < V; q++)
        if (live[q]) p[q] = GCols<V>::at(v, q);
}

// the work item t of a lane: its leaf, its first column, which of its columns are live
template <int V>
__device__ __forceinline__ bool gs_item(int64_t t, int32_t nrhs, const int32_t *mask, int64_t &leaf, int32_t &c, bool *live) {
    const int32_t kv = nrhs / V;
    leaf = t / kv;
    c = (int32_t)(t - leaf * kv) * V;
    bool any = false;
#pragma unroll
    for (int q = 0; q < V; q++) {
        live[q] = mask[c + q] != 0;
        any |= live[q];
    }
    return any;
}

#pragma clang fp contract(off)
// part[(g nch + leaf) nrhs + c] = the leaf's sum of V_g[r, c] * (+-W[r, c]), for the NG basis vectors from Vb on
template <int V, int NG>
__global__ __launch_bounds__(256) void k_gs_project(int64_t rows, int32_t nrhs, int64_t nch, const double *__restrict__ Vb,
                                                    int64_t stride, const double *__restrict__ W,
                                                    const int32_t *__restrict__ mask, int negate, double *__restrict__ part) {
    typedef typename GCols<V>::T T;
    const int64_t items = nch * (nrhs / V), step = (int64_t)gridDim.x * 256;
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < items; t += step) {
        int64_t leaf;
        int32_t c;
        bool live[V];
        if (!gs_item<V>(t, nrhs, mask, leaf, c, live)) continue;
        const int64_t r0 = leaf * GS_CHUNK, r1 = r0 + GS_CHUNK < rows ? r0 + GS_CHUNK : rows;
        T acc[NG];
#pragma unroll
        for (int g = 0; g < NG; g++) acc[g] = GCols<V>::zero();
#pragma unroll 4
        for (int64_t r = r0; r < r1; r++) {
            const int64_t o = r * nrhs + c;
            T w = GCols<V>::load(W + o);
            if (negate) w = -w;
#pragma unroll
            for (int g = 0; g < NG; g++) {
                const T p = GCols<V>::load(Vb + g * stride + o) * w;
                acc[g] = acc[g] + p;
            }
        }
#pragma unroll
        for (int g = 0; g < NG; g++) gs_store<V>(part + ((int64_t)g * nch + leaf) * nrhs + c, acc[g], live);
    }
}

// W[r, c] <- (+-W[r, c]) - h[0, c] V_0[r, c] - ... - h[nv - 1, c] V_{nv-1}[r, c] in ascending i, and part[leaf nrhs + c] = the
// leaf's sum of the squares of the new W.  GS_TILE rows per load of a coefficient.  W is read and written by the one lane.
template <int V>
__global__ __launch_bounds__(256) void k_gs_update(int64_t rows, int32_t nrhs, int32_t nv, const double *__restrict__ Vb,
                                                   int64_t stride, double *W, const int32_t *__restrict__ mask, int negate,
                                                   const double *__restrict__ h, double *__restrict__ part) {
    typedef typename GCols<V>::T T;
    const int64_t nch = (rows + GS_CHUNK - 1) / GS_CHUNK;
    const int64_t items = nch * (nrhs / V), step = (int64_t)gridDim.x * 256;
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < items; t += step) {
        int64_t leaf;
        int32_t c;
        bool live[V];
        if (!gs_item<V>(t, nrhs, mask, leaf, c, live)) continue;
        const int64_t r0 = leaf * GS_CHUNK, r1 = r0 + GS_CHUNK < rows ? r0 + GS_CHUNK : rows;
        T acc = GCols<V>::zero();
        for (int64_t r = r0; r < r1; r += GS_TILE) {
            T w[GS_TILE];
#pragma unroll
            for (int u = 0; u < GS_TILE; u++) {
                w[u] = r + u < r1 ? GCols<V>::load(W + (r + u) * nrhs + c) : GCols<V>::zero();
                if (negate) w[u] = -w[u];
            }
            for (int32_t i = 0; i < nv; i++) {
                const T hc = GCols<V>::load(h + (int64_t)i * nrhs + c);
                const double *Vi = Vb + i * stride;
                T v[GS_TILE];
#pragma unroll
                for (int u = 0; u < GS_TILE; u++) v[u] = r + u < r1 ? GCols<V>::load(Vi + (r + u) * nrhs + c) : GCols<V>::zero();
#pragma unroll
                for (int u = 0; u < GS_TILE; u++) {
                    const T p = hc * v[u];
                    w[u] = w[u] - p;
                }
            }
#pragma unroll
            for (int u = 0; u < GS_TILE; u++)
                if (r + u < r1) {
                    gs_store<V>(W + (r + u) * nrhs + c, w[u], live);
                    const T q = w[u] * w[u];
                    acc = acc + q;
                }
        }
        gs_store<V>(part + leaf * nrhs + c, acc, live);
    }
}

// U[r, c] = y[0, c] V_0[r, c] + ... + y[len_c - 1, c] V_{len_c - 1}[r, c]: the first product, then one rounded addition per
// further product, ascending; +0.0 for len_c == 0
template <int V>
__global__ __launch_bounds__(256) void k_gs_combine(int64_t rows, int32_t nrhs, int32_t nv, const double *__restrict__ Vb,
                                                    int64_t stride, double *__restrict__ U, const int32_t *__restrict__ mask,
                                                    const int32_t *__restrict__ len, const double *__restrict__ y) {
    typedef typename GCols<V>::T T;
    const int64_t nch = (rows + GS_CHUNK - 1) / GS_CHUNK;
    const int64_t items = nch * (nrhs / V), step = (int64_t)gridDim.x * 256;
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < items; t += step) {
        int64_t leaf;
        int32_t c;
        bool live[V];
        if (!gs_item<V>(t, nrhs, mask, leaf, c, live)) continue;
        const int64_t r0 = leaf * GS_CHUNK, r1 = r0 + GS_CHUNK < rows ? r0 + GS_CHUNK : rows;
        int32_t ln[2] = {0, 0}, most = 0;
#pragma unroll
        for (int q = 0; q < V; q++) {
            ln[q] = live[q] ? len[c + q] : 0;
            ln[q] = ln[q] < nv ? ln[q] : nv;
            most = most > ln[q] ? most : ln[q];
        }
        for (int64_t r = r0; r < r1; r += GS_TILE) {
            T u[GS_TILE];
#pragma unroll
            for (int s = 0; s < GS_TILE; s++) u[s] = GCols<V>::zero();
            for (int32_t i = 0; i < most; i++) {
                const T yc = GCols<V>::load(y + (int64_t)i * nrhs + c);
                const double *Vi = Vb + i * stride;
                T v[GS_TILE];
#pragma unroll
                for (int s = 0; s < GS_TILE; s++) v[s] = r + s < r1 ? GCols<V>::load(Vi + (r + s) * nrhs + c) : GCols<V>::zero();
#pragma unroll
                for (int s = 0; s < GS_TILE; s++) {
                    const T p = yc * v[s];
                    const T a = u[s] + p;
                    // the first product stands as it is; a column past its own length keeps what it has
                    u[s] = GCols<V>::pick(i < ln[0], i < ln[1], i == 0 ? p : a, u[s]);
                }
            }
#pragma unroll
            for (int s = 0; s < GS_TILE; s++)
                if (r + s < r1) gs_store<V>(U + (r + s) * nrhs + c, u[s], live);
        }
    }
}

// Vs[r, c] = W[r, c] / s[c] on the live columns, a grid-stride stream over the rows x nrhs / V lane items
template <int V>
__global__ __launch_bounds__(256) void k_gs_scale(int64_t rows, int32_t nrhs, const double *__restrict__ W, double *__restrict__ Vs,
                                                  const int32_t *__restrict__ mask, const double *__restrict__ s) {
    typedef typename GCols<V>::T T;
    const int32_t kv = nrhs / V;
    const int64_t items = rows * kv, step = (int64_t)gridDim.x * 256;
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < items; t += step) {
        const int32_t c = (int32_t)(t % kv) * V;
        bool live[V], any = false;
#pragma unroll
        for (int q = 0; q < V; q++) {
            live[q] = mask[c + q] != 0;
            any |= live[q];
        }
        if (!any) continue;
        const T q = GCols<V>::load(W + t * V) / GCols<V>::load(s + c);
        gs_store<V>(Vs + t * V, q, live);
    }
}

// out[(g cout + j) nrhs + c] = in[(g cin + FAN j) nrhs + c] + ... over the node's children in ascending order, from +0.0
__global__ __launch_bounds__(256) void k_gs_level(int64_t cin, int64_t cout, int32_t nrhs, int32_t ng, const double *__restrict__ in,
                                                  double *__restrict__ out, const int32_t *__restrict__ mask) {
    const int64_t total = (int64_t)ng * cout * nrhs, step = (int64_t)gridDim.x * 256;
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += step) {
        const int32_t c = (int32_t)(t % nrhs);
        if (!mask[c]) continue;
        const int64_t node = t / nrhs, g = node / cout, j = node - g * cout;
        const int64_t i0 = j * GS_FAN, i1 = i0 + GS_FAN < cin ? i0 + GS_FAN : cin;
        double s = 0.0;
        for (int64_t i = i0; i < i1; i++) s = s + in[(g * cin + i) * nrhs + c];
        out[t] = s;
    }
}
#pragma clang fp contract(fast)

namespace {

unsigned gs_blocks(int64_t items) {
    const int64_t want = (items + 255) / 256, cap = (int64_t)ctx().cus * 8;
    return (unsigned)(want < cap ? (want > 0 ? want : 1) : cap);
}

// one call's view of the work vector
struct GsWork {
    int32_t *mask = nullptr, *len = nullptr;
    double *coef = nullptr, *out = nullptr, *partA = nullptr, *partB = nullptr;
    int64_t nch = 1;
};

constexpr int64_t GS_MAX_ROWS = (int64_t)1 << 40;

// the arguments every entry point shares: the basis (nblocks of them addressed), the block, the work vector, apart from each other
int gs_open(Vec *B, int32_t nblocks, Vec *W, Vec *work, int64_t rows, int32_t nrhs, const int32_t *mask, GsWork &w) {
    if (!B || !W || !work || !mask || nrhs < 1 || nblocks < 1 || rows < 0 || rows > GS_MAX_ROWS) return CSX_EINVAL;
    const int64_t block = rows * nrhs;
    if (B->len / nblocks < block || W->len < block) return CSX_EINVAL;
    const int64_t need = gs_work_len(rows, nrhs, nblocks);
    if (work->len < need) return CSX_EINVAL;
    if (ranges_overlap(B->d, block * nblocks, W->d, block) || ranges_overlap(work->d, need, W->d, block) ||
        ranges_overlap(work->d, need, B->d, block * nblocks))
        return CSX_EINVAL;
    w.nch = gs_chunks(rows);
    double *d = (double *)work->d;
    w.mask = (int32_t *)d;
    w.len = w.mask + nrhs;
    w.coef = d + nrhs;
    w.out = w.coef + (int64_t)nblocks * nrhs;
    w.partA = w.out + (int64_t)nblocks * nrhs;
    w.partB = w.partA + (int64_t)GS_GROUP * w.nch * nrhs;
    return CSX_OK;
}

// the mask, the lengths (or none) and ncoef coefficients (or none) to the work vector in one copy
int gs_stage(const GsWork &w, int32_t nrhs, const int32_t *mask, const int32_t *len, const double *coef, int64_t ncoef) {
    std::vector<double> host((size_t)(nrhs + ncoef));
    int32_t *ints = (int32_t *)host.data();
    std::memcpy(ints, mask, (size_t)nrhs * sizeof(int32_t));
    if (len) std::memcpy(ints + nrhs, len, (size_t)nrhs * sizeof(int32_t));
    else std::memset(ints + nrhs, 0, (size_t)nrhs * sizeof(int32_t));
    if (ncoef) std::memcpy(host.data() + nrhs, coef, (size_t)ncoef * sizeof(double));
    CSX_HIP(hipMemcpyAsync(w.mask, host.data(), host.size() * sizeof(double), hipMemcpyHostToDevice, ctx().stream));
    CSX_HIP(hipStreamSynchronize(ctx().stream));   // the staging array is pageable and ends with this call
    return CSX_OK;
}

bool gs_pairs(int32_t nrhs, const void *a, const void *b, const void *c) {
    return nrhs % 2 == 0 && ((uintptr_t)a % 16) == 0 && ((uintptr_t)b % 16) == 0 && ((uintptr_t)c % 16) == 0;
}

// the inner levels of the ordered sum of ng vectors' leaf partials in partA (nch > 1), the last one into `out`
int gs_levels(const GsWork &w, int32_t nrhs, int32_t ng, double *out) {
    int64_t count = w.nch;
    const double *in = w.partA;
    while (count > 1) {
        const int64_t next = (count + GS_FAN - 1) / GS_FAN;
        double *to = next == 1 ? out : (in == w.partA ? w.partB : w.partA);
        hipLaunchKernelGGL(k_gs_level, dim3(gs_blocks((int64_t)ng * next * nrhs)), dim3(256), 0, ctx().stream, count, next, nrhs, ng,
                           in, to, (const int32_t *)w.mask);
        CSX_LAUNCH_CHECK();
        in = to;
        count = next;
    }
    return CSX_OK;
}

// host[t] = dev[t] for t over cnt rows of nrhs columns, on the live columns only; synchronises
int gs_fetch(const double *dev, int64_t cnt, int32_t nrhs, const int32_t *mask, double *host) {
    std::vector<double> tmp((size_t)(cnt * nrhs));
    CSX_HIP(hipMemcpyAsync(tmp.data(), dev, tmp.size() * sizeof(double), hipMemcpyDeviceToHost, ctx().stream));
    CSX_HIP(hipStreamSynchronize(ctx().stream));
    for (int64_t i = 0; i < cnt; i++)
        for (int32_t c = 0; c < nrhs; c++)
            if (mask[c]) host[i * nrhs + c] = tmp[(size_t)(i * nrhs + c)];
    return CSX_OK;
}

template <int V>
void launch_project(int ng, unsigned blocks, int64_t rows, int32_t nrhs, int64_t nch, const double *Vb, int64_t stride,
                    const double *W, const int32_t *mask, int negate, double *part) {
    hipStream_t s = ctx().stream;
#define CSX_GSP(NG)                                                                                                         \
    case NG:                                                                                                                \
        hipLaunchKernelGGL((k_gs_project<V, NG>), dim3(blocks), dim3(256), 0, s, rows, nrhs, nch, Vb, stride, W, mask, negate, \
                           part);                                                                                           \
        break
    switch (ng) {
        CSX_GSP(1);
        CSX_GSP(2);
        CSX_GSP(3);
        CSX_GSP(4);
        CSX_GSP(5);
        CSX_GSP(6);
        CSX_GSP(7);
        CSX_GSP(8);
    }
#undef CSX_GSP
    static_assert(GS_GROUP == 8, "one case per size of a register group");
}

}  // namespace
}  // namespace csx

using namespace csx;

extern "C" int csx_gs_project(csx_handle_t hV, int32_t nv, csx_handle_t hW, csx_handle_t hwork, int64_t rows, int32_t nrhs,
                              const int32_t *mask, int negate, double *h) {
    CSX_TRY(require_ready());
    Vec *B = vec(hV), *W = vec(hW), *work = vec(hwork);
    GsWork w;
    CSX_TRY(gs_open(B, nv, W, work, rows, nrhs, mask, w));
    if (!h) return CSX_EINVAL;
    if (rows == 0) {
        for (int64_t t = 0; t < (int64_t)nv * nrhs; t++)
            if (mask[t % nrhs]) h[t] = 0.0;
        return CSX_OK;
    }
    CSX_TRY(gs_stage(w, nrhs, mask, nullptr, nullptr, 0));
    const double *Vd = (const double *)B->d, *Wd = (const double *)W->d;
    const int64_t stride = rows * nrhs;
    const bool pairs = gs_pairs(nrhs, Vd, Wd, Wd);
    const unsigned blocks = gs_blocks(w.nch * (nrhs / (pairs ? 2 : 1)));
    for (int32_t g0 = 0; g0 < nv; g0 += GS_GROUP) {
        const int ng = nv - g0 < GS_GROUP ? nv - g0 : GS_GROUP;
        double *sums = w.out + (int64_t)g0 * nrhs;
        double *part = w.nch == 1 ? sums : w.partA;
        if (pairs) launch_project<2>(ng, blocks, rows, nrhs, w.nch, Vd + g0 * stride, stride, Wd, w.mask, negate, part);
        else launch_project<1>(ng, blocks, rows, nrhs, w.nch, Vd + g0 * stride, stride, Wd, w.mask, negate, part);
        CSX_LAUNCH_CHECK();
        CSX_TRY(gs_levels(w, nrhs, ng, sums));
    }
    return gs_fetch(w.out, nv, nrhs, mask, h);
}

extern "C" int csx_gs_update(csx_handle_t hV, int32_t nv, csx_handle_t hW, csx_handle_t hwork, int64_t rows, int32_t nrhs,
                             const int32_t *mask, int negate, const double *h, double *nrm2) {
    CSX_TRY(require_ready());
    Vec *B = vec(hV), *W = vec(hW), *work = vec(hwork);
    GsWork w;
    CSX_TRY(gs_open(B, nv, W, work, rows, nrhs, mask, w));
    if (!h || !nrm2) return CSX_EINVAL;
    if (rows == 0) {
        for (int32_t c = 0; c < nrhs; c++)
            if (mask[c]) nrm2[c] = 0.0;
        return CSX_OK;
    }
    CSX_TRY(gs_stage(w, nrhs, mask, nullptr, h, (int64_t)nv * nrhs));
    const double *Vd = (const double *)B->d;
    double *Wd = (double *)W->d;
    const bool pairs = gs_pairs(nrhs, Vd, Wd, w.coef);
    const unsigned blocks = gs_blocks(w.nch * (nrhs / (pairs ? 2 : 1)));
    double *part = w.nch == 1 ? w.out : w.partA;
    if (pairs)
        hipLaunchKernelGGL(k_gs_update<2>, dim3(blocks), dim3(256), 0, ctx().stream, rows, nrhs, nv, Vd, rows * nrhs, Wd,
                           (const int32_t *)w.mask, negate, (const double *)w.coef, part);
    else
        hipLaunchKernelGGL(k_gs_update<1>, dim3(blocks), dim3(256), 0, ctx().stream, rows, nrhs, nv, Vd, rows * nrhs, Wd,
                           (const int32_t *)w.mask, negate, (const double *)w.coef, part);
    CSX_LAUNCH_CHECK();
    CSX_TRY(gs_levels(w, nrhs, 1, w.out));
    return gs_fetch(w.out, 1, nrhs, mask, nrm2);
}

extern "C" int csx_gs_scale(csx_handle_t hW, csx_handle_t hV, int32_t slot, csx_handle_t hwork, int64_t rows, int32_t nrhs,
                            const int32_t *mask, const double *s) {
    CSX_TRY(require_ready());
    if (slot < 0 || slot == INT32_MAX) return CSX_EINVAL;
    Vec *B = vec(hV), *W = vec(hW), *work = vec(hwork);
    GsWork w;
    CSX_TRY(gs_open(B, slot + 1, W, work, rows, nrhs, mask, w));
    if (!s) return CSX_EINVAL;
    if (rows == 0) return CSX_OK;
    CSX_TRY(gs_stage(w, nrhs, mask, nullptr, s, nrhs));
    const double *Wd = (const double *)W->d;
    double *Vs = (double *)B->d + (int64_t)slot * rows * nrhs;
    const bool pairs = gs_pairs(nrhs, Vs, Wd, w.coef);
    const unsigned blocks = gs_blocks(rows * (nrhs / (pairs ? 2 : 1)));
    if (pairs)
        hipLaunchKernelGGL(k_gs_scale<2>, dim3(blocks), dim3(256), 0, ctx().stream, rows, nrhs, Wd, Vs, (const int32_t *)w.mask,
                           (const double *)w.coef);
    else
        hipLaunchKernelGGL(k_gs_scale<1>, dim3(blocks), dim3(256), 0, ctx().stream, rows, nrhs, Wd, Vs, (const int32_t *)w.mask,
                           (const double *)w.coef);
    CSX_LAUNCH_CHECK();
    return CSX_OK;
}

extern "C" int csx_gs_combine(csx_handle_t hV, int32_t nv, csx_handle_t hU, csx_handle_t hwork, int64_t rows, int32_t nrhs,
                              const int32_t *mask, const double *y, const int32_t *len) {
    CSX_TRY(require_ready());
    Vec *B = vec(hV), *U = vec(hU), *work = vec(hwork);
    GsWork w;
    CSX_TRY(gs_open(B, nv, U, work, rows, nrhs, mask, w));
    if (!y || !len) return CSX_EINVAL;
    for (int32_t c = 0; c < nrhs; c++)
        if (mask[c] && (len[c] < 0 || len[c] > nv)) return CSX_EINVAL;
    if (rows == 0) return CSX_OK;
    CSX_TRY(gs_stage(w, nrhs, mask, len, y, (int64_t)nv * nrhs));
    const double *Vd = (const double *)B->d;
    double *Ud = (double *)U->d;
    const bool pairs = gs_pairs(nrhs, Vd, Ud, w.coef);
    const unsigned blocks = gs_blocks(w.nch * (nrhs / (pairs ? 2 : 1)));
    if (pairs)
        hipLaunchKernelGGL(k_gs_combine<2>, dim3(blocks), dim3(256), 0, ctx().stream, rows, nrhs, nv, Vd, rows * nrhs, Ud,
                           (const int32_t *)w.mask, (const int32_t *)w.len, (const double *)w.coef);
    else
        hipLaunchKernelGGL(k_gs_combine<1>, dim3(blocks), dim3(256), 0, ctx().stream, rows, nrhs, nv, Vd, rows * nrhs, Ud,
                           (const int32_t *)w.mask, (const int32_t *)w.len, (const double *)w.coef);
    CSX_LAUNCH_CHECK();
    return CSX_OK;
}
