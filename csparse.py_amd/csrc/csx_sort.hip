// Device primitives: exclusive scan, column expansion, stable LSD radix sort,
// segment boundaries.  These carry the integer side of cs_cumsum
// (csparse.py:767-784) and of the stable counting sort inside cs_transpose
// (csparse.py:2305-2314) on the device.
//
// Stability matters: cs_transpose emits each output column in ascending
// (source column, source position) order, and p[]/i[] must be bit-exact.  The
// sort is therefore a least-significant-digit radix sort whose scatter ranks
// equal digits by (workgroup, wave, round, lane), i.e. by source position.
#include "csx_internal.h"

namespace csx {

// ---------------------------------------------------------------- scan ----
constexpr int SCAN_THREADS = 256;
constexpr int SCAN_ITEMS = 8;
constexpr int SCAN_TILE = SCAN_THREADS * SCAN_ITEMS;

__device__ __forceinline__ int wave_inclusive_scan(int v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        int t = __shfl_up(v, d, 64);
        if (lane >= d) v += t;
    }
    return v;
}

// block-wide exclusive scan of one value per thread (256 threads); returns the
// exclusive prefix and the block total
__device__ __forceinline__ int block_exclusive_scan(int v, int *total) {
    __shared__ int wsum[SCAN_THREADS / 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int inc = wave_inclusive_scan(v, lane);
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    int off = 0, tot = 0;
#pragma unroll
    for (int k = 0; k < SCAN_THREADS / 64; k++) {
        int s = wsum[k];
        if (k < w) off += s;
        tot += s;
    }
    __syncthreads();
    *total = tot;
    return off + inc - v;
}

__global__ __launch_bounds__(SCAN_THREADS) void k_scan_block_sums(const int32_t *in, int64_t n, int32_t *sums) {
    int64_t base = (int64_t)blockIdx.x * SCAN_TILE;
    int acc = 0;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; k++) {
        int64_t idx = base + (int64_t)k * SCAN_THREADS + threadIdx.x;
        if (idx < n) acc += in[idx];
    }
    int tot;
    block_exclusive_scan(acc, &tot);
    if (threadIdx.x == 0) sums[blockIdx.x] = tot;
}

__global__ __launch_bounds__(SCAN_THREADS) void k_scan_apply(const int32_t *in, int32_t *out, int64_t n,
                                                             const int32_t *block_off) {
    // thread t owns SCAN_ITEMS consecutive elements so that the scan order is the array order
    int64_t base = (int64_t)blockIdx.x * SCAN_TILE + (int64_t)threadIdx.x * SCAN_ITEMS;
    int v[SCAN_ITEMS];
    int acc = 0;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; k++) {
        v[k] = (base + k < n) ? in[base + k] : 0;
        acc += v[k];
    }
    int tot;
    int pre = block_exclusive_scan(acc, &tot) + (block_off ? block_off[blockIdx.x] : 0);
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; k++) {
        if (base + k < n) out[base + k] = pre;
        pre += v[k];
        if (base + k == n - 1) out[n] = pre;
    }
}

__global__ void k_set_i32(int32_t *p, int32_t v) { *p = v; }

int scan_exclusive_i32(const int32_t *in, int32_t *out, int64_t n, int64_t *total_host) {
    hipStream_t s = ctx().stream;
    if (n <= 0) {
        hipLaunchKernelGGL(k_set_i32, dim3(1), dim3(1), 0, s, out, 0);
        CSX_LAUNCH_CHECK();
        if (total_host) *total_host = 0;
        return CSX_OK;
    }
    int64_t nb = (n + SCAN_TILE - 1) / SCAN_TILE;
    DevBuf<int32_t> sums;   // (freed with no wait: the pool's blocks are used on the context's stream only, whoever gets this one
                            // next queues behind the scan)
    if (nb > 1) {
        CSX_TRY(sums.alloc((size_t)nb + 1));
        hipLaunchKernelGGL(k_scan_block_sums, dim3((unsigned)nb), dim3(SCAN_THREADS), 0, s, in, n, sums);
        CSX_LAUNCH_CHECK();
        CSX_TRY(scan_exclusive_i32(sums, sums, nb, nullptr));
    }
    hipLaunchKernelGGL(k_scan_apply, dim3((unsigned)nb), dim3(SCAN_THREADS), 0, s, in, out, n, sums);
    CSX_LAUNCH_CHECK();
    if (total_host) {
        int32_t t = 0;
        CSX_HIP(hipMemcpyAsync(&t, out + n, sizeof t, hipMemcpyDeviceToHost, s));
        CSX_HIP(hipStreamSynchronize(s));
        *total_host = t;
    }
    return CSX_OK;
}

// ------------------------------------------------------ column expansion ----
__global__ __launch_bounds__(256) void k_expand_columns(const int32_t *Ap, int32_t n, int32_t *col) {
    const int lane = threadIdx.x & 63;
    int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t j = wave; j < n; j += nwaves) {
        int32_t b = Ap[j], e = Ap[j + 1];
        for (int32_t p = b + lane; p < e; p += 64) col[p] = (int32_t)j;
    }
}

constexpr int EXPAND_GRID_MAX = 65536;   // workgroups of four waves; more columns than that wrap in the kernel's loop

int expand_columns(const int32_t *Ap, int32_t n, int32_t nnz, int32_t *col) {
    if (n == 0 || nnz == 0) return CSX_OK;
    int64_t blocks = ((int64_t)n + 3) / 4;
    if (blocks > EXPAND_GRID_MAX) blocks = EXPAND_GRID_MAX;
    hipLaunchKernelGGL(k_expand_columns, dim3((unsigned)blocks), dim3(256), 0, ctx().stream, Ap, n, col);
    CSX_LAUNCH_CHECK();
    return CSX_OK;
}

// ---------------------------------------------------------- radix sort ----
constexpr int RS_THREADS = 256;
constexpr int RS_WAVES = RS_THREADS / 64;
constexpr int RS_ROUNDS = 8;
constexpr int RS_TILE = RS_THREADS * RS_ROUNDS;  // records per workgroup
constexpr int RS_BINS = 256;

// Between two passes a record with both payloads travels as its key (4 bytes, an array of its own: the next pass's
// histogram reads nothing else) and (a, v) packed into 12 bytes: a tile's run in a bucket is then 16 x 12 = 192
// contiguous bytes instead of 64 + 128 in two places, and runs below 128 bytes are what slows a scatter down
// (tools/ubench/scatter_runs.hip: 64-byte runs 81 %, 32-byte runs 49 % of the rate of 128-byte runs).
struct __attribute__((packed, aligned(4))) Pay {
    uint32_t a, vlo, vhi;
};

// hist[tile][digit]: one coalesced 1 KiB row per tile
__global__ __launch_bounds__(RS_THREADS) void k_rs_hist(const uint32_t *key, int64_t count, int shift, uint32_t mask,
                                                        int32_t *hist) {
    __shared__ int h[RS_BINS];
    h[threadIdx.x] = 0;
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * RS_TILE;
    if (base + RS_TILE <= count && (reinterpret_cast<uintptr_t>(key) & 15) == 0) {
        // full tile: 16-byte loads, a wave instruction covers 1 KiB (the order of the keys does not matter here)
        typedef uint32_t u32x4h __attribute__((ext_vector_type(4)));
        const u32x4h *k4 = reinterpret_cast<const u32x4h *>(key + base);
        u32x4h v[RS_ROUNDS / 4];
#pragma unroll
        for (int r = 0; r < RS_ROUNDS / 4; r++) v[r] = k4[r * RS_THREADS + threadIdx.x];
#pragma unroll
        for (int r = 0; r < RS_ROUNDS / 4; r++) {
            atomicAdd(&h[(v[r].x >> shift) & mask], 1);
            atomicAdd(&h[(v[r].y >> shift) & mask], 1);
            atomicAdd(&h[(v[r].z >> shift) & mask], 1);
            atomicAdd(&h[(v[r].w >> shift) & mask], 1);
        }
    } else {
#pragma unroll 4
        for (int r = 0; r < RS_ROUNDS; r++) {
            int64_t idx = base + (int64_t)r * RS_THREADS + threadIdx.x;
            if (idx < count) atomicAdd(&h[(key[idx] >> shift) & mask], 1);
        }
    }
    __syncthreads();
    hist[(size_t)blockIdx.x * RS_BINS + threadIdx.x] = h[threadIdx.x];
}

// the same for 16-bit keys (the short-key mode of a transpose, see stable_sort_by_key_ex)
__global__ __launch_bounds__(RS_THREADS) void k_rs_hist16(const uint16_t *key, int64_t count, int shift, uint32_t mask,
                                                          int32_t *hist) {
    __shared__ int h[RS_BINS];
    h[threadIdx.x] = 0;
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * RS_TILE;
    if (base + RS_TILE <= count && (reinterpret_cast<uintptr_t>(key) & 15) == 0) {
        typedef uint32_t u32x2h __attribute__((ext_vector_type(2)));
        const u32x2h *k2 = reinterpret_cast<const u32x2h *>(key + base);      // four keys per load
        u32x2h v[RS_ROUNDS / 4];
#pragma unroll
        for (int r = 0; r < RS_ROUNDS / 4; r++) v[r] = k2[r * RS_THREADS + threadIdx.x];
#pragma unroll
        for (int r = 0; r < RS_ROUNDS / 4; r++) {
            const uint32_t w2[2] = {v[r].x, v[r].y};
#pragma unroll
            for (int q = 0; q < 2; q++) {
                atomicAdd(&h[((w2[q] & 0xffffu) >> shift) & mask], 1);
                atomicAdd(&h[((w2[q] >> 16) >> shift) & mask], 1);
            }
        }
    } else {
#pragma unroll 4
        for (int r = 0; r < RS_ROUNDS; r++) {
            int64_t idx = base + (int64_t)r * RS_THREADS + threadIdx.x;
            if (idx < count) atomicAdd(&h[((uint32_t)key[idx] >> shift) & mask], 1);
        }
    }
    __syncthreads();
    hist[(size_t)blockIdx.x * RS_BINS + threadIdx.x] = h[threadIdx.x];
}

// hist[tile][digit] -> goff[tile][digit] = records with a smaller digit + records with this digit in earlier tiles,
// i.e. the exclusive scan in (digit, tile) order, done on the tile-major matrix in three small steps: sums over
// chunks of tiles, one workgroup that scans the chunk sums in (digit, chunk) order, running sums inside a chunk.
__global__ __launch_bounds__(RS_BINS) void k_rs_colsum(const int32_t *hist, uint32_t nblocks, uint32_t chunk,
                                                       int32_t *part) {
    const uint32_t t0 = blockIdx.x * chunk, t1 = min(t0 + chunk, nblocks);
    int s = 0;
#pragma unroll 8
    for (uint32_t t = t0; t < t1; t++) s += hist[(size_t)t * RS_BINS + threadIdx.x];
    part[(size_t)blockIdx.x * RS_BINS + threadIdx.x] = s;
}

// one workgroup, thread = (segment of chunks, digit): running sums over the chunks per digit, and dbase[d] = records
// with a smaller digit
constexpr int RS_SEGS = 4;
__global__ __launch_bounds__(RS_BINS * RS_SEGS) void k_rs_chunkscan(int32_t *part, uint32_t nchunks, int32_t *dbase) {
    __shared__ int segsum[RS_SEGS][RS_BINS];
    const int d = threadIdx.x & (RS_BINS - 1), sg = threadIdx.x / RS_BINS;
    const uint32_t per = (nchunks + RS_SEGS - 1) / RS_SEGS;
    const uint32_t c0 = min(sg * per, nchunks), c1 = min(c0 + per, nchunks);
    int run = 0;
#pragma unroll 8
    for (uint32_t c = c0; c < c1; c++) run += part[(size_t)c * RS_BINS + d];
    segsum[sg][d] = run;
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int k = 0; k < RS_SEGS; k++) {
        const int v = segsum[k][d];
        if (k < sg) before += v;
        total += v;
    }
    run = before;
#pragma unroll 8
    for (uint32_t c = c0; c < c1; c++) {
        const int v = part[(size_t)c * RS_BINS + d];
        part[(size_t)c * RS_BINS + d] = run;
        run += v;
    }
    // exclusive scan of the digit totals by the first segment's threads (wave scans + 4 wave sums)
    __shared__ int wtot[RS_BINS / 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int inc = 0;
    if (sg == 0) {
        inc = wave_inclusive_scan(total, lane);
        if (lane == 63) wtot[w] = inc;
    }
    __syncthreads();
    if (sg == 0) {
        int off = 0;
#pragma unroll
        for (int k = 0; k < RS_BINS / 64; k++)
            if (k < w) off += wtot[k];
        dbase[d] = off + inc - total;
    }
}

__global__ __launch_bounds__(RS_BINS) void k_rs_tileprefix(int32_t *hist, const int32_t *part, const int32_t *dbase,
                                                           uint32_t nblocks, uint32_t chunk) {
    const uint32_t t0 = blockIdx.x * chunk, t1 = min(t0 + chunk, nblocks);
    int run = part[(size_t)blockIdx.x * RS_BINS + threadIdx.x] + dbase[threadIdx.x];
#pragma unroll 8
    for (uint32_t t = t0; t < t1; t++) {
        const int v = hist[(size_t)t * RS_BINS + threadIdx.x];
        hist[(size_t)t * RS_BINS + threadIdx.x] = run;
        run += v;
    }
}

// cs_transpose's first pass needs the column of every record.  One 512-byte descriptor per tile, written before the
// pass and read by the tile with a single load that depends on nothing: word 0 = j0, the column that holds the tile's
// first position (largest j with Ap[j] <= tile base); word 1 = K, the number of columns that start strictly inside the
// tile; then the first RS_DESC_STARTS of those starts, relative to the tile base, 16 bits each.
constexpr int RS_DESC_WORDS = 128;
constexpr int RS_DESC_STARTS = (RS_DESC_WORDS - 2) * 2;

__global__ void k_rs_tiledesc_head(const int32_t *Ap, int32_t n, int64_t count, uint32_t nblocks, uint32_t *desc) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nblocks) return;
    const int64_t tb = (int64_t)t * RS_TILE;
    int64_t te = tb + RS_TILE - 1;
    if (te > count - 1) te = count - 1;
    int32_t lo = 0, hi = n - 1;   // largest j with Ap[j] <= tb
    while (lo < hi) {
        const int32_t mid = lo + (hi - lo + 1) / 2;
        if ((int64_t)Ap[mid] <= tb) lo = mid;
        else hi = mid - 1;
    }
    const int32_t j0 = lo;
    hi = n - 1;                   // largest j with Ap[j] <= te (>= j0)
    while (lo < hi) {
        const int32_t mid = lo + (hi - lo + 1) / 2;
        if ((int64_t)Ap[mid] <= te) lo = mid;
        else hi = mid - 1;
    }
    desc[(size_t)t * RS_DESC_WORDS] = (uint32_t)j0;
    desc[(size_t)t * RS_DESC_WORDS + 1] = (uint32_t)(lo - j0);
}

__global__ void k_rs_tiledesc_starts(const int32_t *Ap, int32_t n, int64_t count, uint32_t *desc) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const int64_t p = Ap[j];
    if (p >= count) return;                       // empty columns at the end start in no tile
    const int64_t t = p / RS_TILE;
    const uint32_t rel = (uint32_t)(p - t * RS_TILE);
    if (rel == 0) return;                         // at the tile base: that is j0 or an empty column before it
    const int64_t k = j - (int64_t)desc[(size_t)t * RS_DESC_WORDS] - 1;
    if (k < RS_DESC_STARTS) reinterpret_cast<uint16_t *>(desc + (size_t)t * RS_DESC_WORDS + 2)[k] = (uint16_t)rel;
}

struct RsArgs {
    const uint32_t *key, *a;   // inputs: keys; 32-bit payload as an array (or none / expanded / inside pay)
    const double *v;           //         64-bit payload as an array
    const Pay *pay;            //         (a, v) records of the previous pass
    uint32_t *okey, *oa;       // outputs (okey may be null)
    double *ov;
    Pay *opay;
    const int32_t *goff;       // [tile][digit] global slot of the tile's first record with that digit
    const int32_t *xp;         // not null: a = column of the record's position under the column pointers xp
    const uint32_t *desc;      //           and the per-tile descriptors for it
    int32_t *optr;             // not null (last pass): optr[key] = min(position of a record with that key)
    int64_t count;
    int shift;
    uint32_t mask, nblocks;
    int flat;
    // short-key mode (KM != 0): 16-bit keys between the passes, the first digit riding in the top bits of `a`
    const uint16_t *key16;
    uint16_t *okey16;
    int k16_w0;                // bits of the first digit
};

// Stable scatter of one workgroup tile (RS_TILE = 2048 records).  Ranks follow (wave, round, lane) = source
// order.  Records are first placed in LDS in their sorted order inside the tile, then written out
// position by position: consecutive threads write consecutive slots of a bucket, so the stores are
// runs of whole 64/128-byte pieces instead of 4/8-byte singles.
// KM (short-key mode of a three-pass sort with derived columns -- a transpose): 0 = off; 1 = first pass: 32-bit keys in,
// key >> w0 out as 16 bits, the first digit packed into the top w0 bits of the column; 2 = middle pass: 16-bit keys in and
// out; 3 = last pass: 16-bit keys in, the column unpacked, the full key rebuilt for the pointer array.  Saves 2 bytes of
// every key read and written after the first digit is spent: 12 bytes per record over the three passes and their histograms.
template <bool HAS_A, bool HAS_V, bool IN_AOS, bool OUT_AOS, int KM = 0>
__global__ __launch_bounds__(RS_THREADS) void k_rs_scatter(const RsArgs g) {
    static_assert(!(IN_AOS || OUT_AOS) || (HAS_A && HAS_V), "packed records carry both payloads");
    __shared__ int wh[RS_WAVES][RS_BINS];
    __shared__ int gbase[RS_BINS];  // global slot of a bucket's first record minus its local start
    __shared__ uint32_t s_key[RS_TILE];
    int *const wsum = reinterpret_cast<int *>(s_key);   // (the scan's wave totals: s_key is idle between the counting and the placement)
    __shared__ __attribute__((aligned(16))) unsigned char s_raw[(HAS_A || HAS_V) ? (HAS_A ? 4 : 0) * RS_TILE + (HAS_V ? 8 : 0) * RS_TILE : 16];
    uint32_t *const s_a = reinterpret_cast<uint32_t *>(s_raw);
    double *const s_v = reinterpret_cast<double *>(s_raw + (HAS_A ? 4 * RS_TILE : 0));
    Pay *const s_pay = reinterpret_cast<Pay *>(s_raw);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t count = g.count;
    const int shift = g.shift;
    const uint32_t mask = g.mask, nblocks = g.nblocks;
#pragma unroll
    for (int k = 0; k < RS_WAVES; k++) wh[k][threadIdx.x] = 0;
    // Workgroups are dealt to the 8 XCDs round-robin; give each XCD a contiguous range of tiles, so that
    // neighbouring tiles -- whose runs in a bucket are adjacent in memory -- meet in the same L2 and the
    // partial lines at the run boundaries are merged there.
    uint32_t tile = blockIdx.x;
    if (!g.flat) {
        const uint32_t q = nblocks >> 3, rem = nblocks & 7u, x = blockIdx.x & 7u, kk = blockIdx.x >> 3;
        tile = x * q + (x < rem ? x : rem) + kk;
    }
    // wave w owns the contiguous sub-tile [w*64*ROUNDS, (w+1)*64*ROUNDS) of this workgroup's tile
    const int64_t tbase = (int64_t)tile * RS_TILE;
    const int64_t wbase = tbase + (int64_t)w * 64 * RS_ROUNDS;
    // the whole sub-tile goes to registers first: every load of the tile is in flight before the
    // (latency-bound) ranking rounds start, instead of one exposed round trip per round
    uint32_t kreg[RS_ROUNDS], areg[HAS_A ? RS_ROUNDS : 1];
    double vreg[HAS_V ? RS_ROUNDS : 1];
    // cs_transpose's first pass: the tile's descriptor is requested with the records
    const bool expand = HAS_A && !IN_AOS && g.xp != nullptr;
    uint32_t d0 = 0, d1 = 0;
    if (expand) {
        d0 = g.desc[(size_t)tile * RS_DESC_WORDS + lane];
        d1 = g.desc[(size_t)tile * RS_DESC_WORDS + 64 + lane];
    }
    // keys first, payloads after: loads return in order, so the counting and ranking below wait for the keys only and
    // the payloads keep arriving meanwhile (the barriers of this kernel order LDS, not global memory: lds_barrier)
#pragma unroll
    for (int r = 0; r < RS_ROUNDS; r++) {
        const int64_t idx = wbase + r * 64 + lane;
        kreg[r] = KM >= 2 ? (uint32_t)g.key16[idx < count ? idx : count - 1] : g.key[idx < count ? idx : count - 1];   // clamped: count > 0
    }
#pragma unroll
    for (int r = 0; r < RS_ROUNDS; r++) {
        const int64_t idx = wbase + r * 64 + lane;
        const int64_t cl = idx < count ? idx : count - 1;
        if (IN_AOS) {
            const Pay pr = g.pay[cl];
            areg[r] = pr.a;
            vreg[r] = __hiloint2double((int)pr.vhi, (int)pr.vlo);
        } else {
            if (HAS_A && !g.xp) areg[r] = g.a[cl];
            if (HAS_V) vreg[r] = g.v[cl];
        }
    }
    if (expand) {
        // the 32-bit payload is the record's column
        const int32_t j0 = __builtin_amdgcn_readlane((int)d0, 0), K = __builtin_amdgcn_readlane((int)d0, 1);
        const int32_t j1 = j0 + K;
        if (K <= RS_DESC_STARTS) {
            // every start is in the descriptor: wave w paints the positions of the columns w, w + 4, ... (and of j0,
            // which holds the positions before the first start) with their column, then each record reads its own
            uint32_t *const s_col = reinterpret_cast<uint32_t *>(s_raw);   // free until the ranking rounds
            const int wu = __builtin_amdgcn_readfirstlane(w);
            for (int c = wu - 1; c < K; c += RS_WAVES) {
                int b = 0, e = RS_TILE;
                if (c >= 0) {
                    const int h = c + 4;
                    const uint32_t wd = (h >> 1) < 64 ? (uint32_t)__builtin_amdgcn_readlane((int)d0, (h >> 1) & 63)
                                                      : (uint32_t)__builtin_amdgcn_readlane((int)d1, (h >> 1) & 63);
                    b = (int)((wd >> (16 * (h & 1))) & 0xffffu);
                }
                if (c + 1 < K) {
                    const int h = c + 5;
                    const uint32_t wd = (h >> 1) < 64 ? (uint32_t)__builtin_amdgcn_readlane((int)d0, (h >> 1) & 63)
                                                      : (uint32_t)__builtin_amdgcn_readlane((int)d1, (h >> 1) & 63);
                    e = (int)((wd >> (16 * (h & 1))) & 0xffffu);
                }
                for (int q = b + lane; q < e; q += 64) s_col[q] = (uint32_t)(j0 + 1 + c);
            }
            lds_barrier();
#pragma unroll
            for (int r = 0; r < RS_ROUNDS; r++) areg[r] = s_col[w * 64 * RS_ROUNDS + r * 64 + lane];
        } else if (K <= RS_TILE) {
            // many short columns: their starts are listed in LDS (s_key is free until the ranking rounds) and every
            // record counts the starts at or before its position, 16 searches side by side
            for (int k = threadIdx.x; k < K; k += RS_THREADS) s_key[k] = (uint32_t)((int64_t)g.xp[j0 + 1 + k] - tbase);
            lds_barrier();
            int lo[RS_ROUNDS];
#pragma unroll
            for (int r = 0; r < RS_ROUNDS; r++) lo[r] = 0;
            int top = 1;
            while (top * 2 <= K) top *= 2;
            for (int half = top; half > 0; half >>= 1) {
#pragma unroll
                for (int r = 0; r < RS_ROUNDS; r++) {
                    const uint32_t li = (uint32_t)(w * 64 * RS_ROUNDS + r * 64 + lane);
                    const int mid = lo[r] + half;
                    if (mid <= K && s_key[mid - 1] <= li) lo[r] = mid;
                }
            }
#pragma unroll
            for (int r = 0; r < RS_ROUNDS; r++) areg[r] = (uint32_t)(j0 + lo[r]);
        } else {  // a stretch of empty columns: search the pointer array itself
#pragma unroll 1
            for (int r = 0; r < RS_ROUNDS; r++) {
                const int64_t pos = wbase + r * 64 + lane;
                int32_t lo = j0, hi = j1;
                while (lo < hi) {
                    const int32_t mid = lo + (hi - lo + 1) / 2;
                    if ((int64_t)g.xp[mid] <= pos) lo = mid;
                    else hi = mid - 1;
                }
                areg[r] = (uint32_t)lo;
            }
        }
    }
    if (KM == 1) {
#pragma unroll
        for (int r = 0; r < RS_ROUNDS; r++) areg[r] |= (kreg[r] & mask) << (32 - g.k16_w0);   // the digit this pass spends
    }
    lds_barrier();
    // Counting and ranking share one multi-split per round: the lanes of a round that hold the same digit are found by
    // ballots (one per digit bit); the first of them adds the whole group to the wave's histogram, every lane keeps its
    // rank in the group for the placement below.  (One LDS atomic per lane instead -- the earlier form -- serialises when a
    // round's keys are clustered: the last pass of a transpose sees runs of 64 equal rows, 64 lanes on one counter.)
    const unsigned long long lt = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    int rk[RS_ROUNDS];   // rank in the group | group size << 8
#pragma unroll
    for (int r = 0; r < RS_ROUNDS; r++) {
        const int64_t idx = wbase + r * 64 + lane;
        const bool valid = idx < count;
        const uint32_t d = (kreg[r] >> shift) & mask;
        unsigned long long peers = __ballot(valid);
#pragma unroll
        for (int b = 0; b < 8; b++) {
            unsigned long long bal = __ballot((d >> b) & 1u);
            peers &= ((d >> b) & 1u) ? bal : ~bal;
        }
        const int rank = __popcll(peers & lt), cnt = __popcll(peers);
        rk[r] = rank | (cnt << 8);
        if (valid && rank == 0) atomicAdd(&wh[w][d], cnt);
    }
    lds_barrier();
    {
        // digit d = threadIdx.x: local start of the bucket inside the tile = exclusive scan over digits
        const int d = threadIdx.x;
        int tot = 0;
#pragma unroll
        for (int k = 0; k < RS_WAVES; k++) tot += wh[k][d];
        int inc = tot;
#pragma unroll
        for (int dd = 1; dd < 64; dd <<= 1) {
            int t = __shfl_up(inc, dd, 64);
            if (lane >= dd) inc += t;
        }
        if (lane == 63) wsum[w] = inc;
        lds_barrier();
        int off = 0;
#pragma unroll
        for (int k = 0; k < RS_WAVES; k++)
            if (k < w) off += wsum[k];
        int run = off + inc - tot;  // local start of bucket d
        gbase[d] = g.goff[(size_t)tile * RS_BINS + d] - run;
#pragma unroll
        for (int k = 0; k < RS_WAVES; k++) {
            int c = wh[k][d];
            wh[k][d] = run;
            run += c;
        }
    }
    lds_barrier();
#pragma unroll
    for (int r = 0; r < RS_ROUNDS; r++) {
        int64_t idx = wbase + r * 64 + lane;
        bool valid = idx < count;
        uint32_t k = kreg[r];
        uint32_t d = (k >> shift) & mask;
        const int rank = rk[r] & 255;
        int pos = 0;
        if (valid) pos = wh[w][d] + rank;
        __builtin_amdgcn_wave_barrier();
        if (valid && rank == 0) wh[w][d] = pos + (rk[r] >> 8);
        __builtin_amdgcn_wave_barrier();
        if (valid) {
            s_key[pos] = k;
            if (OUT_AOS) {
                Pay pr;
                pr.a = areg[r];
                pr.vlo = (uint32_t)__double2loint(vreg[r]);
                pr.vhi = (uint32_t)__double2hiint(vreg[r]);
                s_pay[pos] = pr;
            } else {
                if (HAS_A) s_a[pos] = areg[r];
                if (HAS_V) s_v[pos] = vreg[r];
            }
        }
    }
    lds_barrier();
    const int tcount = (int)((count - tbase) < RS_TILE ? (count - tbase) : RS_TILE);
    for (int i = threadIdx.x; i < tcount; i += RS_THREADS) {
        const uint32_t k = s_key[i];
        const int64_t gp = (int64_t)gbase[(k >> shift) & mask] + i;
        if (KM == 1) g.okey16[gp] = (uint16_t)(k >> g.k16_w0);
        else if (KM == 2) g.okey16[gp] = (uint16_t)k;
        else if (KM == 0 && g.okey) g.okey[gp] = k;
        if (OUT_AOS) {
            g.opay[gp] = s_pay[i];
        } else if (KM == 3) {
            // the column without the packed digit; the full key = the 16 bits that travelled and that digit
            const int ps = 32 - g.k16_w0;
            const uint32_t a = s_a[i], full = (k << g.k16_w0) | (a >> ps);
            g.oa[gp] = a & ((1u << ps) - 1u);
            if (HAS_V) g.ov[gp] = s_v[i];
            if (g.optr && (i == 0 || s_key[i - 1] != k || (s_a[i - 1] >> ps) != (a >> ps))) atomicMin(&g.optr[full], (int32_t)gp);
        } else {
            if (HAS_A) g.oa[gp] = s_a[i];
            if (HAS_V) g.ov[gp] = s_v[i];
        }
        // last pass: equal keys are neighbours in a bucket; the first of each group in this tile proposes its slot
        if (KM == 0 && g.optr && (i == 0 || s_key[i - 1] != k)) atomicMin(&g.optr[k], (int32_t)gp);
    }
}

// the instances of k_rs_scatter a sort can launch, as csx_prim_sort_info names them (include/csx.h)
enum RsInstance : int { RSI_NONE = 0, RSI_KEYS, RSI_A, RSI_V, RSI_AV_FLAT_FLAT, RSI_AV_FLAT_PACKED, RSI_AV_PACKED_PACKED,
                        RSI_AV_PACKED_FLAT, RSI_SHORT_FIRST, RSI_SHORT_MIDDLE, RSI_SHORT_LAST };

template <bool HAS_A, bool HAS_V>
static int launch_scatter(bool in_aos, bool out_aos, dim3 grid, hipStream_t s, const RsArgs &g) {
    if constexpr (HAS_A && HAS_V) {
        if (in_aos && out_aos) {
            hipLaunchKernelGGL((k_rs_scatter<true, true, true, true>), grid, dim3(RS_THREADS), 0, s, g);
            return RSI_AV_PACKED_PACKED;
        }
        if (in_aos) {
            hipLaunchKernelGGL((k_rs_scatter<true, true, true, false>), grid, dim3(RS_THREADS), 0, s, g);
            return RSI_AV_PACKED_FLAT;
        }
        if (out_aos) {
            hipLaunchKernelGGL((k_rs_scatter<true, true, false, true>), grid, dim3(RS_THREADS), 0, s, g);
            return RSI_AV_FLAT_PACKED;
        }
        hipLaunchKernelGGL((k_rs_scatter<true, true, false, false>), grid, dim3(RS_THREADS), 0, s, g);
        return RSI_AV_FLAT_FLAT;
    } else {
        hipLaunchKernelGGL((k_rs_scatter<HAS_A, HAS_V, false, false>), grid, dim3(RS_THREADS), 0, s, g);
        return HAS_A ? RSI_A : HAS_V ? RSI_V : RSI_KEYS;
    }
}

// read-back for the tests (host state only): what the last stable_sort_by_key_ex of this process decided, in the order of
// csx_prim_sort_info
constexpr int RS_MAX_PASSES = 4;
struct SortInfo {
    int64_t bits = 0, passes = 0, width[RS_MAX_PASSES] = {0, 0, 0, 0}, nblocks = 0, chunk = 0, nchunks = 0, packed = 0, k16 = 0,
            key_misalign = 0, instance[RS_MAX_PASSES] = {0, 0, 0, 0}, count = 0;
};
static SortInfo g_sort_info;

// ---- reverse running minimum: p[r] = min(p[r], ..., p[n-1]) (turns "first slot of each key" into column pointers) ----
constexpr int SM_ITEMS = 8;
constexpr int SM_TILE = SCAN_THREADS * SM_ITEMS;

__global__ __launch_bounds__(SCAN_THREADS) void k_sufmin_block(const int32_t *p, int64_t n, int32_t *bm) {
    __shared__ int wmin[SCAN_THREADS / 64];
    const int64_t base = (int64_t)blockIdx.x * SM_TILE;
    int m = 0x7fffffff;
#pragma unroll
    for (int k = 0; k < SM_ITEMS; k++) {
        const int64_t idx = base + (int64_t)k * SCAN_THREADS + threadIdx.x;
        if (idx < n) m = min(m, p[idx]);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) m = min(m, __shfl_xor(m, d, 64));
    if ((threadIdx.x & 63) == 0) wmin[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 1; k < SCAN_THREADS / 64; k++) m = min(m, wmin[k]);
        bm[blockIdx.x] = m;
    }
}

// bm_suffix: already the reverse running minimum of the block minima (or null for a single block)
__global__ __launch_bounds__(SCAN_THREADS) void k_sufmin_apply(int32_t *p, int64_t n, const int32_t *bm_suffix,
                                                               int64_t nb) {
    __shared__ int tmin[SCAN_THREADS];
    const int64_t base = (int64_t)blockIdx.x * SM_TILE + (int64_t)threadIdx.x * SM_ITEMS;
    int v[SM_ITEMS];
    int m = 0x7fffffff;
#pragma unroll
    for (int k = SM_ITEMS - 1; k >= 0; k--) {
        v[k] = (base + k < n) ? p[base + k] : 0x7fffffff;
        m = min(m, v[k]);
    }
    tmin[threadIdx.x] = m;
    __syncthreads();
    // minimum over the threads after this one: suffix scan over 256 values (Hillis-Steele in LDS)
    for (int d = 1; d < SCAN_THREADS; d <<= 1) {
        const int o = (threadIdx.x + d < SCAN_THREADS) ? tmin[threadIdx.x + d] : 0x7fffffff;
        __syncthreads();
        tmin[threadIdx.x] = min(tmin[threadIdx.x], o);
        __syncthreads();
    }
    int carry = (bm_suffix && (int64_t)blockIdx.x + 1 < nb) ? bm_suffix[blockIdx.x + 1] : 0x7fffffff;
    if (threadIdx.x + 1 < SCAN_THREADS) carry = min(carry, tmin[threadIdx.x + 1]);
#pragma unroll
    for (int k = SM_ITEMS - 1; k >= 0; k--) {
        carry = min(carry, v[k]);
        if (base + k < n) p[base + k] = carry;
    }
}

int suffix_min_i32(int32_t *p, int64_t n) {
    if (n <= 0) return CSX_OK;
    hipStream_t s = ctx().stream;
    const int64_t nb = (n + SM_TILE - 1) / SM_TILE;
    DevBuf<int32_t> bm;
    if (nb > 1) {
        CSX_TRY(bm.alloc((size_t)nb));
        hipLaunchKernelGGL(k_sufmin_block, dim3((unsigned)nb), dim3(SCAN_THREADS), 0, s, p, n, bm);
        CSX_LAUNCH_CHECK();
        CSX_TRY(suffix_min_i32(bm, nb));
    }
    hipLaunchKernelGGL(k_sufmin_apply, dim3((unsigned)nb), dim3(SCAN_THREADS), 0, s, p, n, bm, nb);
    CSX_LAUNCH_CHECK();
    if (bm) CSX_HIP(hipStreamSynchronize(s));  // bm is freed on return
    return CSX_OK;
}

__global__ void k_ptr_init(int32_t *ptr, int32_t nkeys, int32_t count) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nkeys) ptr[i] = 0x7fffffff;
    else if (i == nkeys) ptr[i] = count;
}

// the digit scan works on chunks of tiles: RS_CHUNK_DIV chunks at the most, none shorter than RS_CHUNK_MIN tiles
constexpr uint32_t RS_CHUNK_MIN = 64, RS_CHUNK_DIV = 1024;

int stable_sort_by_key_ex(const uint32_t *key, const uint32_t *a, const double *v, int64_t count, uint32_t key_limit,
                          uint32_t *out_key, uint32_t *out_a, double *out_v, const SortExtra *ex) {
    hipStream_t s = ctx().stream;
    const int32_t *xp = ex ? ex->expand_ptr : nullptr;
    int32_t *optr = ex ? ex->out_ptr : nullptr;
    if (optr) {
        const int64_t nk = (int64_t)ex->nkeys + 1;
        hipLaunchKernelGGL(k_ptr_init, dim3((unsigned)((nk + 255) / 256)), dim3(256), 0, s, optr, ex->nkeys,
                           (int32_t)(count > 0 ? count : 0));
        CSX_LAUNCH_CHECK();
    }
    g_sort_info = SortInfo();
    if (count <= 0) return optr ? suffix_min_i32(optr, (int64_t)ex->nkeys + 1) : CSX_OK;
    int bits = 1;
    while (bits < 32 && (1ull << bits) < (unsigned long long)key_limit) bits++;
    const int passes = (bits + 7) / 8;
    const uint32_t nblocks = (uint32_t)((count + RS_TILE - 1) / RS_TILE);
    uint32_t chunk = (nblocks + RS_CHUNK_DIV - 1) / RS_CHUNK_DIV;
    if (chunk < RS_CHUNK_MIN) chunk = RS_CHUNK_MIN;
    const uint32_t nchunks = (nblocks + chunk - 1) / chunk;
    const bool has_a = a != nullptr || xp != nullptr, has_v = v != nullptr;
    const bool packed = has_a && has_v;   // (a, v) travel as 12-byte records between passes
    // Short keys (a transpose with values of a matrix with fewer than 2^(32 - w0) columns and 17 .. 24 key bits): after the
    // first pass has spent its digit the keys travel as 16 bits, that digit in the top bits of the column word.
    const int w0 = bits / passes + (0 < bits % passes ? 1 : 0);
    const bool k16 = xp != nullptr && packed && passes == 3 && optr != nullptr && out_key == nullptr && bits - w0 <= 16 &&
                     (uint64_t)ex->expand_n <= (1ull << (32 - w0)) && ctx().opt.sort_short_keys;
    SortInfo &info = g_sort_info;
    info.bits = bits;
    info.passes = passes;
    info.nblocks = nblocks;
    info.chunk = chunk;
    info.nchunks = nchunks;
    info.packed = packed ? 1 : 0;
    info.k16 = k16 ? 1 : 0;
    info.key_misalign = (int64_t)((reinterpret_cast<uintptr_t>(key) & 15) / sizeof(uint32_t));
    info.count = count;

    DevBuf<int32_t> hist, part;
    DevBuf<uint32_t> desc;
    DevBuf<uint32_t> tk[2], ta[2];
    DevBuf<double> tv[2];
    DevBuf<Pay> tp[2];
    DevBuf<uint16_t> tk16[2];
    CSX_TRY(hist.alloc((size_t)RS_BINS * nblocks));
    CSX_TRY(part.alloc((size_t)RS_BINS * (nchunks + 1)));
    int32_t *const dbase = part + (size_t)RS_BINS * nchunks;
    if (xp) CSX_TRY(desc.alloc((size_t)nblocks * RS_DESC_WORDS));
    const int ntmp = passes > 2 ? 2 : passes - 1;
    for (int t = 0; t < ntmp; t++) {
        if (k16) CSX_TRY(tk16[t].alloc((size_t)count + 8));
        else CSX_TRY(tk[t].alloc((size_t)count));
        if (packed) {
            CSX_TRY(tp[t].alloc((size_t)count));
        } else {
            if (has_a) CSX_TRY(ta[t].alloc((size_t)count));
            if (has_v) CSX_TRY(tv[t].alloc((size_t)count));
        }
    }
    if (xp) {
        hipLaunchKernelGGL(k_rs_tiledesc_head, dim3((nblocks + 255) / 256), dim3(256), 0, s, xp, ex->expand_n, count, nblocks,
                           desc);
        CSX_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_rs_tiledesc_starts, dim3((unsigned)(((int64_t)ex->expand_n + 255) / 256)), dim3(256), 0, s, xp,
                           ex->expand_n, count, desc);
        CSX_LAUNCH_CHECK();
    }
    RsArgs g{};
    g.key = key;
    g.a = a;
    g.v = v;
    g.xp = xp;
    g.desc = desc;
    g.count = count;
    g.nblocks = nblocks;
    g.flat = ablation_env("CSX_SORT_FLAT") ? 1 : 0;
    bool in_aos = false;
    int shift = 0;
    for (int ps = 0; ps < passes; ps++) {
        const bool last = ps == passes - 1;
        const int width = bits / passes + (ps < bits % passes ? 1 : 0);   // digits as even as the key allows
        const bool out_aos = packed && !last;
        g.shift = shift;
        g.mask = (1u << width) - 1u;
        g.okey = last ? out_key : tk[ps & 1];
        g.oa = last ? out_a : ta[ps & 1];
        g.ov = last ? out_v : tv[ps & 1];
        g.opay = last ? nullptr : tp[ps & 1];
        g.optr = last ? optr : nullptr;
        g.goff = hist;
        if (k16) {
            g.k16_w0 = w0;
            g.okey16 = last ? nullptr : tk16[ps & 1];
            g.okey = nullptr;
            if (ps > 0) g.shift = shift - w0;            // in the 16-bit key the first digit is gone
        }
        if (k16 && ps > 0) hipLaunchKernelGGL(k_rs_hist16, dim3(nblocks), dim3(RS_THREADS), 0, s, g.key16, count, g.shift, g.mask, hist);
        else hipLaunchKernelGGL(k_rs_hist, dim3(nblocks), dim3(RS_THREADS), 0, s, g.key, count, g.shift, g.mask, hist);
        hipLaunchKernelGGL(k_rs_colsum, dim3(nchunks), dim3(RS_BINS), 0, s, hist, nblocks, chunk, part);
        hipLaunchKernelGGL(k_rs_chunkscan, dim3(1), dim3(RS_BINS * RS_SEGS), 0, s, part, nchunks, dbase);
        hipLaunchKernelGGL(k_rs_tileprefix, dim3(nchunks), dim3(RS_BINS), 0, s, hist, part, dbase, nblocks, chunk);
        int inst;
        if (k16 && ps == 0) {
            hipLaunchKernelGGL((k_rs_scatter<true, true, false, true, 1>), dim3(nblocks), dim3(RS_THREADS), 0, s, g);
            inst = RSI_SHORT_FIRST;
        } else if (k16 && !last) {
            hipLaunchKernelGGL((k_rs_scatter<true, true, true, true, 2>), dim3(nblocks), dim3(RS_THREADS), 0, s, g);
            inst = RSI_SHORT_MIDDLE;
        } else if (k16) {
            hipLaunchKernelGGL((k_rs_scatter<true, true, true, false, 3>), dim3(nblocks), dim3(RS_THREADS), 0, s, g);
            inst = RSI_SHORT_LAST;
        } else if (has_a && has_v) inst = launch_scatter<true, true>(in_aos, out_aos, dim3(nblocks), s, g);
        else if (has_a) inst = launch_scatter<true, false>(false, false, dim3(nblocks), s, g);
        else if (has_v) inst = launch_scatter<false, true>(false, false, dim3(nblocks), s, g);
        else inst = launch_scatter<false, false>(false, false, dim3(nblocks), s, g);
        CSX_LAUNCH_CHECK();
        info.width[ps] = width;
        info.instance[ps] = inst;
        g.key = g.okey;
        g.key16 = g.okey16;
        g.a = g.oa;
        g.v = g.ov;
        g.pay = g.opay;
        g.xp = nullptr;
        in_aos = out_aos;
        shift += width;
    }
    if (optr) CSX_TRY(suffix_min_i32(optr, (int64_t)ex->nkeys + 1));
    CSX_HIP(hipStreamSynchronize(s));   // the temporaries go back now
    return CSX_OK;
}

int stable_sort_by_key(const uint32_t *key, const uint32_t *a, const double *v, int64_t count, uint32_t key_limit,
                       uint32_t *out_key, uint32_t *out_a, double *out_v) {
    return stable_sort_by_key_ex(key, a, v, count, key_limit, out_key, out_a, out_v, nullptr);
}

// ----------------------------------------------------------- boundaries ----
// position q (0..count) closes the keys (sorted_key[q-1], sorted_key[q]]: ptr[r] = q for those r.
// Four positions per thread through one 16-byte load (boundaries are rare, the key stream is the cost).
__global__ __launch_bounds__(256) void k_boundaries(const uint32_t *skey, int64_t count, int32_t nkeys, int32_t *ptr) {
    typedef uint32_t u32x4b __attribute__((ext_vector_type(4)));
    const int64_t q0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (q0 > count) return;
    int64_t prev = (q0 == 0) ? -1 : (int64_t)skey[q0 - 1];
    if (q0 + 4 <= count && (reinterpret_cast<uintptr_t>(skey) & 15) == 0) {
        const u32x4b v = *reinterpret_cast<const u32x4b *>(skey + q0);
        const uint32_t k4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int64_t cur = (int64_t)k4[k];
            for (int64_t r = prev + 1; r <= cur; r++) ptr[r] = (int32_t)(q0 + k);
            prev = cur;
        }
        return;
    }
    const int64_t qend = q0 + 4 <= count ? q0 + 4 : count + 1;   // the last, partial group closes with q = count
    for (int64_t q = q0; q < qend; q++) {
        const int64_t cur = (q == count) ? (int64_t)nkeys : (int64_t)skey[q];
        for (int64_t r = prev + 1; r <= cur; r++) ptr[r] = (int32_t)q;
        prev = cur;
    }
}

int boundaries_from_sorted(const uint32_t *sorted_key, int64_t count, int32_t nkeys, int32_t *ptr) {
    const int64_t threads = count / 4 + 1;
    const int64_t blocks = (threads + 255) / 256;
    hipLaunchKernelGGL(k_boundaries, dim3((unsigned)blocks), dim3(256), 0, ctx().stream, sorted_key, count, nkeys, ptr);
    CSX_LAUNCH_CHECK();
    return CSX_OK;
}

}  // namespace csx

using namespace csx;

extern "C" int csx_cumsum(csx_handle_t hp, csx_handle_t hc, int64_t n, int64_t *total) {
    CSX_TRY(require_ready());
    Vec *p = ivec(hp), *c = ivec(hc);
    if (!p || !c || n < 0 || p->len < n + 1 || c->len < n) return CSX_EINVAL;
    CSX_TRY(scan_exclusive_i32((const int32_t *)c->d, (int32_t *)p->d, n, total));
    if (n)
        CSX_HIP(hipMemcpyAsync(c->d, p->d, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToDevice, ctx().stream));
    return CSX_OK;
}

// ---- read-backs and entry points for the tests (include/csx.h has the field lists) ----------------------------------------------
// Each csx_prim_* copies its host arrays to device buffers, runs the one primitive as its callers run it and copies the results
// back; the device copies of the INPUTS are copied back over the host arrays too, so that a primitive that wrote to an input
// shows.  Arguments a primitive would index memory with (pointer arrays, keys under a pointer output) are checked on the host
// first.  None of this is on a path production code takes.
extern "C" int csx_prim_limits(int32_t *out) {   // (no device needed)
    if (!out) return CSX_EINVAL;
    const int32_t v[9] = {SCAN_TILE, SM_TILE, RS_TILE, RS_BINS, RS_DESC_STARTS, RS_SEGS, (int32_t)RS_CHUNK_MIN, (int32_t)RS_CHUNK_DIV,
                          EXPAND_GRID_MAX};
    for (int k = 0; k < 9; k++) out[k] = v[k];
    return CSX_OK;
}

extern "C" int csx_prim_sort_info(int64_t *out, int32_t cap) {   // (host state only)
    if (!out || cap < 0) return CSX_EINVAL;
    const SortInfo &f = g_sort_info;
    const int64_t v[] = {f.bits, f.passes, f.width[0], f.width[1], f.width[2], f.width[3], f.nblocks, f.chunk, f.nchunks, f.packed,
                         f.k16, f.key_misalign, f.instance[0], f.instance[1], f.instance[2], f.instance[3], f.count};
    const int32_t nf = (int32_t)(sizeof v / sizeof v[0]);
    for (int32_t k = 0; k < nf && k < cap; k++) out[k] = v[k];
    return CSX_OK;
}

namespace {
template <class T>
int to_host(T *h, const T *d, size_t count) {
    if (count) CSX_HIP(hipMemcpyAsync(h, d, count * sizeof(T), hipMemcpyDeviceToHost, ctx().stream));
    return CSX_OK;
}
template <class T>
int to_device(T *d, const T *h, size_t count) {
    if (count) CSX_HIP(hipMemcpyAsync(d, h, count * sizeof(T), hipMemcpyHostToDevice, ctx().stream));
    return CSX_OK;
}
// room for count keys that start `words` 4-byte words past a 16-byte boundary
int alloc_misaligned(DevBuf<uint32_t> &buf, size_t count, int words, uint32_t **keys) {
    CSX_TRY(buf.alloc(count + 8));
    const uintptr_t base = (reinterpret_cast<uintptr_t>(buf.get()) + 15) & ~(uintptr_t)15;
    *keys = reinterpret_cast<uint32_t *>(base) + words;
    return CSX_OK;
}
// An output array with PRIM_GUARD bytes of a known pattern behind it: a primitive that stored past the end of an output is an
// error of the call, not a silent store into the slack of the pool's block.
constexpr size_t PRIM_GUARD = 256;
template <class T>
struct GuardedOut {
    DevBuf<T> d;
    size_t count = 0;
    unsigned char seen[PRIM_GUARD];
    int put(const T *h, size_t n) {   // the caller's contents first: slots a primitive leaves alone keep them
        count = n;
        CSX_TRY(d.alloc(n + PRIM_GUARD / sizeof(T)));
        CSX_TRY(to_device(d.get(), h, n));
        CSX_HIP(hipMemsetAsync(d.get() + n, 0xA5, PRIM_GUARD, ctx().stream));
        return CSX_OK;
    }
    int take(T *h) {   // enqueues the copies back; intact() holds once the stream is synchronised
        CSX_TRY(to_host(h, (const T *)d.get(), count));
        CSX_HIP(hipMemcpyAsync(seen, d.get() + count, PRIM_GUARD, hipMemcpyDeviceToHost, ctx().stream));
        return CSX_OK;
    }
    bool intact() const {
        for (size_t k = 0; k < PRIM_GUARD; k++)
            if (seen[k] != 0xA5) return false;
        return true;
    }
};
int guard_verdict(bool intact, const char *what) {
    if (intact) return CSX_OK;
    set_error("%s: a store past the end of an output array", what);
    return CSX_ERUNTIME;
}
// column pointers of n columns over exactly `count` positions
bool pointers_ok(const int32_t *p, int64_t n, int64_t count) {
    if (p[0] != 0 || (int64_t)p[n] != count) return false;
    for (int64_t j = 0; j < n; j++)
        if (p[j] > p[j + 1]) return false;
    return true;
}
}  // namespace

extern "C" int csx_prim_scan(int32_t *in, int32_t *out, int64_t n, int in_place, int64_t *total) {
    if (n < 0 || !out || (n > 0 && !in)) return CSX_EINVAL;
    CSX_TRY(require_ready());
    DevBuf<int32_t> din;
    GuardedOut<int32_t> dout;
    CSX_TRY(dout.put(out, (size_t)n + 1));
    if (in_place) {
        CSX_TRY(to_device(dout.d.get(), (const int32_t *)in, (size_t)n));
        CSX_TRY(scan_exclusive_i32(dout.d, dout.d, n, total));
    } else {
        CSX_TRY(upload(din, (const int32_t *)in, (size_t)n));
        CSX_TRY(scan_exclusive_i32(din, dout.d, n, total));
        CSX_TRY(to_host(in, (const int32_t *)din.get(), (size_t)n));
    }
    CSX_TRY(dout.take(out));
    CSX_HIP(hipStreamSynchronize(ctx().stream));
    return guard_verdict(dout.intact(), "csx_prim_scan");
}

extern "C" int csx_prim_suffix_min(int32_t *p, int64_t n) {
    if (n < 0 || (n > 0 && !p)) return CSX_EINVAL;
    CSX_TRY(require_ready());
    GuardedOut<int32_t> d;
    CSX_TRY(d.put(p, (size_t)n));
    CSX_TRY(suffix_min_i32(d.d, n));
    CSX_TRY(d.take(p));
    CSX_HIP(hipStreamSynchronize(ctx().stream));
    return guard_verdict(d.intact(), "csx_prim_suffix_min");
}

extern "C" int csx_prim_expand_columns(int32_t *Ap, int32_t n, int32_t nnz, int32_t *col) {
    if (n < 0 || nnz < 0 || !Ap || (nnz > 0 && !col) || !pointers_ok(Ap, n, nnz)) return CSX_EINVAL;
    CSX_TRY(require_ready());
    DevBuf<int32_t> dp;
    GuardedOut<int32_t> dc;
    CSX_TRY(upload(dp, (const int32_t *)Ap, (size_t)n + 1));
    CSX_TRY(dc.put(col, (size_t)nnz));
    CSX_TRY(expand_columns(dp, n, nnz, dc.d));
    CSX_TRY(to_host(Ap, (const int32_t *)dp.get(), (size_t)n + 1));
    CSX_TRY(dc.take(col));
    CSX_HIP(hipStreamSynchronize(ctx().stream));
    return guard_verdict(dc.intact(), "csx_prim_expand_columns");
}

extern "C" int csx_prim_boundaries(uint32_t *sorted_key, int64_t count, int32_t nkeys, int32_t *ptr, int misalign_words) {
    if (count < 0 || nkeys < 0 || !ptr || (count > 0 && !sorted_key) || misalign_words < 0 || misalign_words > 3) return CSX_EINVAL;
    for (int64_t q = 0; q < count; q++)   // sorted keys in [0, nkeys): the kernel writes ptr[key]
        if (sorted_key[q] >= (uint32_t)nkeys || (q > 0 && sorted_key[q - 1] > sorted_key[q])) return CSX_EINVAL;
    CSX_TRY(require_ready());
    DevBuf<uint32_t> kbuf;
    GuardedOut<int32_t> dp;
    uint32_t *dk = nullptr;
    CSX_TRY(alloc_misaligned(kbuf, (size_t)count, misalign_words, &dk));
    CSX_TRY(to_device(dk, (const uint32_t *)sorted_key, (size_t)count));
    CSX_TRY(dp.put(ptr, (size_t)nkeys + 1));
    CSX_TRY(boundaries_from_sorted(dk, count, nkeys, dp.d));
    CSX_TRY(to_host(sorted_key, (const uint32_t *)dk, (size_t)count));
    CSX_TRY(dp.take(ptr));
    CSX_HIP(hipStreamSynchronize(ctx().stream));
    return guard_verdict(dp.intact(), "csx_prim_boundaries");
}

extern "C" int csx_prim_sort(uint32_t *key, uint32_t *a, double *v, int64_t count, uint32_t key_limit, uint32_t *out_key,
                             uint32_t *out_a, double *out_v, int32_t *expand_ptr, int32_t expand_n, int32_t *out_ptr, int32_t nkeys,
                             int misalign_words) {
    if (count < 0 || (count > 0 && !key) || misalign_words < 0 || misalign_words > 3) return CSX_EINVAL;
    if (((a || expand_ptr) && !out_a) || (v && !out_v)) return CSX_EINVAL;   // an output missing where its input is given
    if (a && expand_ptr) return CSX_EINVAL;   // the 32-bit payload is given or derived, not both
    if (expand_ptr && (expand_n < 1 || !pointers_ok(expand_ptr, expand_n, count))) return CSX_EINVAL;
    if (out_ptr) {
        if (nkeys < 0) return CSX_EINVAL;
        for (int64_t q = 0; q < count; q++)   // the last pass writes out_ptr[key]
            if (key[q] >= (uint32_t)nkeys) return CSX_EINVAL;
    }
    CSX_TRY(require_ready());
    hipStream_t s = ctx().stream;
    const size_t cnt = (size_t)count;
    DevBuf<uint32_t> kbuf, da;
    DevBuf<double> dv;
    DevBuf<int32_t> dxp;
    GuardedOut<uint32_t> dok, doa;
    GuardedOut<double> dov;
    GuardedOut<int32_t> dop;
    uint32_t *dk = nullptr;
    CSX_TRY(alloc_misaligned(kbuf, cnt, misalign_words, &dk));
    CSX_TRY(to_device(dk, (const uint32_t *)key, cnt));
    if (a) CSX_TRY(upload(da, (const uint32_t *)a, cnt));
    if (v) CSX_TRY(upload(dv, (const double *)v, cnt));
    if (expand_ptr) CSX_TRY(upload(dxp, (const int32_t *)expand_ptr, (size_t)expand_n + 1));
    const bool with_a = a || expand_ptr;
    if (out_key) CSX_TRY(dok.put(out_key, cnt));
    if (with_a) CSX_TRY(doa.put(out_a, cnt));
    if (v) CSX_TRY(dov.put(out_v, cnt));
    if (out_ptr) CSX_TRY(dop.put(out_ptr, (size_t)nkeys + 1));
    const SortExtra ex{expand_ptr ? dxp.get() : nullptr, expand_n, out_ptr ? dop.d.get() : nullptr, nkeys};
    CSX_TRY(stable_sort_by_key_ex(dk, a ? da.get() : nullptr, v ? dv.get() : nullptr, count, key_limit, out_key ? dok.d.get() : nullptr,
                                  with_a ? doa.d.get() : nullptr, v ? dov.d.get() : nullptr, (expand_ptr || out_ptr) ? &ex : nullptr));
    CSX_TRY(to_host(key, (const uint32_t *)dk, cnt));
    if (a) CSX_TRY(to_host(a, (const uint32_t *)da.get(), cnt));
    if (v) CSX_TRY(to_host(v, (const double *)dv.get(), cnt));
    if (expand_ptr) CSX_TRY(to_host(expand_ptr, (const int32_t *)dxp.get(), (size_t)expand_n + 1));
    if (out_key) CSX_TRY(dok.take(out_key));
    if (with_a) CSX_TRY(doa.take(out_a));
    if (v) CSX_TRY(dov.take(out_v));
    if (out_ptr) CSX_TRY(dop.take(out_ptr));
    CSX_HIP(hipStreamSynchronize(s));
    return guard_verdict((!out_key || dok.intact()) && (!with_a || doa.intact()) && (!v || dov.intact()) && (!out_ptr || dop.intact()),
                         "csx_prim_sort");
}
