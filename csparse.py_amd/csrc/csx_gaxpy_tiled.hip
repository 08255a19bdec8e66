// cs_gaxpy (csparse.py:1199-1213), LDS-resident plan for matrices whose rows share
// no columns (uniformly random structure, the "G-rand" benchmark input).
//
// Why: with y and x of 40 MB each (n = 5e6) every one of the 3.2e8 entries of A
// makes one random 8-byte access to a vector that fits neither LDS nor an XCD's
// 4 MiB L2.  Gathering x row by row fetches a 128-byte line per entry; scattering
// into y needs memory-side atomics.  Both run far below the HBM rate.
//
// Plan: regroup the entries once (stable radix sort, csx_sort.hip) into tiles
//      tile(b, s) = { A(i, j) : i in row block b, j in column slab s },
// row-block-major, column order kept inside a tile.
//   * One workgroup owns one row block for the whole kernel: its slice of y
//     (m / 256 rows, up to 156 KiB) is loaded into LDS once, takes every random
//     accumulation as ds_add_f64, and is written back once.  No partial sums in
//     memory, no second kernel, no inter-workgroup communication.  With 3-byte
//     keys the tile moves in and out in bulk: eight 16-byte loads (LDS reads) per
//     thread in flight before the first wait.
//   * All workgroups walk the column slabs in the same order and at the same
//     pace (equal work per tile for a random matrix), so the slab of x in use
//     (<= 1 MiB) is shared through each XCD's L2.
//   * Entries are stored in groups of 256 (tiles padded to a multiple of 256),
//     INTERLEAVED so that the 16-byte key load of lane l returns entries
//     l, l+64, l+128, l+192 of the group: the k-th gather instruction of a wave
//     then covers 64 CONSECUTIVE entries of the column-sorted tile, i.e. ~16
//     cache lines of x instead of 64.  Measured: the texture addresser handles
//     about one distinct line per clock, and with 4 consecutive entries per lane
//     the gathers alone cost 0.6 ms of a 1.3 ms kernel (profiles/ablation_r01.md).
//   * The entry stream (4-byte packed (col,row) key + 8-byte value = the same 12
//     bytes per entry as CSC) is read once, coalesced, non-temporal, one step ahead:
//     a step issues its gathers, puts the key and value loads of the next step
//     behind them and waits for the gathers alone (TiledStep::step).  A step whose
//     groups all exist -- all but a row block's last -- runs without a test or a
//     branch: the walk is decided by scalar compares on wave-uniform counters.
//     (Keys TWO steps ahead, in a ring of three key sets, were built and measured:
//     slower.  They live on in the ablation build; profiles/tiled_pipeline_ablation.md.)
//   * 3-byte keys.  A gather instruction covers 64 consecutive entries of the column-sorted tile; when every such
//     run spans fewer than 512 columns (always, for a matrix like G-rand: a run spans 256 +- 32) an entry needs its
//     row in the block (15 bits) and its column's offset from the run's first column (9 bits): 3 bytes, the run's
//     base column being four words per group of 256.  The stream is then 11 bytes per entry instead of 12.  A matrix
//     with a wider run anywhere keeps the 4-byte keys.
//
// HBM bytes per call ~ 12 nnz (+0.4 % padding) + 16 m + 8 n * (#XCDs that read x).
#include <cstdint>
#include <cstdlib>

#include "csx_internal.h"

namespace csx {

constexpr int TL_WAVES = 4, TL_NG = 5;          // waves per workgroup, groups per wave and step of the shipped kernel (see k_gaxpy_tiled)
constexpr int TL_GROUP = 256;                   // entries per group = 64 lanes x 4
constexpr int TL_LDS_BYTES = 160 * 1024 - 256;  // leave a little headroom below the CU's 160 KiB
constexpr int TL_LDS_ROWS = TL_LDS_BYTES / 8 - 2;  // y rows per tile (one slot is the padding dummy)
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x3 __attribute__((ext_vector_type(3)));
typedef u32x3 u32x3_a4 __attribute__((aligned(4)));    // the 12-byte key record of a lane: 4-byte aligned
typedef double f64x2 __attribute__((ext_vector_type(2)));

__global__ __launch_bounds__(256) void k_tile_keys(int64_t nnz, const int32_t *__restrict__ Ai,
                                                   const int32_t *__restrict__ col, int rb_bits, int32_t row_block,
                                                   int32_t slab_cols, int32_t nslab, uint32_t *__restrict__ tile_id,
                                                   uint32_t *__restrict__ packed) {
    int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= nnz) return;
    const uint32_t i = (uint32_t)Ai[p], j = (uint32_t)col[p];
    const uint32_t s = j / (uint32_t)slab_cols, lc = j - s * (uint32_t)slab_cols;
    const uint32_t b = i / (uint32_t)row_block, lr = i - b * (uint32_t)row_block;
    tile_id[p] = b * (uint32_t)nslab + s;
    packed[p] = (lc << rb_bits) | lr;
}

__global__ __launch_bounds__(256) void k_padded_lengths(int64_t ntiles, const int32_t *__restrict__ sptr,
                                                        int32_t *__restrict__ ngroups) {
    int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < ntiles) ngroups[t] = (sptr[t + 1] - sptr[t] + TL_GROUP - 1) / TL_GROUP;
}

// group_info[g] = (slab << 9) | entries in the group (1..256)
__global__ __launch_bounds__(256) void k_group_info(int64_t ntiles, int32_t nslab, const int32_t *__restrict__ sptr,
                                                    const int32_t *__restrict__ gptr, uint32_t *__restrict__ info) {
    int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= ntiles) return;
    const int32_t len = sptr[t + 1] - sptr[t];
    const uint32_t slab = (uint32_t)(t % nslab);
    int32_t g = gptr[t];
    for (int32_t left = len; left > 0; left -= TL_GROUP, g++) info[g] = (slab << 9) | (uint32_t)min(left, TL_GROUP);
}

// sorted position q (tile t, rank e inside the tile) -> interleaved slot
__global__ __launch_bounds__(256) void k_interleave(int64_t nnz, const uint32_t *__restrict__ stid,
                                                    const int32_t *__restrict__ sptr, const int32_t *__restrict__ gptr,
                                                    const uint32_t *__restrict__ skey, const double *__restrict__ sval,
                                                    uint32_t *__restrict__ okey, double *__restrict__ oval) {
    int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nnz) return;
    const uint32_t t = stid[q];
    const int32_t e = (int32_t)(q - sptr[t]);
    const int32_t g = e / TL_GROUP, w = e % TL_GROUP;
    // entry w of a group goes to lane l = w & 63, component k = w >> 6.  Keys: lane l's 16-byte
    // word (slots 4l..4l+3).  Values: two planes of 128 doubles, plane k >> 1, lane l's 16-byte
    // word (slots 2l, 2l+1) -- so that EACH value load instruction of a wave covers one contiguous
    // 1 KiB (whole 128-byte lines).  With values at slots 4l..4l+3 each instruction touched only
    // half of every line and issued twice as many (64-byte) requests.
    const int64_t gbase = ((int64_t)gptr[t] + g) * TL_GROUP;
    const int l = w & 63, k = w >> 6;
    if (okey) okey[gbase + l * 4 + k] = skey[q];
    oval[gbase + (k >> 1) * 128 + l * 2 + (k & 1)] = sval[q];
}

// 3-byte keys: is every run of 64 consecutive entries of a tile narrower than 512 columns?
__global__ __launch_bounds__(256) void k_run_span(int64_t nnz, const uint32_t *__restrict__ stid,
                                                  const int32_t *__restrict__ sptr, const uint32_t *__restrict__ skey,
                                                  int rb_bits, int *too_wide) {
    int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nnz) return;
    const int32_t e = (int32_t)(q - sptr[stid[q]]);
    const int64_t first = q - (e & 63);
    if ((skey[q] >> rb_bits) - (skey[first] >> rb_bits) >= 512u) *too_wide = 1;
}

// key24 of entry w of a group: bytes 12 l + 3 k .. + 2 of the group's 768 (lane l = w & 63, run k = w >> 6), value
// row | (column - first column of the run) << 15; base[4 g + k] = that first column
__global__ __launch_bounds__(256) void k_interleave24(int64_t nnz, const uint32_t *__restrict__ stid,
                                                      const int32_t *__restrict__ sptr, const int32_t *__restrict__ gptr,
                                                      const uint32_t *__restrict__ skey, int rb_bits,
                                                      uint8_t *__restrict__ okey, uint32_t *__restrict__ obase) {
    int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nnz) return;
    const uint32_t t = stid[q];
    const int32_t e = (int32_t)(q - sptr[t]);
    const int32_t g = e / TL_GROUP, w = e % TL_GROUP;
    const int l = w & 63, k = w >> 6;
    const uint32_t rmask = (1u << rb_bits) - 1u;
    const uint32_t col = skey[q] >> rb_bits, col0 = skey[q - l] >> rb_bits;
    const uint32_t v = (skey[q] & rmask) | ((col - col0) << 15);
    const int64_t gg = (int64_t)gptr[t] + g;
    uint8_t *o = okey + gg * (TL_GROUP * 3) + l * 12 + k * 3;
    o[0] = (uint8_t)v;
    o[1] = (uint8_t)(v >> 8);
    o[2] = (uint8_t)(v >> 16);
    if (l == 0) obase[gg * 4 + k] = col;
}

__global__ __launch_bounds__(256) void k_fill_key24(uint8_t *p, int64_t nslots, uint32_t v) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < nslots; i += stride) {
        p[3 * i] = (uint8_t)v;
        p[3 * i + 1] = (uint8_t)(v >> 8);
        p[3 * i + 2] = (uint8_t)(v >> 16);
    }
}

__global__ __launch_bounds__(256) void k_fill_keys(uint32_t *p, int64_t n, uint32_t v) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) p[i] = v;
}

// What a lane holds of a group of 256 entries, in two records that are loaded at different times: the key record a
// step's gathers need (and its atomics, for the row), the value record only its atomics need.
struct KeyRegs {
    u32x4 kk;      // 4-byte keys as stored; 3-byte keys: x, y, z = the lane's 12 bytes AS STORED (unpacked where they are
                   // used -- unpacking where they are loaded would wait for the load two steps early)
    u32x4 base;    // 3-byte keys: first column of the four runs
    uint32_t info;
};
struct ValRegs {
    f64x2 v0, v1;
};

// Parts of the step that the ablation build can switch off one by one (profiles/tiled_pipeline_ablation.md); the shipped
// library holds tl_parts(NW, NG) alone.
constexpr int TP_KEYS2 = 1;      // keys run two steps ahead of their gathers (three key sets); off: one step ahead (two sets)
constexpr int TP_FULLSTEP = 2;   // a step whose NG groups all exist takes a body without per-group tests
constexpr int TP_KEY12 = 4;      // the 12-byte record of 3-byte keys is ONE load
constexpr int TP_BULKTILE = 8;   // the y tile moves in batches of eight 16-byte accesses per thread
constexpr int TP_ALL = 15;

template <bool NT, bool K24, bool KEY12>
__device__ __forceinline__ KeyRegs load_keys_t(const uint32_t *__restrict__ key, const uint32_t *__restrict__ info,
                                               const uint32_t *__restrict__ base, int32_t g, int lane) {
    KeyRegs r;
    // (Tried: g = readfirstlane(g), which turns the group's info word and base record into scalar loads -- two of nine
    // vector memory instructions per group gone, same time, 2.4 % more bytes at the memory side.  Not kept.)
    if (K24) {
        // `key` is the byte array of 3-byte keys: 12 bytes per lane, 768 per group
        const uint32_t *kp = key + (int64_t)g * (TL_GROUP * 3 / 4) + 3 * lane;
        if (KEY12) {
            const u32x3 k = __builtin_nontemporal_load(reinterpret_cast<const u32x3_a4 *>(kp));
            r.kk.x = k.x;
            r.kk.y = k.y;
            r.kk.z = k.z;
        } else {
            r.kk.x = __builtin_nontemporal_load(kp);
            r.kk.y = __builtin_nontemporal_load(kp + 1);
            r.kk.z = __builtin_nontemporal_load(kp + 2);
        }
        r.kk.w = 0;
        r.base = *reinterpret_cast<const u32x4 *>(base + 4 * (int64_t)g);
    } else {
        const uint32_t *kp = key + (int64_t)g * TL_GROUP + 4 * lane;
        r.kk = NT ? __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(kp)) : *reinterpret_cast<const u32x4 *>(kp);
        r.base = u32x4{0, 0, 0, 0};
    }
    r.info = info[g];
    return r;
}

template <bool NT>
__device__ __forceinline__ ValRegs load_vals_t(const double *__restrict__ val, int32_t g, int lane) {
    ValRegs r;
    const f64x2 *vp = reinterpret_cast<const f64x2 *>(val + (int64_t)g * TL_GROUP + 2 * lane);
    r.v0 = NT ? __builtin_nontemporal_load(vp) : *vp;
    r.v1 = NT ? __builtin_nontemporal_load(vp + 64) : vp[64];
    return r;
}

// the four keys of a lane as row | column part << shift (3-byte keys: shift 15, column part = offset in the run)
template <bool K24>
__device__ __forceinline__ u32x4 unpack_keys(const KeyRegs &k) {
    if (!K24) return k.kk;
    const uint32_t ka = k.kk.x, kb = k.kk.y, kc = k.kk.z;
    u32x4 r;
    r.x = ka & 0xFFFFFFu;
    r.y = (ka >> 24) | ((kb & 0xFFFFu) << 8);
    r.z = (kb >> 16) | ((kc & 0xFFu) << 16);
    r.w = kc >> 8;
    return r;
}

// how x is gathered: 0 plain (L1-allocating), 1 sc1 (agent-scope relaxed: bypasses L1), 2 non-temporal
template <int HOW>
__device__ __forceinline__ double load_x(const double *p) {
    if (HOW == 1) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (HOW == 2) return __builtin_nontemporal_load(p);
    return *p;
}

// The y tile, global memory -> LDS.  Every thread has up to eight 16-byte loads in flight before it waits for the first
// (a row block of 19 532 rows is 5 batches for 256 threads, not 77 dependent round trips).  The pairs start at the first
// 16-byte-aligned address of the source; a row before it and a row after the last pair are moved singly.  The LDS
// address of a pair is 8-byte aligned only (odd when the source began odd): two 8-byte writes.  An index past the end
// is clamped to the last pair, for the load AND for the write (the last pair is then written more than once, with the
// same bytes): a batch holds no branch -- under a branch the compiler sinks a load to its use and waits for it alone.
// Eight pairs per thread and batch up to 256 threads, four with 512 (two waves per SIMD share the registers; either way
// 32 KiB per CU in flight).
constexpr int tile_batch(int threads) { return threads > 256 ? 4 : 8; }

template <int T>
__device__ __forceinline__ void tile_fill(double *ytile, const double *__restrict__ src, int32_t rows) {
    constexpr int NB = tile_batch(T);
    const int tid = threadIdx.x;
    const int32_t head = (rows > 0 && (reinterpret_cast<uintptr_t>(src) & 8)) ? 1 : 0;
    const int32_t npairs = (rows - head) >> 1;
    const f64x2 *s2 = reinterpret_cast<const f64x2 *>(src + head);
    double *d = ytile + head;
    for (int32_t p0 = 0; p0 < npairs; p0 += NB * T) {
        f64x2 v[NB];
        int32_t q[NB];
#pragma unroll
        for (int i = 0; i < NB; i++) {
            const int32_t p = p0 + i * T + tid;
            q[i] = p < npairs ? p : npairs - 1;
            v[i] = s2[q[i]];
        }
#pragma unroll
        for (int i = 0; i < NB; i++) {
            d[2 * q[i]] = v[i].x;
            d[2 * q[i] + 1] = v[i].y;
        }
    }
    if (tid == 0 && head) ytile[0] = src[0];
    if (tid == T - 1 && ((rows - head) & 1)) ytile[rows - 1] = src[rows - 1];
}

// ... and back: LDS reads batched, one wait per batch, 16-byte stores
template <int T>
__device__ __forceinline__ void tile_drain(const double *ytile, double *__restrict__ dst, int32_t rows) {
    const int tid = threadIdx.x;
    const int32_t head = (rows > 0 && (reinterpret_cast<uintptr_t>(dst) & 8)) ? 1 : 0;
    const int32_t npairs = (rows - head) >> 1;
    f64x2 *d2 = reinterpret_cast<f64x2 *>(dst + head);
    const double *s = ytile + head;
    constexpr int NB = tile_batch(T);
    for (int32_t p0 = 0; p0 < npairs; p0 += NB * T) {
        f64x2 v[NB];
        int32_t q[NB];
#pragma unroll
        for (int i = 0; i < NB; i++) {
            const int32_t p = p0 + i * T + tid;
            q[i] = p < npairs ? p : npairs - 1;
            v[i].x = s[2 * q[i]];
            v[i].y = s[2 * q[i] + 1];
        }
#pragma unroll
        for (int i = 0; i < NB; i++) d2[q[i]] = v[i];
    }
    if (tid == 0 && head) dst[0] = ytile[0];
    if (tid == T - 1 && ((rows - head) & 1)) dst[rows - 1] = ytile[rows - 1];
}

// The kernel.  NW waves per workgroup (one workgroup per CU), NG groups per wave and step.
// Measured on G-rand 5M x 5M (profiles/r02_ablation.md): FEWER waves are faster -- 16 waves 0.97 ms, 12 waves
// 0.83 ms, 8 waves 0.86 ms -- the x lines a wave's gathers bring into the 32 KiB L1 are shared by the
// neighbouring lanes' entries only if they survive until the whole gather instruction has been served, and
// the more waves stream through the same L1 the fewer do.
//
// VARIANT (timing experiments, compiled only with -DCSX_ABLATION; the shipped library holds VARIANT 0 alone).
// Results are wrong for variants 1, 3, 4, 5, 7:
//   1 = skip the x gather, 2 = full kernel with plain instead of nt stream loads, 3 = stream only,
//   4 = gather from a 2 KB footprint (L1 hits),
//   5 = gather from a 256 KB footprint (L2 hits, L1 misses)
//   6 = full kernel, x gathered with L1-bypassing sc1 loads (computes y)
//   7 = real x gathers, but the entry stream re-reads the first 32 groups of the row block (L2-resident)
// PARTS: the TP_ bits above (results are right for every value).
template <int VARIANT, int NW, int NG, bool K24, int PARTS>
struct TiledStep {
    static constexpr bool GATHER = !(VARIANT & 1) || VARIANT >= 5, ATOMIC = VARIANT != 3;
    static constexpr bool STREAM_NT = VARIANT != 2;
    static constexpr uint32_t CMASK = VARIANT == 5 ? 32767u : (VARIANT == 4 ? 255u : 0xffffffffu);
    static constexpr int XLOAD = VARIANT == 6 ? 1 : 0;
    static constexpr bool RING = VARIANT == 7;
    static constexpr int KD = (PARTS & TP_KEYS2) ? 2 : 1;   // steps the keys run ahead
    static constexpr int NK = KD + 1;                       // key sets: the one in use and KD in flight
    static constexpr int PERIOD = NK == 3 ? 6 : 2;          // steps after which key set AND value set repeat
    static constexpr int STRIDE = NG * NW;                  // groups a workgroup takes per step

    // The group a lane loads for position gq of the wave's walk: clamped to the row block's last group instead of
    // predicated, so that no branch stands round a stream load.  `gq` is wave-uniform (it decides the branches of the
    // step with scalar compares); the index handed to the loads is rebuilt from the lane's own wave number so that
    // they stay vector loads (see load_keys_t).
    static __device__ __forceinline__ int32_t clamp_group(int32_t gq, int32_t g0, int32_t gend, int32_t wave_s, int32_t wave_v) {
        int32_t gg = gq < gend ? gq : gend - 1;
        if (RING) gg = g0 + ((gg - g0) & 31);
        return gg - wave_s + wave_v;
    }
    static __device__ __forceinline__ void load_key_set(KeyRegs (&r)[NG], const uint32_t *__restrict__ key,
                                                        const uint32_t *__restrict__ info, const uint32_t *__restrict__ base,
                                                        int32_t g, int32_t g0, int32_t gend, int32_t wave_s, int32_t wave_v,
                                                        int lane) {
#pragma unroll
        for (int j = 0; j < NG; j++)
            r[j] = load_keys_t<STREAM_NT, K24, (PARTS & TP_KEY12) != 0>(key, info, base,
                                                                         clamp_group(g + j * NW, g0, gend, wave_s, wave_v), lane);
    }
    static __device__ __forceinline__ void load_val_set(ValRegs (&r)[NG], const double *__restrict__ val, int32_t g,
                                                        int32_t g0, int32_t gend, int32_t wave_s, int32_t wave_v, int lane) {
#pragma unroll
        for (int j = 0; j < NG; j++)
            r[j] = load_vals_t<STREAM_NT>(val, clamp_group(g + j * NW, g0, gend, wave_s, wave_v), lane);
    }

    // Step number P (mod PERIOD) of a wave's walk, at group g.  In this order: the gathers of this step, whose keys were
    // asked for KD steps ago; the key loads of step P + KD; the value loads of step P + 1; then the atomics of this
    // step, which wait for the gathers alone -- vector memory loads return in issue order, so a counted wait for the
    // gathers leaves everything issued after them in flight, and this step's values, asked for a whole step ago, are
    // in front of them.  PRED: some of the NG groups may not exist (a row block's last step); every group but the first
    // is tested.  LOADS: whether a later step exists to load for.
    template <int P, bool PRED, bool LOADS>
    static __device__ __forceinline__ void step(KeyRegs (&K)[NK][NG], ValRegs (&V)[2][NG], double *ytile,
                                                const uint32_t *__restrict__ key, const double *__restrict__ val,
                                                const uint32_t *__restrict__ info, const uint32_t *__restrict__ base,
                                                const double *__restrict__ x, int32_t g, int32_t g0, int32_t gend,
                                                int32_t wave_s, int32_t wave_v, int lane, int rb_bits, uint32_t rmask,
                                                int32_t slab_cols, double &sink) {
        constexpr int kc = P % NK, kn = (P + KD) % NK, vc = P % 2, vn = (P + 1) % 2;
        const int cshift = K24 ? 15 : rb_bits;
        double xv[NG][4];
        u32x4 kk[NG];
#pragma unroll
        for (int j = 0; j < NG; j++) {
            xv[j][0] = xv[j][1] = xv[j][2] = xv[j][3] = 1.0;
            kk[j] = unpack_keys<K24>(K[kc][j]);
            if (GATHER && (!PRED || j == 0 || g + j * NW < gend)) {
                const double *xs = x + (int64_t)(K[kc][j].info >> 9) * slab_cols;
                const u32x4 b = K[kc][j].base;     // zero with 4-byte keys
                xv[j][0] = load_x<XLOAD>(xs + ((b.x + (kk[j].x >> cshift)) & CMASK));
                xv[j][1] = load_x<XLOAD>(xs + ((b.y + (kk[j].y >> cshift)) & CMASK));
                xv[j][2] = load_x<XLOAD>(xs + ((b.z + (kk[j].z >> cshift)) & CMASK));
                xv[j][3] = load_x<XLOAD>(xs + ((b.w + (kk[j].w >> cshift)) & CMASK));
            }
        }
        if (LOADS) {
            load_key_set(K[kn], key, info, base, g + KD * STRIDE, g0, gend, wave_s, wave_v, lane);
            load_val_set(V[vn], val, g + STRIDE, g0, gend, wave_s, wave_v, lane);
        }
#pragma unroll
        for (int j = 0; j < NG; j++) {
            if (!PRED || j == 0 || g + j * NW < gend) {
                if (ATOMIC) {
                    unsafeAtomicAdd(&ytile[kk[j].x & rmask], V[vc][j].v0.x * xv[j][0]);
                    unsafeAtomicAdd(&ytile[kk[j].y & rmask], V[vc][j].v0.y * xv[j][1]);
                    unsafeAtomicAdd(&ytile[kk[j].z & rmask], V[vc][j].v1.x * xv[j][2]);
                    unsafeAtomicAdd(&ytile[kk[j].w & rmask], V[vc][j].v1.y * xv[j][3]);
                } else {
                    sink += V[vc][j].v0.x * xv[j][0] + V[vc][j].v0.y * xv[j][1] + V[vc][j].v1.x * xv[j][2] +
                            V[vc][j].v1.y * xv[j][3] + (double)((kk[j].x ^ kk[j].y ^ kk[j].z ^ kk[j].w) & 1u);
                }
            }
        }
    }

    // One step of the walk; true when it was the row block's last.  A full step (all NG groups exist: one scalar
    // compare) takes the body without tests; the last step of a row block, when it is short, takes the predicated
    // body and loads nothing.
    template <int P>
    static __device__ __forceinline__ bool advance(KeyRegs (&K)[NK][NG], ValRegs (&V)[2][NG], double *ytile,
                                                   const uint32_t *__restrict__ key, const double *__restrict__ val,
                                                   const uint32_t *__restrict__ info, const uint32_t *__restrict__ base,
                                                   const double *__restrict__ x, int32_t &g, int32_t g0, int32_t gend,
                                                   int32_t wave_s, int32_t wave_v, int lane, int rb_bits, uint32_t rmask,
                                                   int32_t slab_cols, double &sink) {
        if (PARTS & TP_FULLSTEP) {
            if (g + (NG - 1) * NW < gend) {
                step<P, false, true>(K, V, ytile, key, val, info, base, x, g, g0, gend, wave_s, wave_v, lane, rb_bits, rmask,
                                     slab_cols, sink);
            } else {
                step<P, true, false>(K, V, ytile, key, val, info, base, x, g, g0, gend, wave_s, wave_v, lane, rb_bits, rmask,
                                     slab_cols, sink);
                return true;
            }
        } else {
            step<P, true, true>(K, V, ytile, key, val, info, base, x, g, g0, gend, wave_s, wave_v, lane, rb_bits, rmask,
                                slab_cols, sink);
        }
        g += STRIDE;
        return g >= gend;
    }
};

// Which parts the shipped kernel carries, by what each was measured to be worth (profiles/tiled_pipeline_ablation.md):
// with 3-byte keys the test-free full step and the bulk tile copy; with 4-byte keys none -- there every combination
// measured was slower than the step without them.  Keys two steps ahead and the single 12-byte key load did not pay
// anywhere and exist in the ablation build only.
constexpr int tl_parts(bool k24) { return k24 ? TP_FULLSTEP | TP_BULKTILE : 0; }

template <int VARIANT, int NW, int NG, bool K24, int PARTS>
__global__ __launch_bounds__(64 * NW) void k_gaxpy_tiled(const int32_t *__restrict__ rb_gptr,
                                                         const uint32_t *__restrict__ group_info,
                                                         const uint32_t *__restrict__ tile_key,
                                                         const uint32_t *__restrict__ tile_base,
                                                         const double *__restrict__ tile_val,
                                                         const double *__restrict__ x, double *__restrict__ y,
                                                         int32_t m, int32_t nrb, int32_t row_block,
                                                         int32_t slab_cols, int rb_bits) {
    extern __shared__ __attribute__((aligned(16))) double ytile[];  // row_block doubles + the padding dummy row
    typedef TiledStep<VARIANT, NW, NG, K24, PARTS> S;
    const uint32_t rmask = K24 ? 0x7FFFu : (1u << rb_bits) - 1u;
    const int lane = threadIdx.x & 63;
    const int32_t wave_v = threadIdx.x >> 6, wave_s = __builtin_amdgcn_readfirstlane(wave_v);
    double sink = 0.0;
    for (int32_t rb = blockIdx.x; rb < nrb; rb += gridDim.x) {
        const int64_t row0 = (int64_t)rb * row_block;
        const int32_t rows = (int32_t)((row0 + row_block <= m) ? row_block : (m - row0));
        const int32_t gend = rb_gptr[rb + 1];
        const int32_t g0 = rb_gptr[rb];
        // Each wave walks its groups NG at a time (g, g + NW, ...) with a ring of key sets and two value sets, all
        // named by the step number (no copies: a copy would wait for the load).  The first loads of the walk -- the
        // keys of steps 0 .. KD - 1 and the values of step 0 -- go out BEFORE the y tile is filled, so the stream
        // starts under the fill.  Padding entries point at a dummy LDS row.
        int32_t g = g0 + wave_s;
        KeyRegs K[S::NK][NG];
        ValRegs V[2][NG];
        if (g < gend) {
#pragma unroll
            for (int d = 0; d < S::KD; d++)
                S::load_key_set(K[d], tile_key, group_info, tile_base, g + d * S::STRIDE, g0, gend, wave_s, wave_v, lane);
            S::load_val_set(V[0], tile_val, g, g0, gend, wave_s, wave_v, lane);
        }
        if (PARTS & TP_BULKTILE) {
            tile_fill<64 * NW>(ytile, y + row0, rows);
        } else {
            for (int k = threadIdx.x; k < rows; k += 64 * NW) ytile[k] = y[row0 + k];
        }
        __syncthreads();
        if (g < gend) {
#define CSX_TILED_ADVANCE(P)                                                                                          \
    if (S::template advance<P>(K, V, ytile, tile_key, tile_val, group_info, tile_base, x, g, g0, gend, wave_s, wave_v, \
                               lane, rb_bits, rmask, slab_cols, sink))                                                 \
        break;
            for (;;) {
                CSX_TILED_ADVANCE(0)
                CSX_TILED_ADVANCE(1)
                if constexpr (S::PERIOD == 6) {
                    CSX_TILED_ADVANCE(2)
                    CSX_TILED_ADVANCE(3)
                    CSX_TILED_ADVANCE(4)
                    CSX_TILED_ADVANCE(5)
                }
            }
#undef CSX_TILED_ADVANCE
        }
        __syncthreads();
        if (!S::ATOMIC && sink == 12345.678) ytile[0] = sink;  // keep the ablated arithmetic alive
        if (PARTS & TP_BULKTILE) {
            tile_drain<64 * NW>(ytile, y + row0, rows);
        } else {
            for (int k = threadIdx.x; k < rows; k += 64 * NW) y[row0 + k] = ytile[k];
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void k_rb_group_ptr(int32_t nrb, int32_t nslab, const int32_t *__restrict__ gptr,
                                                      int32_t *__restrict__ rb_gptr) {
    int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b <= nrb) rb_gptr[b] = gptr[(int64_t)b * nslab];
}

static int gaxpy_tiled_pick_shape(Csc *A);

int gaxpy_tiled_prepare(Csc *A) {
    if (A->tiled) return CSX_OK;
    if (!A->x) return CSX_EINVAL;
    hipStream_t s = ctx().stream;
    // one row block per workgroup, one workgroup per CU; more rounds only if a block would not fit LDS
    const int32_t nwg = ctx().cus > 0 ? ctx().cus : 256;
    const int32_t cap = TL_LDS_ROWS;
    int32_t rounds = 1;
    int32_t row_block;
    for (;;) {
        const int64_t nrb_try = (int64_t)nwg * rounds;
        row_block = (int32_t)(((int64_t)A->m + nrb_try - 1) / nrb_try);
        if (row_block <= cap) break;
        rounds++;
    }
    if (row_block < 1) row_block = 1;
    const int32_t nrb = (int32_t)(((int64_t)A->m + row_block - 1) / row_block);
    int rb_bits = 1;
    while ((1 << rb_bits) <= row_block) rb_bits++;  // local row index row_block itself = dummy slot for padding
    double slab_kb = 1024.0;
#ifdef CSX_ABLATION
    if (const char *e = std::getenv("CSX_TILED_SLAB_KB")) slab_kb = std::atof(e) >= 8.0 ? std::atof(e) : slab_kb;
#endif
    int64_t slab_cols = (int64_t)(slab_kb * 1024 / 8);
    const int64_t max_cols_key = 1ll << (32 - rb_bits);
    if (slab_cols > max_cols_key) slab_cols = max_cols_key;
    if (slab_cols > A->n) slab_cols = A->n > 0 ? A->n : 1;
    int32_t nslab = (int32_t)(((int64_t)A->n + slab_cols - 1) / slab_cols);
    if (nslab < 1) nslab = 1;
    const int64_t ntiles = (int64_t)nrb * nslab;
    if (ntiles > 0x3fffffffll || nslab >= (1 << 22)) return CSX_EINVAL;

    std::unique_ptr<TiledPlan> t(new TiledPlan());
    t->rb_bits = rb_bits;
    t->row_block = row_block;
    t->nrb = nrb;
    t->nslab = nslab;
    t->slab_cols = (int32_t)slab_cols;
    {
        DevBuf<int32_t> col, sptr, gptr;
        DevBuf<uint32_t> tid, packed, stid, skey;
        DevBuf<double> sval;
        int64_t ngroups = 0;
        CSX_TRY(col.alloc((size_t)A->nnz));
        CSX_TRY(tid.alloc((size_t)A->nnz));
        CSX_TRY(packed.alloc((size_t)A->nnz));
        CSX_TRY(stid.alloc((size_t)A->nnz));
        CSX_TRY(skey.alloc((size_t)A->nnz));
        CSX_TRY(sval.alloc((size_t)A->nnz));
        CSX_TRY(sptr.alloc((size_t)ntiles + 1));
        CSX_TRY(gptr.alloc((size_t)ntiles + 1));
        CSX_TRY(t->tile_ptr.alloc((size_t)nrb + 1));
        CSX_TRY(expand_columns(A->p, A->n, A->nnz, col));
        if (A->nnz > 0) {
            int64_t blocks = ((int64_t)A->nnz + 255) / 256;
            hipLaunchKernelGGL(k_tile_keys, dim3((unsigned)blocks), dim3(256), 0, s, (int64_t)A->nnz, A->i, col, rb_bits,
                               row_block, t->slab_cols, t->nslab, tid, packed);
            CSX_LAUNCH_CHECK();
        }
        CSX_TRY(stable_sort_by_key(tid, packed, A->x, A->nnz, (uint32_t)ntiles, stid, skey, sval));
        CSX_TRY(boundaries_from_sorted(stid, A->nnz, (int32_t)ntiles, sptr));
        const unsigned tb = (unsigned)((ntiles + 256) / 256);
        hipLaunchKernelGGL(k_padded_lengths, dim3(tb), dim3(256), 0, s, ntiles, sptr, gptr);
        CSX_TRY(scan_exclusive_i32(gptr, gptr, ntiles, &ngroups));
        // 3-byte keys when every 64-entry run is narrower than 512 columns (and the row fits 15 bits: always, LDS bounds it)
        bool k24 = false;
        if (ngroups > 0 && rb_bits <= 15 && ctx().opt.gaxpy_keys24) {
            DevBuf<int> flag;
            int h = 1;
            CSX_TRY(flag.alloc(1));
            (void)hipMemsetAsync(flag, 0, sizeof(int), s);
            hipLaunchKernelGGL(k_run_span, dim3((unsigned)(((int64_t)A->nnz + 255) / 256)), dim3(256), 0, s, (int64_t)A->nnz,
                               stid, sptr, skey, rb_bits, flag);
            CSX_HIP(hipMemcpyAsync(&h, flag, sizeof(int), hipMemcpyDeviceToHost, s));
            CSX_HIP(hipStreamSynchronize(s));
            k24 = h == 0;
        }
        t->ngroups = ngroups;
        CSX_TRY(t->tile_len.alloc((size_t)ngroups));  // group_info
        if (!k24) CSX_TRY(t->tile_key.alloc((size_t)ngroups * TL_GROUP));
        if (k24) CSX_TRY(t->tile_key24.alloc((size_t)ngroups * TL_GROUP * 3 + 16));
        if (k24) CSX_TRY(t->tile_base.alloc((size_t)ngroups * 4));
        CSX_TRY(t->tile_val.alloc((size_t)ngroups * TL_GROUP));
        if (ngroups > 0) {
            // padding slots: column 0 of the slab / offset 0 of the run, dummy row, value 0 -> adds 0 * x into an unused LDS slot
            if (k24) {
                hipLaunchKernelGGL(k_fill_key24, dim3(2048), dim3(256), 0, s, t->tile_key24, (int64_t)ngroups * TL_GROUP,
                                   (uint32_t)row_block);
                (void)hipMemsetAsync(t->tile_base, 0, (size_t)ngroups * 4 * sizeof(uint32_t), s);
            } else {
                hipLaunchKernelGGL(k_fill_keys, dim3(2048), dim3(256), 0, s, t->tile_key, (int64_t)ngroups * TL_GROUP,
                                   (uint32_t)row_block);
            }
            (void)hipMemsetAsync(t->tile_val, 0, (size_t)ngroups * TL_GROUP * sizeof(double), s);
            hipLaunchKernelGGL(k_group_info, dim3(tb), dim3(256), 0, s, ntiles, nslab, sptr, gptr, (uint32_t *)t->tile_len.get());
            hipLaunchKernelGGL(k_interleave, dim3((unsigned)(((int64_t)A->nnz + 255) / 256)), dim3(256), 0, s,
                               (int64_t)A->nnz, stid, sptr, gptr, skey, sval, t->tile_key, t->tile_val);
            if (k24)
                hipLaunchKernelGGL(k_interleave24, dim3((unsigned)(((int64_t)A->nnz + 255) / 256)), dim3(256), 0, s,
                                   (int64_t)A->nnz, stid, sptr, gptr, skey, rb_bits, t->tile_key24, t->tile_base);
        }
        hipLaunchKernelGGL(k_rb_group_ptr, dim3((unsigned)((nrb + 256) / 256)), dim3(256), 0, s, nrb, nslab, gptr,
                           t->tile_ptr);
        CSX_LAUNCH_CHECK();
        CSX_HIP(hipStreamSynchronize(s));
    }
    A->tiled = std::move(t);
#ifndef CSX_ABLATION
    // Off by default ("gaxpy.tune_shape"): on every box and run seen 4 x 5 was the fastest or within the noise of the
    // fastest, and a choice made from two short timings is itself noisy (under the profiler it picked 8 x 4, which
    // moves 13 % more bytes).  A plan that is not tuned launches 4 x 5.
    if (ctx().opt.gaxpy_tune_shape) CSX_TRY(gaxpy_tiled_pick_shape(A));
#endif
    return CSX_OK;
}

// Launch shapes offered to the plan: the same kernel body, plan and LDS tile, only waves per workgroup x groups per wave
// and step differ.  4 x 5 and 2 x 10 are within 1 % of each other on the boxes measured (profiles/r02_ablation.md, 1),
// 8 x 4 and 2 x 8 within 5 %, and the whole kernel varies by 8 % from box to box -- so the plan times them where it runs.
constexpr int TL_NSHAPES = 4;
static int gaxpy_tiled_launch(const Csc *A, const double *x, double *y, int shape);

static int gaxpy_tiled_pick_shape(Csc *A) {
    TiledPlan *t = A->tiled.get();
    if ((int64_t)A->nnz < (int64_t)1 << 24) return CSX_OK;      // small matrices: the default shape, no 10 ms of tuning
    hipStream_t s = ctx().stream;
    DevBuf<double> x, y;
    if (x.alloc((size_t)A->n) != CSX_OK || y.alloc((size_t)A->m) != CSX_OK) return CSX_OK;   // no room: default
    CSX_HIP(hipMemsetAsync(x, 0, (size_t)A->n * sizeof(double), s));   // the gathers go where they always go; values do not matter
    CSX_HIP(hipMemsetAsync(y, 0, (size_t)A->m * sizeof(double), s));
    hipEvent_t e0, e1;
    CSX_HIP(hipEventCreate(&e0));
    CSX_HIP(hipEventCreate(&e1));
    int best = 0;
    int st = CSX_OK;
    for (int round = 0; round < 2 && st == CSX_OK; round++)             // second round: best of two per shape
        for (int sh = 0; sh < TL_NSHAPES && st == CSX_OK; sh++) {
            if (round == 0) st = gaxpy_tiled_launch(A, x, y, sh);       // not timed: first launch of this instantiation
            if (st != CSX_OK) break;
            (void)hipEventRecord(e0, s);
            for (int rep = 0; rep < 3 && st == CSX_OK; rep++) st = gaxpy_tiled_launch(A, x, y, sh);
            (void)hipEventRecord(e1, s);
            if (hipEventSynchronize(e1) != hipSuccess) st = CSX_ERUNTIME;
            float ms = 0.f;
            (void)hipEventElapsedTime(&ms, e0, e1);
            ms /= 3;
            if (round == 0 || ms < t->shape_ms[sh]) t->shape_ms[sh] = ms;
        }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (st != CSX_OK) return st;
    for (int sh = 1; sh < TL_NSHAPES; sh++)
        if (t->shape_ms[sh] < t->shape_ms[best]) best = sh;
    t->shape = best;
    return CSX_OK;
}

// The launch shape in force: "gaxpy.shape" when it names one (read here, at launch time: one plan runs at any of the
// four), otherwise the plan's own (the tuner's pick, or 4 x 5 when it was not timed).
int gaxpy_tiled_shape(const TiledPlan *t) {
    const int forced = ctx().opt.gaxpy_shape;
    if (forced >= 0 && forced < TL_NSHAPES) return forced;
    return t->shape >= 0 && t->shape < TL_NSHAPES ? t->shape : 0;
}

int gaxpy_tiled_run(const Csc *A, const double *x, double *y) {
    return gaxpy_tiled_launch(A, x, y, gaxpy_tiled_shape(A->tiled.get()));
}

// csx_gaxpy_plan_geometry / csx_gaxpy_plan_groups: groups[b] = groups of 256 entries of row block b (nrb counts)
int gaxpy_tiled_group_counts(const TiledPlan *t, std::vector<int32_t> &groups) {
    std::vector<int32_t> ptr((size_t)t->nrb + 1);
    hipStream_t s = ctx().stream;
    CSX_HIP(hipMemcpyAsync(ptr.data(), t->tile_ptr, ptr.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    CSX_HIP(hipStreamSynchronize(s));
    groups.resize((size_t)t->nrb);
    for (int32_t b = 0; b < t->nrb; b++) groups[b] = ptr[b + 1] - ptr[b];
    return CSX_OK;
}

// A kernel instance may use the whole LDS: asked for once per instance and device, not at every launch.
template <int V, int NW, int NG, bool K24, int PARTS>
static hipError_t gaxpy_tiled_allow_lds() {
    static int done_on = -1;
    if (done_on == ctx().device) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_gaxpy_tiled<V, NW, NG, K24, PARTS>),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, TL_LDS_BYTES);
    if (e == hipSuccess) done_on = ctx().device;
    return e;
}

static int gaxpy_tiled_launch(const Csc *A, const double *x, double *y, int shape) {
    const TiledPlan *t = A->tiled.get();
    hipStream_t s = ctx().stream;
    const size_t lds = (((size_t)(t->row_block + 1) * sizeof(double)) + 15) & ~(size_t)15;  // + dummy row
    const int32_t nwg = ctx().cus > 0 ? ctx().cus : 256;
    const unsigned grid = (unsigned)(t->nrb < nwg ? t->nrb : nwg);
#define CSX_TILED_LAUNCH_K(V, NW, NG, K24, PARTS)                                                                    \
    {                                                                                                                \
        CSX_HIP((gaxpy_tiled_allow_lds<V, NW, NG, K24, PARTS>()));                                                   \
        hipLaunchKernelGGL((k_gaxpy_tiled<V, NW, NG, K24, PARTS>), dim3(grid), dim3(64 * NW), lds, s, t->tile_ptr,   \
                           (const uint32_t *)t->tile_len.get(),                                                      \
                           K24 ? reinterpret_cast<const uint32_t *>(t->tile_key24.get()) : t->tile_key.get(),        \
                           t->tile_base,                                                                             \
                           t->tile_val, x, y, A->m, t->nrb, t->row_block, t->slab_cols, t->rb_bits);                 \
    }
#define CSX_TILED_LAUNCH_P(V, NW, NG, P24, P32)                                                                      \
    {                                                                                                                \
        if (t->tile_key24) CSX_TILED_LAUNCH_K(V, NW, NG, true, P24) else CSX_TILED_LAUNCH_K(V, NW, NG, false, P32)   \
    }
#define CSX_TILED_LAUNCH(V, NW, NG) CSX_TILED_LAUNCH_P(V, NW, NG, tl_parts(true), tl_parts(false))
#ifdef CSX_ABLATION
    // CSX_TILED_VARIANT = V + 100 * NW + 10000 * NG (NW, NG default to the shipped TL_WAVES, TL_NG).
    // V = 0..7: the VARIANTs of k_gaxpy_tiled.  V = 10 + mask (4 x 5 only): the full kernel with the parts in `mask`
    // switched OFF -- 1 keys two steps ahead, 2 test-free full step, 4 one 12-byte key load, 8 bulk tile copy;
    // 25 = all four off, the step as it was before them.
    int code = 0;
    if (const char *e = std::getenv("CSX_TILED_VARIANT")) code = std::atoi(e);
    const int v = code % 100, nw = (code / 100) % 100 ? (code / 100) % 100 : TL_WAVES, ng = code / 10000 ? code / 10000 : TL_NG;
#define CSX_V(V)                                             \
    if (v == V) {                                            \
        if (nw == 16 && ng == 2) CSX_TILED_LAUNCH(V, 16, 2)  \
        else if (nw == 4 && ng == 5) CSX_TILED_LAUNCH(V, 4, 5) \
        else if (nw == 2 && ng == 10) CSX_TILED_LAUNCH(V, 2, 10) \
        else return CSX_EINVAL;                              \
    } else
#define CSX_OFF(MASK)                                                        \
    if (v == 10 + MASK) {                                                    \
        if (nw == 4 && ng == 5) CSX_TILED_LAUNCH_P(0, 4, 5, TP_ALL & ~(MASK), TP_ALL & ~(MASK)) \
        else return CSX_EINVAL;                                              \
    } else
    if (v == 0) {
        if (nw == 16 && ng == 1) CSX_TILED_LAUNCH(0, 16, 1)
        else if (nw == 16 && ng == 2) CSX_TILED_LAUNCH(0, 16, 2)
        else if (nw == 12 && ng == 2) CSX_TILED_LAUNCH(0, 12, 2)
        else if (nw == 12 && ng == 4) CSX_TILED_LAUNCH(0, 12, 4)
        else if (nw == 8 && ng == 2) CSX_TILED_LAUNCH(0, 8, 2)
        else if (nw == 8 && ng == 3) CSX_TILED_LAUNCH(0, 8, 3)
        else if (nw == 8 && ng == 4) CSX_TILED_LAUNCH(0, 8, 4)
        else if (nw == 4 && ng == 4) CSX_TILED_LAUNCH(0, 4, 4)
        else if (nw == 4 && ng == 5) CSX_TILED_LAUNCH(0, 4, 5)
        else if (nw == 4 && ng == 6) CSX_TILED_LAUNCH(0, 4, 6)
        else if (nw == 2 && ng == 6) CSX_TILED_LAUNCH(0, 2, 6)
        else if (nw == 2 && ng == 7) CSX_TILED_LAUNCH(0, 2, 7)
        else if (nw == 2 && ng == 8) CSX_TILED_LAUNCH(0, 2, 8)
        else if (nw == 2 && ng == 9) CSX_TILED_LAUNCH(0, 2, 9)
        else if (nw == 2 && ng == 10) CSX_TILED_LAUNCH(0, 2, 10)
        else if (nw == 2 && ng == 12) CSX_TILED_LAUNCH(0, 2, 12)
        else if (nw == 1 && ng == 10) CSX_TILED_LAUNCH(0, 1, 10)
        else if (nw == 1 && ng == 12) CSX_TILED_LAUNCH(0, 1, 12)
        else if (nw == 3 && ng == 5) CSX_TILED_LAUNCH(0, 3, 5)
        else if (nw == 3 && ng == 6) CSX_TILED_LAUNCH(0, 3, 6)
        else if (nw == 3 && ng == 7) CSX_TILED_LAUNCH(0, 3, 7)
        else if (nw == 3 && ng == 8) CSX_TILED_LAUNCH(0, 3, 8)
        else if (nw == 5 && ng == 4) CSX_TILED_LAUNCH(0, 5, 4)
        else if (nw == 6 && ng == 3) CSX_TILED_LAUNCH(0, 6, 3)
        else if (nw == 4 && ng == 7) CSX_TILED_LAUNCH(0, 4, 7)
        else return CSX_EINVAL;
    } else
    CSX_V(1) CSX_V(2) CSX_V(3) CSX_V(4) CSX_V(5) CSX_V(6) CSX_V(7)
    CSX_OFF(0) CSX_OFF(1) CSX_OFF(2) CSX_OFF(3) CSX_OFF(4) CSX_OFF(5) CSX_OFF(6) CSX_OFF(7) CSX_OFF(8) CSX_OFF(9)
    CSX_OFF(10) CSX_OFF(11) CSX_OFF(12) CSX_OFF(13) CSX_OFF(14) CSX_OFF(15) return CSX_EINVAL;
#undef CSX_V
#undef CSX_OFF
    (void)shape;
#else
    switch (shape) {
        case 1: CSX_TILED_LAUNCH(0, 2, 10) break;
        case 2: CSX_TILED_LAUNCH(0, 8, 4) break;
        case 3: CSX_TILED_LAUNCH(0, 2, 8) break;
        default: CSX_TILED_LAUNCH(0, TL_WAVES, TL_NG) break;     // 0 and -1 (not tuned): 4 x 5
    }
#endif
#undef CSX_TILED_LAUNCH
#undef CSX_TILED_LAUNCH_P
#undef CSX_TILED_LAUNCH_K
    CSX_LAUNCH_CHECK();
    return CSX_OK;
}

}  // namespace csx
