// Internal declarations shared by the libcsx translation units (gfx950 only).
#pragma once
#include <cstdlib>
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <memory>
#include <string>
#include <vector>

#include "../../include/csx.h"

namespace csx {

// Experiment switches exist only in the -DCSX_ABLATION build (libcsx_ablation.so, build.py --ablation): in the
// shipped library no environment variable can change which kernel runs or what it computes.
inline const char *ablation_env(const char *name) {
#ifdef CSX_ABLATION
    return std::getenv(name);
#else
    (void)name;
    return nullptr;
#endif
}


void set_error(const char *fmt, ...);

#define CSX_HIP(call)                                                                      \
    do {                                                                                   \
        hipError_t _e = (call);                                                            \
        if (_e != hipSuccess) {                                                            \
            csx::set_error("%s:%d %s -> %s", __FILE__, __LINE__, #call, hipGetErrorString(_e)); \
            return CSX_ERUNTIME;                                                           \
        }                                                                                  \
    } while (0)

#define CSX_TRY(call)            \
    do {                         \
        int _s = (call);         \
        if (_s != CSX_OK) return _s; \
    } while (0)

#define CSX_LAUNCH_CHECK() CSX_HIP(hipGetLastError())

// device allocation helpers (bytes may be 0 -> still returns a valid pointer)
int dmalloc(void **p, size_t bytes);
template <class T>
inline int dalloc(T **p, size_t count) { return dmalloc((void **)p, count * sizeof(T)); }
void dfree(void *p);
void pool_trim();                               // release every idle block to the driver
void pool_stats(size_t *cached, size_t *live);  // bytes idle in the cache / handed out
void pool_set_limit(size_t bytes);              // cap of the cache (0: the default quarter of the device)

// Owner of one device array from the pool: dfree'd when the buffer is destroyed, reset or allocated again.  Move-only, host
// only.  It converts to T *, so launches, copies and kernel-argument structs take it where they took the raw pointer.
template <class T>
class DevBuf {
  public:
    DevBuf() = default;
    explicit DevBuf(T *owned) : p_(owned) {}   // takes over a block from dmalloc
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p_(o.release()) {}
    DevBuf &operator=(DevBuf &&o) noexcept {
        if (this != &o) {
            reset();
            p_ = o.release();
        }
        return *this;
    }
    ~DevBuf() { dfree(p_); }
    int alloc(size_t count) {   // count may be 0 (still a valid pointer)
        reset();
        return dalloc(&p_, count);
    }
    void reset() {
        dfree(p_);
        p_ = nullptr;
    }
    T *get() const { return p_; }
    operator T *() const { return p_; }
    T *release() {   // for an owner that records its ownership itself (Csc, Vec)
        T *p = p_;
        p_ = nullptr;
        return p;
    }

  private:
    T *p_ = nullptr;
};

enum Kind : int { K_FREE = 0, K_CSC, K_VEC, K_IVEC, K_TRIPLAN, K_CHOLPLAN, K_SHARDPLAN, K_BTFPLAN, K_LUREFPLAN, K_ASMPLAN, K_CHOLREFPLAN, K_MULPLAN, K_ADDPLAN, K_LDLFACTOR, K_SLUFACTOR, K_HQRFACTOR, K_SCHURFACTOR, K_SLUBATCH, K_LDLBATCH, K_HQRBATCH };

struct Csc;

// Row-gather layout used by the wave/exact SpMV and the triangular solves:
// for row r, entries [ptr[r], ptr[r+1]) hold (idx, val) in the order the
// reference updates that row.
struct Gather {
    int32_t rows = 0;
    DevBuf<int32_t> ptr, idx;
    DevBuf<double> val;
};

// LDS-resident SpMV plan (csx_gaxpy_tiled.hip): entries regrouped into (row block, column slab)
// tiles, row-block-major, column order kept inside a tile, stored in interleaved groups of 256.
struct TiledPlan {
    int32_t row_block = 0;         // rows per LDS tile (one tile per workgroup)
    int32_t nrb = 0;               // number of row blocks
    int32_t nslab = 0;             // number of column slabs
    int32_t slab_cols = 0;         // columns per slab
    int64_t ngroups = 0;           // groups of 256 entries over all tiles (padding included)
    DevBuf<int32_t> tile_ptr;      // [nrb + 1] first group of every row block
    DevBuf<int32_t> tile_len;      // [ngroups] group info: (slab << 9) | entries in the group
    DevBuf<uint32_t> tile_key;     // packed (local col << rb_bits) | local row; null when the 3-byte keys are in use
    DevBuf<double> tile_val;
    int rb_bits = 0;
    // 3-byte keys (row | column offset << 15), used when every run of 64 column-sorted entries spans < 512 columns:
    DevBuf<uint8_t> tile_key24;    // [ngroups * 768]
    DevBuf<uint32_t> tile_base;    // [ngroups * 4] slab-local column of the first entry of each 64-entry run
    // launch shape (waves per workgroup x groups per wave and step), picked when the plan is built by timing the
    // candidates on this device (gaxpy_tiled_prepare); -1: the default shape
    int shape = -1;
    float shape_ms[4] = {0, 0, 0, 0};
};

// Order in which the reflections of a matrix of Householder vectors can be applied in parallel (csx_qr.hip):
// reflections of one level touch disjoint rows.
constexpr int32_t HAPPLY_MAX_LEVELS = 4096;   // beyond that (a chain of dependent reflections) one launch walks them all
struct HouseLevels {
    int32_t nlevels = 0;
    std::vector<int32_t> ptr;      // host: [nlevels + 1] into cols
    DevBuf<int32_t> cols;          // device: columns ordered by level, ascending inside a level
};

// Order in which the columns of a Cholesky factor take their entries of the inverse (csx_sparseinv.hip): the columns of one
// depth of the elimination forest (roots 0) are independent.
struct InvSchedule {
    int32_t ndepths = 0;
    int32_t widest = 0;            // columns in the widest depth
    int64_t terms = 0;             // sum over the columns of (entries below the diagonal)^2
    std::vector<int32_t> ptr;      // host: [ndepths + 1] into cols
    std::vector<int32_t> rows;     // host: [ndepths] the most entries below the diagonal of a column of that depth
    DevBuf<int32_t> cols;          // device: columns ordered by depth, ascending inside a depth
};

struct CliqueForest;   // csx_cholclique.h

// A matrix's arrays are the library's (dfree'd by ~Csc) unless `owns` is false (csx_csc_wrap: the caller's).  Not copyable:
// a copy would free them twice.
struct Csc {
    Csc();    // (both in csx_core.hip, where CliqueForest is complete)
    ~Csc();
    Csc(const Csc &) = delete;
    Csc &operator=(const Csc &) = delete;
    int32_t m = 0, n = 0, nnz = 0;
    int32_t *p = nullptr;
    int32_t *i = nullptr;
    double *x = nullptr;  // nullptr: pattern only
    bool owns = true;
    bool trusted = true;  // structure made or checked by the library; false for csx_csc_wrap until csc_validate has passed
    // cached plans (built on demand, freed with the matrix)
    std::unique_ptr<Gather> rows;         // stable transpose = rows of A in ascending column order
    std::unique_ptr<TiledPlan> tiled;
    std::unique_ptr<HouseLevels> house;   // csx_happly's level schedule (pattern only; dropped by csx_csc_invalidate too)
    std::unique_ptr<InvSchedule> inv;     // csx_chol_inverse's depth schedule (pattern only, so it outlives csx_updown_block; dropped by
                                          // csx_csc_invalidate too)
    std::unique_ptr<CliqueForest> clique; // csx_schol's finding "a forest of cliques on consecutive columns" (tree, counts, block list
                                          // on the device), kept for the csx_chol that follows; pattern only, dropped by
                                          // csx_csc_invalidate too
    bool rows_pending = false;      // i == nullptr ON PURPOSE: every column holds the consecutive rows j, j + 1, ... (the factor of a
                                    // forest of cliques, csx_cholsol_factor), so i[] follows from p[] alone and is written by
                                    // csc_fill_rows the first time a handle to the matrix is resolved (csc() below)
};

// d is the library's (dfree'd by ~Vec) unless `owns` is false (csx_vec_wrap: the caller's)
struct Vec {
    Vec() = default;
    ~Vec() {
        if (owns) dfree(d);
    }
    Vec(const Vec &) = delete;
    Vec &operator=(const Vec &) = delete;
    int64_t len = 0;
    void *d = nullptr;
    bool owns = true;
};

struct TriPlan;   // csx_trisolve.hip
struct CholPlan;  // csx_chol.hip
struct ShardPlan; // csx_comm.hip
struct SnPlan;    // csx_snsolve.hip
struct BtfPlan;   // csx_btf.hip
// delete p, in the file where the type is complete (csx_free)
void destroy(TriPlan *p);
void destroy(CholPlan *p);
void destroy(ShardPlan *p);
void destroy(BtfPlan *p);
void destroy(SnPlan *p);
// csx_trisolve.hip, for the plans that are built on triangular plans (cholsol, btf_factor, lusol_factor)
int tri_analyse_raw(const Csc *T, int kind, TriPlan **out);          // *out is set on success only
int tri_solve_raw(TriPlan *P, double *X, int32_t nrhs, bool relaxed);
int tri_solve_host_raw(TriPlan *P, double *x, bool *taken);          // "tri.host_chains"
int tri_route_info_raw(TriPlan *P, int32_t nrhs, bool relaxed, int64_t *out, int32_t cap, int32_t *count);   // csx_tri_route_info
int tri_launches_raw(const TriPlan *P, int64_t *out, int32_t cap, int32_t *count);                            // csx_tri_launches
void tri_set_mate(TriPlan *P, TriPlan *mate);
void tri_set_level_hint(TriPlan *P, std::vector<int32_t> &&level);
void tri_gather_arrays(const TriPlan *P, const int32_t **ptr, const int32_t **idx, const double **val, const double **diag);
struct Refactor;   // csx_refactor.hip
struct LuRefPlan;  // csx_refactor.hip
void destroy(Refactor *p);
void destroy(LuRefPlan *p);
struct AsmPlan;    // csx_assemble_plan.hip (all three built on FoldCore, csx_fold.h)
void destroy(AsmPlan *p);
struct MulPlan;    // csx_multiply_plan.hip
void destroy(MulPlan *p);
struct AddPlan;    // csx_add_plan.hip
void destroy(AddPlan *p);
struct CholAnalysis;  // csx_chol.hip
struct CholRefPlan;   // csx_chol_refactor.hip
void destroy(CholAnalysis *p);
void destroy(CholRefPlan *p);
struct LdlFactor;     // csx_ldl.h: the one partial-LDL' factor behind K_LDLFACTOR and K_SCHURFACTOR (csx_ldl.hip, csx_schur.hip)
void destroy(LdlFactor *p);
struct SluFactor;     // csx_slu.h (csx_slu.hip)
void destroy(SluFactor *p);
struct SluBatch;      // csx_slu_batch.hip: B value sets on a borrowed SluFactor
void destroy(SluBatch *p);
struct LdlBatch;      // csx_ldl_batch.hip: B value sets on a borrowed LdlFactor
void destroy(LdlBatch *p);
struct HqrFactor;     // csx_hqr.h (csx_hqr.hip)
void destroy(HqrFactor *p);
struct HqrBatch;      // csx_hqr_batch.hip: B value sets on a borrowed HqrFactor
void destroy(HqrBatch *p);
int house_levels(Csc *V);   // csx_qr.hip: V->house, the levels of V's reflections (pattern only), made once
// csx_host.cpp: csx_hqr_symbolic_host on vectors that grow (no capacities)
int hqr_symbolic(int32_t m, int32_t n, int32_t m2, const int32_t *Ap, const int32_t *Ai, const int32_t *q, const int32_t *parent,
                 const int32_t *pinv, const int32_t *leftmost, std::vector<int32_t> &Vp, std::vector<int32_t> &Vi,
                 std::vector<int32_t> &Rp, std::vector<int32_t> &Ri);

struct Object {
    Kind kind = K_FREE;
    void *ptr = nullptr;
    uint32_t gen = 0;   // bumped on every reuse of the slot (upper half of the handle)
};

// Kernel-selection overrides for TESTS of the kernels a plan would not pick by itself (csx_set_option).  Every
// setting computes correct results; none is read from the environment.
struct Options {
    int chol_band = 1;                // cs_chol: register-window kernel for chain-like banded factors
    int chol_wband = 1;               // cs_chol: blocked dense-band kernels for chain-like factors: 0 never, 1 for half-widths
                                      // above 80 (below, the register-window kernel), 2 whenever the tree is chain-like
    int chol_wband_nb = 16;           // ... columns per step (16 or 32)
    int chol_supernodes = 1;      // cs_chol: fundamental supernodes of >= 8 columns factored as dense trapezoids in place
    int chol_dense_trees = 1;     // cs_chol: LDS dense-block kernel for trees that are dense blocks
    int chol_forest = 1;          // ... and forests of small SPARSE trees on consecutive columns (blocks of <= 64 columns closed under
                                  // their upper entries): symbolic analysis on 64-bit row masks in registers, the block kernel with
                                  // a compacted store (needs chol.clique)
    int chol_exact = 1;           // cs_chol on forests of dense blocks: 1 = the reference's operations in the reference's order, L.x
                                  // bit-identical (default); 0 = fused multiply-adds and refined reciprocal square roots in the block
                                  // kernel: L.x equal to rounding, 1.5x the rate (opt-in; BASELINE grants x[] 1e-10)
    int chol_clique = 1;          // cs_schol / cs_chol / cholsol plan: forests of cliques on consecutive columns recognised from
                                  // A (or L) itself and handled without the general pattern machine (csx_cholclique.hip)
    int cholsol_dense_blocks = 1; // cholsol: dense-block kernels (false: the fused per-tree kernel)
    int spgemm_one_pass = 1;      // cs_multiply: one-walk LDS hash kernel (false: the two-pass kernel)
    int tri_chain_walker = 1;     // tri-solve: blocked chain walker for runs of narrow levels
    int tri_components = 1;       // tri-solve: one wave per small connected component (false: level sets)
    int tri_push = 1;             // tri-solve: component kernels in column-push form for L / U with few RHS
    int tri_columns = 1;          // tri-solve: small chain-like systems by the column loop, x in LDS
    int gaxpy_keys24 = 1;         // tiled cs_gaxpy plan: 3-byte keys when the matrix allows them
    int gaxpy_tune_shape = 0;    // tiled cs_gaxpy plan: time the launch shapes when the plan is built and keep the fastest
    int gaxpy_shape = -1;        // tiled cs_gaxpy: -1 = the plan's own launch shape, 0..3 = that shape; read at every launch, so
                                 // one plan can be run at all four (any other value reads back as -1)
    int gaxpy_block_route = 0;   // csx_gaxpy_block AUTO: 0 = its own rule, 1 = the block kernel, 2 = the column route
    int tri_row_waves = 1;        // level-scheduled solves: a wave per row for few right-hand sides and long rows
    int tri_levels_where = 0;         // level analysis: 0 = device for big factors, host for small; 1 = host; 2 = device
    int sort_short_keys = 1;          // cs_transpose: 16-bit keys between the radix passes where the matrix allows (0: always 32-bit)
    int tri_host_chains = 0;          // ONE host right-hand side on a chain-like factor (levels > n / 4, < 5e7 entries): 1 = the reference's
                                      // loop on the host (same bits), a case the device loses 10 - 40x; 0 (default) = the device, always
    int tri_graph = 2;                // supernodal solves: replay the launches of a solve as a hipGraph while the block of right-hand
                                      // sides stays in place: 0 never, 1 always, 2 when a solve is more than 256 launches and the
                                      // block has been the block of the two solves before it too (the third consecutive solve captures)
    int tri_supernodes = 1;           // cholsol: supernodal forward / backward solves on factors with supernodes (0 never, 1 yes,
                                      // 2 yes but the triangles by substitution out of LDS instead of on the matrix cores)
    int spgemm_ordered = 0;           // cs_multiply: sum every entry's products in the reference's order (bit-identical x)
    int sparseinv_walk = 1;           // csx_chol_inverse: a run of depths of one column each is walked by one workgroup in one
                                      // launch (0: one launch per depth, same bits)
    int assemble_long = 64;           // csx_assemble_plan: a slot of more than this many terms is folded by a wave of its own, a shorter
                                      // one by one lane (read when a plan is built; >= 1)
    int multiply_long = 64;           // csx_multiply_plan: a slot of more than this many products is folded by a wave of its own, a
                                      // shorter one by one lane (read when a plan is built; >= 1).  The default is assemble.long's,
                                      // UNMEASURED for products
    int add_long = 64;                // csx_add_plan: a slot of more than this many terms is folded by a wave of its own, a shorter
                                      // one by one lane (read when a plan is built; >= 1).  The default is assemble.long's,
                                      // UNMEASURED for the terms of a sum
    int lu_etree = 0;                 // cs_lu of one connected matrix on the device, columns scheduled by the column etree:
                                      // 0 never (the default since round 4: measured at best a tie with one host core, on the
                                      // shape it was made for -- profiles/r04_ablation.md), 1 for shallow trees with short
                                      // columns, 2 always (tests: L, U, pinv bit-identical to the host loop and the CPU restatement of the reference loop)
};

struct Context {
    Options opt;
    bool ready = false;
    int device = -1;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    hipStream_t side = nullptr;      // a second stream for copies that run beside a kernel of `stream` (csx_chol's check of S); made
                                     // and used once in csx_init: a stream's first copy from pageable memory costs tens of ms
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    int cus = 0;
    std::vector<Object> objects;  // handle = generation << 32 | index + 1 (csx_core.hip: put / get)
};

Context &ctx();
int require_ready();
csx_handle_t put(Kind k, void *ptr);
void *get(csx_handle_t h, Kind k);
int csc_fill_rows(Csc *A);   // csx_cholclique.hip: the row indices of a matrix with rows_pending
inline Csc *csc(csx_handle_t h) {
    Csc *A = (Csc *)get(h, K_CSC);
    if (A && A->rows_pending && csc_fill_rows(A) != CSX_OK) return nullptr;
    return A;
}
inline Vec *vec(csx_handle_t h) { return (Vec *)get(h, K_VEC); }
inline Vec *ivec(csx_handle_t h) { return (Vec *)get(h, K_IVEC); }

template <class T>
int upload(DevBuf<T> &d, const T *h, size_t count) {
    CSX_TRY(d.alloc(count));
    if (count) CSX_HIP(hipMemcpyAsync(d.get(), h, count * sizeof(T), hipMemcpyHostToDevice, ctx().stream));
    return CSX_OK;
}
template <class T>
int upload(DevBuf<T> &d, const std::vector<T> &h) { return upload(d, h.data(), h.size()); }
// h = d[0 .. count), synchronising the context's stream
inline int download_i32(std::vector<int32_t> &h, const int32_t *d, size_t count) {
    h.resize(count);
    if (count) CSX_HIP(hipMemcpyAsync(h.data(), d, count * sizeof(int32_t), hipMemcpyDeviceToHost, ctx().stream));
    CSX_HIP(hipStreamSynchronize(ctx().stream));
    return CSX_OK;
}

// csx_snsolve.hip: supernodal schedule of a Cholesky-shaped factor for the rounding-equal order of a cholsol plan
int sn_build(const Csc *L, const int32_t *parent, const int32_t *Lp_h, const int32_t *Gp_h, const int32_t *Gp, const int32_t *Gi,
             const double *Gx, int32_t col_levels, SnPlan **out);
int sn_solve(SnPlan *P, bool forward, const int32_t *Gp, const int32_t *Gi, const double *Gx, const double *Gd, const Csc *L,
             double *X, int32_t nrhs);
int64_t sn_generation(const SnPlan *P);   // changes whenever sn_prepare moved the work space
int sn_prepare(SnPlan *P, int32_t nrhs);   // work space of a solve with nrhs right-hand sides (sn_solve calls it; a capture calls it first)
void sn_info(const SnPlan *P, int32_t *nsn, int32_t *levels, int32_t *max_w);
void sn_info2(const SnPlan *P, int32_t *matrix_cores, double *growth);
int sn_geometry(const SnPlan *P, int64_t *out, int32_t cap);   // fields of csx_cholsol_sn_geometry; returns how many there are
int sn_launches(const SnPlan *P, int64_t *out, int32_t cap);   // counters of csx_cholsol_sn_launches; returns how many there are
bool sn_usable(const SnPlan *P);   // with the options in force (a plan with relaxed supernodes needs the matrix-core triangles)

// ---- device primitives (csx_scan.hip, csx_sort.hip) ----
// out[k] = sum(in[0..k-1]) for k in [0, n]; out has n+1 slots; in may alias out
// (then the last slot is written too).  total (host) optional.
int scan_exclusive_i32(const int32_t *in, int32_t *out, int64_t n, int64_t *total_host);
// col[p] = j for p in [Ap[j], Ap[j+1])
int expand_columns(const int32_t *Ap, int32_t n, int32_t nnz, int32_t *col);
// Stable sort of `count` records by key in [0, key_limit).  a = 32-bit payload,
// v = 64-bit payload (nullptr: none).  Inputs are not modified; outputs may not
// alias inputs.  out_key may be nullptr.
int stable_sort_by_key(const uint32_t *key, const uint32_t *a, const double *v, int64_t count,
                       uint32_t key_limit, uint32_t *out_key, uint32_t *out_a, double *out_v);
// The same sort with what cs_transpose adds to it (both optional): expand_ptr -- the 32-bit payload is not read but
// is the column of the record's position under these column pointers (expand_n columns); out_ptr -- the segment
// starts of the sorted keys, out_ptr[r] = first slot with key >= r for r in [0, nkeys], written by the last pass
// itself (then out_key may be null and no pass over the sorted keys is needed).
struct SortExtra {
    const int32_t *expand_ptr;
    int32_t expand_n;
    int32_t *out_ptr;
    int32_t nkeys;
};
int stable_sort_by_key_ex(const uint32_t *key, const uint32_t *a, const double *v, int64_t count, uint32_t key_limit,
                          uint32_t *out_key, uint32_t *out_a, double *out_v, const SortExtra *ex);
// p[r] = min(p[r], ..., p[n-1]) in place (reverse running minimum)
int suffix_min_i32(int32_t *p, int64_t n);
// ptr[r] = first position q with sorted_key[q] >= r, r in [0, nkeys]; ptr has nkeys+1 slots
int boundaries_from_sorted(const uint32_t *sorted_key, int64_t count, int32_t nkeys, int32_t *ptr);

// ---- building blocks shared across files ----
int build_row_gather(Csc *A);   // fills A->rows (values required)
// csx_residual.hip: h[0 .. width) (host) = the maxima, as unsigned integers, over the `count` rows of part (device, count x width,
// not written); synchronises the context's stream
int max_partials_host(const uint64_t *part, int64_t count, int32_t width, uint64_t *h);
// csx_residual.hip: omega / rnorm (host, nrhs each, either may be null) from a residual kernel's partials (blocks x 2 x nrhs bit
// patterns); zeros when blocks == 0 (no rows, part not read)
int residual_maxima(const uint64_t *part, int64_t blocks, int32_t nrhs, double *omega, double *rnorm);
// csx_residual.hip: zero[0 .. rows] = 0, the row pointers of a gather without entries
int empty_row_ptr(DevBuf<int32_t> &zero, int32_t rows);
// Do a[0 .. alen) and b[0 .. blen) (doubles on the device) share a byte?  Two wrapped views of one buffer may; an empty range
// shares nothing.
inline bool ranges_overlap(const void *a, int64_t alen, const void *b, int64_t blen) {
    const uintptr_t ab = (uintptr_t)a, ae = ab + (uintptr_t)alen * sizeof(double);
    const uintptr_t bb = (uintptr_t)b, be = bb + (uintptr_t)blen * sizeof(double);
    return alen > 0 && blen > 0 && ab < be && bb < ae;
}
// The blocks of a residual call: X holds xlen doubles, B and R (null: none) blen; X is another vector than B and R and lies apart
// from both; R is B (in place: the same handle or the same address) or lies apart from it.
inline bool residual_blocks_ok(const Vec *X, int64_t xlen, const Vec *B, const Vec *R, int64_t blen) {
    if (X->len < xlen || B->len < blen || (R && R->len < blen)) return false;
    if (B == X || R == X) return false;
    if (ranges_overlap(X->d, xlen, B->d, blen) || (R && ranges_overlap(X->d, xlen, R->d, blen))) return false;
    return !(R && R->d != B->d && ranges_overlap(B->d, blen, R->d, blen));
}
// Structure check of a matrix whose arrays the library did not make (csx_csc_wrap): p non-decreasing from 0 to nnz,
// every row index in [0, m), in one device pass.  CSX_EINVAL (IndexError in Python) otherwise; remembered in A->trusted.
int csc_validate(Csc *A);
// *out: a new matrix, not yet a handle, with the pattern p / i (device; copied on the context's stream) and, when `values`,
// room for nnz values that the caller fills
int csc_copy_pattern(int32_t m, int32_t n, int32_t nnz, const int32_t *p, const int32_t *i, bool values,
                     std::unique_ptr<Csc> *out);
int transpose_device(const Csc *A, bool values, Csc *C);  // C fields allocated here
int gaxpy_device(Csc *A, const double *x, double *y, int mode);                 // csx_gaxpy.hip: y += A x, raw pointers
int gaxpy_prepare_device(Csc *A, int mode);                                     // ... the plan `mode` needs, cached on A
int col_block_device(const Csc *A, int32_t first, int32_t count, Csc *C);      // csx_assemble.hip: columns [first, first + count)

// ---- refactor (csx_refactor.hip) ----
// The schedule of a refactor of cs_lu's L, U with new values: A in the factorisation's column order (pattern), pinv (host),
// gid (host: the group of every position; empty = the connected components of L + U).  refactor_run writes the new values
// into Lx, Ux (device scratch) and synchronises; refactor_counts: columns on the device / on the host.
constexpr int RF_MAX = 96;    // rows of the largest group refactored on the device (csx_lu_blocks' and btf's limit)
constexpr int RF_WAVES = 4;   // waves per workgroup, each on a group of its own
int refactor_build(const Csc *A, const int32_t *pinv, const Csc *L, const Csc *U, const std::vector<int32_t> &gid,
                   Refactor **out);
int refactor_run(Refactor *R, const Csc *A, const double *Ax, const Csc *L, const Csc *U, double *Lx, double *Ux, int *ok,
                 double *ratio);
void refactor_counts(const Refactor *R, int64_t *cols);
int rf_gather(int64_t cnt, const int32_t *map, const double *src, double *dst);   // dst[t] = src[map[t]]
int rf_index_copy(const Csc *A, csx_handle_t *out);                                // A's pattern, x[t] = t
int rf_index_map(const double *x, int64_t cnt, DevBuf<int32_t> &map);             // map[t] = (int) x[t]
int rf_keep_pattern(const Csc *A, DevBuf<int32_t> &p, DevBuf<int32_t> &i);
// *differ: a[0 .. cnt) != b[0 .. cnt) somewhere, or a2 / b2 over cnt2; flag: one int of device scratch; synchronises
int rf_differ(int64_t cnt, const int32_t *a, const int32_t *b, int *flag, int *differ, int64_t cnt2 = 0,
              const int32_t *a2 = nullptr, const int32_t *b2 = nullptr);
// the values of A2 (a matrix with the pattern p0 / i0, or a vector of nnz values), CSX_EINVAL for anything else
int rf_values(csx_handle_t A2, int32_t m, int32_t n, int32_t nnz, const int32_t *p0, const int32_t *i0, int *flag,
              const double **x);

// ---- Cholesky refactor (csx_chol.hip, csx_chol_refactor.hip) ----
// The general path's analysis of a factor that exists: tree and counts read off L (host copies Lp_h, and parent_h made by the
// caller), row view from L's pattern, entry map from A's pattern (A: p / i only) through pinv (host, or null).  *foreign: an
// upper entry of A has no slot in L.  Synchronises.
int chol_analysis_of_factor(const Csc *A, const int32_t *pinv, const Csc *L, const int32_t *parent_h, const int32_t *Lp_h,
                            CholAnalysis **out, bool *foreign);
// Lx (lnz doubles, not necessarily L's own) <- the factor of the values Ax on the kept analysis; *notspd: some pivot <= 0.
// done (or null) is recorded after the last launch.  Synchronises.
int chol_analysis_refactor(CholAnalysis *An, const Csc *L, const double *Ax, double *Lx, hipEvent_t done, bool *notspd);
void chol_analysis_info(const CholAnalysis *An, int32_t *info);   // info[1..5] of csx_chol_refactor
int32_t chol_analysis_window(const CholAnalysis *An);             // BW of the k_chol_band instance the last run launched, 0: none
// Lx[q] = win[q] >= 0 ? Ax[win[q]] : 0 over the lnz slots of L (csx_chol_refactor.hip)
int chol_scatter(int64_t lnz, const int32_t *win, const double *Ax, double *Lx);
// csx_chol.hip: the entry map alone (k_chol_winner): win[q] = the entry of A that lands in slot q of L, -1 for fill; *bad
// (device) set when an upper entry of A has no slot; pinv device or null; queued on the context's stream
int chol_entry_map(const Csc *A, const int32_t *pinv, const int32_t *Lp, const int32_t *Li, int32_t lnz, int32_t *win, int *bad);
// csx_cholsym.hip: the pattern of chol(P A P') under the caller's S (host parent, cp, pinv) with its row view; CSX_EINVAL when S
// is not A's
int chol_symbolic_device(const Csc *A, const int32_t *parent, const int32_t *cp, const int32_t *pinv, int32_t **Lp_out,
                         int32_t **Li_out, DevBuf<int32_t> *row_ptr_out, DevBuf<int32_t> *row_col_out, DevBuf<int32_t> *row_pos_out,
                         int32_t *cp_host_out);
// csx_cholsym.hip: the row view of a factor's pattern (col[q] = the column of entry q)
int chol_row_view(int32_t n, int64_t lnz, const uint32_t *col, const int32_t *Li, DevBuf<int32_t> *row_ptr, DevBuf<int32_t> *row_col,
                  DevBuf<int32_t> *row_pos);

// Workgroup barrier that orders LDS only.  __syncthreads() carries a fence over global memory as well: it waits for
// every global load the wave has in flight (s_waitcnt vmcnt(0)), which puts the latency of software-pipelined loads
// back on the critical path of a kernel that synchronises once or twice per step.  Use where only LDS is shared
// across the barrier.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// Magnitudes are compared and reduced as the bit patterns of fabs, unsigned: exact, independent of the order, a NaN above inf.
__device__ __forceinline__ uint64_t abs_bits(double v) { return __builtin_bit_cast(uint64_t, __builtin_fabs(v)); }
__device__ __forceinline__ uint64_t umax64(uint64_t a, uint64_t b) { return a > b ? a : b; }

// sizes
constexpr int WAVE = 64;

}  // namespace csx
