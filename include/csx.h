/* csx.h -- C ABI of libcsx.so, the MI355X (gfx950) implementation of the
 * CSparse.py sparse-direct hot path.
 *
 * The reference (rwl/CSparse.py) is one pure-Python module with no FFI: its
 * "plugin interface" for this path is the module namespace (cs_gaxpy, cs_multiply,
 * cs_transpose, cs_lsolve ... called as `csparse.cs_gaxpy(A, x, y)`,
 * csparse_test.py:24,146,262).  This header is the C boundary the drop-in module
 * csparse.py_amd/csparse.py binds with ctypes; every compute entry point names the
 * reference function (csparse.py:LINE) whose loop it replaces.  INTEGRATION.md
 * shows the binding a reference maintainer would add.
 *
 * Conventions
 *   - extern "C", plain C types only.  Indices are int32_t, values are double
 *     (IEEE binary64, what a Python float is); nnz < 2^31.
 *   - Host buffers belong to the caller.  Device buffers belong to the library,
 *     behind opaque 64-bit handles, unless created with a *_wrap call (then the
 *     caller keeps ownership of the device memory: torch tensors can be passed
 *     as raw device pointers this way).
 *   - Dense right-hand-side blocks are n-by-k, row-major (element (i, r) at
 *     i*k + r): the k values of one matrix row are contiguous.
 *   - Every function returns a status.  No exceptions, no exit().  On
 *     CSX_ERUNTIME the message is in csx_last_error().
 *   - One context per process (one process per GPU).  Calls are serialised on
 *     the context's HIP stream; results are complete after the call returns only
 *     for functions that copy to host, otherwise after csx_sync().
 */
#ifndef CSX_H
#define CSX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef uint64_t csx_handle_t;

enum {
    CSX_OK = 0,
    CSX_EINVAL = 1,     /* bad argument: the Python layer returns False / None / -1 */
    CSX_EZEROPIVOT = 2, /* zero diagonal in a triangular solve: Python raises ZeroDivisionError */
    CSX_ENOTSPD = 3,    /* non-positive pivot in cs_chol: Python returns None (csparse.py:612) */
    CSX_ERUNTIME = 4    /* HIP runtime failure; see csx_last_error() */
};

/* triangular-solve kinds (csparse.py:1330, :1348, :2368, :2460) */
enum { CSX_TRI_L = 0, CSX_TRI_LT = 1, CSX_TRI_U = 2, CSX_TRI_UT = 3 };

/* cs_gaxpy execution modes */
enum {
    CSX_GAXPY_AUTO = 0,  /* best available plan for the matrix */
    CSX_GAXPY_EXACT = 1, /* reference summation order, no FMA: bit-identical to csparse.py:1211-1212 */
    CSX_GAXPY_WAVE = 2,  /* one wavefront (or sub-wave group) per row of the cached transpose */
    CSX_GAXPY_TILED = 3, /* LDS-tiled plan for matrices without locality (G-rand) */
    CSX_GAXPY_ATOMIC = 4 /* direct CSC scatter with fp64 atomics, no plan */
};

/* ---- context ---------------------------------------------------------- */
int csx_init(int device);                 /* idempotent; selects the HIP device, creates the stream */
int csx_finalize(void);                   /* frees every handle and the stream */
const char *csx_last_error(void);
int csx_sync(void);                       /* wait for the context's stream */
int csx_set_stream(void *hip_stream);     /* run on a caller-provided hipStream_t (NULL: own stream) */
int csx_device_info(char *name, int name_cap, int *compute_units, int64_t *hbm_bytes);
/* Device memory is served by a caching allocator (freed blocks are reused instead of returned to the
 * driver; cap = 1/4 of the device, CSX_POOL_LIMIT_MB / CSX_NO_POOL=1 override).  csx_mem_trim returns
 * every idle block to the driver; csx_mem_info reports idle bytes, bytes in use, and hipMemGetInfo's free.
 * Reuse is ordered on the context's stream: a block whose pointer was exported (csx_vec_ptr, csx_csc_ptrs)
 * must not be freed while work on another stream still uses it (csx_free waits for the context's stream only). */
int csx_mem_trim(void);
int csx_mem_info(int64_t *cached_bytes, int64_t *live_bytes, int64_t *device_free_bytes);
/* Kernel-selection overrides, for tests that must reach a kernel the planner would not pick for a given input.
 * Every setting computes correct results; no environment variable changes which kernel runs or what it computes
 * (the environment is read for the allocator's cap above and for CSX_CHOL_TIMING=1, which prints cs_chol's phase
 * times to stderr).  Names (default 1): "chol.dense_trees", "chol.band", "cholsol.dense_blocks", "spgemm.one_pass",
 * "tri.chain_walker", "tri.components", "tri.columns", "tri.push", "tri.row_waves", "gaxpy.keys24"; "gaxpy.tune_shape" (default 0);
 * "gaxpy.shape" (default -1: a tiled csx_gaxpy launches the plan's own shape; 0..3 = that shape, read at every launch); "tri.levels_where" (default 0: level
 * analysis of a triangular plan on the device for big factors and on the host for small ones; 1 = host, 2 = device);
 * "chol.wband" (blocked dense-band cs_chol for chain-like factors: default 1 = for half-widths above 80, 0 = never,
 * 2 = whenever the tree is chain-like) and "chol.wband_nb" (columns per step: 16 (default) or 32; any other value
 * reads back as 16); "chol.supernodes" (default 1); "pool.limit_mb" (cap of the device-memory cache in MB,
 * 0 = the default quarter of the device).  Round 3: "tri.supernodes" (supernodal schedule of a cholsol plan in the
 * rounding-equal order: 1 = yes, triangles on the matrix cores where their guard allows (default); 2 = yes, triangles by
 * substitution out of LDS, no relaxed supernodes; 0 = never), "tri.graph" (the launches of a supernodal solve captured
 * into a hipGraph and replayed while the block of right-hand sides stays in place: 2 (default) = when a solve is more than
 * 256 launches and the block has been the block of the two solves before it as well (round 5; round 4 captured on the second
 * solve of a block, which cost more than it saved), 1 = always, 0 = never),
 * "spgemm.ordered" (default 0; 1 = cs_multiply sums every entry's products in the reference's order: bit-identical
 * values, about twenty times the time),
 * "sort.short_keys" (default 1: a transpose with values carries 16-bit keys between its radix passes where the matrix allows),
 * "lu.etree" (cs_lu inside one connected matrix by levels of the column elimination tree: 0 = never (default since round
 * 4: at best a tie with one host core), 1 = shallow trees with short columns, 2 = always).  Round 4:
 * "chol.clique" (default 1: csx_schol / csx_chol / csx_cholsol_plan recognise forests of cliques on consecutive columns
 * -- block-diagonal matrices with dense blocks -- from the matrix itself and skip the general pattern machine; 0 = the
 * general path), "chol.forest" (default 1: where that rule fails, csx_schol / csx_chol look for blocks of <= 64 consecutive
 * columns closed under their upper entries -- forests of small sparse trees -- and analyse / factor a block in one wave;
 * 0 = the general path for them).  Round 5: "chol.exact" (default 1: cs_chol's block kernel keeps the reference's operations and
 * their order, L.x bit-identical; 0, opt-in: fused multiply-adds and refined reciprocal square roots in that kernel -- forests of
 * dense blocks only -- L.x equal to rounding; equal blocks of 16 / 32 / 48 / 64 columns are then factored on the matrix cores, 1.8x
 * the rate), "tri.host_chains" (default 0; 1: csx_tri_solve_list / csx_cholsol_solve_list take one host right-hand side on a
 * chain-like factor to the host).  "gaxpy.block_route" (default 0: csx_gaxpy_block AUTO's own rule; 1 = the block kernel,
 * 2 = the column route).  Unknown name: CSX_EINVAL. */
int csx_set_option(const char *name, int value);
int csx_get_option(const char *name, int *value);   /* the value in force (after csx_set_option's normalisation) */
int csx_timer_start(void);                /* hipEvent on the context's stream */
int csx_timer_stop(double *ms);           /* second hipEvent, synchronises, elapsed ms */

/* ---- CSC matrices: the reference's `cs` object with nz == -1 (csparse.py:37-54) ---- */
int csx_csc_upload(int32_t m, int32_t n, const int32_t *p, const int32_t *i, const double *x /* or NULL */,
                   csx_handle_t *out);
int csx_csc_alloc(int32_t m, int32_t n, int32_t nnz, int values, csx_handle_t *out);
int csx_csc_wrap(int32_t m, int32_t n, int32_t nnz, void *d_p, void *d_i, void *d_x /* or NULL */,
                 csx_handle_t *out);
int csx_csc_info(csx_handle_t A, int32_t *m, int32_t *n, int32_t *nnz, int *has_values);
int csx_csc_download(csx_handle_t A, int32_t *p, int32_t *i, double *x /* or NULL */);
int csx_csc_ptrs(csx_handle_t A, void **d_p, void **d_i, void **d_x);
/* csx_gaxpy caches plans on the matrix (a row-major copy, the LDS-tiled regrouping) that hold COPIES of its
 * values and structure; csx_schol leaves its finding there when the matrix is a forest of cliques (tree, counts, block list: pattern
 * only), for the csx_chol that follows.  Arrays handed out by csx_csc_ptrs, or wrapped by csx_csc_wrap, must not be changed
 * in place without telling the library: call csx_csc_invalidate afterwards (drops the cached plans; the next
 * csx_gaxpy rebuilds them).  Plans that are handles of their own (csx_tri_analyse, csx_cholsol_plan) also copy
 * the values they need: rebuild them after a change. */
int csx_csc_invalidate(csx_handle_t A);
int csx_free(csx_handle_t h);             /* any handle kind; handles carry a generation, a stale one is CSX_EINVAL */

/* ---- dense vectors / row-major blocks (float64) and index vectors (int32) ---- */
int csx_vec_alloc(int64_t len, csx_handle_t *out);          /* zero-filled */
int csx_vec_upload(const double *src, int64_t len, csx_handle_t *out);
int csx_vec_wrap(void *d_ptr, int64_t len, csx_handle_t *out);
int csx_vec_download(csx_handle_t v, double *dst, int64_t len);
int csx_vec_write(csx_handle_t v, const double *src, int64_t len);
int csx_vec_fill(csx_handle_t v, double value);
int csx_vec_copy(csx_handle_t src, csx_handle_t dst);
int csx_vec_ptr(csx_handle_t v, void **d_ptr, int64_t *len);
int csx_ivec_upload(const int32_t *src, int64_t len, csx_handle_t *out);
int csx_ivec_download(csx_handle_t v, int32_t *dst, int64_t len);

/* ---- hot path --------------------------------------------------------- */

/* cs_gaxpy, csparse.py:1199-1213: y += A x.  x has >= n, y >= m entries. */
int csx_gaxpy(csx_handle_t A, csx_handle_t x, csx_handle_t y, int mode);
/* Build (and cache on A) the plan `mode` needs, outside any timed region. */
int csx_gaxpy_prepare(csx_handle_t A, int mode);
/* Which plans the matrix holds: the row-major copy (EXACT / WAVE), the LDS-tiled regrouping (TILED), and the bytes
 * per key of the latter: 4 (column, row packed) or 3 (row + 9-bit column offset inside a run of 64 column-sorted
 * entries; chosen when every run is narrower than 512 columns); 0 without a tiled plan.  Any pointer may be NULL. */
int csx_gaxpy_plan_info(csx_handle_t A, int *has_rows, int *has_tiled, int *key_bytes);
/* With csx_set_option("gaxpy.tune_shape", 1) (default 0) the tiled plan times its launch shapes (waves per workgroup
 * x groups per wave and step: same kernel, plan and results) on the device when it is built and keeps the fastest:
 * *shape = 0 (4 x 5), 1 (2 x 10), 2 (8 x 4), 3 (2 x 8), or -1 (not timed: 4 x 5); ms4[0..3] = the candidates' ms per
 * pass (0 when not timed).  CSX_EINVAL without a tiled plan. */
int csx_gaxpy_plan_shape(csx_handle_t A, int *shape, double *ms4);
/* csx_set_option("gaxpy.shape", s) (default -1: the plan's own shape; 0..3 = that shape whatever the plan picked; any other
 * value reads back as -1) is read at every tiled csx_gaxpy, not when the plan is built: one plan runs at all four shapes,
 * with the same results up to the order of the LDS additions.  The tuner times every candidate whatever it says.
 * csx_gaxpy_plan_geometry: info[10] = rows per row block, row blocks, column slabs, columns per slab, bits of the row
 * field of a 4-byte key, groups of 256 entries (padding included), bytes per key (3 or 4), the launch shape in force (0..3:
 * "gaxpy.shape" if set, otherwise the plan's own, 0 when it was not timed), the fewest and the most groups of a row block.
 * csx_gaxpy_plan_groups: groups[b] = groups of row block b, for all info[1] row blocks.  Both CSX_EINVAL without a tiled
 * plan. */
int csx_gaxpy_plan_geometry(csx_handle_t A, int64_t *info);
int csx_gaxpy_plan_groups(csx_handle_t A, int32_t *groups);
/* One-shot form for host arrays (the reference's list signature): y[0..m) += A x in the reference's
 * summation order (bit-identical), nothing left on the device.  x (values) must be present. */
int csx_gaxpy_host(int32_t m, int32_t n, const int32_t *p, const int32_t *i, const double *x, const double *xv,
                   double *yv);
/* Y[0..m) x [0..nrhs) += A X, X n-by-nrhs and Y m-by-nrhs, both row-major (csparse.py:1199-1213 applied to
 * every column).  mode: CSX_GAXPY_EXACT or CSX_GAXPY_AUTO; any other mode is CSX_EINVAL.
 *   EXACT  every column of Y bit-identical to csx_gaxpy(..., CSX_GAXPY_EXACT) on that column; deterministic.
 *   AUTO   the block kernel (the same kernel and bits as EXACT) or, for blocks of at most 4 columns on a matrix
 *          for which csx_gaxpy AUTO uses the LDS-tiled plan, the column route: csx_gaxpy AUTO once per column on
 *          transposed copies of X and Y (n nrhs + m nrhs doubles of device memory for the call), every column
 *          bit-identical to csx_gaxpy AUTO on it.  Deterministic wherever csx_gaxpy AUTO is, i.e. except on the
 *          column route (the tiled plan sums in LDS with atomics).  csx_set_option("gaxpy.block_route", 1 | 2)
 *          forces the block kernel | the column route (0: the rule above).
 * nrhs == 1 is csx_gaxpy with the same mode.  Reads A's cached row gather (csx_gaxpy_prepare(A, CSX_GAXPY_EXACT)
 * builds it ahead of time); AUTO makes csx_gaxpy AUTO's plan decision first, the same way.  CSX_EINVAL for a
 * pattern-only A, nrhs < 1, X shorter than n nrhs or Y shorter than m nrhs entries, X and Y the same handle or
 * overlapping device ranges.  m == 0, n == 0 or nnz == 0: nothing to do, CSX_OK. */
int csx_gaxpy_block(csx_handle_t A, csx_handle_t X, csx_handle_t Y, int32_t nrhs, int mode);

/* ---- residual and componentwise backward error of a block of solutions ----
 * R = B - op(A) X for row-major blocks of nrhs columns, with the componentwise backward error of every column.
 * trans == 0: op(A) = A (m x n): X has >= n nrhs, B and R >= m nrhs entries; reads A's cached row gather
 *             (built on demand, as csx_gaxpy_block does).
 * trans != 0: op(A) = A' (n x m): X has >= m nrhs, B and R >= n nrhs entries; reads A.p / A.i / A.x as they are stored:
 *             no plan is built or needed.
 * R == 0: the residual is not stored (omega / rnorm only).  omega, rnorm: host arrays of nrhs doubles, either may be NULL.
 * One order, fixed by the matrix, the same on the device and on the host: for output row i of op(A) and column c the
 * row's terms (a_q, j_q) in the row gather's order (ascending (column, storage position); trans == 0) or in the storage
 * order of column i of A (trans != 0):
 *     r = B[i,c];    for each term:  t = a_q * X[j_q,c]      (rounded);   r = r - t   (rounded)
 *     d = |B[i,c]|;  for each term:  u = |a_q| * |X[j_q,c]|  (rounded);   d = d + u   (rounded)
 *     ratio[i,c] = 0 when |r| == 0 and d == 0, else |r| / d   (IEEE division; NaN and inf propagate)
 *     omega[c] = max_i ratio[i,c],  rnorm[c] = max_i |r|      (0 for an operator without rows)
 * The maxima are taken over the bit patterns of the non-negative doubles: a NaN in a column makes its omega and rnorm
 * NaN, and no run depends on an order.  R may be the same handle as B (in place).  CSX_EINVAL for a pattern-only A,
 * nrhs < 1, short blocks, R or B the same handle as X, overlapping device ranges (R and B: anything but the same
 * range).  m == 0, n == 0 or nnz == 0 are legal: R = B, omega by the 0 / 0 rule, rnorm = max |B|. */
int csx_residual_block(csx_handle_t A, csx_handle_t X, csx_handle_t B, csx_handle_t R, int32_t nrhs, int trans,
                       double *omega, double *rnorm);
/* the same rule on host arrays (no device); R may be B or NULL */
int csx_residual_host(int32_t m, int32_t n, const int32_t *p, const int32_t *i, const double *x, int32_t nrhs, int trans,
                      const double *X, const double *B, double *R /* or NULL */, double *omega, double *rnorm);
/* ---- the same for the symmetric matrix a Cholesky factorisation sees in A ----
 * R = B - S X for row-major blocks of nrhs columns (each >= n nrhs entries), with the componentwise backward error of every
 * column, where S is what csx_chol reads of the n x n matrix A: the stored entries with row <= column, mirrored below the
 * diagonal.  The strictly lower entries of A are never used as values, so a matrix stored as its upper triangle, stored in
 * full, or carrying other values below the diagonal give the same bytes.  A's columns may be unsorted and hold duplicates
 * (summed, as a matrix sums them; csx_chol keeps the last duplicate of an entry, so the two agree only on matrices without
 * duplicates in the upper triangle).  Reads A.p / A.i / A.x as stored AND A's cached row gather (built on demand).
 * One order, the same on the device and on the host: for output row i and column c the terms (a, j) are
 *     phase 1: the entries q of stored column i, in storage order, with A.i[q] <= i:  (A.x[q], A.i[q])
 *     phase 2: the entries of row i in the row gather's order (ascending (column, storage position)) with column > i:
 *              (value, column)
 * and with them
 *     r = B[i,c];    for each term:  t = a * X[j,c]      (rounded);   r = r - t   (rounded)
 *     d = |B[i,c]|;  for each term:  u = |a| * |X[j,c]|  (rounded);   d = d + u   (rounded)
 *     ratio[i,c] = 0 when |r| == 0 and d == 0, else |r| / d   (IEEE division; NaN and inf propagate)
 *     omega[c] = max_i ratio[i,c],  rnorm[c] = max_i |r|      (0 for n == 0)
 * An entry that fails its phase's test is skipped, never added as a zero.  A strictly upper entry is used twice (once per
 * phase, in two rows), a diagonal entry once.  For a fully stored symmetric matrix with sorted columns the terms of every
 * row are those of csx_residual_block(trans = 0), and so are the bytes.  The maxima are taken over the bit patterns of
 * the non-negative doubles.  R == 0, R the same handle as B, omega and rnorm as in csx_residual_block.  CSX_EINVAL for
 * m != n, a pattern-only A, nrhs < 1, short blocks, R or B the same handle as X, overlapping device ranges (R and B:
 * anything but the same range).  n == 0 is legal; nnz == 0: R = B. */
int csx_residual_sym_block(csx_handle_t A, csx_handle_t X, csx_handle_t B, csx_handle_t R, int32_t nrhs, double *omega,
                           double *rnorm);
/* the same rule on host arrays (no device; the row order is built by the call); R may be B or NULL */
int csx_residual_sym_host(int32_t n, const int32_t *p, const int32_t *i, const double *x, int32_t nrhs, const double *X,
                          const double *B, double *R /* or NULL */, double *omega, double *rnorm);
/* *out = |S|_1 = max_i sum |a| over row i's terms, in the rule's order (phase 1, then phase 2; sequential, rounded), the
 * maximum over the bit patterns.  CSX_EINVAL for m != n or a pattern-only A; 0.0 for n == 0. */
int csx_norm1_sym(csx_handle_t A, double *out);
/* out[i, c] = mask[c] ? X[i, c] + D[i, c] : X[i, c]   (one rounding);   dst[i, c] = src[i, c] where mask[c].
 * mask: nrhs host int32, uploaded by the call.  Blocks of rows x nrhs, row-major; out may be X or D, src and dst apart. */
int csx_block_add_cols(csx_handle_t X, csx_handle_t D, csx_handle_t out, int64_t rows, int32_t nrhs, const int32_t *mask);
int csx_block_select_cols(csx_handle_t src, csx_handle_t dst, int64_t rows, int32_t nrhs, const int32_t *mask);

/* cs_transpose, csparse.py:2292-2315: stable counting sort by row. */
int csx_transpose(csx_handle_t A, int values, csx_handle_t *out);

/* cs_cumsum, csparse.py:767-784, on int32 device vectors: p[0..n] = exclusive
 * scan of c[0..n-1], c overwritten with p[0..n-1]; *total = sum. */
int csx_cumsum(csx_handle_t p, csx_handle_t c, int64_t n, int64_t *total);

/* The integer primitives under every structure of this library (csx_sort.hip), one at a time, for the tests: each csx_prim_*
 * below copies its HOST arrays to device buffers, runs the one primitive as its callers run it, and copies the results back.  The
 * device copies of the inputs are copied back over the host arrays as well, so that a primitive that wrote to an input shows;
 * outputs are uploaded before the run, so that slots a primitive must leave alone can be told by what the caller put there, and
 * every output array has guard bytes behind it on the device: a store past its end is CSX_ERUNTIME, with the reason.
 * Production code calls none of them.  CSX_EINVAL, before anything touches the device: a negative count, a missing array, an
 * output missing where its input is given, misalign_words outside 0 .. 3, column pointers that do not run from 0 to the count
 * without decreasing, keys that are not below nkeys where a pointer array is written (or, for csx_prim_boundaries, not sorted).
 * csx_prim_limits: the constants the primitives are cut by, without a device: out[9] = SCAN_TILE (elements a workgroup of the
 * scan, and one level of its recursion), SM_TILE (the same of the reverse running minimum), RS_TILE (records a workgroup of the
 * radix sort), RS_BINS (bins of a digit), RS_DESC_STARTS (column starts a tile descriptor holds), RS_SEGS (segments the chunk
 * scan splits the chunks over), RS_CHUNK_MIN (tiles a chunk of the digit scan at least), RS_CHUNK_DIV (chunks at most),
 * EXPAND_GRID_MAX (workgroups of four columns each that expand_columns launches at most).
 * csx_prim_scan: out[0 .. n] = the exclusive sums of in[0 .. n-1] (scan_exclusive_i32), *total (or NULL) = out[n]; in_place != 0:
 * one device array is input and output, as the tiled gaxpy plan and the symbolic Cholesky call it (`in` is then not written).
 * csx_prim_suffix_min: p[r] = min(p[r .. n-1]) in place (suffix_min_i32).
 * csx_prim_expand_columns: col[q] = j for q in [Ap[j], Ap[j+1]) (expand_columns); Ap[n] = nnz.
 * csx_prim_boundaries: ptr[r] = the first position whose key is >= r, r in [0, nkeys] (boundaries_from_sorted).
 * csx_prim_sort: stable_sort_by_key_ex.  a, v, out_key, expand_ptr, out_ptr may each be NULL as there (a and expand_ptr not both
 * given); out_a is the sorted a, or with expand_ptr (expand_n columns over the count positions) the column of every sorted
 * record; out_ptr[0 .. nkeys] the first slot of every key.
 * misalign_words (both): the device key array starts that many 4-byte words past a 16-byte boundary, which the row indices of a
 * wrapped matrix (csx_csc_wrap) may do; the kernels that read keys 16 bytes at a time then take their one-by-one path.
 * csx_prim_sort_info (host state only, nothing is launched): what the last sort of this process decided, out[0 .. min(cap, 17)):
 * bits (of key_limit - 1), passes, the digit width of passes 0 .. 3 (0: no such pass), nblocks (tiles), chunk, nchunks, packed
 * ((a, v) travel as 12-byte records between passes), k16 (the short-key mode), the 4-byte words the key array lay past a 16-byte
 * boundary, the k_rs_scatter instance passes 0 .. 3 launched (0 none, 1 keys only, 2 a, 3 v, 4 a + v arrays in and out, 5 arrays
 * in and records out, 6 records in and out, 7 records in and arrays out, 8 / 9 / 10 the first / middle / last pass of the short-key
 * mode), count (0: that sort was empty and launched no pass). */
int csx_prim_limits(int32_t *out);
int csx_prim_scan(int32_t *in, int32_t *out, int64_t n, int in_place, int64_t *total);
int csx_prim_suffix_min(int32_t *p, int64_t n);
int csx_prim_expand_columns(int32_t *Ap, int32_t n, int32_t nnz, int32_t *col);
int csx_prim_boundaries(uint32_t *sorted_key, int64_t count, int32_t nkeys, int32_t *ptr, int misalign_words);
int csx_prim_sort(uint32_t *key, uint32_t *a, double *v, int64_t count, uint32_t key_limit, uint32_t *out_key, uint32_t *out_a,
                  double *out_v, int32_t *expand_ptr, int32_t expand_n, int32_t *out_ptr, int32_t nkeys, int misalign_words);
int csx_prim_sort_info(int64_t *out, int32_t cap);

/* cs_multiply (+ cs_scatter), csparse.py:1608-1642, :1961-1989: C = A*B with
 * each column of C in first-touch order; pattern only if A or B has no values.
 * p[] and i[] are exactly the reference's.  x[]: the products of an entry are summed by LDS / memory atomics in the
 * order they arrive, not in the reference's order, so x[] equals the reference's to rounding (tests: 1e-10 relative to
 * the sum of |products|) and may differ in the last bits from one run to the next -- the one result of this library
 * that is not reproducible bit for bit.  The same holds for the sums cs_dupl and cs_add form from duplicate entries
 * (csx_dupl, csx_add); entries without duplicates come out exact. */
int csx_multiply(csx_handle_t A, csx_handle_t B, csx_handle_t *out);
/* Read-backs of cs_multiply's decisions for the tests (host state only; neither launches anything, production code calls neither).
 * csx_spgemm_limits: the constants csx_spgemm.hip is cut by, without a device: out[40] = SG_SEG (entries of B(:,j) the two-pass
 * kernel stages at a time), SG_THREADS, SG_DENSE_MAX (rows up to which the accumulator is dense in LDS), SG_GLOBAL_WGS
 * (workgroups with an accumulator in memory), SG_HASH_MAXP (products a column of the hash bins may have), the products a column of
 * hash bin 0 .. 7 may have, H2_MAXSEG, H2_MAXLEN, H2_MAXP (entries of B(:,j), entries of the longest column of A it names and
 * products of a narrow column), H1_SEG, H1_MAXP, H1_UN (entries staged, bitmap bits, entries in flight per half-wave of the
 * general one-pass kernel), SGO_MAX (entries of C(:,j) up to which the ordered pass keeps its sums in LDS), (slots, entries) of
 * its three size classes, SGO_DENSE_WAVES (waves of its dense-map kernel at most), SG_GRID_PER_CU (workgroups per CU of the
 * two-pass grid), the number of fields of csx_spgemm_info, the waves per CU of the three ordered classes, SG_UN (256-product
 * chunks per step of the two-pass kernel), SG_MIN_SLOTS (the smallest two-pass table), SG_LDS_BUDGET and SG_WGS_PER_CU_MAX (the
 * one-pass grids hold min(SG_WGS_PER_CU_MAX, SG_LDS_BUDGET / (LDS of a workgroup + 256)) workgroups per CU), the number of hash
 * bins, of narrow bins, of launch sites, 0.
 * csx_spgemm_info: what the last C = A*B on the device of this process decided (csx_multiply, and csx_add / csx_assemble where
 * they multiply): out[0 .. min(cap, *count)) written, *count (or NULL) = the number of fields.  The fields: the columns of C in
 * each of the 32 bins (0 dense LDS, 1 .. 8 hash by products, 9 .. 14 narrow by products, 15 memory accumulator, 31 no product;
 * all 0 when the product was empty by its shape), whether the one-pass path ran, the workgroups with an accumulator in memory,
 * the CUs the grids were cut by, whether the ordered pass ran, the four flags of the ordered pass (some column of C in class 0,
 * 1, 2, beyond SGO_MAX); then for every launch site first the launches, then (again for every site) the grid of its last launch.
 * The sites: k_sg_products; k_spgemm as 3 * (0 symbolic, 1 numeric with values, 2 numeric pattern-only) + (0 dense, 1 hash,
 * 2 memory); k_sg_hash1 as 8 * (values) + hash bin; k_sg_hash2 as 6 * (values) + narrow bin; k_sg_compact; k_sg_dup_cols;
 * k_sg_values_ordered2 by class; k_sg_values_ordered.  A counter is bumped beside the launch call: a launch that fails is counted
 * too, and the call then returns its error. */
int csx_spgemm_limits(int32_t *out);
int csx_spgemm_info(int64_t *out, int32_t cap, int32_t *count);

/* cs_lsolve / cs_ltsolve / cs_usolve / cs_utsolve, csparse.py:1330-1365,
 * :2368-2385, :2460-2475.  Analyse once (level sets, gather layout in the
 * reference's update order, zero-pivot check), then solve any number of
 * right-hand sides in place: X is n-by-nrhs, row-major. */
int csx_tri_analyse(csx_handle_t T, int kind, csx_handle_t *plan);
int csx_tri_info(csx_handle_t plan, int32_t *n, int32_t *levels, int32_t *sequential);
int csx_tri_solve(csx_handle_t plan, csx_handle_t X, int32_t nrhs);
/* The order of a plan's solves.  exact = 1 (the default of every plan): the reference's operations in the reference's order,
 * bit-identical to cs_lsolve / cs_ltsolve / cs_usolve / cs_utsolve (csparse.py:1330-1365, :2368-2385, :2460-2475).  exact = 0
 * (round 5): equal to rounding (x[] within 1e-10).  It changes the solve of a factor that falls into many small independent
 * components of at most 80 rows with more than 8 right-hand sides: every component is made dense in sweep order, padded to a
 * multiple of 16 and solved as a blocked substitution on the matrix cores (16 x 16 tiles, explicit inverses of the diagonal
 * tiles, built at the first such solve) -- unless || |inv(T_ii)| |T_ii| ||_inf of a diagonal tile exceeds 1e3, then the exact
 * kernels stay.  Every other plan shape solves exactly in either order.  csx_tri_order_info: whether the matrix-core form is in
 * use (after the first solve in that order) and the guard's measure; either pointer may be NULL. */
/* "tri.host_chains" = 1 (csx_set_option; opt-in, default 0): ONE right-hand side in host memory on a factor whose dependency graph
 * is a chain (more than n / 4 levels, fewer than 5e7 entries) is solved by the reference's own loop on the host, on a copy of the
 * factor the plan downloads once -- the same operations in the same order, the same bits, 10 - 40x sooner than one dependent
 * subtraction per term on the device.  *taken = 0: the option is off or the factor is no chain: x untouched, call csx_tri_solve.
 * csx_cholsol_solve_list: the same for cs_cholsol's whole solve sequence (csparse.py:640-643) on b[n]. */
int csx_tri_solve_list(csx_handle_t plan, double *x, int *taken);
int csx_cholsol_solve_list(csx_handle_t plan, double *b, int *taken);
int csx_tri_set_order(csx_handle_t plan, int exact);
int csx_tri_order_info(csx_handle_t plan, int32_t *matrix_cores, double *growth);
/* After the first solve: the number of connected components of the dependency graph when the plan solves
 * them one wave each (many components of <= 256 rows: block-diagonal factors), 0 when it level-schedules. */
int csx_tri_components(csx_handle_t plan, int32_t *ncomp);
/* Read-backs of the triangular solve's decisions for the tests (host state only; none of them launches a solve kernel).
 * csx_tri_limits: the constants tri_route, make_segments, walk_levels and analyse cut by, without a device: out[32] = NARROW, CHB,
 * CH_SUF, TRW_MIN_ROW, TRW_MAX_RHS, TR64_MIN_RHS, TR64_RUN, TR64_RUN_MIN, TC_MAX_N, TC_THREADS, COMP_MIN_COUNT, COMP_MAX_ROWS,
 * PUSH_MAX_RHS (right-hand sides of the column-push component sweep), FEW_MAX_RHS (of the few-right-hand-side sweeps), FEW_CPW
 * (components per wave of the all-in-LDS one), COMP_LDS_MAX, FEW_TILE_LDS, WINDOW_LDS_MAX, COLUMNS_LDS_MAX (bytes of LDS: the
 * component sweeps' programs, the X tiles of k_tri_few, the window of x, x of one right-hand side), CHAIN_LINKS_NUM,
 * CHAIN_LINKS_DEN (a chain by its links: links * NUM > n * DEN), CHAIN_LEVELS_NUM (by its levels: levels * NUM > n),
 * WCOL_WIDE_ENTRIES, WCHAIN_WIDE_ENTRIES (entries a column above which the window kernels take 1 024 threads / 12 rounds),
 * WINDOW_SLACK (the window holds band + so many entries of x), STRIP_SHORT_COLS (entries a column from which analyse strips the
 * diagonals of L 64 lanes a column), TL_WAVES_MAX, LV_MAX_ROUNDS, LV_DEVICE_MIN_TERMS, the number of counters of
 * csx_tri_launches, 0, 0.
 * csx_tri_route_info: what csx_tri_solve(plan, X, nrhs) would run in the process's order, and what decided it (the plan's lazy
 * analyses run as far as that decision needs them, as in a solve).  30 fields: route (0 Ragged, 1 CompPush, 2 FewLds, 3 Few,
 * 4 Local, 5 WColumns, 6 WColChain, 7 Columns, 8 ColChain, 9 Sequential, 10 Levels), and of the route taken lds (bytes of dynamic
 * LDS), grid, G, waves, tile_rows, chunks, window, threads, rounds, mate; then the plan's facts: band (-1: not measured,
 * 0x7fffffff: no proper triangle), links, col_state (0 not examined, 1 columns may be pushed, 2 a row twice in a column),
 * levels (0: not scheduled), sequential, chain_ok, ncomp and comp_max (0: no component route), push_terms, few_cpw, few_rows,
 * few_terms, the matrix-core guard (0 not asked, 1 passed, 2 refused, 3 NaN), the schedule's source (0 none, 1 the caller's
 * hint, 2 the device pass, 3 the host pass, 4 the host pass after the device pass gave up at LV_MAX_ROUNDS), the components and
 * the rows of the largest one as found (kept or not), kind, n, the terms of the gather structure.
 * csx_tri_launches: how many launches of each solve-kernel instance the plan's last solve enqueued (a fused csx_lusol_solve
 * counts on both plans), 30 counters: k_tri_level, k_tri_levels_one_wg, k_tri_chain, k_tri_sequential, k_tri_local<true>,
 * <false>, k_tri_few<true>, <false>, k_tri_few_lds<true, 4>, <false, 4>, k_tri_comp_push<true>, <false>, the matrix-core sweep
 * (ragged_solve), k_tri_columns<L>, <U>, k_tri_colchain<LT>, <UT>, k_tri_wcolumns<256>, <1024>, k_tri_wcolchain<LT, 2>, <LT, 12>,
 * <UT, 2>, <UT, 12>, k_tri_level_rows, k_tri_run_prefix_rows, k_tri_levels_rows_one_wg, k_tri_level_rows64, k_tri_run_prefix64,
 * k_tri_levels_rows64_one_wg, k_tri_level_of.
 * A counter is bumped beside the launch call: a launch that fails is counted too, and the solve then returns its error.
 * The last two: out[0 .. min(cap, *count)) written, *count = the number of fields; CSX_EINVAL for a handle that is no plan.
 * csx_cholsol_tri_route_info / csx_cholsol_tri_launches: the same two of the triangular plans inside a csx_cholsol_plan
 * (backward = 0: the plan of L x = b, 1: of L' x = b), in the order that plan solves in (csx_cholsol_set_order: its rounding-equal
 * order is the relaxed order of the level walk and lets L' run on the rows of L, mate = 1); CSX_EINVAL when the plan holds no
 * triangular plans (a forest of cliques). */
int csx_tri_limits(int32_t *out);
int csx_tri_route_info(csx_handle_t plan, int32_t nrhs, int64_t *out, int32_t cap, int32_t *count);
int csx_tri_launches(csx_handle_t plan, int64_t *out, int32_t cap, int32_t *count);
int csx_cholsol_tri_route_info(csx_handle_t plan, int backward, int32_t nrhs, int64_t *out, int32_t cap, int32_t *count);
int csx_cholsol_tri_launches(csx_handle_t plan, int backward, int64_t *out, int32_t cap, int32_t *count);

/* cs_ipvec / cs_pvec, csparse.py:1264-1277, :1779-1792, on n-by-nrhs blocks:
 * inverse != 0: x[p[k], :] = b[k, :] (ipvec); else x[k, :] = b[p[k], :] (pvec).
 * p == 0 is the identity permutation. */
int csx_permute_vec(csx_handle_t p, csx_handle_t b, csx_handle_t x, int32_t n, int32_t nrhs, int inverse);
/* The solve phase of cs_lusol for an n-by-nrhs block, csparse.py:1470-1473 (cs_ipvec(pinv), cs_lsolve, cs_usolve, cs_ipvec(q)):
 * b overwritten with the solutions; planL / planU: csx_tri_analyse plans of L (CSX_TRI_L) and U (CSX_TRI_U); pinv, q: int vectors
 * or 0 (identity); work: another n-by-nrhs block.  Each plan solves in the order csx_tri_set_order gave it.  When both are
 * in the rounding-equal order and both factors are forests of small components, the two permutations are fused into the two
 * sweeps (four passes over the block instead of eight): *fused = 1.  Otherwise the four steps run one after the other. */
int csx_lusol_solve(csx_handle_t planL, csx_handle_t planU, csx_handle_t pinv, csx_handle_t q, csx_handle_t b, csx_handle_t work,
                    int32_t nrhs, int *fused);
/* The transposed solve A' x = b on the same factors (L U = A(p, q)): y = b(q) (cs_pvec), cs_utsolve(U),
 * cs_ltsolve(L), x = y(pinv) (cs_pvec).  planUT / planLT: csx_tri_analyse plans of U (CSX_TRI_UT) and L (CSX_TRI_LT); the
 * rest as csx_lusol_solve, the same validation and errors (CSX_EINVAL also for plans of another kind).  Fused (*fused = 1)
 * in the same cases: the sweep over U' loads its rows through q, the sweep over L' stores them through p = inverse(pinv). */
int csx_lusol_solve_trans(csx_handle_t planUT, csx_handle_t planLT, csx_handle_t pinv, csx_handle_t q, csx_handle_t b,
                          csx_handle_t work, int32_t nrhs, int *fused);

/* cs_schol (natural order), csparse.py:2051-2072: host C++ symbolic analysis of
 * the upper triangle of a host CSC pattern.  parent[n], cp[n+1]. */
int csx_schol_host(int32_t n, const int32_t *Ap, const int32_t *Ai, int32_t *parent, int32_t *cp);
/* cs_counts, csparse.py:703-764: column counts of chol(A) (ata = 0; A square, upper triangle used) or chol(A'A) (ata != 0;
 * A m-by-n) from the elimination tree parent[n] and its postorder post[n] (cs_etree / cs_post of the same matrix), host C++.
 * colcount[n].  CSX_EINVAL for an index out of range, a parent outside [-1, n), a post that is no permutation. */
int csx_counts_host(int32_t m, int32_t n, const int32_t *Ap, const int32_t *Ai, const int32_t *parent, const int32_t *post,
                    int ata, int32_t *colcount);
/* The same for a device-resident square matrix.  A forest of cliques on consecutive columns (block-diagonal with dense
 * blocks; recognised in one pass over A's pattern from the smallest upper row of every column): tree and counts on the
 * device, no pattern of L formed.  Otherwise: elimination tree on the device for many small components, else on the
 * host; column counts of L on the device (the row-subtree walks of csx_chol).  parent[n] and cp[n+1] are host arrays. */
int csx_schol(csx_handle_t A, int32_t *parent, int32_t *cp);

/* A fill-reducing ordering for order = 1 (Cholesky; the reference's cs_amd, csparse.py:214-556, does not
 * run): nested dissection of the graph of A + A' by breadth-first level separators, which yields the wide
 * elimination-tree levels the device kernels want.  Host arrays; perm[k] = original index of the k-th
 * row/column of P A P'. */
int csx_order_nd_host(int32_t n, const int32_t *Ap, const int32_t *Ai, int32_t *perm);

/* cs_chol numeric, csparse.py:561-619.  A: device CSC (upper triangle used);
 * parent/cp: host arrays from csx_schol / csx_schol_host; pinv: host permutation or NULL.
 * Output L (device CSC, diagonal first, rows ascending).  CSX_EINVAL when parent / cp are not A's. */
int csx_chol(csx_handle_t A, const int32_t *parent, const int32_t *cp, const int32_t *pinv,
             csx_handle_t *L);
/* What the last successful csx_chol of this process did.  *path: 1 = A's elimination forest is a set of cliques on
 * consecutive columns (block-diagonal with dense blocks of <= 64 columns; recognised from A itself, L.p / L.i follow from
 * the counts, every block factored in the registers of one wave, L.x bit-identical to csparse.py:587-617), 2 = blocks of
 * <= 64 consecutive columns closed under their upper entries whose trees are NOT cliques (symbolic elimination on 64-bit row
 * masks in one wave per block, the same block kernel with a compacted store; L.x bit-identical where the trees are chains,
 * equal to rounding where they branch -- as path 0; "chol.forest" = 0 switches this recognition off), 0 = the general
 * path (pattern of L by row-subtree walks and sorts, column kernels by tree level).  *numeric_ms: HIP-event time of the
 * numeric part (path 1: the block kernel alone; path 0: everything after the pattern of L).  Either pointer may be NULL;
 * CSX_EINVAL before the first csx_chol.  "chol.clique" = 0 (csx_set_option) forces path 0. */
int csx_chol_info(int32_t *path, double *numeric_ms);

/* The solve phase of cs_cholsol, csparse.py:640-643, for nrhs right-hand sides:
 * B (n-by-nrhs, row-major) is overwritten with the solutions.  The plan of a factor that is a forest of equal dense
 * blocks of 8 / 16 / 32 / 64 columns (recognised from L itself, also from an L that came over the wire or from the host)
 * is the block list: the default exact kernel and the matrix-core kernel read the blocks' packed columns in L.x itself (round 5);
 * any other factor gets two triangular-solve analyses and the forest partition.  The plan BORROWS L's arrays either way (lazy
 * builds read them too): free the plan before L. */
int csx_cholsol_plan(csx_handle_t L, const int32_t *pinv /* host, or NULL */, csx_handle_t *plan);
/* cs_cholsol's factor sequence in natural order -- S = cs_schol(0, A); N = cs_chol(A, S), csparse.py:636-639 -- and the solve
 * plan of csparse.py:640-643 in ONE call, the symbolic analysis never leaving the device (round 5; replaces csx_schol's 40 MB of
 * parent / cp going to the host at 5M columns, csx_chol's upload-and-compare of the same arrays, and for forests of equal dense
 * blocks the three kernels that read L back to re-arrange it).  A: device CSC, square, upper triangle used.  exact: the order the
 * plan starts in (csx_cholsol_set_order changes it later).  *L: the factor (device CSC, diagonal first, rows ascending; for a forest
 * of equal dense blocks factored with exact = 0 the row indices are written when a handle to L is first used, its values and
 * column pointers at once); *plan: the solve plan, which borrows L's arrays -- free the plan before L.  CSX_ENOTSPD as csx_chol.
 * The analysis it implies is cs_schol(0, A)'s: S.cp = L.p, S.parent[j] = the first row below the diagonal of column j of L. */
int csx_cholsol_factor(csx_handle_t A, int exact, csx_handle_t *L, csx_handle_t *plan);
/* What the last successful csx_cholsol_factor did.  *path: 3 = forest of equal dense blocks of 16 / 32 / 64 columns, rounding-equal
 * order: the block kernel wrote the matrix-core solve's operands beside L.x, no other kernel touched L; 1 = forest of cliques (block
 * kernel, then the plan cut out of L.x); 2 = forest of small sparse trees; 0 = the general path (csx_schol + csx_chol +
 * csx_cholsol_plan behind the one entry).  *analysis_ms: host clock up to the end of the symbolic analysis; *numeric_ms: HIP-event
 * time of the numeric kernel(s); *call_ms: host clock of the whole call.  Any pointer may be NULL. */
int csx_cholsol_factor_info(int32_t *path, double *analysis_ms, double *numeric_ms, double *call_ms);
/* csx_cholsol_forest_plan: the kind of solve plan csx_cholsol_factor makes for a forest of blocks (paths 1 / 2 / 3 above), without
 * a device -- the library's own decision, for the tests (DESIGN.md §34 has the table).  sparse: the blocks are small sparse trees,
 * not cliques; min_bs / max_bs: the narrowest and widest block in columns; exact: the order asked for; dense_blocks:
 * "cholsol.dense_blocks" at factor time.  "Equal" below: cliques all of 8, 16, 32 or 64 columns.  *kind:
 *   0 General         the general analysis of L (the option off; sparse trees in the exact order)
 *   1 EmitEqual       equal blocks of 16 / 32 / 64, rounding-equal order: the block kernel writes the matrix-core operands (path 3)
 *   2 Programs        equal blocks of 8, rounding-equal order: the dense programs cut out of L.x
 *   3 BlockListExact  equal blocks, exact order: the block list; the exact kernel reads L.x
 *   4 EmitRagged      cliques not equal, rounding-equal order: the block list; the block kernel writes the ragged fragments
 *   5 BlockListLite   cliques not equal in the exact order, sparse trees in the rounding-equal order: the block list alone
 * CSX_EINVAL: min_bs > max_bs, max_bs < 1, kind NULL. */
int csx_cholsol_forest_plan(int sparse, int32_t min_bs, int32_t max_bs, int exact, int dense_blocks, int32_t *kind);
/* *path: the route the plan's next solve takes, in its current order (csx_cholsol_set_order) and under the options in force --
 * with "cholsol.dense_blocks" = 0 a forest of dense blocks reports 1, not 2 or 3.  0 = level-scheduled generic, 1 = fused
 * per-tree kernel (X tile in LDS), 2 = dense-block substitution (the reference's operations in the exact order -- cliques of
 * unequal sizes padded to size classes included -- FMA in the rounding-equal order), 3 = dense blocks as a blocked TRSM on the
 * matrix cores (fp64 MFMA; blocks of 16/32/64 whose block inverses are benign); 4 = supernodal schedule of a big elimination
 * tree (csx_cholsol_sn_info); 5 = a forest of small trees that are not equal dense blocks (cliques of unequal sizes, small sparse
 * trees, at most 80 columns each) made dense tree by tree, bucketed by size class (16 / 32 / 48 / 64 / 80) and solved on the
 * matrix cores (round 5; guard: || |inv(T_ii)| |T_ii| ||_inf <= 1e3 for every diagonal tile); 3 - 5 only in the rounding-equal
 * order.  A plan of csx_cholsol_factor whose solve goes to the general plan of the same factor reports that plan's route, trees
 * and largest tree (the general plan is made by this call if no solve has made it yet). */
int csx_cholsol_info(csx_handle_t plan, int32_t *path, int32_t *ntrees, int32_t *max_nodes);
int csx_cholsol_solve(csx_handle_t plan, csx_handle_t B, int32_t nrhs);
/* exact = 1 (the default of every plan): every right-hand side is solved in the reference's operation order,
 * bit-identical to cs_lsolve + cs_ltsolve on the same L, on every path (substitution kernels).
 * exact = 0: equal to the reference to rounding (1e-10 budget).  Forests of dense blocks go to the dense-block
 * kernels: blocks of 16/32/64 as a blocked TRSM on the matrix cores with explicit inverses of the diagonal
 * tiles (built by this call), unless an inverse is large (max|inv(L_ii)| max|L| > 1e3), then -- like blocks of
 * 8 -- FMA substitution with the unknowns in registers; on big elimination trees the blocked
 * chain walker may subtract a row's out-of-block terms first.  csx_cholsol_info reports the path in use;
 * csx_cholsol_growth the guard's measure (0 before the first exact = 0). */
int csx_cholsol_set_order(csx_handle_t plan, int exact);
int csx_cholsol_growth(csx_handle_t plan, double *growth);
/* The supernodal schedule of a plan in the rounding-equal order (path 4 of csx_cholsol_info; zeros when the plan has
 * none): number of supernodes outside the leaf subtrees, dependent steps of the forward solve, widest supernode,
 * whether the triangles of the supernodes are solved on the matrix cores (blocked TRSM with explicit inverses of the
 * 16 x 16 diagonal blocks) and the guard's measure for that: the largest || |inv(L_ii)| |L_ii| ||_inf over all diagonal
 * blocks; past 1e3, or with "tri.supernodes" = 2, the triangles are solved by substitution out of LDS.  Any pointer
 * may be NULL. */
int csx_cholsol_sn_info(csx_handle_t plan, int32_t *supernodes, int32_t *steps, int32_t *max_width, int32_t *matrix_cores,
                        double *growth);
/* Read-backs of the supernodal schedule for tests that must show which edge of it an input reached.  Both write
 * out[0 .. min(cap, *count)) and set *count to the number of fields; EINVAL when the plan holds no supernodal schedule.
 * csx_cholsol_sn_geometry, what the build decided (27 fields):
 *   0 columns per chunk (128 or 64), 1 whether some supernodes are relaxed runs, 2 whether the fragments for the matrix
 *   cores were built and passed the guard, 3 leaf subtrees, 4 leaf columns, 5 leaf tasks (pieces of the leaf columns' rows
 *   outside their subtrees), 6 leaf partial slots, 7 fundamental supernodes, 8 relaxed supernodes;
 *   then for the forward sweep (9 - 17) and for the backward sweep (18 - 26): steps, tasks of all steps, tasks of the
 *   largest step, lines cut into pieces, partial slots, chunks of at most 16 columns, of 17 to 32, of more, steps of
 *   exactly one triangle.
 * csx_cholsol_sn_launches, the kernels the plan's last forward sweep enqueued (fields 0 - 18) and its last backward sweep
 * (19 - 37); a replayed graph enqueues none, so count under "tri.graph" = 0:
 *   0 k_sn_outside_wg, 1 k_sn_outside, 2 - 7 k_sn_outside_thin<1 | 2 | 4 | 8 | 16 | 32>, 8 k_sn_combine,
 *   9 k_sn_mfma<., false, 1, 8> (chunks of 128), 10 k_sn_mfma<., true, 1, 4> and 11 k_sn_mfma<., true, 4, 4> (leaf subtrees),
 *   12 k_sn_mfma<., false, 1, 4> and 13 k_sn_mfma<., false, 4, 4> (chunks of 64), 14 k_sn_tri<1, 16, .>, 15 k_sn_tri<2, 32, .>,
 *   16 k_sn_tri<4, 64, .>, 17 k_sn_leaf, 18 of the k_sn_mfma launches: those of one triangle whose descriptor went with
 *   the launch. */
int csx_cholsol_sn_geometry(csx_handle_t plan, int64_t *out, int32_t cap, int32_t *count);
int csx_cholsol_sn_launches(csx_handle_t plan, int64_t *out, int32_t cap, int32_t *count);

/* "tri.graph": how many times this plan's supernodal solve has been captured into a hipGraph so far, and the host time of the
 * last capture + instantiate in ms (the option's default, 2, captures on the third consecutive solve of one block).  Either
 * pointer may be NULL. */
int csx_cholsol_graph_info(csx_handle_t plan, int32_t *captures, double *last_capture_ms);

/* ---- assembly and reshaping around the hot path ---------
 * Every function returns a NEW matrix handle.  p[] / i[] bit-identical to the reference's result.
 * cs_compress, csparse.py:647-673: host triplets (row Ti[k], column Tj[k], value Tx[k] or NULL) -> CSC,
 *   entries of a column in triplet order (stable counting sort by column).
 * cs_add, csparse.py:163-192: alpha*A + beta*B; column pattern in first-touch order over A(:,j) then B(:,j).
 * cs_dupl, csparse.py:1035-1065: duplicates summed into their first occurrence.
 * cs_dropzeros / cs_droptol, csparse.py:1019-1031 / 1002-1014: mode 0 keeps a != 0, mode 1 keeps |a| > tol;
 *   order preserved.  Needs values.
 * cs_permute, csparse.py:1666-1693: C = P A Q (pinv: host, length m, or NULL; q: host, length n, or NULL).
 * cs_symperm, csparse.py:2220-2255: upper triangle of P A P' (pinv host permutation or NULL), A square. */
int csx_compress(int32_t m, int32_t n, int64_t nz, const int32_t *Ti, const int32_t *Tj, const double *Tx,
                 csx_handle_t *out);
int csx_add(csx_handle_t A, csx_handle_t B, double alpha, double beta, csx_handle_t *out);
int csx_dupl(csx_handle_t A, csx_handle_t *out);
int csx_drop(csx_handle_t A, int mode, double tol, csx_handle_t *out);
int csx_permute(csx_handle_t A, const int32_t *pinv, const int32_t *q, int values, csx_handle_t *out);
int csx_symperm(csx_handle_t A, const int32_t *pinv, int values, csx_handle_t *out);
/* cs_norm, csparse.py:1647-1663: 1-norm (largest column sum of |a|), column sums in storage order (the
 * reference's bits).  Needs values. */
int csx_norm1(csx_handle_t A, double *out);
/* Columns [first, first + count) of A as a new m x count matrix: the unit of a column-sharded SpMV. */
int csx_csc_col_block(csx_handle_t A, int32_t first, int32_t count, csx_handle_t *out);

/* cs_updown, csparse.py:2318-2365: L L' + sigma w w' (sigma = +1 update, -1 downdate) applied to the device
 * factor L in place; w is given as host arrays (rows Ci[0..cnz), values Cx), parent = elimination tree (host,
 * length n).  *ok = 0 when a downdate is not positive definite (L is then changed exactly as far as the
 * reference's loop gets).  Solve plans built from L before the call hold stale values: rebuild them. */
int csx_updown(csx_handle_t L, int sigma, int32_t cnz, const int32_t *Ci, const double *Cx, const int32_t *parent,
               int *ok);

/* updown_block: the k rank-1 terms L L' + sigma[t] w_t w_t', w_t = column t of C (device, n x k; rows
 * assigned in storage order, a later duplicate wins; rows off the path of f_t = min row of C(:,t) never read), applied to the
 * device factor L (diagonal first, rows ascending) in ONE pass over the union of their elimination-tree paths.  L.x comes out
 * byte-equal to `for t in 0..k-1: if (!cs_updown(L, sigma[t], C(:,t))) break`.  sigma: host, k values, each +1 or -1.
 * parent: host, n, or NULL: the tree is read from L (parent[j] = the row of the second entry of column j, -1 for none); a
 *   given parent is checked against it on the device.
 * flags: 1 all or nothing (a downdate that is not positive definite leaves L as it was), 2 check that every row of C(:,t) lies
 *   in the pattern of L(:, f_t).
 * *applied: k on success (empty columns are successes that change nothing); t when the downdate of column t is not positive
 *   definite (without flag 1 L is then the loop's partial state; with it, unchanged); -1 the pattern check failed (nothing
 *   changed); -2 parent is not L's elimination tree (nothing changed).  CSX_EINVAL for a row out of range, a sigma other than
 *   +1 / -1, C->m != n, or an L that is not Cholesky-shaped along the paths (nothing changed).
 * csx_updown_block_info: the last call's chunks (64 terms of a tree per chunk), union columns and groups (trees, summed over
 *   the chunks) and the time of its block kernels.
 * csx_updown_block_classes: the route of the last call.  counts[c] = the groups its first pass launched in class
 *   c = (block == 256) + 2 * (W in LDS), summed over the chunks: a tree runs on 256 lanes when its longest union column
 *   (diagonal included) has more than 64 entries, with W in LDS when ucnt * nterm * 8 <= 60 KB.  *replayed = 1 when a
 *   failing downdate made the chunks run again with terms [0, t] (never with flag 1). */
int csx_updown_block(csx_handle_t L, csx_handle_t C, const int32_t *sigma, const int32_t *parent, int flags, int32_t *applied);
int csx_updown_block_info(int32_t *chunks, int32_t *union_columns, int32_t *groups, double *kernel_ms);
int csx_updown_block_classes(int32_t counts[4], int32_t *replayed);

/* sparseinv: the entries of inv(L L') on the pattern of the device Cholesky factor L (square, values,
 * every column non-empty with its diagonal first, positive and finite, rows strictly ascending: cs_chol's), by the Takahashi
 * recurrence.  *Z: a new device matrix with copies of L.p, L.i; Z.x holds the lower triangle of the symmetric inverse,
 * byte-equal to the loop (d = L(j,j), S_j = the rows below the diagonal of column j in storage order, Zs(a,b) = the stored
 * Z(max(a,b), min(a,b)), every product and sum rounded on its own)
 *   for j = n-1 .. 0:  for i in S_j: Z(i,j) = (-sum_{k in S_j} L(k,j) * Zs(i,k)) / d;
 *                      Z(j,j) = (1/d - sum_{k in S_j} L(k,j) * Z(k,j)) / d.
 * One launch per depth of the elimination forest read off L (parent[j] = the row of the second entry of column j); the
 * schedule is cached on L with its pattern.  CSX_EINVAL, a message in csx_last_error() and no Z for an L that fails the
 * checks above (made on the device before any value is written) or whose pattern is not a Cholesky pattern (a pair i, k of
 * one column that is stored in neither column; nothing is read out of range).  L is never changed.
 * csx_chol_inverse_info: the last call's depths, columns in the widest depth, terms (sum of |S_j|^2) and the device time of
 *   its launches between two events; all zero when that call failed.
 * csx_csc_diag: out[j] = the value of the first entry of column j of M (0.0 for an empty column), out a device vector of at
 *   least n entries: the diagonal of a Cholesky factor or of Z. */
int csx_chol_inverse(csx_handle_t L, csx_handle_t *Z);
int csx_chol_inverse_info(int32_t *depths, int32_t *widest, int64_t *terms, double *kernel_ms);
int csx_csc_diag(csx_handle_t M, csx_handle_t out);
/* sparseinv for the two other factorisations on a Cholesky pattern: the same schedule, lookups and
 * kernels under another column policy.  Both take plain matrix / vector handles (not factor handles), as csx_chol_inverse does.
 * csx_ldl_inverse: Z = inv(L D L') on the pattern of L.  L: unit lower, diagonal first (stored, never read), rows ascending; d: a
 *   device vector of at least n doubles, every one finite and non-zero.  *Z as for csx_chol_inverse, byte-equal to
 *   for j = n-1 .. 0:  for i in S_j: Z(i,j) = -sum_{k in S_j} L(k,j) * Zs(i,k);   Z(j,j) = 1/d[j] - sum_{k in S_j} L(k,j) * Z(k,j).
 * csx_slu_inverse: Z = inv(L U), U = Ut', Ut on the SAME p and i as L (the same device arrays or equal ones: compared on the
 *   device after n and nnz), column j of Ut = row j of U with the pivot d = Ut(j,j) first, finite and non-zero.  Two new
 *   matrices on that pattern: ZL(i,j) = Z(i,j) and ZUt(i,j) = Z(j,i) for i >= j (the diagonal in both), byte-equal to
 *   for j = n-1 .. 0:  for i in S_j: ZL(i,j) = -sum_k L(k,j) * Z(i,k);  ZUt(i,j) = (-sum_k Ut(k,j) * Z(k,i)) / d;
 *                      ZL(j,j) = ZUt(j,j) = 1/d - sum_k L(k,j) * ZUt(k,j)
 *   (Z(i,k) = ZL(i,k) for i > k, ZUt(k,i) for i < k, the diagonal of column i for i == k; Z(k,i) is the same slot of the other
 *   array), every product and sum rounded on its own, the sums in storage order.
 * Both: CSX_EINVAL, a message in csx_last_error() and no output handle for an input that fails the checks (made on the device
 *   before any value is written: csx_chol_inverse's structure checks, the pivots, Ut's pattern) or whose pattern is not a
 *   Cholesky pattern; nothing is read out of range, L, d and Ut are never changed.  csx_chol_inverse_info answers for the last
 *   call of any of the three.  A static-pivot factor is not backward stable and the recurrence inherits its growth.
 * csx_inverse_at: out[t] = Z(a, b), a = rmap[rows[t]], b = cmap[cols[t]], t < count, read off the pattern: a > b from column b
 *   of ZL, a < b from column a of ZUt (ZUt = 0: of ZL, a symmetric Z), a == b the first entry of column a.  rmap, cmap: device
 *   int vectors of at least n entries (csx_ivec_upload; csx_permute_vec's kind) or 0 for the identity; rows, cols: host
 *   arrays of count int32 (as csx_csc_upload takes its indices); out: a device vector of at least count doubles.  A pair that
 *   is not on the pattern yields NaN and is counted in *missing (may be null).  CSX_EINVAL for an index outside [0, n). */
int csx_ldl_inverse(csx_handle_t L, csx_handle_t d, csx_handle_t *Z);
int csx_slu_inverse(csx_handle_t L, csx_handle_t Ut, csx_handle_t *ZL, csx_handle_t *ZUt);
int csx_inverse_at(csx_handle_t ZL, csx_handle_t ZUt, csx_handle_t rmap, csx_handle_t cmap, int64_t count, const int32_t *rows,
                   const int32_t *cols, csx_handle_t out, int64_t *missing);

/* cs_lu, csparse.py:1370-1451 (+ cs_spsolve :2078-2113), natural column order: host C++
 * left-looking LU with threshold partial pivoting.  It produces the L (unit diagonal first)
 * and U (diagonal last) that cs_lsolve / cs_usolve consume in cs_lusol (csparse.py:1474-1477).
 * Output arrays are malloc'ed here; release each with csx_host_free.  Returns CSX_ENOTSPD for a
 * singular matrix (the reference returns None, csparse.py:1423). */
int csx_lu_host(int32_t n, const int32_t *Ap, const int32_t *Ai, const double *Ax, double tol,
                int32_t **Lp, int32_t **Li, double **Lx, int32_t **Up, int32_t **Ui, double **Ux,
                int32_t *pinv);
void csx_host_free(void *p);

/* cs_qr numeric phase, csparse.py:1797-1870 (+ cs_house :1238-1261, cs_happly :1216-1235): sparse Householder QR on
 * the host (C++), A m-by-n with the symbolic analysis of cs_sqr(order 0, qr): parent (column etree of A'A), pinv
 * (length m2), leftmost (length m), m2 rows incl. fictitious ones.  V (m2-by-n) and R (diagonal last in every column)
 * are written into caller arrays of capacity vcap / rcap entries (cs_sqr's counts), beta has n entries.
 * csx_qr_apply_host: x <- Q' x (transpose != 0) or Q x, x of length m2. */
int csx_qr_host(int32_t m, int32_t n, int32_t m2, const int32_t *Ap, const int32_t *Ai, const double *Ax,
                const int32_t *q /* or NULL */, const int32_t *parent, const int32_t *pinv, const int32_t *leftmost,
                int32_t vcap, int32_t rcap, int32_t *Vp, int32_t *Vi, double *Vx, int32_t *Rp, int32_t *Ri, double *Rx,
                double *beta);
int csx_qr_apply_host(int32_t n, const int32_t *Vp, const int32_t *Vi, const double *Vx, const double *beta, int transpose,
                      double *x);
/* cs_happly (csparse.py:1216-1235) applied for every reflection of V to a block of nrhs vectors on the device: X (length
 * V.m * nrhs, row-major: row r of all vectors contiguous) <- Q' X (transpose != 0: reflections 0 .. n-1) or Q X
 * (n-1 .. 0); beta: device vector of V.n entries.  One lane per vector runs the reference's loops: bit-identical to
 * cs_happly called reflection by reflection on each column. */
int csx_happly(csx_handle_t V, csx_handle_t beta, csx_handle_t X, int32_t nrhs, int transpose);
/* cs_sqr for QR, natural column order (csparse.py:2187-2217 with cs_etree of A'A :1136-1169, cs_post :1711-1742,
 * cs_counts :703-764, cs_vcount :2118-2184), on the host: parent and cp (column counts of R) have n entries, pinv m + n,
 * leftmost m; *m2 = rows of V including the fictitious ones, *vnz / *rnz = entries of V / R. */
int csx_sqr_host(int32_t m, int32_t n, const int32_t *Ap, const int32_t *Ai, int32_t *parent, int32_t *cp, int32_t *pinv,
                 int32_t *leftmost, int32_t *m2, int64_t *vnz, int64_t *rnz);
/* cs_qr's numeric phase on the device for a SQUARE matrix that is a batch of small independent blocks (connected
 * components of at most 96 rows, at least 64 of them), natural column order, no fictitious rows (m2 == m): one lane per
 * block runs csx_qr_host's loop.  parent / pinv / leftmost: host arrays of n entries from cs_sqr.  V, R: new device
 * matrices; beta: host, n entries.  All three bit-identical to csx_qr_host.  *done = 0 when the matrix (or the
 * analysis) is not of that shape: use csx_qr_host. */
int csx_qr_blocks(csx_handle_t A, const int32_t *parent, const int32_t *pinv, const int32_t *leftmost, int32_t m2,
                  csx_handle_t *V, csx_handle_t *R, double *beta, int *done);
/* The same factorisation on the device for a matrix that is a batch of small independent blocks (at least 64 connected
 * components of at most 96 rows, found on the device): one lane per block runs csx_lu_host's loop -- the same reach
 * order, update order and first-maximum pivot rule, duplicates and unsorted columns included.  *done = 0 when the matrix
 * is not of that shape: use csx_lu_host.  L, U: new device matrices (unit diagonal first / diagonal last, row indices in
 * pivot order); pinv: host, n.  All three bit-identical to csx_lu_host.  CSX_ENOTSPD: a singular block. */
int csx_lu_blocks(csx_handle_t A, double tol, csx_handle_t *L, csx_handle_t *U, int32_t *pinv, int *done);

/* For the tests of the two block routes and of csx_happly; production code calls neither.
 * csx_block_limits: the cuts, without a device: out[5] = LU_MAX_M (rows of the largest block csx_lu_blocks takes),
 * LU_MIN_COMPONENTS (blocks it needs at least; also the smallest n), QR_MAX_M, QR_MIN_COMPONENTS (the same of csx_qr_blocks),
 * HAPPLY_MAX_LEVELS (levels beyond which csx_happly walks all reflections in one launch).  CSX_EINVAL: out is NULL.
 * csx_prim_components: the connected-components pass under both routes, the triangular-solve planner and the symbolic
 * Cholesky, on HOST arrays: the graph has an edge (r, i[q]) for q in [p[r] + skip_first, p[r + 1] - skip_last); order 0: any
 * neighbour, 1: every neighbour must be < r, 2: > r (what the planner passes for a forward / backward solve).  Runs
 * connected_components, then group_by_root, as csx_lu_blocks does.  root[v] = the smallest vertex of v's component; nodes =
 * the vertices grouped by root, ascending inside a group; first[c], count[c] = component c's slice of nodes (capacity n
 * each, *ncomp written); comp_of_pos[k] = the component of nodes[k]; *maxc = the largest count.  *malformed = 1: an index
 * outside [0, n) or on the wrong side for the order -- the other outputs are then not written, as every caller stops
 * there.  The device copies of p and i are copied back over the host arrays, so that a kernel that wrote to them shows.
 * CSX_EINVAL, before the device is touched: n < 0, a missing array, p[0] != 0 or p decreasing, skip_first / skip_last not
 * 0 or 1, order not 0 .. 2. */
int csx_block_limits(int32_t *out);
int csx_prim_components(int32_t n, int32_t *p, int32_t *i, int skip_first, int skip_last, int order, int32_t *root,
                        uint32_t *nodes, int32_t *first, int32_t *count, int32_t *comp_of_pos, int32_t *ncomp, int32_t *maxc,
                        int *malformed);

/* cs_lu of ONE connected matrix on the device, natural column order: the columns are scheduled by the column elimination
 * tree (the tree of A'A, csparse.py:1136-1169): columns that are not ancestor and descendant reach disjoint rows, so a
 * level of the tree is one launch with one lane per column running csx_lu_host's loop.  L (unit diagonal first), U
 * (diagonal last), pinv bit-identical to csx_lu_host.  *done = 0 when the tree is too deep for its size (a chain: a
 * banded matrix in natural order), n < 2048 or tol <= 0: use csx_lu_host.  CSX_ENOTSPD: singular. */
int csx_lu_etree(csx_handle_t A, double tol, csx_handle_t *L, csx_handle_t *U, int32_t *pinv, int *done);

/* cs_spsolve (csparse.py:2078-2113) with cs_reach (:1939-1958) and cs_dfs (:789-829), for every column of B at once:
 * X(:,k) solves G X(:,k) = B(:,k), G n-by-n lower (lo != 0, diagonal first in every column) or upper (diagonal last)
 * triangular, B n-by-nb sparse.  pinv (host, n entries, or NULL): column pinv[j] of G belongs to node j, a negative
 * entry = no column (the partial permutation cs_lu hands over).  Column k of X lists the reach of B(:,k) in the
 * reference's xi[top..n-1] order with the solution beside it -- pattern order and values bit-identical to calling the
 * reference column by column.  values == 0: pattern only (cs_reach for every column; G and B need no values).
 * One lane per column of B runs the reference's own loops; work space n * 17 bytes per column in flight. */
int csx_spsolve(csx_handle_t G, csx_handle_t B, const int32_t *pinv /* or NULL */, int lo, int values, csx_handle_t *X);

/* ---- multi-GPU exchange: RCCL over xGMI inside the library, one process per GPU ----------------
 * The reference is one Python process (no collective call site); what shards are its sequences
 * csparse.py:640-643 (cs_ipvec, cs_lsolve, cs_ltsolve, cs_pvec: right-hand-side blocks are independent) and
 * csparse.py:1210-1212 (cs_gaxpy: column blocks give partial y vectors that are summed).
 * Set-up: rank 0 calls csx_comm_unique_id, the launcher's side channel (csparse.py_amd/shard.py: a TCP hand-shake on
 * MASTER_ADDR) carries the 128 bytes to the other ranks, every rank calls csx_comm_init(rank, world, id) after csx_init.
 * RCCL (librccl.so.1) is bound by csx_comm_init, not when libcsx is loaded.  world == 1 with id == NULL makes no RCCL
 * call at all (every exchange is a device copy); world == 1 with an id is a real RCCL communicator of one rank.
 * Every exchange works on device buffers behind handles and is enqueued on the context's stream, in order with the
 * kernels around it: no synchronisation between a kernel and the collective that ships its result.  Host results
 * (csx_comm_allreduce_host, csx_comm_bcast_host, csx_comm_barrier) are complete when the call returns. */
#define CSX_COMM_ID_BYTES 128
int csx_comm_unique_id(uint8_t *id128);
int csx_comm_init(int rank, int world, const uint8_t *id128 /* NULL: world of one, no RCCL */);
int csx_comm_finalize(void);
int csx_comm_info(int *rank, int *world, int *uses_rccl);
int csx_comm_barrier(void);                                        /* stream drained + every rank arrived */
int csx_comm_allreduce_host(double *vals, int count, int op);      /* op 0 = sum, 1 = max; count <= 1024 (timings, checks) */
int csx_comm_bcast_host(void *buf, int64_t bytes, int root);       /* small control data */
/* Factor once on `root`, ship the factor: *A (the root's matrix) arrives as a NEW matrix handle on every other rank
 * (sizes, then p, i, x: three ncclBroadcast).  The root's handle is unchanged. */
int csx_comm_bcast_csc(csx_handle_t *A, int root);
int csx_comm_bcast_vec(csx_handle_t v, int root);                  /* in place, same length on every rank */
/* `full` has world * len(out) entries; out = entries [rank len, (rank + 1) len) of the sum over ranks (ncclReduceScatter) */
int csx_comm_reduce_scatter_vec(csx_handle_t full, csx_handle_t out);
int csx_comm_allreduce_vec(csx_handle_t v);                        /* in place sum */
/* Right-hand-side blocks leave the root / solution blocks return to it: `src` / `out` (root only) hold world blocks of
 * len doubles in rank order; world - 1 point-to-point transfers in one RCCL group, the root's own block a device copy. */
int csx_comm_scatter_blocks(csx_handle_t src, csx_handle_t dst, int64_t len, int root);
int csx_comm_gather_blocks(csx_handle_t block, csx_handle_t out, int64_t len, int root);
/* Columns [c0, c0 + k) of the n x K row-major block B as a contiguous n x k block `out` (back == 0), or `out` written
 * back into those columns of B (back != 0): a rank's share of a batch of right-hand sides. */
int csx_block_cols(csx_handle_t B, int64_t n, int32_t K, int32_t c0, int32_t k, csx_handle_t out, int back);
/* ONE cs_gaxpy sharded by columns: rank r holds A_r = columns [first_r, first_r + count_r) of an m x n matrix
 * (csx_csc_col_block) and the matching slice x_r of x; y = sum_r A_r x_r, and rank r ends up with rows
 * [r chunk, min((r + 1) chunk, m)), chunk = ceil(m / world) (csx_gaxpy_sharded_rows).
 * csx_gaxpy_sharded(plan, x_r, y_mine, how): y_mine (chunk entries) += this rank's rows of the sum.
 *   how 0: one SpMV into a full-length partial y, then one ncclReduceScatter;
 *   how 1: the block is cut by rows into the world pieces y is owned in; rank r computes the piece of rank r + 1
 *          first and its own last, and a finished piece leaves for its owner over the direct link (ncclSend /
 *          ncclRecv on a second stream) while the next piece is computed; the owner adds the world partial pieces
 *          in ascending rank order, so the result has the same bits on every run.
 * The plan keeps a pointer to the block: free the plan first. */
int csx_gaxpy_sharded_plan(csx_handle_t block, csx_handle_t *plan);
int csx_gaxpy_sharded_rows(csx_handle_t plan, int32_t *first, int32_t *count);
int csx_gaxpy_sharded(csx_handle_t plan, csx_handle_t x, csx_handle_t y_mine, int how);
/* The steps of how == 1 one at a time, for a transport that is not RCCL (shard.py's host stand-in, which carries the
 * N > 1 tests on a one-GPU box): a plan cut for `world` ranks; piece q's partial sums into the plan's work buffer
 * (piece q at work + q * chunk); the buffers (recv: world - 1 arrival slots of chunk doubles, senders in ascending
 * rank order); the owner's sum of the world pieces in ascending rank order into y_mine. */
int csx_gaxpy_sharded_plan_for(csx_handle_t block, int world, csx_handle_t *plan);
int csx_gaxpy_sharded_piece(csx_handle_t plan, int q, csx_handle_t x);
int csx_gaxpy_sharded_buffers(csx_handle_t plan, void **work, void **recv, int64_t *chunk);
int csx_gaxpy_sharded_sum(csx_handle_t plan, int rank, int world, csx_handle_t y_mine);

/* ---- Dulmage-Mendelsohn decomposition (csparse.py:905 cs_dmperm, :1527 cs_maxtrans, :1992 cs_scc) ----
 * Entries are structural: a stored 0.0 counts, pattern-only matrices are accepted.  Outputs go to caller-owned host
 * buffers.  Deterministic: the same matrix and seed give the same arrays on every call.  seed sets the priority of
 * rows and columns when ties are broken (0 natural, -1 reversed, otherwise the order of splitmix64 keys, as
 * csparse.cs_randperm); the matching and the order inside a block depend on it, the sets, nb and sprank do not.
 * csx_maxtrans: a maximum matching, jimatch[i] (i < m) = column of row i, jimatch[m + j] = row of column j, -1 if
 *   unmatched (m + n slots); sprank (optional) = its cardinality.
 * csx_scc: square A only (CSX_EINVAL otherwise).  p (n) and r (n + 1 slots, nb + 1 used): A(p,p) is block upper
 *   triangular -- for every entry (i, j) the block of row i comes no later than the block of column j -- and every
 *   diagonal block r[k] .. r[k+1]-1 is strongly connected.
 * csx_dmperm: p (m), q (n), r (m + 6), s (n + 6), rr (5), cc (5) as cs_dalloc sizes them, unused slots 0.
 *   cc = [0, |C0|, |C0|+|C1|, |C0|+|C1|+|C2|, n], rr = [0, |R1|, |R1|+|R2|, |R1|+|R2|+|R3|, m], sprank = rr[3];
 *   row rr[0]+k is matched to column cc[1]+k (R1/C1), rr[1]+k to cc[2]+k (R2/C2), rr[2]+k to cc[3]+k (R3/C3).
 *   Fine blocks (csparse.py:982-996): A(R1, C0 C1) if cc[2] > 0, the SCCs of A(R2, C2) in block upper triangular
 *   order, A(R3 R0, C3) if rr[2] < m.
 * csx_dmperm_times: device times (ms) of the last csx_dmperm / csx_maxtrans / csx_scc: initial matching,
 *   augmentation, coarse decomposition, fine decomposition (the SCCs), whole call.
 * csx_dmperm_rounds: round counts of the same call: augmentation levels (all phases), augmentation phases, trim
 *   rounds, colouring rounds (propagations and backward searches; at most 2 (m + n + 1) in all, else CSX_ERUNTIME), block
 *   order rounds. */
int csx_maxtrans(csx_handle_t A, int64_t seed, int32_t *jimatch, int32_t *sprank);
int csx_scc(csx_handle_t A, int32_t *p, int32_t *r, int32_t *nb);
int csx_dmperm(csx_handle_t A, int64_t seed, int32_t *p, int32_t *q, int32_t *r, int32_t *s, int32_t *nb, int32_t *rr,
               int32_t *cc);
int csx_dmperm_times(double *ms);
int csx_dmperm_rounds(int64_t *rounds);

/* ---- block triangular LU (btf_factor in csparse.py) ---------------------------------------
 * Definition.  A square, structurally nonsingular A with the fine blocks of csx_dmperm (p, q, r, nb: every block a
 * strongly connected component, A(p, q) block upper triangular with a zero-free diagonal) is factored as
 * C = A(p', q') = D + F: D the entries inside the diagonal blocks, F the strictly block upper rest, both in C's column
 * storage order.  A block's level is 0 when its rows have no entries outside the block, else 1 + the largest level of
 * the blocks those entries reach; p', q', r' list the blocks by level, highest first, in the given order inside a level
 * (C stays block upper triangular).  L, U, pinv = cs_lu(D) (unit diagonal first / diagonal last, pivots inside their
 * block: the caller's dispatch).  A solve of A x = b, for every right-hand side: c = b(p'); blocks from last to first:
 * c_i -= F_ij z_j for every row i of the block in cs_gaxpy's order (ascending column, storage order within a column;
 * multiply and subtract rounded separately), then the block's part of cs_ipvec(pinv), cs_lsolve(L), cs_usolve(U),
 * operation for operation; x(q') = z.  One order, fixed by the factors: every run and every right-hand side of a block
 * gives the bits of a one-column solve.
 * csx_btf_split: p, q (n), r (nb + 1) from csx_dmperm; writes p_out, q_out (n), r_out (nb + 1), level (nb, non-increasing),
 *   *nlevels, and the NEW matrix handles *D and *F.  Level analysis on the host (one pass over A's pattern), the
 *   permutation and the split on the device.
 * csx_btf_plan: a NEW plan handle (freed by csx_free) from L, U (cs_lu of D), F and the host arrays pinv (n), p, q (n),
 *   r (nb + 1), level (nb) that csx_btf_split returned.  The plan keeps copies of everything the forward solve reads, and
 *   the handles L, U, F for the transposed solve's programs (made on its first call: the caller keeps the three alive
 *   while it may ask for one).  Blocks of at
 *   most 96 rows are solved one wave per (block, 64 right-hand sides) with the tile in LDS, one launch per level;
 *   larger blocks by a product with F over their rows and csx_tri_analyse-style exact plans of their own parts of L
 *   and U (a few launches each).
 * csx_btf_solve: B (n-by-nrhs, row-major) overwritten with X; work: another block of at least n nrhs entries.  B's rows
 *   are read before any is written (the last launch writes x(q)).  No atomics.
 * csx_btf_info: info[8] = blocks, levels, largest block, nnz(L), nnz(U), nnz(F), blocks on the large-block path,
 *   launches of a solve not counting the large blocks' own.
 * Errors: CSX_EINVAL for a stale or wrong-kind handle, a non-square or pattern-only matrix, p / q / pinv that are not
 *   permutations, r not strictly increasing from 0 to n, A(p, q) not block upper triangular, levels that do not fall,
 *   pivots outside their block, L / U rows without their diagonal or with entries outside the block, F entries that
 *   reach a block of the same or a higher level, B and work the same vector or shorter than n nrhs, nrhs < 1.
 * Memory: the plan holds n (4 ints) + nnz(L) + nnz(U) + nnz(F) entries (12 bytes each) + n (2 doubles) on the device,
 *   and the two parts of every large block's factors with their plans. */
int csx_btf_split(csx_handle_t A, const int32_t *p, const int32_t *q, const int32_t *r, int32_t nb, int32_t *p_out,
                  int32_t *q_out, int32_t *r_out, int32_t *level, int32_t *nlevels, csx_handle_t *D, csx_handle_t *F);
int csx_btf_plan(csx_handle_t L, csx_handle_t U, csx_handle_t F, const int32_t *pinv, const int32_t *p, const int32_t *q,
                 const int32_t *r, const int32_t *level, int32_t nb, csx_handle_t *plan);
int csx_btf_solve(csx_handle_t plan, csx_handle_t B, csx_handle_t work, int32_t nrhs);
/* csx_btf_solve_trans: B overwritten with the X of A' X = B: C' w = b(q) block lower triangular, blocks by
 *   level from the highest; per column j of a block c_j = b(q_j) - F(:, j)' w in F's column storage order, then the block's
 *   part of cs_utsolve(U), cs_ltsolve(L), cs_pvec(pinv); x(p) = w.  The first call builds the column programs of U, L and F
 *   from the plan's L, U, F handles (CSX_EINVAL when one is gone, when a column of U lacks its diagonal last or one of L its
 *   diagonal first, or an index leaves its block or its side); the same kernels as csx_btf_solve, one launch per level. */
int csx_btf_solve_trans(csx_handle_t plan, csx_handle_t B, csx_handle_t work, int32_t nrhs);
int csx_btf_info(csx_handle_t plan, int64_t *info);
/* For the tests of the btf solve and of the refactor kernel; production code does not call it.  The cuts and strides, without a
 * device: out[6] = BTF_SMALL (rows of the largest block solved with its tile in LDS), RF_MAX (rows of the largest group
 * refactored on the device), RF_WAVES (groups of a workgroup of the refactor kernel), the right-hand sides of a tile of the
 * small-block kernel, the terms of a row program loaded at a time, the terms applied as one group.  CSX_EINVAL: out is NULL. */
int csx_btf_limits(int32_t *out);

/* ---- refactor: new values, the same pivots (btf_factor / lusol_factor .refactor) -----------------
 * Definition.  Given cs_lu's L, U, pinv of a matrix and new values A2 of the same pattern, column k of the factorisation (in
 * its column order) is recomputed in pivot-row space: x = 0 on the rows of U(:,k) and L(:,k); x[pinv[i]] = A2(i, k) in
 * storage order (assignment, as cs_spsolve); for every entry J of U(:,k) but the last, in storage order: U.x = x[J],
 * x[L.i[t]] -= L.x[t] x[J] for t over L(:,J) after its unit diagonal (multiply and subtract rounded separately); the pivot
 * x[k] goes last into U(:,k); L.x = x / pivot after the unit diagonal.  The stored order is the order cs_lu solved in: L and
 * U are byte-equal to cs_lu(A2)'s whenever it chooses the same pinv.  *ok = 0 when a pivot is 0 or not finite; *ratio = the
 * minimum over the columns of |pivot| / max |x_i| over L(:,k)'s rows (pivot included): 1.0 when every kept pivot is a
 * largest candidate of its column.
 * csx_lu_refactor_host: the rule on host arrays for all n columns, A's column k = column k of the factorisation; writes
 *   Lx and Ux (the caller's, the patterns' lengths).  CSX_EINVAL when an index leaves [0, n), pinv is not a permutation, a
 *   column of U lacks its diagonal last or one of L its diagonal first, or A(:,k) has a row outside L(:,k) and U(:,k).
 * Device path (csx_btf_refactor, csx_lu_refactor): the columns fall into groups that do not depend on one another (btf: the
 *   diagonal blocks; lusol: the connected components of the pattern of L + U); a group of at most 96 rows whose columns of A
 *   have no duplicate rows is refactored by one wave with x in LDS, the others by the host loop.  A2 is checked against A's
 *   pattern on the device (CSX_EINVAL for a different one); its values are gathered through maps built on the first call.
 *   Nothing the solves read changes unless *ok = 1, and an error status before the commit (an allocation, a plan of a large
 *   block) leaves everything as it was; *ok = -1 (CSX_OK) when A2's pattern or length differs from A's, nothing changed.
 *   cols (or NULL): [0] columns refactored on the device, [1] on the host.  The host groups run while the launch does.
 * csx_btf_refactor: plan from csx_btf_plan; A: the matrix the plan was factored from, read on the FIRST call only (its pattern
 *   and the maps; 0 afterwards); A2: a matrix with A's pattern or a vector of nnz(A) values in A's storage order; D: the D of
 *   csx_btf_split (its values are replaced too) or 0.  On success L, U, F (the plan's handles) and D hold the new values, the
 *   forward programs are refreshed in place, the large blocks re-make their triangular plans, and the transposed programs are
 *   made again on the next transposed solve.  Cached plans of L, U, F, D (csx_gaxpy's, the triangular solves') are stale:
 *   csx_csc_invalidate them.
 * csx_btf_refactor_dx: D2's values of the last csx_btf_refactor call (nnz(D) doubles, D's storage order) into host Dx: for a D
 *   whose device copy is gone (then pass D = 0 to csx_btf_refactor).
 * csx_lu_refactor_plan: a NEW plan handle (csx_free) for L, U (device, cs_lu's, kept alive by the caller), A (the matrix they
 *   were factored from: pattern only), q (n, the factorisation's column order, or NULL: natural) and pinv (host, n).
 * csx_lu_refactor: A2 as above; on success L's and U's values are replaced (plans made from them are stale). */
int csx_lu_refactor_host(int32_t n, const int32_t *Ap, const int32_t *Ai, const double *Ax, const int32_t *pinv,
                         const int32_t *Lp, const int32_t *Li, double *Lx, const int32_t *Up, const int32_t *Ui, double *Ux,
                         int *ok, double *ratio);
int csx_btf_refactor(csx_handle_t plan, csx_handle_t A, csx_handle_t A2, csx_handle_t D, int *ok, double *ratio,
                     int64_t *cols);
int csx_btf_refactor_dx(csx_handle_t plan, double *Dx);
int csx_lu_refactor_plan(csx_handle_t L, csx_handle_t U, csx_handle_t A, const int32_t *q, const int32_t *pinv,
                         csx_handle_t *plan);
int csx_lu_refactor(csx_handle_t plan, csx_handle_t A2, int *ok, double *ratio, int64_t *cols);

/* ---- Cholesky refactor: new values on the kept analysis (cholsol_factor .refactor) ---------------
 * Definition.  Given the factor L of cs_chol (L L' = P A P', diagonal first, rows ascending) of a matrix A and new values A2 on
 * A's pattern, L.x is replaced by the values cs_chol gives for A2 with the same S: the same kernels in the same order as a
 * fresh csx_chol / csx_cholsol_factor under the options in force, so L.x is byte-equal to that fresh factor's -- with one
 * exception: under "chol.exact" = 0 (opt-in) a csx_cholsol_factor made with exact = 0 lets its block kernel emit the
 * matrix-core solve's operands, which for cliques of unequal sizes is another kernel (the blocked factorisation per size
 * class) than the refactor's; L.x then agrees with the fresh factor's to rounding, which is all that option promises of L.x.
 * L.p and L.i are never written, and L.x keeps its address (solve plans borrow it).
 * csx_chol_refactor_plan: a NEW plan handle (csx_free) for A (the matrix L was factored from: only its pattern is read, its
 *   upper triangle counts, lower entries are ignored as cs_chol ignores them), L (device; BORROWED like a cholsol plan borrows
 *   it: free the plan before L) and pinv (host, n, or NULL: natural order).  The elimination tree and the column counts are
 *   read off L (parent[j] = the row of the second entry of column j, cp = L.p): no S is passed.  The plan keeps a copy of A's
 *   pattern and, on the general route, what csx_chol builds and lets go: the row view of L, the entry map (for every slot of L
 *   the entry of A that lands there, of duplicates the last, -1 for fill), the forest partition, the level lists, the supernode
 *   groups and the band decision (taken here once, the free-memory test of the blocked dense band included: a refactor does not
 *   change route); about 16 bytes of int32 arrays per entry of L.  On the forest route (pinv NULL and A's elimination forest
 *   is cliques or small sparse trees on consecutive columns: paths 1 / 2 / 3 of csx_cholsol_factor_info) it keeps that forest
 *   instead; the block kernel runs without an emission, in the arithmetic "chol.exact" asks for at the call.  CSX_EINVAL with a message in csx_last_error() when an upper entry of A has no slot in L or L is not
 *   Cholesky-shaped.
 * csx_chol_refactor: A2 a matrix with A's pattern or a vector of nnz(A) values in A's storage order.  *ok = -1 (CSX_OK): another
 *   pattern or length, nothing changed.  *ok = 0: A2 is not positive definite; L.x and everything the solves read are byte
 *   for byte as before.  *ok = 1: L.x holds the factor of A2.  The new factor is computed in a scratch array of nnz(L) doubles
 *   (made by the first call, kept) and copied over L.x only when no pivot failed; an error status before that copy leaves
 *   everything as it was.  Plans made from L (csx_cholsol_plan, the triangular solves') hold stale values afterwards: the
 *   caller makes them again, as after csx_updown.  info (8 values, or NULL): [0] route: 0 general, 1 forest; [1] launches of
 *   the level walk; [2] supernodes; [3] small trees given to the tree kernel; [4] dense trees; [5] band kernel: 0 none,
 *   1 register window, 2 blocked dense band; [6] 1 when this call made the plan's scratch arrays; [7] 0.
 * csx_chol_refactor_info: the last csx_chol_refactor that ran: HIP-event time from the scatter of the values to the last
 *   launch, and the host clock over the whole call, pattern check and commit included.  CSX_EINVAL before the first.
 * csx_chol_refactor_window: the register-window instance (k_chol_band's BW: 48, 80, 112, 144 or 176) that the plan's last
 *   csx_chol_refactor launched, written down at the launch itself; 0 when it launched none (another band kind, the column
 *   kernels, the forest route, no refactor yet).  Reads host state only.
 * csx_chol_limits: the constants the general numeric path is cut by, without a device: out[16] = CH_ACC (entries of a column
 *   a wave of the column kernels keeps in LDS), CH_NARROW (columns of a level up to which a workgroup takes each), CH_SMALL_TREE
 *   (columns of a tree up to which the tree kernels take it), CD_MAX (columns of a dense tree), CC_ACC (doubles of partial
 *   columns in the cooperative kernel), CC_MAP (n up to which it keeps a row map in LDS), CC_RUN_MIN, CC_RUN_MAX (narrow levels
 *   of a two-phase run), CC_WAVES, SN_MIN_WIDTH, the five register-window widths ascending, the largest need (half-bandwidth
 *   + 1) a register window takes. */
int csx_chol_refactor_plan(csx_handle_t A, csx_handle_t L, const int32_t *pinv, csx_handle_t *plan);
int csx_chol_refactor(csx_handle_t plan, csx_handle_t A2, int *ok, int32_t *info);
int csx_chol_refactor_info(double *numeric_ms, double *call_ms);
int csx_chol_refactor_window(csx_handle_t plan, int32_t *window);
int csx_chol_limits(int32_t *out);

/* ---- assembly plan: new triplet values into a fixed CSC pattern (assembly_plan) --------------------
 * Definition.  Given the triplets (Ti[k], Tj[k]), k = 0 .. nz-1, of an m-by-n matrix, let C = cs_dupl(cs_compress(T)) as the
 * reference computes it.
 * Pattern: C.p and C.i are the reference's: columns in order, inside a column the rows in order of first appearance in the
 *   triplet list (cs_compress is a stable counting sort by column, cs_dupl keeps the first occurrence in place).
 * Plan: for every stored slot s of C, the triplets that land in it, ascending: sp[0 .. nnz] (slot pointers) and src[0 .. nz)
 *   (triplet indices grouped by slot), both int32.
 * Values: C.x[s] = (((v[t0]) + v[t1]) + v[t2]) + ... over src[sp[s] .. sp[s+1]), in that order, one IEEE double addition per
 *   term.  The first term is ASSIGNED, not added to zero (the reference does Ax[nz] = Ax[p] for a first occurrence): a slot
 *   whose terms are all -0.0 is -0.0.  No atomics, no reassociation; the same bits on every run.
 * csx_assemble_plan_host: the rule on host arrays -- a counting sort by column, then a first-occurrence scan with m marks;
 *   sequential, O(nz + m + n).  The caller's Cp, Ci, sp, src have room for n+1, nz, nz+1, nz entries; *nnz: the slots.
 *   CSX_EINVAL for an index outside [0, m) x [0, n) or nz > 2^31 - 1; nz = 0, n = 0 and empty columns are legal.
 * csx_assemble_host: the fold on host arrays: Cx[0 .. nnz) from Tx through sp, src.
 * csx_assemble_plan: Ti, Tj HOST arrays; runs the host rule once and uploads p, i, sp, src: a NEW plan handle (csx_free) that
 *   owns them -- 4 nz + 4 (nnz + 1) bytes beside the pattern (sp is not kept when nz == nnz: nothing reads it).  The slots
 *   are classified: one of more than "assemble.long" terms (csx_set_option, read here; default 64) is folded by a wave of its
 *   own -- 64 sources loaded per step, added in index order -- a shorter one by one lane; with no duplicates at all the
 *   fold is the permuted copy out[s] = Tx[src[s]].
 * csx_assemble_matrix: a NEW CSC handle with the plan's pattern (copied: plan and matrix have independent lifetimes), its
 *   values assembled from the vector Tx, or pattern only when Tx is 0.
 * csx_assemble: Tx a device vector of at least nz doubles; out a device vector of at least nnz doubles (not Tx), or a CSC
 *   handle with the plan's m, n, nnz and values, whose x is overwritten in place (the SpMV plans cached on it are dropped;
 *   triangular-solve plans made from it are stale).  CSX_EINVAL on a size mismatch, nothing written.  One launch queued on
 *   the context's stream; no host synchronisation.
 * csx_assemble_plan_info: info[6] = nz, nnz, the most terms of a slot, the slots folded by a wave, microseconds of the host
 *   build, microseconds of the last launch (between two events; waits for it). */
int csx_assemble_plan_host(int32_t m, int32_t n, int64_t nz, const int32_t *Ti, const int32_t *Tj, int32_t *Cp, int32_t *Ci,
                           int32_t *sp, int32_t *src, int32_t *nnz);
int csx_assemble_host(int32_t nnz, const int32_t *sp, const int32_t *src, const double *Tx, double *Cx);
int csx_assemble_plan(int32_t m, int32_t n, int64_t nz, const int32_t *Ti, const int32_t *Tj, csx_handle_t *plan);
int csx_assemble_matrix(csx_handle_t plan, csx_handle_t Tx, csx_handle_t *A);
int csx_assemble(csx_handle_t plan, csx_handle_t Tx, csx_handle_t out);
int csx_assemble_plan_info(csx_handle_t plan, int64_t *info);

/* ---- multiply plan: new values into the fixed pattern of A*B (multiply_plan) -----------------------
 * Definition.  A is m-by-k, B is k-by-n, both CSC; row indices inside a column in any order, duplicates inside a column legal,
 * exactly as csx_multiply accepts them.  Let C = cs_multiply(A, B) as the reference computes it.
 * Pattern: C.p and C.i are the reference's: columns in order, inside a column the rows in first-touch order, trimmed to nnz.
 * Plan: for every stored slot s of C, the products that land in it, in the reference's order: sp[0 .. nnz] (slot pointers) and
 *   pair[2t], pair[2t+1] = (ia, ib): product t is A.x[ia] times B.x[ib]; all int32.  Inside a slot of column j the order is: ib
 *   ascending through the STORED order of B(:,j) (p in B.p[j] .. B.p[j+1]), and for equal ib, ia ascending through A's column
 *   B.i[ib] -- the order of the reference's two nested loops, not an order of row indices.  products = sp[nnz] must fit in
 *   int32: CSX_EINVAL with a message in csx_last_error() otherwise.
 * Values:   beta_t = B.x[ib_t]                    (unscaled)
 *           beta_t = d[B.i[ib_t]] * B.x[ib_t]     (scaled by d, a vector of k doubles: C = A diag(d) B; one rounding)
 *           term_t = beta_t * A.x[ia_t]           (one rounding; NEVER fused with the addition that follows)
 *           C.x[s] = term_0;  then  C.x[s] = C.x[s] + term_t  for the slot's remaining products, in order.
 *   The first term is ASSIGNED (the reference does x[i] = beta * Ax[p] on first touch): a slot whose terms are all -0.0 is
 *   -0.0.  The scaled form is, by definition, cs_multiply(A, B2) with B2.x[p] = d[B.i[p]] * B.x[p].  For finite values the
 *   bytes are the reference's, the same on every run; NaN payloads are not promised.  No atomics, no hash table, no
 *   reassociation.
 * csx_multiply_plan_count: the two sizes on host arrays, *nnz and *products, as int64 (products may exceed int32 here).
 * csx_multiply_plan_host: the rule on host arrays by the reference's own loops on the indices alone -- an m-sized mark array
 *   for first touch, then a pass that drops each product at the next free place of its slot; sequential,
 *   O(products + m + n + nnz(A) + nnz(B)).  The caller's Cp, Ci, sp, pair have room for n+1, nnz, nnz+1, 2 products entries
 *   (sizes from csx_multiply_plan_count).  CSX_EINVAL for an index out of range, pointers that do not start at 0 or decrease,
 *   or products > 2^31 - 1.  k = 0, n = 0, empty columns and products = 0 are legal.  (A.n != B.m cannot be said here: there
 *   is one k.  csx_multiply_plan refuses it.)
 * csx_multiply_fold_host: the value rule on host arrays: Cx[0 .. nnz) from Ax, Bx through sp, pair.  The scaled form is this
 *   function on B2.x.
 * csx_multiply_plan: A, B device CSC handles (only their patterns are read; CSX_EINVAL when A.n != B.m); runs the host rule once
 *   and uploads p, i, sp, pair: a NEW plan handle (csx_free) that owns them and a copy of B.i -- 8 bytes per product + 4 per
 *   slot beside the pattern.  A and B themselves are not kept.  The slots are classified: one of more than "multiply.long"
 *   products (csx_set_option, read here; default 64, unmeasured) is folded by a wave of its own -- 64 pairs loaded per step,
 *   every lane forming one term, the terms added in index order -- a shorter one by one lane.
 * csx_multiply_plan_run: Ax / Bx are each a CSC handle with values, or a device vector of EXACTLY nnz(A) / nnz(B) doubles in
 *   storage order.  A CSC handle must have the operand's shape (m-by-k for Ax, k-by-n for Bx) and entry count; those are
 *   checked, its PATTERN IS NOT: the caller vouches for it (csx_chol_refactor's A2 is the same convention, except that there
 *   the pattern is compared).  d is 0 or a vector of at least k doubles.  out is a vector of at least nnz doubles, aliasing no
 *   input, or a CSC handle with the plan's m, n, nnz and values, whose x is overwritten in place (the SpMV plans cached on it
 *   are dropped; triangular-solve plans made from it are stale).  CSX_EINVAL on a size mismatch, nothing written.  One launch,
 *   two when scaled (d[B.i[p]] * B.x[p] into a scratch vector of nnz(B) doubles the plan makes at its first scaled step and
 *   keeps; the same fold then reads it in place of B.x), queued on the context's stream; no host synchronisation.
 * csx_multiply_plan_matrix: a NEW CSC handle with the plan's pattern (copied: plan and matrix have independent lifetimes), its
 *   values folded from Ax, Bx, d as above, or pattern only when Ax and Bx are both 0.
 * csx_multiply_plan_info: info[8] = m, n, nnz, products, the most products of a slot, the slots folded by a wave, microseconds
 *   of the host build, microseconds of the last step (between two events, both launches when scaled; waits for it). */
int csx_multiply_plan_count(int32_t m, int32_t k, int32_t n, const int32_t *Ap, const int32_t *Ai, const int32_t *Bp,
                            const int32_t *Bi, int64_t *nnz, int64_t *products);
int csx_multiply_plan_host(int32_t m, int32_t k, int32_t n, const int32_t *Ap, const int32_t *Ai, const int32_t *Bp,
                           const int32_t *Bi, int32_t *Cp, int32_t *Ci, int32_t *sp, int32_t *pair);
int csx_multiply_fold_host(int32_t nnz, const int32_t *sp, const int32_t *pair, const double *Ax, const double *Bx, double *Cx);
int csx_multiply_plan(csx_handle_t A, csx_handle_t B, csx_handle_t *plan);
int csx_multiply_plan_matrix(csx_handle_t plan, csx_handle_t Ax, csx_handle_t Bx, csx_handle_t d, csx_handle_t *C);
int csx_multiply_plan_run(csx_handle_t plan, csx_handle_t Ax, csx_handle_t Bx, csx_handle_t d, csx_handle_t out);
int csx_multiply_plan_info(csx_handle_t plan, int64_t *info);

/* ---- add plan: new values into the fixed pattern of a sum of matrices (add_plan) ---------------------
 * Definition.  Operands A_0 .. A_{k-1}, 2 <= k <= 8, all m-by-n CSC; row indices inside a column in any order, duplicates
 * inside a column legal, exactly as csx_add accepts them.  Coefficients c_0 .. c_{k-1}.  Let C be the reference's chain
 *   C_1 = cs_add(A_0, A_1, c_0, c_1),   C_r = cs_add(C_{r-1}, A_r, 1, c_r) for r >= 2,   C = C_{k-1}
 * (for k = 2, cs_add itself).
 * Pattern: C.p and C.i are the reference's: columns in order, inside column j the rows in first-touch order through A_0(:,j) as
 *   stored, then A_1(:,j), and so on.
 * Plan: for every stored slot s of C, the operand entries that land in it, in operand order, then stored position inside the
 *   operand's column -- the order in which the reference's loops touch them: sp[0 .. nnz] (slot pointers) and src[0 .. terms),
 *   both int32.  src[t] is an index into the concatenation of the operands' value arrays: entry e of A_r is off[r] + e,
 *   off[r] = sum of nnz(A_q) over q < r.  terms = sum of nnz(A_r) must fit in int32: CSX_EINVAL with a message in
 *   csx_last_error() otherwise.
 * Values:   term_t = c_r * A_r.x[e]               (one rounding; NEVER fused with the addition that follows)
 *           C.x[s] = term_0;  then  C.x[s] = C.x[s] + term_t  for the slot's remaining terms, in list order.
 *   The first term is ASSIGNED (cs_scatter does x[i] = beta * Ax[p] on first touch): a slot whose terms are all -0.0 is -0.0.
 *   For k > 2 this is the chain bit for bit: a sum so far has no duplicates, so each of its entries is the first term of its
 *   slot in the next cs_add, and the chain's 1 * x is exact for every finite x and keeps the sign of zero.  For finite values
 *   the bytes are the reference's, the same on every run; NaN payloads are not promised.  No atomics, no reassociation.
 * csx_add_plan_host: the rule on host arrays by the reference's own two loops on the indices alone -- an m-sized mark array for
 *   first touch and a sequential walk that counts, then places, the terms of each column; O(terms + m + n).  Ap, Ai: k
 *   pointers to the operands' p and i.  The caller's Cp, Ci, sp, src have room for n+1, terms, terms+1, terms entries; *nnz:
 *   the slots.  CSX_EINVAL for an index out of range, pointers that do not start at 0 or decrease, k outside 2 .. 8, or
 *   terms > 2^31 - 1.  n = 0, m = 0, empty columns and empty operands are legal.
 * csx_add_fold_host: the value rule on host arrays: Cx[0 .. nnz) from the k value arrays X[r] and coefficients coef[r] through
 *   sp, src and off[0 .. k].
 * csx_add_plan: k device CSC handles of one shape (only their patterns are read; the same handle may appear more than once:
 *   A + A; CSX_EINVAL on a shape mismatch); runs the host rule once and uploads the lists: a NEW plan handle (csx_free).  The
 *   operands themselves are not kept.  The step is one of two classes, decided here:
 *     aligned -- every operand has exactly C's pattern in C's order (nnz(A_r) = nnz for all r and src restricted to each operand
 *       is the identity: K + sigma M).  The step reads no index at all: out[s] = (c_0 x_0[s] + c_1 x_1[s]) + ..., streamed with
 *       16-byte accesses; 8 (k + 1) nnz bytes.  The plan keeps only the pattern.
 *     general -- the ordered fold: 4 bytes per term + 4 per slot beside the pattern.  A slot of more than "add.long" terms
 *       (csx_set_option, read here; default 64, unmeasured) is folded by a wave of its own -- 64 terms loaded per step, every
 *       lane forming one term, the terms added in index order -- a shorter one by one lane.
 * csx_add_plan_run: coef: k HOST doubles.  X: k handles, each a CSC handle with values, or a device vector of EXACTLY nnz(A_r)
 *   doubles in storage order.  A CSC handle must have the plan's shape and the operand's entry count; those are checked, its
 *   PATTERN IS NOT: the caller vouches for it (the convention of csx_multiply_plan_run).  out is a vector of at least nnz
 *   doubles, aliasing no input, or a CSC handle with the plan's m, n, nnz and values, whose x is overwritten in place (the SpMV
 *   plans cached on it are dropped; triangular-solve plans made from it are stale).  CSX_EINVAL on a mismatch, nothing written.
 *   One launch queued on the context's stream; no host synchronisation, no allocation.
 * csx_add_plan_matrix: a NEW CSC handle with the plan's pattern (copied: plan and matrix have independent lifetimes), its
 *   values those of a step on coef, X, or pattern only when X is NULL (coef is not read then).
 * csx_add_plan_info: info[11] = k, m, n, nnz, terms, the most terms of a slot, the slots folded by a wave (0 when aligned),
 *   aligned (0 / 1), microseconds of the host build, microseconds of the last step (between two events; waits for it), and the
 *   nzmax the reference's chain leaves (cs_add does not trim: the entries of the last cs_add's two operands). */
int csx_add_plan_host(int32_t m, int32_t n, int32_t k, const int32_t *const *Ap, const int32_t *const *Ai, int32_t *Cp,
                      int32_t *Ci, int32_t *sp, int32_t *src, int32_t *nnz);
int csx_add_fold_host(int32_t nnz, int32_t k, const int32_t *sp, const int32_t *src, const int32_t *off, const double *coef,
                      const double *const *X, double *Cx);
int csx_add_plan(int32_t k, const csx_handle_t *operands, csx_handle_t *plan);
int csx_add_plan_matrix(csx_handle_t plan, const double *coef, const csx_handle_t *X, csx_handle_t *C);
int csx_add_plan_run(csx_handle_t plan, const double *coef, const csx_handle_t *X, csx_handle_t out);
int csx_add_plan_info(csx_handle_t plan, int64_t *info);

/* ---- LDL' with static 1x1 pivots: symmetric indefinite matrices (ldlsol_factor) ------------------------
 * Definition.  A is a square CSC matrix with values, pinv a permutation or NULL, S = (parent, cp) the symbolic Cholesky analysis
 * of P A P' (csx_schol).  C = upper(P A P') exactly as cs_chol reads it: the stored entries with row <= column, of duplicates the
 * last, lower entries ignored.  L has the pattern of the Cholesky factor (L.p = cp; rows ascending, the diagonal first in each
 * column) and an EXPLICIT unit diagonal; d is a vector of n doubles; L diag(d) L' = C up to rounding.  No pivot search: the
 * order is the caller's, the pivots are 1x1.
 * Values, compiled without contraction on host and device:
 *   for every column j (any order that puts descendants in the elimination tree first):
 *     acc[r] = C(r, j) for the rows r of column j of L (0.0 in fill slots)
 *     for every column k < j with L(j,k) in the pattern, k ASCENDING:
 *       w = L(j,k) * d[k]                                          (rounded)
 *       for every stored p of column k from the slot of L(j,k) to the column's end:
 *         acc[L.i[p]] = acc[L.i[p]] - L.x[p] * w                   (product rounded, then the subtraction rounded)
 *     d[j] = acc[j]
 *     if tau > 0 and |d[j]| < tau:  d[j] = copysign(tau, d[j]), counted as a perturbed pivot
 *     if d[j] == 0 or d[j] is not finite:  breakdown at j (the smallest such j is reported)
 *     L(j,j) = 1.0;  L(r,j) = acc[r] / d[j]                        (IEEE division)
 *   On the device one wave owns a column and applies its updates one after another: L.x and d are byte-equal to
 *   csx_ldl_host, the same on every run.  No floating-point atomics.
 * csx_ldl_factor: *ok = 1 and a NEW factor handle (csx_free) that keeps the analysis (pattern and row view of L, entry map,
 *   height levels of the elimination tree) and owns L and d; *ok = 0 and *F = 0 on breakdown.  tau is the perturbation
 *   threshold (0: none).  CSX_EINVAL for a pattern-only or non-square A, an S or pinv that does not belong to A, tau < 0 or NaN.
 * csx_ldl_refactor: new values on the kept analysis: A2 a CSC handle with A's shape, entry count and pattern (compared), or a
 *   vector of exactly nnz(A) values in A's storage order; CSX_EINVAL (*ok = -1, nothing changed) otherwise.  The factor is
 *   computed into scratch arrays and copied over L.x and d only when no column broke down (*ok = 1); on breakdown (*ok = 0) L,
 *   d and every plan made from them are exactly as before.  L.x and d keep their addresses.
 * csx_ldl_parts: BORROWED handles of L (CSC) and d (vector of n doubles): the factor owns them, the caller must not free them,
 *   and they die with the factor.
 * csx_ldl_info: info[13] = n, entries of L, height levels of the tree, numeric launches of the last run, positive pivots, negative
 *   pivots (both of the committed factor), perturbed pivots of the last run, the smallest broken column of the last run or -1,
 *   microseconds of the last run between two events, then: launches of the level kernel, launches of the run walker (one
 *   workgroup walking consecutive levels of at most 4 columns), the columns of the last run that took the in-place path (longer
 *   than the LDS window, updated in global memory; counted by the kernels), the LDS window in entries.
 * csx_ldl_window: the LDS window in entries, without a device or a factor.
 * csx_ldl_stats: out[3] = min |d|, max |d|, max |l| off the diagonal of the committed factor (0.0 where there is none).
 * csx_block_div_rows: X[i, c] = X[i, c] / d[i] for the first `rows` rows of a row-major block of nrhs columns (X a vector of at
 *   least rows nrhs doubles, d of at least rows; CSX_EINVAL otherwise); queued on the context's stream.
 * csx_ldl_host: the rule on host arrays, no device: Lp / Li the pattern of L, Lx (Lp[n] doubles) and d (n doubles) written;
 *   info[4] = positive pivots, negative pivots, perturbed pivots, the smallest broken column or -1 (then Lx and d are not a
 *   factorisation).  CSX_EINVAL for a malformed pattern, an upper entry of A without a slot in L, tau < 0 or NaN. */
int csx_ldl_factor(csx_handle_t A, const int32_t *parent, const int32_t *cp, const int32_t *pinv, double tau, csx_handle_t *F,
                   int *ok);
int csx_ldl_refactor(csx_handle_t F, csx_handle_t A2, double tau, int *ok);
int csx_ldl_parts(csx_handle_t F, csx_handle_t *L, csx_handle_t *d);
int csx_ldl_info(csx_handle_t F, int64_t *info);
int csx_ldl_stats(csx_handle_t F, double *out);
int csx_ldl_window(int32_t *entries);
int csx_block_div_rows(csx_handle_t X, csx_handle_t d, int64_t rows, int32_t nrhs);
int csx_ldl_host(int32_t n, const int32_t *Ap, const int32_t *Ai, const double *Ax, const int32_t *pinv, const int32_t *Lp,
                 const int32_t *Li, double tau, double *Lx, double *d, int64_t *info);

/* ---- Partial LDL' with the Schur complement of a kept index set (schur_factor) ---------------------------
 * Definition.  A is a square CSC matrix with values, read as cs_chol reads it: the stored entries with row <= column, of
 * duplicates the last, lower entries ignored.  pinv is a permutation (or NULL) that numbers the n1 INTERIOR indices first and the
 * ns = n - n1 KEPT indices last (the caller's order among them); C = upper(P A P'); S_sym = (parent, cp) is the FULL symbolic
 * Cholesky analysis of P A P' (csx_schol of the permuted matrix), whose pattern Lf (rows ascending, the diagonal first) carries
 * the row view that the trailing columns need.
 * Values, compiled without contraction on host and device:
 *   columns j < n1: exactly csx_ldl_factor's rule (pivot rule, tau, breakdown) -- the first n1 columns of the LDL' of C
 *   columns j >= n1 (no pivot, no division, any order, independent of each other):
 *     acc[r] = C(r, j) for r >= j (0.0 where nothing is stored)
 *     for every k < n1 with L(j,k) in the pattern, k ASCENDING:
 *       w = L(j,k) * d[k]                                          (rounded)
 *       for every stored p of column k from the slot of L(j,k) to the column's end:
 *         acc[L.i[p]] = acc[L.i[p]] - L.x[p] * w                   (product rounded, then the subtraction rounded)
 *     S(r - n1, j - n1) = S(j - n1, r - n1) = acc[r]               (+0.0 outside the pattern)
 * Outputs.  Lp: an n x n CSC matrix, columns < n1 the columns of L (unit diagonal stored, rows >= n1 included), every column
 * >= n1 the single entry 1.0: Lp.p[j] = cp[j] for j <= n1, Lp.p[j] = cp[n1] + j - n1 beyond.  d: n1 doubles.  S: ns ns doubles,
 * symmetric, both triangles the same bytes.  P A P' = Lp blockdiag(diag(d), S) Lp' up to rounding.  Only an interior pivot can
 * break down: a zero or non-finite diagonal of S is data.
 *   On the device the interior columns are csx_ldl_factor's launches over the height levels of the first n1 columns (the walker of
 *   narrow levels cut at 256 levels a launch); the trailing columns are one launch, one wave per (column j, chunk of at most
 *   `window` consecutive rows of j .. n - 1), the chunk's sums in LDS, every update of row j with k < n1 applied in ascending k.
 *   Lp.x, d and S are byte-equal to csx_schur_host, the same on every run.  No floating-point atomics.
 * csx_schur_factor: *ok = 1 and a NEW factor handle (csx_free) that keeps the analysis and owns Lp, d and S; *ok = 0 and *F = 0 on
 *   an interior breakdown.  CSX_EINVAL for a pattern-only or non-square A, an S_sym or pinv that does not belong to A, n1 outside
 *   0 .. n, ns ns >= 2^31, tau < 0 or NaN.
 * csx_schur_refactor: new values on the kept analysis, A2 as for csx_ldl_refactor (*ok = -1 and CSX_EINVAL for a foreign pattern
 *   or length, nothing changed).  Everything is computed into scratch arrays; Lp.x, d and S are overwritten only when no interior
 *   column broke down (*ok = 1), and keep their addresses; on breakdown (*ok = 0) they and every plan made from Lp are as before.
 * csx_schur_parts: BORROWED handles of Lp (CSC), d (vector of n1 doubles) and S (vector of ns ns doubles): the factor owns them.
 * csx_schur_info: info[17] = n, n1, ns, entries of Lp, height levels of the interior tree, numeric launches of the last run
 *   (level + run + schur), launches of the level kernel, launches of the walker, launches of the trailing-column kernel, its
 *   (column, chunk) pairs, positive pivots, negative pivots (of the committed d), perturbed pivots of the last run, the smallest
 *   broken column of the last run or -1, microseconds of the last run between two events, interior columns of the last run
 *   updated in place (longer than the LDS window), the LDS window in entries.
 * csx_schur_stats: out[3] = min |d|, max |d|, max |l| off the diagonal over the interior columns of the committed factor.
 * csx_schur_host: the rule on host arrays, no device: Lfp / Lfi the FULL pattern Lf; Lpx (Lfp[n1] + ns doubles, the values of
 *   Lp), d (n1 doubles) and S (ns ns doubles) written; info[4] as csx_ldl_host's, over the interior.  CSX_EINVAL for a malformed
 *   pattern, an upper entry of A without a slot, n1 outside 0 .. n, ns ns >= 2^31, tau < 0 or NaN. */
int csx_schur_factor(csx_handle_t A, const int32_t *parent, const int32_t *cp, const int32_t *pinv, int32_t n1, double tau,
                     csx_handle_t *F, int *ok);
int csx_schur_refactor(csx_handle_t F, csx_handle_t A2, double tau, int *ok);
int csx_schur_parts(csx_handle_t F, csx_handle_t *Lp, csx_handle_t *d, csx_handle_t *S);
int csx_schur_info(csx_handle_t F, int64_t *info);
int csx_schur_stats(csx_handle_t F, double *out);
int csx_schur_host(int32_t n, const int32_t *Ap, const int32_t *Ai, const double *Ax, const int32_t *pinv, const int32_t *Lfp,
                   const int32_t *Lfi, int32_t n1, double tau, double *Lpx, double *d, double *S, int64_t *info);

/* ---- L U with static pivots: general unsymmetric matrices in one connected piece (slusol_factor) --------
 * Definition.  A is a square CSC matrix with values; prow a row permutation or NULL, A1 = A(prow, :) (row k of A1 is row prow[k]
 * of A: a matching puts a zero-free diagonal there); pinv a symmetric permutation or NULL, C = P A1 P' (C(pinv[i], pinv[j]) =
 * A1(i, j)); S = (parent, cp) the symbolic Cholesky analysis of the pattern of A1 + A1' under pinv (csx_schol of that pattern).
 * Of duplicate entries of A the last counts.  L and Ut are two matrices on ONE pattern, the Cholesky pattern of S (L.p = Ut.p =
 * cp; rows ascending, the diagonal first): L is unit lower triangular with the 1.0 stored, column k of Ut is row k of U with the
 * pivot U(k,k) first, so U = Ut'.  L U = C up to rounding.  No pivot search.
 * Values, compiled without contraction on host and device:
 *   for every column j (any order that puts descendants in the elimination tree first):
 *     accL[r] = C(r, j), accU[r] = C(j, r) for the rows r >= j of column j of the pattern (0.0 in fill and one-sided slots)
 *     for every column k < j with (j,k) in the pattern, k ASCENDING:
 *       l = L(j,k), u = Ut(j,k)
 *       for every stored p of column k from the slot of row j to the column's end, r = L.i[p]:
 *         accL[r] = accL[r] - L.x[p] * u;  accU[r] = accU[r] - Ut.x[p] * l      (product rounded, then the subtraction rounded)
 *     d = accU[j]                                                               (accL[j] has the same bits)
 *     if tau > 0 and |d| < tau:  d = copysign(tau, d), counted as a perturbed pivot
 *     if d == 0 or d is not finite:  breakdown at j (the smallest such j is reported)
 *     Ut(j,j) = d, Ut(r,j) = accU[r];  L(j,j) = 1.0, L(r,j) = accL[r] / d        (r > j; IEEE division)
 *   On the device one wave owns a column and applies its updates one after another: L.x and Ut.x are byte-equal to csx_slu_host,
 *   the same on every run.  No floating-point atomics.
 * csx_slu_factor: *ok = 1 and a NEW factor handle (csx_free) that keeps the analysis (pattern and row view, the two entry maps,
 *   A's pattern, height levels of the elimination tree) and owns L and Ut; *ok = 0 and *F = 0 on breakdown.  tau: the
 *   perturbation threshold (0: none).  CSX_EINVAL for a pattern-only or non-square A, an S or pinv that does not belong to the
 *   pattern of A1 + A1', a prow that is not a permutation, tau < 0 or NaN.
 * csx_slu_refactor: new values on the kept analysis, A2 as for csx_ldl_refactor (*ok = -1 and CSX_EINVAL for a foreign pattern
 *   or length, nothing changed); computed into scratch and copied over L.x and Ut.x only without a breakdown (*ok = 1); on
 *   breakdown (*ok = 0) both factors and every plan made from them are exactly as before.  The addresses never change.
 * csx_slu_parts: BORROWED handles of L and Ut (CSC, sharing p and i): the factor owns them, they die with it.
 * csx_slu_info: info[14] = n, entries of the pattern, height levels, numeric launches of the last run, launches of the level
 *   kernel, launches of the run walker (one workgroup walking at most `run cap` consecutive levels of at most 4 columns each per
 *   launch), perturbed pivots of the last run, the smallest broken column of the last run or -1, microseconds of the last run
 *   between two events, the columns of the last run updated in place (longer than the LDS window; counted by the kernels), the
 *   LDS window in entries, the run cap in levels, positive pivots, negative pivots (both of the committed factor).
 * csx_slu_stats: out[4] = min |d|, max |d|, max |l|, max |u| off the diagonal of the committed factor (0.0 where there is none).
 * csx_slu_window: the LDS window in entries and the run cap in levels, without a device or a factor.
 * csx_slu_host: the rule on host arrays, no device: Lp / Li the pattern, Lx and Utx (Lp[n] doubles each) written; info[4] =
 *   positive pivots, negative pivots, perturbed pivots, the smallest broken column or -1 (then Lx and Utx are not a
 *   factorisation).  CSX_EINVAL for a malformed pattern, a prow or pinv that is not a permutation, an entry of C without a slot,
 *   tau < 0 or NaN. */
int csx_slu_factor(csx_handle_t A, const int32_t *parent, const int32_t *cp, const int32_t *prow, const int32_t *pinv, double tau,
                   csx_handle_t *F, int *ok);
int csx_slu_refactor(csx_handle_t F, csx_handle_t A2, double tau, int *ok);
int csx_slu_parts(csx_handle_t F, csx_handle_t *L, csx_handle_t *Ut);
int csx_slu_info(csx_handle_t F, int64_t *info);
int csx_slu_stats(csx_handle_t F, double *out);
int csx_slu_window(int32_t *entries, int32_t *run_levels);
int csx_slu_host(int32_t n, const int32_t *Ap, const int32_t *Ai, const double *Ax, const int32_t *prow, const int32_t *pinv,
                 const int32_t *Lp, const int32_t *Li, double tau, double *Lx, double *Utx, int64_t *info);

/* ---- many value sets on the analysis of one csx_slu_factor (csx_slu_batch.hip) ----
 * A batch BORROWS the analysis of a factor F (pattern, row view, entry maps, height levels, launch schedule, permutations) and
 * owns B value sets: L.x and Ut.x of every member (B x lnz doubles each), its flags, statistics and threshold.  F must outlive
 * the batch (every call checks that F's handle still resolves and returns CSX_EINVAL otherwise); F's own L.x, Ut.x and scratch
 * are never written.  The members are independent: every one's L.x / Ut.x is byte-equal to csx_slu_host of its values alone.
 * All members go through F's launch schedule together: one launch per entry of it whatever B is (the member is a grid dimension).
 * There is NO scratch-then-commit: a member whose factorisation breaks down is marked failed (ok[m] = 0) and its values mean
 * nothing, where csx_slu_refactor keeps the old factor -- keeping B old factors would double B x lnz.  It disturbs no other member.
 * V: a device vector (csx_vec_*) holding an nnz(A) x B block, row-major: entry q of member m (A's storage order) at V[q * B + m].
 * B: 1 .. limits[0]; a larger B is CSX_EINVAL with a text (split the family into several batches).
 * csx_slu_batch_factor: a NEW batch handle (csx_free) with every member factored; tau: B thresholds (each >= 0) or NULL (none);
 *   ok: B ints.
 * csx_slu_batch_refactor: the same on the batch's own arrays (B is fixed); a member that failed before is computed afresh.
 * csx_slu_batch_norm1: out[m] = |A_m|_1 over F's kept pattern by csx_norm1's rule (one sequential sum per column, the maximum
 *   over the bit patterns of the sums that are not NaN): the very double csx_norm1 returns for member m alone.
 * csx_slu_batch_solve: X a device vector holding an n x (B r) block, row-major; columns m r .. m r + r - 1 belong to member m and
 *   are overwritten with A_m^-1 b (trans = 0) or A_m'^-1 b.  The permutations are the single solver's and are applied inside the
 *   call: x(pinv o prow^-1) = b, the two sweeps, x = x(pinv); swapped for trans.  The sweeps run over F's height levels and
 *   produce every component by the reference's operation sequence, every product and difference rounded on its own:
 *     ascending levels  (cs_lsolve of L; of Ut for trans):   x_j = ((x_j - v1 x_k1) - v2 x_k2) - ... over the entries (j, k) of row j,
 *                        k ascending, then / d_j for Ut (nothing for unit L)
 *     descending levels (cs_ltsolve of Ut; of L for trans):  the same chain over column j's stored entries below the diagonal in
 *                        storage order, then / d_j for Ut
 *   so every column is byte-equal to the single factor's solve in the exact order.  A wide level is one launch for all members and
 *   right-hand sides, a run of narrow levels one launch of a workgroup per member: two launches per entry of F's schedule.  The
 *   columns of a failed member are filled with NaN; a NaN or inf in a right-hand side stays in that member's column.
 * csx_slu_batch_info: shared[8] = n, entries of the pattern, height levels, numeric launches of the last run, of the level
 *   kernel, of the run walker, microseconds of the last run between two events, B; members[5 B] = per member: perturbed pivots,
 *   the smallest broken column or -1, columns updated in place, positive pivots, negative pivots.
 * csx_slu_batch_stats: out[4 B] = per member min |d|, max |d|, max |l|, max |u| off the diagonal.
 * csx_slu_batch_member: L.x and Ut.x of member m into host arrays of lnz doubles each.
 * csx_slu_batch_limits: out[6] = the most members of a batch (the y extent of a grid), the columns of a level a walker takes (a
 *   wider level is a launch of its own), the (row, column) pairs a solve workgroup of a wide level takes (a thread each), the
 *   terms of a chain such a thread fetches together, the (row, right-hand side) pairs a solve walker takes at a time (a wave
 *   each), the terms of a chain such a wave fetches together.  No device or factor needed. */
int csx_slu_batch_factor(csx_handle_t F, csx_handle_t V, int32_t B, const double *tau, csx_handle_t *batch, int *ok);
int csx_slu_batch_refactor(csx_handle_t batch, csx_handle_t V, const double *tau, int *ok);
int csx_slu_batch_norm1(csx_handle_t F, csx_handle_t V, int32_t B, double *out);
int csx_slu_batch_solve(csx_handle_t batch, csx_handle_t X, int32_t r, int trans);
int csx_slu_batch_info(csx_handle_t batch, int64_t *shared, int64_t *members);
int csx_slu_batch_stats(csx_handle_t batch, double *out);
int csx_slu_batch_member(csx_handle_t batch, int32_t m, double *Lx, double *Utx);
int csx_slu_batch_limits(int32_t *out);

/* ---- many symmetric value sets on the analysis of one csx_ldl_factor (csx_ldl_batch.hip) ----
 * The LDL' counterpart of the batch above: K - sigma_j M over shifts, quasi-definite KKT systems over scenarios.  A batch BORROWS
 * the analysis of a factor F of csx_ldl_factor (pattern, row view, entry map, height levels, launch schedule, permutation; a
 * factor of csx_schur_factor is refused with CSX_EINVAL and a text) and owns B value sets: L.x of every member (B x lnz doubles),
 * its pivots d (B x n), flags, statistics and threshold.  F must outlive the batch (every call checks that F's handle still
 * resolves and returns CSX_EINVAL with a text otherwise); F's own L.x, d, scratch and counters are never written.  The members
 * are independent: every one's L.x and d are byte-equal to csx_ldl_host of its values alone.  All members go through F's launch
 * schedule together: one launch per entry of it whatever B is.  There is NO scratch-then-commit: a member whose factorisation
 * breaks down is marked failed (ok[m] = 0) and its values mean nothing until a refactor mends it; it disturbs no other member.
 * V: a device vector holding an nnz(A) x B block, row-major: entry q of member m (A's storage order) at V[q * B + m]; read as
 *   csx_ldl_factor reads A (entries with row <= column, of duplicates the last).
 * B: 1 .. limits[0]; a larger B is CSX_EINVAL with a text (split the family into several batches).
 * csx_ldl_batch_factor: a NEW batch handle (csx_free) with every member factored; tau: B thresholds (each >= 0) or NULL (none);
 *   ok: B ints.
 * csx_ldl_batch_refactor: the same on the batch's own arrays (B is fixed); a member that failed before is computed afresh.
 * csx_ldl_batch_norm1: out[m] = |S_m|_1 of the symmetric matrix the factorisation sees, by csx_norm1_sym's rule (per row r first
 *   the entries of stored column r with row <= r in storage order, then the entries of row r with column > r in ascending
 *   (column, position), one sequential rounded sum; the maximum over the bit patterns of fabs of the sums, a NaN above inf): the
 *   very double csx_norm1_sym returns for member m alone.  The row view of A's pattern is made on the first call on F and kept.
 * csx_ldl_batch_solve: X a device vector holding an n x (B r) block, row-major; columns m r .. m r + r - 1 belong to member m and
 *   are overwritten with A_m^-1 b in the exact order: W[pinv[i], :] = X[i, :], cs_lsolve(L), / d, cs_ltsolve(L),
 *   X[i, :] = W[pinv[i], :], over F's height levels by the sweeps of csx_slu_batch_solve --
 *     ascending levels:   x_j = ((x_j - l1 x_k1) - l2 x_k2) - ... over the entries (j, k) of row j of L, k ascending
 *     descending levels:  s = x_j / d_j, then ((s - l1 x_i1) - l2 x_i2) - ... over column j's stored entries below the diagonal
 *   The division by D has no pass of its own: it opens row j's backward chain, which reads only finished x_i, i > j, so the bits
 *   are those of the three steps one after the other.  Every column is byte-equal to the single factor's solve in the exact
 *   order; two launches per entry of F's schedule for any B.  The columns of a failed member are filled with NaN; a NaN or inf
 *   in a right-hand side stays in its column.
 * csx_ldl_batch_info: shared[8] as csx_slu_batch_info's; members[5 B] = per member: perturbed pivots, the smallest broken column
 *   or -1, columns updated in place, positive pivots, negative pivots (the inertia, by Sylvester's law).
 * csx_ldl_batch_stats: out[3 B] = per member min |d|, max |d|, max |l| off the diagonal.
 * csx_ldl_batch_member: L.x (lnz doubles) and d (n doubles) of member m into host arrays.
 * csx_ldl_batch_d: the pivots of all members, B x n doubles member-major, in one download.
 * csx_ldl_batch_limits: out[6] = csx_slu_batch_limits' six constants (the level walk and the sweeps are shared).  No device or
 *   factor needed. */
int csx_ldl_batch_factor(csx_handle_t F, csx_handle_t V, int32_t B, const double *tau, csx_handle_t *batch, int *ok);
int csx_ldl_batch_refactor(csx_handle_t batch, csx_handle_t V, const double *tau, int *ok);
int csx_ldl_batch_norm1(csx_handle_t F, csx_handle_t V, int32_t B, double *out);
int csx_ldl_batch_solve(csx_handle_t batch, csx_handle_t X, int32_t r);
int csx_ldl_batch_info(csx_handle_t batch, int64_t *shared, int64_t *members);
int csx_ldl_batch_stats(csx_handle_t batch, double *out);
int csx_ldl_batch_member(csx_handle_t batch, int32_t m, double *Lx, double *d);
int csx_ldl_batch_d(csx_handle_t batch, double *out);
int csx_ldl_batch_limits(int32_t *out);

/* ---- many value sets on the analysis of one csx_hqr_factor (csx_hqr_batch.hip) ----
 * The Householder QR counterpart of the two batches above: reweighted least squares W_j A, Gauss-Newton Jacobians over scenarios,
 * regularisation sweeps on a stacked [A; lambda_j I].  A batch BORROWS the analysis of a factor F of csx_hqr_factor (the patterns
 * of V and R, the slot views, the entry maps, the height levels of the column elimination tree, the launch schedule, the
 * permutations q and pinv) and owns B value sets: V.x of every member (B x vnz doubles), R.x (B x rnz), beta (B x n), flags and
 * statistics.  F must outlive the batch (every call checks that F's handle still resolves and returns CSX_EINVAL with a text
 * otherwise); F's own V.x, R.x, beta, scratch and counters are never written.  The members are independent: every one's V.x,
 * R.x and beta are byte-equal to csx_hqr_host of its values alone.  All members go through F's launch schedule together: one
 * launch per entry of it whatever B is.  There is NO scratch-then-commit: a member with a non-finite diagonal of R is marked
 * failed (ok[m] = 0) and its values mean nothing until a refactor mends it; it disturbs no other member.
 * V: a device vector holding an nnz(A) x B block, row-major: entry q of member m at V[q * B + m], q in the storage order of
 *   the matrix F was made of (for a wide matrix that is its transpose: the caller reorders); empty slots of V and R are +0.0
 *   and of duplicate entries the one csx_hqr_factor takes (the last stored) is taken.
 * B: 1 .. limits[0]; a larger B is CSX_EINVAL with a text (split the family into several batches).
 * csx_hqr_batch_factor: a NEW batch handle (csx_free) with every member factored; ok: B ints.
 * csx_hqr_batch_refactor: the same on the batch's own arrays (B is fixed); a member that failed before is computed afresh.
 * csx_hqr_batch_solve: Xin a device vector holding a rows_in x (B r) block, row-major, columns m r .. m r + r - 1 belonging to
 *   member m; Xout another vector, filled with the rows_out x (B r) result.  With F of an m x n matrix (m >= n) and m2 rows of V:
 *     second == 0 (rows_in = m, rows_out = n): W[pinv[i], :] = Xin[i, :] into a zeroed m2 x (B r) block, Q' W, R \ W,
 *       Xout[q[k], :] = W[k, :] -- the least-squares solution, cs_qrsol's first sequence;
 *     second != 0 (rows_in = n, rows_out = m): W[k, :] = Xin[q[k], :], R' \ W, Q W, Xout[i, :] = W[pinv[i], :] -- cs_qrsol's
 *       second sequence: the minimum-norm solution of the transposed system.
 *   Every column has the bytes of the reference's operations in the reference's order: cs_happly reflection by reflection (the
 *   dot product in storage order, then tau *= beta, then the update), by csx_happly's levels and route with a lane per column
 *   reading its member's V.x and beta; cs_usolve as a gather over the rows of R from the top level of the column elimination tree
 *   down, x_i = (((x_i - R(i,j1) x_j1) - ...) / R(i,i)), j descending; cs_utsolve as a dot over column j's entries before its
 *   diagonal, x_j = ((x_j - sum R(i,j) x_i in storage order) / R(j,j)), from the leaves up.  The diagonal of R is the LAST stored
 *   entry of its column.  R(i,j) != 0 makes i a descendant of j in the tree, so F's levels order both sweeps: one launch per
 *   entry of F's schedule a sweep and csx_happly's launches for the reflections, for any B.  The row view of R is made on the
 *   first call on F and kept.  The columns of a failed member are filled with NaN; a NaN or inf in a right-hand side stays in
 *   its column.  An exact zero on R's diagonal is no breakdown of the factorisation (ok[m] stays 1 and the count is in
 *   csx_hqr_batch_info), but a solve with such a member ends as the single solver's does, where the reference divides by it:
 *   CSX_EZEROPIVOT with a text that names the member, nothing computed.
 * csx_hqr_batch_info: shared[12] = m, n, m2, vnz, rnz, levels, launches, level launches, run launches, kernel_us, B of the last
 *   run, and the kernel launches of the last solve; members[3 B] = per member: the smallest column with a non-finite diagonal
 *   or -1, columns updated in place, exact zeros on R's diagonal.
 * csx_hqr_batch_stats: out[2 B] = per member min |r_kk|, max |r_kk|.
 * csx_hqr_batch_member: V.x (vnz doubles), R.x (rnz doubles) and beta (n doubles) of member m into host arrays.
 * csx_hqr_batch_r_diag: the diagonals of all members' R, B x n doubles member-major, in one download.
 * csx_hqr_batch_limits: out[8] = csx_slu_batch_limits' six constants (the level walk and the sweeps are shared), the columns of
 *   X a workgroup of the reflection kernels takes (a lane each) and HAPPLY_MAX_LEVELS.  No device or factor needed. */
int csx_hqr_batch_factor(csx_handle_t F, csx_handle_t V, int32_t B, csx_handle_t *batch, int *ok);
int csx_hqr_batch_refactor(csx_handle_t batch, csx_handle_t V, int *ok);
int csx_hqr_batch_solve(csx_handle_t batch, csx_handle_t Xin, csx_handle_t Xout, int32_t r, int second);
int csx_hqr_batch_info(csx_handle_t batch, int64_t *shared, int64_t *members);
int csx_hqr_batch_stats(csx_handle_t batch, double *out);
int csx_hqr_batch_member(csx_handle_t batch, int32_t m, double *Vx, double *Rx, double *beta);
int csx_hqr_batch_r_diag(csx_handle_t batch, double *out);
int csx_hqr_batch_limits(int32_t *out);

/* ---- sparse Householder QR of a matrix in one connected piece, on the device (csx_hqr.hip) ----
 * A (m-by-n, m >= n, values) with cs_sqr's analysis of A(:, q): q (column order, n entries, or null), parent (column
 * elimination tree), pinv (row permutation, rows of A to 0 .. m2-1), leftmost (m entries), m2 (rows including fictitious ones).
 * Householder QR searches for no pivot, so the patterns are known before the values: V (m2-by-n, the diagonal first in every
 * column, then the rows in the order csx_qr_host finds them) and R (n-by-n, the entries in the order the reflections are
 * applied in, the diagonal last) have csx_qr_host's p and i exactly.  The values, compiled without contraction on host and device:
 *   for every column k (any order that puts descendants in the column elimination tree first):
 *     the slots of R(:,k) and V(:,k) = +0.0; A(:, q[k]) scattered at pinv[row], of duplicate entries the last stored
 *     for every c = R.i[t], t over the column's entries before its diagonal, in stored order:
 *       part[l] = +0.0, l = 0 .. 63
 *       for p = V.p[c] + l, step 64:  part[l] = part[l] + V.x[p] * work[V.i[p]]        (product rounded, then the sum)
 *       for s = 32, 16, 8, 4, 2, 1:   part[l] = part[l] + part[l + s] for l < s
 *       tau = part[0] * beta[c]
 *       work[V.i[p]] = work[V.i[p]] - V.x[p] * tau for every p of column c             (product rounded, then the subtraction)
 *       R.x[t] = work[c]
 *     V.x[p] = work[V.i[p]] for the column's slots
 *     tail2 = the same 64 strided sums and tree over V.x[p]^2, p after the head (lane l: V.p[k] + 1 + l, step 64)
 *     cs_house on (head, tail2), statement for statement as csx_qr_host (IEEE sqrt and division): the head of V(:,k), beta[k], and
 *     s = R's diagonal
 *   V.x, R.x and beta are byte-equal to csx_hqr_host, the same on every run, and equal to csx_qr_host's (cs_qr's) to rounding only:
 *   that loop sums a reflection's dot product entry by entry.  No floating-point atomics.
 * csx_hqr_symbolic_host: the patterns alone on host arrays, no device: csx_qr_host's loop without the values, Vp / Rp n + 1
 *   entries, Vi / Ri up to vcap / rcap.  CSX_EINVAL for m < n, capacities too small, or an analysis that is not this matrix's.
 * csx_hqr_host: the rule on host arrays, no device; csx_qr_host's arguments.
 * csx_hqr_factor: *ok = 1 and a NEW factor handle (csx_free) that keeps the analysis (A's pattern, the two entry maps, the sorted
 *   view of every column's slots, height levels of the tree) and owns V, R and beta; *ok = 0 and *F = 0 when a diagonal of R is
 *   not finite (the only breakdown).  CSX_EINVAL for a pattern-only A, m < n, or symbolic arrays that are not A's.
 * csx_hqr_refactor: new values on the kept analysis, A2 as for csx_ldl_refactor (*ok = -1 and CSX_EINVAL for a foreign pattern
 *   or length, nothing changed); computed into scratch and copied over V.x, R.x and beta only without a breakdown (*ok = 1); on
 *   breakdown (*ok = 0) the factor and every plan made from it are exactly as before.  The addresses never change.
 * csx_hqr_parts: BORROWED handles of V, R (CSC) and beta (a vector of n doubles): the factor owns them, they die with it.
 * csx_hqr_info: info[15] = m, n, m2, entries of V, entries of R, height levels, numeric launches of the last run, launches of
 *   the level kernel, launches of the run walker (one workgroup walking at most `run cap` consecutive levels of at most 4
 *   columns each per launch), the columns of the last run updated in place (more slots than the LDS window; counted by the
 *   kernels), exact zeros on R's diagonal (committed factor), the smallest broken column of the last run or -1, microseconds of
 *   the last run between two events, the LDS window in slots, the run cap in levels.
 * csx_hqr_stats: out[2] = min |r_kk|, max |r_kk| of the committed factor (0.0 for n = 0).
 * csx_hqr_window: the LDS window in slots and the run cap in levels, without a device or a factor.
 * csx_level_schedule: the launches of a numeric run of csx_ldl_factor, csx_schur_factor, csx_slu_factor and csx_hqr_factor over
 *   the height levels of a tree, on host arrays, no device.  level_ptr: nlev + 1 non-decreasing offsets, level l holds
 *   level_ptr[l + 1] - level_ptr[l] columns.  A level of more than `waves` columns is one launch, a wave per column.  A run of
 *   narrower levels goes to the walker (one workgroup, a barrier per level): a launch of it ends before the next wide level,
 *   after run_levels levels, or -- when work is not NULL (nlev figures >= 0) -- before the level that would take the sum of its
 *   levels' work past run_work; a level that alone exceeds run_work is still taken.  The factorisations call it with waves = 4;
 *   run_levels = 2^31 - 1 (LDL') or 256 (Schur, LU, QR); no work but for QR (the slot updates of the level's longest column,
 *   run_work = 2^24).  launches: room for 3 nlev integers, written as *count triples (1 wide / 0 walker, first level, end level)
 *   that cover 0 .. nlev - 1 in order.  CSX_EINVAL for nlev < 0, waves < 1, run_levels < 1, decreasing offsets, a null pointer.
 * csx_row_view: the rows of an n x n CSC pattern (p: n + 1 offsets from 0, i: p[n] rows, in any order, repeats allowed) with their
 *   storage positions, on host arrays, no device: what the value batches build for |S|_1 (A, ascending) and for cs_usolve (R,
 *   descending).  rp: n + 1 offsets; row r holds rc[q] = the column and rpos[q] = the position in i of its entries for q in
 *   [rp[r], rp[r + 1]), ordered by (column, position) ascending, or both descending; a row without entries is empty.
 *   CSX_EINVAL, nothing written: n < 0, p[0] != 0, decreasing offsets, a row outside 0 .. n - 1, a null pointer (i, rc and rpos
 *   may be null when p[n] = 0). */
int csx_hqr_symbolic_host(int32_t m, int32_t n, int32_t m2, const int32_t *Ap, const int32_t *Ai, const int32_t *q,
                          const int32_t *parent, const int32_t *pinv, const int32_t *leftmost, int32_t vcap, int32_t rcap,
                          int32_t *Vp, int32_t *Vi, int32_t *Rp, int32_t *Ri);
int csx_hqr_host(int32_t m, int32_t n, int32_t m2, const int32_t *Ap, const int32_t *Ai, const double *Ax, const int32_t *q,
                 const int32_t *parent, const int32_t *pinv, const int32_t *leftmost, int32_t vcap, int32_t rcap, int32_t *Vp,
                 int32_t *Vi, double *Vx, int32_t *Rp, int32_t *Ri, double *Rx, double *beta);
int csx_hqr_factor(csx_handle_t A, const int32_t *q, const int32_t *parent, const int32_t *pinv, const int32_t *leftmost,
                   int32_t m2, csx_handle_t *F, int *ok);
int csx_hqr_refactor(csx_handle_t F, csx_handle_t A2, int *ok);
int csx_hqr_parts(csx_handle_t F, csx_handle_t *V, csx_handle_t *R, csx_handle_t *beta);
int csx_hqr_info(csx_handle_t F, int64_t *info);
int csx_hqr_stats(csx_handle_t F, double *out);
int csx_hqr_window(int32_t *entries, int32_t *run_levels);
int csx_level_schedule(int32_t nlev, const int32_t *level_ptr, int32_t waves, int32_t run_levels, const int64_t *work,
                       int64_t run_work, int32_t *launches, int32_t *count);
int csx_row_view(int32_t n, const int32_t *p, const int32_t *i, int descending, int32_t *rp, int32_t *rc, int32_t *rpos);

/* ---- the block kernels of restarted GMRES (csx_gmres.hip): classical Gram-Schmidt on a block of columns against
 * a basis of blocks, every column its own system.  Blocks are row-major rows x nrhs.  The basis V is ONE vector holding
 * consecutive blocks V_0, V_1, ...; a call addresses its first nv.  mask: nrhs host int32; a column with mask[c] == 0 is not
 * written (on the device or in a host output array) and has no effect on any other.  work: a vector of at least
 * csx_gs_work_len(rows, nrhs, nv) doubles that the calls stage their coefficients and partial sums in (nothing else is
 * allocated); its contents mean nothing between calls.
 * Value rule (device and csx_gs_host alike, fp contract off): every product is rounded, then added or subtracted.  A sum over
 * the rows of a column is the ORDERED SUM: leaves are GS_CHUNK consecutive rows added in ascending order from +0.0, an inner node
 * is GS_FAN consecutive children added in ascending order from +0.0, levels repeat until one value is left.  The tree depends
 * on `rows` alone.
 *   csx_gs_project: h[i nrhs + c] = ordered sum over r of V_i[r, c] * w, w = W[r, c], or -W[r, c] when negate != 0; i < nv.
 *   csx_gs_update:  W[r, c] <- w - h[0, c] V_0[r, c] - ... - h[nv-1, c] V_{nv-1}[r, c], ascending i, each product and each
 *                   subtraction rounded (w as above); nrm2[c] = ordered sum of the squares of the new W[:, c], same pass.
 *   csx_gs_scale:   V_slot[r, c] = W[r, c] / s[c] (IEEE division).
 *   csx_gs_combine: U[r, c] = y[0, c] V_0[r, c] + ... + y[len[c]-1, c] V_{len[c]-1}[r, c]: the first product as it is, then one
 *                   rounded addition per further product; +0.0 for len[c] == 0.  y: nv x nrhs.
 * CSX_EINVAL: an unknown handle, a null mask or host array, nrhs < 1, rows < 0, nv < 1 (slot < 0), a basis shorter than nv
 * (slot + 1) blocks, a block W / U shorter than rows nrhs, a work vector that is too short, len[c] outside 0 .. nv on a live
 * column, or device ranges that overlap.  rows == 0: the sums are +0.0.
 * csx_gmres_limits: out[4] = GS_CHUNK, GS_FAN, GS_GROUP (basis vectors one pass of csx_gs_project carries in registers: W
 * crosses memory once per GS_GROUP of them), GS_TILE (rows per coefficient load in update / combine); no device needed.
 * csx_gs_host: op 0 .. 3 = project / update / scale / combine on host arrays: V the basis (scale writes block nv of it), W the
 * block (update overwrites it; unused by combine), coef = h / s / y, out = h / nrm2 / - / U. */
int csx_gmres_limits(int32_t *out);
int csx_gs_work_len(int64_t rows, int32_t nrhs, int32_t nblocks, int64_t *len);
int csx_gs_project(csx_handle_t V, int32_t nv, csx_handle_t W, csx_handle_t work, int64_t rows, int32_t nrhs, const int32_t *mask,
                   int negate, double *h);
int csx_gs_update(csx_handle_t V, int32_t nv, csx_handle_t W, csx_handle_t work, int64_t rows, int32_t nrhs, const int32_t *mask,
                  int negate, const double *h, double *nrm2);
int csx_gs_scale(csx_handle_t W, csx_handle_t V, int32_t slot, csx_handle_t work, int64_t rows, int32_t nrhs, const int32_t *mask,
                 const double *s);
int csx_gs_combine(csx_handle_t V, int32_t nv, csx_handle_t U, csx_handle_t work, int64_t rows, int32_t nrhs, const int32_t *mask,
                   const double *y, const int32_t *len);
int csx_gs_host(int op, int64_t rows, int32_t nrhs, int32_t nv, double *V, double *W, const int32_t *mask, int negate,
                const double *coef, const int32_t *len, double *out);

/* ---- the block kernels of eigsh() in which the columns of a block mix (csx_bgs.hip).  Blocks are row-major and
 * 16-byte aligned: the basis V is ONE vector of consecutive rows x b blocks V_0, V_1, ... (a call addresses its first nv), W and
 * U are rows x q, 1 <= b, q <= BGS_MAXW (wider outputs are made in column chunks by the caller).  work: a vector of at least
 * csx_bgs_work_len(rows, b, q, nv) doubles (nothing else is allocated); its contents mean nothing between calls.
 * Value rule: that of the csx_gs_* calls above, on the device and in csx_bgs_host alike: every product is rounded, then added or
 * subtracted; a sum over rows is the ORDERED SUM (leaves of GS_CHUNK rows, nodes of GS_FAN children, ascending from +0.0), whose
 * tree depends on `rows` alone; no floating-point atomics.
 *   csx_bgs_gram:    out[(i b + a) q + c] = ordered sum over r of V_i[r, a] * w, w = W[r, c], or -W[r, c] when negate != 0.
 *                    W is read only and may be a block of the basis.
 *   csx_bgs_update:  W[r, c] <- W[r, c] - H[0, 0, c] V_0[r, 0] - H[0, 1, c] V_0[r, 1] - ..., ascending in (i, a), every product
 *                    and every subtraction rounded.  H: nv x b x q.
 *   csx_bgs_combine: U[r, c] = S[0, 0, c] V_0[r, 0] + ..., ascending in (i, a): the first product as it is, then one rounded
 *                    addition per further product; +0.0 for nv == 0.  S: nv x b x q.
 * CSX_EINVAL: an unknown handle, a null host array, b or q outside 1 .. BGS_MAXW, rows < 0, nv < 0, a basis shorter than nv
 * blocks, a block shorter than rows q, a work vector that is too short or overlaps the basis or the block, a W (update) or U
 * (combine) that overlaps the basis.  rows == 0: the sums are +0.0.
 * csx_bgs_limits: out[5] = GS_CHUNK, GS_FAN, BGS_MAXW, BGS_GROUP (basis blocks whose sums one pass of csx_bgs_gram carries: W
 * crosses memory once per BGS_GROUP of them), BGS_TILE (doubles of a block's row tile in LDS); no device needed.
 * csx_bgs_host: op 0 .. 2 = gram / update / combine on host arrays: V the basis, W the block (update overwrites it; unused by
 * combine), coef = - / H / S, out = the sums / - / U; an array that holds nothing (rows == 0 or nv == 0) may be null. */
int csx_bgs_limits(int32_t *out);
int csx_bgs_work_len(int64_t rows, int32_t b, int32_t q, int32_t nblocks, int64_t *len);
int csx_bgs_gram(csx_handle_t V, int32_t nv, int32_t b, csx_handle_t W, int32_t q, csx_handle_t work, int64_t rows, int negate,
                 double *out);
int csx_bgs_update(csx_handle_t V, int32_t nv, int32_t b, csx_handle_t W, int32_t q, csx_handle_t work, int64_t rows,
                   const double *H);
int csx_bgs_combine(csx_handle_t V, int32_t nv, int32_t b, csx_handle_t U, int32_t q, csx_handle_t work, int64_t rows,
                    const double *S);
int csx_bgs_host(int op, int64_t rows, int32_t b, int32_t q, int32_t nv, const double *V, double *W, int negate, const double *coef,
                 double *out);

/* ---- outer product of two blocks sampled on a pattern: the gradient of a solve with respect to the stored entries
 * (outer_on_pattern, solve_grad) ----
 * U is m x nrhs, V is n x nrhs, row-major.  For the stored entry q of the m x n matrix A at (i, j) = (A.i[q], its column):
 *     mode 0 (general):  out[q] = alpha * sum over c of U[i,c] * V[j,c]
 *     mode 1 (sym; m == n, U and V both n x nrhs): A stands for the symmetric matrix S that csx_residual_sym_block reads in it.
 *         i <  j:  out[q] = alpha * sum over c of (U[i,c] * V[j,c] + U[j,c] * V[i,c])     (the entry stands at two places of S)
 *         i == j:  out[q] = alpha * sum over c of  U[i,c] * V[i,c]
 *         i >  j:  out[q] = +0.0                                                           (not part of S; alpha is not applied)
 * Only A.p and A.i are read: a pattern-only A is legal; duplicate and unsorted row indices are legal, every slot gets its value.
 * Value rule (device and csx_pattern_outer_host alike, fp contract off: every product is rounded, then added).  The order of the
 * sum over c is a function of nrhs alone:
 *     W = min(PO_LANES, smallest power of two >= nrhs) partial sums s[0 .. W).
 *     Partial l takes the columns c = l, l + W, l + 2 W, ... < nrhs, ascending.  Its first product is ASSIGNED, every further
 *     product is one rounded addition, s[l] = s[l] + t.  In sym mode with i < j a column gives two products, U[i,c] * V[j,c]
 *     first, then U[j,c] * V[i,c].  A partial without a column (l >= nrhs) is +0.0 and is combined like any other.
 *     Combine: for d = W/2, W/4, ..., 1:  s[l] = s[l] + s[l + d] for every l < d.
 *     out[q] = alpha * s[0], one rounded product (alpha = -1 is the exact negation).
 * nrhs == 1 is the single rounded product times alpha.  NaN and inf propagate, and only into the entries whose two rows hold
 * them.  No atomics, no scratch allocation, one launch queued on the context's stream, no host synchronisation (a matrix from
 * csx_csc_wrap is checked once, as everywhere).
 * csx_pattern_outer: U, V device vectors of at least m nrhs and n nrhs doubles (they may be the same block), out a device vector
 *   of at least nnz doubles.  CSX_EINVAL, nothing written: an unknown handle, nrhs < 1, a mode other than 0 or 1, sym with
 *   m != n, U, V or out too short, out overlapping U or V.  m == 0, n == 0 and nnz == 0 are legal and write nothing.
 * csx_pattern_outer_host: the rule on host arrays (no device); CSX_EINVAL for the same sizes and modes, a null array that would
 *   be read or written, p not ascending from 0, or a row index outside [0, m).
 * csx_pattern_outer_limits: out[5] = PO_LANES (16: 16 lanes x 8 bytes = one 128-byte line of a block row), PO_CHUNK (entries a
 *   workgroup takes: the kernel is balanced by entries, not columns), PO_WAVE_CHUNK (consecutive entries of the chunk that one
 *   wave takes), PO_FLIGHT (consecutive entries whose row gathers a lane group issues before it consumes the first), PO_KEPT
 *   (for nrhs <= PO_KEPT PO_LANES the rows V[j,:], U[j,:] of an entry's own column stay in registers while the entries of a
 *   step share the column; a wider block reads them per entry -- the same values in the same order); no device needed.
 * ---- the pull-back of an assembly plan: gradient of the assembled values with respect to the triplet values ----
 * C.x[s] is the sum of its triplets, so gT[t] = gA[slot of t]:  out[src[u]] = g[s] for u in [sp[s], sp[s+1]): a copy of bits.
 * csx_assemble_pullback: g a device vector of at least nnz doubles, out one of at least nz doubles; CSX_EINVAL, nothing written,
 *   for an unknown handle, a short vector, or out overlapping g.  One launch, no host synchronisation.
 * csx_assemble_pullback_host: the same on the plan's host arrays (csx_assemble_plan_host); CSX_EINVAL for sp not ascending from 0
 *   to nz or a src outside [0, nz). */
int csx_pattern_outer(csx_handle_t A, csx_handle_t U, csx_handle_t V, int32_t nrhs, int mode, double alpha, csx_handle_t out);
int csx_pattern_outer_host(int32_t m, int32_t n, const int32_t *p, const int32_t *i, int32_t nrhs, int mode, double alpha,
                           const double *U, const double *V, double *out);
int csx_pattern_outer_limits(int64_t *out);
int csx_assemble_pullback(csx_handle_t plan, csx_handle_t g, csx_handle_t out);
int csx_assemble_pullback_host(int32_t nnz, int64_t nz, const int32_t *sp, const int32_t *src, const double *g, double *out);

/* ---- synthetic inputs of the benchmark configs, generated on
 * the device from a counter-based hash so host and device agree bit for bit ---- */
int csx_gen_grand(int32_t n, int32_t per_col, uint64_t seed, csx_handle_t *out);
/* G-rand exactly as SURVEY 8d words it: per_col (<= 64) distinct rows per column drawn uniformly from [0, n),
 * ascending.  csx_gen_grand above draws one row per stratum of n/per_col rows instead (same marginal
 * distribution, row-block loads almost exactly equal); bench.py reports both. */
int csx_gen_grand_uniform(int32_t n, int32_t per_col, uint64_t seed, csx_handle_t *out);
int csx_gen_gspd(int32_t nblocks, int32_t bs, uint64_t seed, csx_handle_t *out);
int csx_gen_vec(int64_t len, uint64_t seed, double lo, double hi, csx_handle_t *out);
int csx_gen_rhs(int32_t n, int32_t nrhs, int32_t col0, csx_handle_t *out);

#ifdef __cplusplus
}
#endif
#endif /* CSX_H */
