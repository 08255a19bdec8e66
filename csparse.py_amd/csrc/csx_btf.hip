// Block triangular LU (btf_factor): the split of a square, structurally nonsingular A into the diagonal blocks D and the
// strictly block upper coupling F of C = A(p, q), the block levels, and the solve of A x = b from cs_lu(D) and F.
//
// The order of a solve is fixed by the factors: c = b(p); blocks from last to first, for every row of a
// block c_i -= F_ij z_j in cs_gaxpy's order (ascending column, storage order inside a column; multiply and subtract
// rounded separately); then the block's part of cs_ipvec(pinv), cs_lsolve(L), cs_usolve(U), operation for operation;
// x(q) = z.  Blocks of one level read only z of lower levels, so a level is one launch.
//
// The transposed solve A' x = b: C' is block LOWER triangular, so C' w = b(q), x(p) = w runs the blocks
// from first to last (highest level first): for every column j of a block c_j = b(q_j) - F(:, j)' w in F's column storage
// order; then the block's part of cs_utsolve(U), cs_ltsolve(L), cs_pvec(pinv).  The same kernels run it (TRANS = true) on
// programs built from the factors' own columns the first time it is asked for.
#include <algorithm>

#include "csx_internal.h"
#include "csx_sweep.h"

#pragma clang fp contract(off)

namespace csx {

constexpr int BTF_SMALL = 96;   // rows of the largest block solved with its tile in LDS (csx_lu_blocks' limit)
constexpr int BTF_TILE = 64;    // right-hand sides of a tile of k_btf_small: one per lane; a row of the LDS tile

struct BtfLarge {   // a block of more than BTF_SMALL rows: its own L and U (local indices) and exact triangular plans of them
    BtfLarge() = default;
    BtfLarge(const BtfLarge &) = delete;
    BtfLarge &operator=(const BtfLarge &) = delete;
    ~BtfLarge() {
        destroy(pl);
        destroy(pu);
        destroy(put);
        destroy(plt);
    }
    int32_t r0 = 0, nr = 0;
    Csc L, U;
    TriPlan *pl = nullptr, *pu = nullptr;
    TriPlan *put = nullptr, *plt = nullptr;   // U' and L' (transposed solves, made on the first one)
};

// What only a refactor needs (csx_btf_refactor), made on its first call: A's pattern, the maps from A's entries to D's and F's,
// the maps from L.x / U.x / F.x to the slots of the forward programs, the schedule, and scratch for the new values
struct BtfRefactor {
    BtfRefactor() = default;
    BtfRefactor(const BtfRefactor &) = delete;
    BtfRefactor &operator=(const BtfRefactor &) = delete;
    ~BtfRefactor() { destroy(R); }
    int32_t anz = 0;
    DevBuf<int32_t> p0, i0;                         // A's pattern
    DevBuf<int32_t> dmap, fmap;                     // entry t of D / F is entry map[t] of A
    Csc Dq;                                         // D's pattern; x holds the gathered values of the current A2
    DevBuf<int32_t> lxmap, ldmap, uxmap, udmap, ftmap;   // program slot -> entry of L.x / U.x / F.x
    DevBuf<double> Fx, Lx, Ux;                      // scratch: committed only when every pivot passed
    DevBuf<int> flag;
    std::vector<int32_t> Lp, Up;                    // host copies (the large blocks' ranges of L.x / U.x)
    Refactor *R = nullptr;
};

struct BtfPlan {
    int32_t n = 0, nb = 0, nlevels = 0, max_block = 0;
    int64_t lnz = 0, unz = 0, fnz = 0;
    DevBuf<int32_t> p, q, pinv, r;
    // row programs: L without its diagonal (ascending column), U without its diagonal (DESCENDING column), F (ascending
    // column); the L / U indices are (column - first row of the block) * 64: LDS offsets of the block's X tile
    DevBuf<int32_t> Lp, Li, Up, Ui;
    DevBuf<double> Lx, Ld, Ux, Ud;
    Csc Ft;                              // F' = the rows of F in cs_gaxpy's order
    DevBuf<int32_t> small;               // small blocks grouped by level (level 0 first), ascending block inside a level
    std::vector<int32_t> small_ptr;      // [nlevels + 1] into small
    std::vector<int32_t> small_rows;     // [nlevels] largest small block of the level
    std::vector<std::vector<int32_t>> large_of_level;   // indices into large
    std::vector<std::unique_ptr<BtfLarge>> large;
    // the transposed solve (btf_trans_plan, made on its first call from the factors the plan was made from -- held by the
    // caller, looked up by handle then): column programs of U without its diagonal (storage order: the diagonal is last) and
    // of L without its diagonal (storage order: the diagonal is first), indices as LDS offsets like the row programs; F's
    // columns with their rows mapped through pinv (the work block holds v, w_i = v(pinv_i))
    csx_handle_t hL = 0, hU = 0, hF = 0;
    std::vector<int32_t> r_h, level_h;   // [nb + 1], [nb]
    bool trans_ready = false;
    DevBuf<int32_t> UTp, UTi, LTp, LTi, Fcp, Fci;
    DevBuf<double> UTx, UTd, LTx, LTd, Fcx;
    std::unique_ptr<BtfRefactor> rf;   // csx_btf_refactor's, from its first call
};

void destroy(BtfPlan *P) { delete P; }

static unsigned grid_for(int64_t count) { return (unsigned)std::max<int64_t>(1, (count + 255) / 256); }

// ------------------------------------------------------------------------------------------------ the split --

// per column j of C: entries whose row lies in column j's block (D) -- the rest are F
__global__ __launch_bounds__(256) void k_btf_count(int32_t n, const int32_t *__restrict__ Cp, const int32_t *__restrict__ Ci,
                                                   const int32_t *__restrict__ blk, int32_t *__restrict__ dcnt,
                                                   int32_t *__restrict__ fcnt) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const int32_t b = blk[j];
    int32_t d = 0;
    for (int32_t t = Cp[j]; t < Cp[j + 1]; t++) d += blk[Ci[t]] == b;
    dcnt[j] = d;
    fcnt[j] = Cp[j + 1] - Cp[j] - d;
}

__global__ __launch_bounds__(256) void k_btf_fill(int32_t n, const int32_t *__restrict__ Cp, const int32_t *__restrict__ Ci,
                                                  const double *__restrict__ Cx, const int32_t *__restrict__ blk,
                                                  const int32_t *__restrict__ Dp, int32_t *__restrict__ Di,
                                                  double *__restrict__ Dx, const int32_t *__restrict__ Fp,
                                                  int32_t *__restrict__ Fi, double *__restrict__ Fx) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const int32_t b = blk[j];
    int32_t d = Dp[j], f = Fp[j];
    for (int32_t t = Cp[j]; t < Cp[j + 1]; t++) {
        const int32_t i = Ci[t];
        if (blk[i] == b) {
            Di[d] = i;
            Dx[d++] = Cx[t];
        } else {
            Fi[f] = i;
            Fx[f++] = Cx[t];
        }
    }
}

static int split_device(const Csc *C, const std::vector<int32_t> &blk_h, Csc *D, Csc *F) {
    hipStream_t s = ctx().stream;
    const int32_t n = C->n;
    DevBuf<int32_t> blk, dcnt, fcnt;
    CSX_TRY(blk.alloc((size_t)n + 1));
    CSX_TRY(dcnt.alloc((size_t)n + 1));
    CSX_TRY(fcnt.alloc((size_t)n + 1));
    if (n) CSX_HIP(hipMemcpyAsync(blk, blk_h.data(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, s));
    if (n) hipLaunchKernelGGL(k_btf_count, dim3(grid_for(n)), dim3(256), 0, s, n, C->p, C->i, blk, dcnt, fcnt);
    CSX_LAUNCH_CHECK();
    for (Csc *M : {D, F}) {
        M->m = M->n = n;
        M->owns = true;
        CSX_TRY(dalloc(&M->p, (size_t)n + 1));
    }
    int64_t dnz = 0, fnz = 0;
    CSX_TRY(scan_exclusive_i32(dcnt, D->p, n, &dnz));
    CSX_TRY(scan_exclusive_i32(fcnt, F->p, n, &fnz));
    D->nnz = (int32_t)dnz;
    F->nnz = (int32_t)fnz;
    CSX_TRY(dalloc(&D->i, (size_t)dnz));
    CSX_TRY(dalloc(&D->x, (size_t)dnz));
    CSX_TRY(dalloc(&F->i, (size_t)fnz));
    CSX_TRY(dalloc(&F->x, (size_t)fnz));
    if (n)
        hipLaunchKernelGGL(k_btf_fill, dim3(grid_for(n)), dim3(256), 0, s, n, C->p, C->i, C->x, blk, D->p, D->i, D->x, F->p,
                           F->i, F->x);
    CSX_LAUNCH_CHECK();
    CSX_HIP(hipStreamSynchronize(s));
    return CSX_OK;
}

// ------------------------------------------------------------------------------------------------- the plan --

// TRANS = false, T the transpose of a factor: row i of L' (= column i of Lt, ascending column, the unit diagonal last) ->
// program row without the diagonal; row i of U' (diagonal first) -> program row in descending column order.
// TRANS = true, T the factor itself: column i of U (diagonal last) and column i of L (diagonal first) -> program row
// without the diagonal, the other entries in storage order.  Every index must lie in row i's block and on the right side of
// the diagonal: *bad = 1 otherwise (the kernels index LDS by these indices).
template <bool TRANS>
__global__ __launch_bounds__(256) void k_btf_strip(int32_t n, int upper, const int32_t *__restrict__ Tp,
                                                   const int32_t *__restrict__ Ti, const double *__restrict__ Tx,
                                                   const int32_t *__restrict__ row_r0, const int32_t *__restrict__ row_r1,
                                                   int32_t *__restrict__ Pp, int32_t *__restrict__ Pi,
                                                   double *__restrict__ Px, double *__restrict__ Pd, int *bad) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n) return;
    if (i == n) {
        Pp[n] = Tp[n] - n;
        return;
    }
    const int32_t a = Tp[i], e = Tp[i + 1];
    Pp[i] = a - (int32_t)i;
    const bool diag_first = TRANS ? !upper : upper;     // where the diagonal sits in T's column i
    const bool above = TRANS ? !upper : upper;          // the other indices lie after i (else before)
    // (a row without its diagonal shifts the program of the rows after it: caught here before anything is written)
    if (e <= a || (int64_t)a - i < 0 || (int64_t)e - i - 1 > (int64_t)Tp[n] - n || Ti[diag_first ? a : e - 1] != i) {
        *bad = 1;
        return;
    }
    const int32_t r0 = row_r0[i], r1 = row_r1[i];
    Pd[i] = Tx[diag_first ? a : e - 1];
    const int32_t cnt = e - a - 1;
    for (int32_t t = 0; t < cnt; t++) {
        const int32_t src = TRANS ? (diag_first ? a + 1 + t : a + t) : (upper ? e - 1 - t : a + t);
        const int32_t j = Ti[src];
        if (above ? (j <= i || j >= r1) : (j >= i || j < r0)) *bad = 1;
        Pi[a - i + t] = (j - r0) * BTF_TILE;
        Px[a - i + t] = Tx[src];
    }
}

// F's columns in row i must lie in blocks after row i's block, of a lower level (solved by an earlier launch)
__global__ __launch_bounds__(256) void k_btf_check_f(int32_t n, const int32_t *__restrict__ Fp, const int32_t *__restrict__ Fi,
                                                     const int32_t *__restrict__ row_r1, const int32_t *__restrict__ row_lev,
                                                     int *bad) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    for (int32_t t = Fp[i]; t < Fp[i + 1]; t++) {
        const int32_t j = Fi[t];
        if (j < row_r1[i] || j >= n || row_lev[j] >= row_lev[i]) *bad = 1;
    }
}

// F's columns for the transposed solve: rows mapped through pinv; every row in a block of a higher level than column j's
// (solved by an earlier launch when the levels run highest first)
__global__ __launch_bounds__(256) void k_btf_tcols(int32_t n, const int32_t *__restrict__ Fp, const int32_t *__restrict__ Fi,
                                                   const int32_t *__restrict__ pinv, const int32_t *__restrict__ row_lev,
                                                   int32_t *__restrict__ Fci, int *bad) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    for (int32_t t = Fp[j]; t < Fp[j + 1]; t++) {
        const int32_t i = Fi[t];
        if (i < 0 || i >= n || row_lev[i] <= row_lev[j]) {
            *bad = 1;
            Fci[t] = 0;
        } else {
            Fci[t] = pinv[i];
        }
    }
}

// rows of a block's own factor: row index - r0 (col_block_device keeps the global rows)
__global__ __launch_bounds__(256) void k_btf_shift_rows(int32_t nnz, int32_t r0, int32_t *__restrict__ Ci) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < nnz) Ci[t] -= r0;
}

static int block_factor(const Csc *M, int32_t r0, int32_t nr, Csc *out) {
    CSX_TRY(col_block_device(M, r0, nr, out));
    out->m = nr;
    if (out->nnz)
        hipLaunchKernelGGL(k_btf_shift_rows, dim3(grid_for(out->nnz)), dim3(256), 0, ctx().stream, out->nnz, r0, out->i);
    CSX_LAUNCH_CHECK();
    return CSX_OK;
}

// trans = false: row programs of M' (M transposed here); trans = true: column programs of M itself
static int strip(const Csc *M, bool upper, bool trans, const int32_t *row_r0, const int32_t *row_r1, int *bad,
                 DevBuf<int32_t> &Pp, DevBuf<int32_t> &Pi, DevBuf<double> &Px, DevBuf<double> &Pd) {
    hipStream_t s = ctx().stream;
    const int32_t n = M->n;
    Csc T;
    if (!trans) CSX_TRY(transpose_device(M, true, &T));
    const Csc *S = trans ? M : &T;
    const int64_t cnt = std::max<int64_t>(0, (int64_t)S->nnz - n);
    CSX_TRY(Pp.alloc((size_t)n + 1));
    CSX_TRY(Pi.alloc((size_t)cnt));
    CSX_TRY(Px.alloc((size_t)cnt));
    CSX_TRY(Pd.alloc((size_t)n));
    if (trans)
        hipLaunchKernelGGL(k_btf_strip<true>, dim3(grid_for((int64_t)n + 1)), dim3(256), 0, s, n, upper ? 1 : 0, S->p, S->i,
                           S->x, row_r0, row_r1, Pp, Pi, Px, Pd, bad);
    else
        hipLaunchKernelGGL(k_btf_strip<false>, dim3(grid_for((int64_t)n + 1)), dim3(256), 0, s, n, upper ? 1 : 0, S->p, S->i,
                           S->x, row_r0, row_r1, Pp, Pi, Px, Pd, bad);
    CSX_LAUNCH_CHECK();
    CSX_HIP(hipStreamSynchronize(s));
    return CSX_OK;
}

// ------------------------------------------------------------------------------------------------ the solve --

// Small blocks of one level: one wave per (block, tile of 64 right-hand sides), the block's rows of the tile in LDS,
// one lane per right-hand side.  Every LDS slot a lane touches is in its own column of the tile: no barrier.
// A solve: p the load map, (Fp, Fi, Fx) F's rows, (Lp ..) L's row programs (ascending), (Up ..) U's (descending), the
// entries scattered by pinv.  TRANS: p = q, F's columns with rows through pinv, U''s then L''s programs in their places,
// no scatter (W then holds v, w = v(pinv)).
template <bool TRANS>
__global__ __launch_bounds__(64) void k_btf_small(const int32_t *__restrict__ blocks, const int32_t *__restrict__ r,
                                                  const int32_t *__restrict__ p, const int32_t *__restrict__ pinv,
                                                  const int32_t *__restrict__ Fp, const int32_t *__restrict__ Fi,
                                                  const double *__restrict__ Fx, const int32_t *__restrict__ Lp,
                                                  const int32_t *__restrict__ Li, const double *__restrict__ Lx,
                                                  const double *__restrict__ Ld, const int32_t *__restrict__ Up,
                                                  const int32_t *__restrict__ Ui, const double *__restrict__ Ux,
                                                  const double *__restrict__ Ud, const double *__restrict__ B,
                                                  double *__restrict__ W, int32_t k) {
    extern __shared__ double X[];
    const int lane = threadIdx.x;
    const int32_t b = blocks[blockIdx.x];
    const int32_t r0 = r[b], nr = r[b + 1] - r0;
    const int32_t col = (int32_t)blockIdx.y * BTF_TILE + lane;
    const bool on = col < k;
    // c = b(p), minus the F terms (the z they read is final: lower levels), scattered by pinv into the tile
    // (TRANS: c = b(q) minus F(:, j)' w, w final: higher levels; slot t)
    for (int32_t t = 0; t < nr; t++) {
        const int32_t i = r0 + t;
        double acc = on ? B[(int64_t)p[i] * k + col] : 0.0;
        const int32_t qe = Fp[i + 1];
        for (int32_t q = Fp[i]; q < qe; q += TERM_CHUNK) {
            const TermRegs T = load_terms(Fi, Fx, q, qe, lane);
            const int ulim = min(TERM_CHUNK, qe - q);
            for (int u = 0; u < ulim; u++) {
                const int32_t j = __builtin_amdgcn_readlane(T.i, u);
                const double z = on ? W[(int64_t)j * k + col] : 0.0;
                const double prod = bcast_f64(T.v, u) * z;
                acc = acc - prod;
            }
        }
        X[(TRANS ? t : pinv[i] - r0) * BTF_TILE + lane] = acc;
    }
    // cs_lsolve on the block: rows ascending, terms in ascending column (TRANS: cs_utsolve, terms in storage order)
    for (int32_t t = 0; t < nr; t++) {
        const int32_t i = r0 + t;
        double acc = X[t * BTF_TILE + lane];
        const int32_t qe = Lp[i + 1];
        for (int32_t q = Lp[i]; q < qe; q += TERM_CHUNK) {
            const TermRegs T = load_terms(Li, Lx, q, qe, lane);
            acc = apply_terms(acc, T, 0, min(TERM_CHUNK, qe - q), X, lane);
        }
        X[t * BTF_TILE + lane] = acc / Ld[i];
    }
    // cs_usolve on the block: rows descending, terms in descending column (TRANS: cs_ltsolve, terms in storage order)
    for (int32_t t = nr - 1; t >= 0; t--) {
        const int32_t i = r0 + t;
        double acc = X[t * BTF_TILE + lane];
        const int32_t qe = Up[i + 1];
        for (int32_t q = Up[i]; q < qe; q += TERM_CHUNK) {
            const TermRegs T = load_terms(Ui, Ux, q, qe, lane);
            acc = apply_terms(acc, T, 0, min(TERM_CHUNK, qe - q), X, lane);
        }
        X[t * BTF_TILE + lane] = acc / Ud[i];
    }
    if (on)
        for (int32_t t = 0; t < nr; t++) W[(int64_t)(r0 + t) * k + col] = X[t * BTF_TILE + lane];
}

// The rows of a large block: W(pinv(i)) = b(p(i)) - F(i, :) z, one thread per (row, right-hand side)
// (TRANS: W(j) = b(q(j)) - F(:, j)' w, p = q and F's columns)
template <bool TRANS>
__global__ __launch_bounds__(256) void k_btf_rows(int32_t r0, int32_t nr, const int32_t *__restrict__ p,
                                                  const int32_t *__restrict__ pinv, const int32_t *__restrict__ Fp,
                                                  const int32_t *__restrict__ Fi, const double *__restrict__ Fx,
                                                  const double *__restrict__ B, double *__restrict__ W, int32_t k) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= (int64_t)nr * k) return;
    const int32_t i = r0 + (int32_t)(g / k), col = (int32_t)(g % k);
    double acc = B[(int64_t)p[i] * k + col];
    for (int32_t t = Fp[i]; t < Fp[i + 1]; t++) {
        const double prod = Fx[t] * W[(int64_t)Fi[t] * k + col];
        acc = acc - prod;
    }
    W[(int64_t)(TRANS ? i : pinv[i]) * k + col] = acc;
}

// x(q) = z   (TRANS: x(p) = w = v(pinv), q = p)
template <bool TRANS>
__global__ __launch_bounds__(256) void k_btf_out(int32_t n, const int32_t *__restrict__ q, const int32_t *__restrict__ pinv,
                                                 const double *__restrict__ W, double *__restrict__ B, int32_t k) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= (int64_t)n * k) return;
    const int32_t t = (int32_t)(g / k), col = (int32_t)(g % k);
    B[(int64_t)q[t] * k + col] = TRANS ? W[(int64_t)pinv[t] * k + col] : W[g];
}

static int btf_solve(BtfPlan *P, const double *B, double *W, double *Bout, int32_t k) {
    hipStream_t s = ctx().stream;
    const unsigned tiles = (unsigned)((k + BTF_TILE - 1) / BTF_TILE);
    for (int32_t l = 0; l < P->nlevels; l++) {
        const int32_t a = P->small_ptr[l], e = P->small_ptr[l + 1];
        if (e > a) {
            const size_t lds = (size_t)P->small_rows[l] * BTF_TILE * sizeof(double);
            hipLaunchKernelGGL(k_btf_small<false>, dim3((unsigned)(e - a), tiles), dim3(64), lds, s, P->small + a, P->r, P->p,
                               P->pinv, P->Ft.p, P->Ft.i, P->Ft.x, P->Lp, P->Li, P->Lx, P->Ld, P->Up, P->Ui, P->Ux, P->Ud, B,
                               W, k);
            CSX_LAUNCH_CHECK();
        }
        for (int32_t li : P->large_of_level[l]) {
            BtfLarge *G = P->large[li].get();
            hipLaunchKernelGGL(k_btf_rows<false>, dim3(grid_for((int64_t)G->nr * k)), dim3(256), 0, s, G->r0, G->nr, P->p,
                               P->pinv, P->Ft.p, P->Ft.i, P->Ft.x, B, W, k);
            CSX_LAUNCH_CHECK();
            double *Wb = W + (int64_t)G->r0 * k;
            CSX_TRY(tri_solve_raw(G->pl, Wb, k, false));
            CSX_TRY(tri_solve_raw(G->pu, Wb, k, false));
        }
    }
    if (P->n)
        hipLaunchKernelGGL(k_btf_out<false>, dim3(grid_for((int64_t)P->n * k)), dim3(256), 0, s, P->n, P->q, nullptr, W, Bout,
                           k);
    CSX_LAUNCH_CHECK();
    return CSX_OK;
}

// The transposed solve's programs, from the factors the plan was made from (CSX_EINVAL when one of them is gone or does not
// pass the checks).  Nothing of it exists until the first transposed solve: btf_factor's time and memory stay as they were.
static int btf_trans_plan(BtfPlan *P) {
    if (P->trans_ready) return CSX_OK;
    Csc *L = csc(P->hL), *U = csc(P->hU), *F = csc(P->hF);
    const int32_t n = P->n, nb = P->nb;
    if (!L || !U || !F || !L->x || !U->x || !F->x || L->n != n || U->n != n || F->n != n || L->m != n || U->m != n || F->m != n)
        return CSX_EINVAL;
    hipStream_t s = ctx().stream;
    std::vector<int32_t> r0h((size_t)n), r1h((size_t)n), levh((size_t)n);
    for (int32_t b = 0; b < nb; b++)
        for (int32_t i = P->r_h[b]; i < P->r_h[b + 1]; i++) {
            r0h[i] = P->r_h[b];
            r1h[i] = P->r_h[b + 1];
            levh[i] = P->level_h[b];
        }
    DevBuf<int32_t> row_r0, row_r1, row_lev;
    DevBuf<int> bad;
    CSX_TRY(upload(row_r0, r0h));
    CSX_TRY(upload(row_r1, r1h));
    CSX_TRY(upload(row_lev, levh));
    CSX_TRY(bad.alloc(1));
    CSX_HIP(hipMemsetAsync(bad, 0, sizeof(int), s));
    CSX_TRY(strip(U, true, true, row_r0, row_r1, bad, P->UTp, P->UTi, P->UTx, P->UTd));
    CSX_TRY(strip(L, false, true, row_r0, row_r1, bad, P->LTp, P->LTi, P->LTx, P->LTd));
    CSX_TRY(P->Fcp.alloc((size_t)n + 1));
    CSX_TRY(P->Fci.alloc((size_t)F->nnz));
    CSX_TRY(P->Fcx.alloc((size_t)F->nnz));
    CSX_HIP(hipMemcpyAsync(P->Fcp, F->p, ((size_t)n + 1) * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    if (F->nnz) CSX_HIP(hipMemcpyAsync(P->Fcx, F->x, (size_t)F->nnz * sizeof(double), hipMemcpyDeviceToDevice, s));
    if (n) hipLaunchKernelGGL(k_btf_tcols, dim3(grid_for(n)), dim3(256), 0, s, n, F->p, F->i, P->pinv, row_lev, P->Fci, bad);
    CSX_LAUNCH_CHECK();
    int hbad = 0;
    CSX_HIP(hipMemcpyAsync(&hbad, bad, sizeof(int), hipMemcpyDeviceToHost, s));
    CSX_HIP(hipStreamSynchronize(s));
    if (hbad) return CSX_EINVAL;
    for (const std::unique_ptr<BtfLarge> &G : P->large) {
        if (!G->put) CSX_TRY(tri_analyse_raw(&G->U, CSX_TRI_UT, &G->put));
        if (!G->plt) CSX_TRY(tri_analyse_raw(&G->L, CSX_TRI_LT, &G->plt));
    }
    CSX_HIP(hipStreamSynchronize(s));
    P->trans_ready = true;
    return CSX_OK;
}

static int btf_solve_trans(BtfPlan *P, const double *B, double *W, double *Bout, int32_t k) {
    hipStream_t s = ctx().stream;
    const unsigned tiles = (unsigned)((k + BTF_TILE - 1) / BTF_TILE);
    for (int32_t l = P->nlevels - 1; l >= 0; l--) {
        const int32_t a = P->small_ptr[l], e = P->small_ptr[l + 1];
        if (e > a) {
            const size_t lds = (size_t)P->small_rows[l] * BTF_TILE * sizeof(double);
            hipLaunchKernelGGL(k_btf_small<true>, dim3((unsigned)(e - a), tiles), dim3(64), lds, s, P->small + a, P->r, P->q,
                               P->pinv, P->Fcp, P->Fci, P->Fcx, P->UTp, P->UTi, P->UTx, P->UTd, P->LTp, P->LTi, P->LTx, P->LTd,
                               B, W, k);
            CSX_LAUNCH_CHECK();
        }
        for (int32_t li : P->large_of_level[l]) {
            BtfLarge *G = P->large[li].get();
            hipLaunchKernelGGL(k_btf_rows<true>, dim3(grid_for((int64_t)G->nr * k)), dim3(256), 0, s, G->r0, G->nr, P->q,
                               P->pinv, P->Fcp, P->Fci, P->Fcx, B, W, k);
            CSX_LAUNCH_CHECK();
            double *Wb = W + (int64_t)G->r0 * k;
            CSX_TRY(tri_solve_raw(G->put, Wb, k, false));
            CSX_TRY(tri_solve_raw(G->plt, Wb, k, false));
        }
    }
    if (P->n)
        hipLaunchKernelGGL(k_btf_out<true>, dim3(grid_for((int64_t)P->n * k)), dim3(256), 0, s, P->n, P->p, P->pinv, W, Bout,
                           k);
    CSX_LAUNCH_CHECK();
    return CSX_OK;
}

static bool is_perm(const int32_t *p, int32_t n) {
    std::vector<char> seen((size_t)n, 0);
    for (int32_t k = 0; k < n; k++) {
        if (p[k] < 0 || p[k] >= n || seen[p[k]]) return false;
        seen[p[k]] = 1;
    }
    return true;
}

static bool is_blocks(const int32_t *r, int32_t nb, int32_t n) {
    if (nb < 0 || r[0] != 0 || r[nb] != n) return false;
    for (int32_t b = 0; b < nb; b++)
        if (r[b + 1] <= r[b]) return false;
    return true;
}

// ---------------------------------------------------------------------------------------------- the refactor --

// per position: first and one-past-last row of its block, its block's level
static void block_rows(const BtfPlan *P, std::vector<int32_t> &r0h, std::vector<int32_t> &r1h, std::vector<int32_t> &levh) {
    r0h.resize((size_t)P->n);
    r1h.resize((size_t)P->n);
    levh.resize((size_t)P->n);
    for (int32_t b = 0; b < P->nb; b++)
        for (int32_t i = P->r_h[b]; i < P->r_h[b + 1]; i++) {
            r0h[i] = P->r_h[b];
            r1h[i] = P->r_h[b + 1];
            levh[i] = P->level_h[b];
        }
}

// program slot -> entry maps of a factor: its forward program built from an index-valued copy
static int program_maps(const Csc *M, bool upper, const int32_t *row_r0, const int32_t *row_r1, int *bad, DevBuf<int32_t> &xmap,
                        DevBuf<int32_t> &dmap) {
    csx_handle_t hI = 0;
    CSX_TRY(rf_index_copy(M, &hI));
    DevBuf<int32_t> Pp, Pi;
    DevBuf<double> Px, Pd;
    const int st = strip(csc(hI), upper, false, row_r0, row_r1, bad, Pp, Pi, Px, Pd);
    csx_free(hI);
    CSX_TRY(st);
    CSX_TRY(rf_index_map(Px, std::max<int64_t>(0, (int64_t)M->nnz - M->n), xmap));
    CSX_TRY(rf_index_map(Pd, M->n, dmap));
    CSX_HIP(hipStreamSynchronize(ctx().stream));
    return CSX_OK;
}

static int btf_refactor_prepare(BtfPlan *P, Csc *A, Csc *L, Csc *U, Csc *F) {
    const int32_t n = P->n;
    if (A->m != n || A->n != n) return CSX_EINVAL;
    hipStream_t s = ctx().stream;
    std::unique_ptr<BtfRefactor> B(new BtfRefactor());
    B->anz = A->nnz;
    CSX_TRY(rf_keep_pattern(A, B->p0, B->i0));
    std::vector<int32_t> p_h, q_h, pinv_h, pinv_new((size_t)n), blk((size_t)n);
    CSX_TRY(download_i32(p_h, P->p, (size_t)n));
    CSX_TRY(download_i32(q_h, P->q, (size_t)n));
    CSX_TRY(download_i32(pinv_h, P->pinv, (size_t)n));
    for (int32_t k = 0; k < n; k++) pinv_new[p_h[k]] = k;
    for (int32_t b = 0; b < P->nb; b++)
        for (int32_t i = P->r_h[b]; i < P->r_h[b + 1]; i++) blk[i] = b;
    // csx_btf_split's steps on an index-valued copy of A: D's and F's values say which entry of A each one is
    csx_handle_t hI = 0, hC = 0;
    CSX_TRY(rf_index_copy(A, &hI));
    int st = csx_permute(hI, pinv_new.data(), q_h.data(), 1, &hC);
    csx_free(hI);
    CSX_TRY(st);
    Csc Fi;
    st = split_device(csc(hC), blk, &B->Dq, &Fi);
    csx_free(hC);
    CSX_TRY(st);
    if (Fi.nnz != F->nnz || B->Dq.nnz + Fi.nnz != A->nnz) return CSX_EINVAL;
    CSX_TRY(rf_index_map(B->Dq.x, B->Dq.nnz, B->dmap));
    CSX_TRY(rf_index_map(Fi.x, Fi.nnz, B->fmap));
    // the forward programs' slots, and F' (cs_gaxpy's row order) of F's entries
    std::vector<int32_t> r0h, r1h, levh;
    block_rows(P, r0h, r1h, levh);
    DevBuf<int32_t> row_r0, row_r1;
    DevBuf<int> bad;
    CSX_TRY(upload(row_r0, r0h));
    CSX_TRY(upload(row_r1, r1h));
    CSX_TRY(bad.alloc(1));
    CSX_HIP(hipMemsetAsync(bad, 0, sizeof(int), s));
    CSX_TRY(program_maps(L, false, row_r0, row_r1, bad, B->lxmap, B->ldmap));
    CSX_TRY(program_maps(U, true, row_r0, row_r1, bad, B->uxmap, B->udmap));
    csx_handle_t hFi = 0;
    CSX_TRY(rf_index_copy(F, &hFi));
    Csc Ft;
    st = transpose_device(csc(hFi), true, &Ft);
    csx_free(hFi);
    CSX_TRY(st);
    if (Ft.nnz != P->Ft.nnz) return CSX_EINVAL;
    CSX_TRY(rf_index_map(Ft.x, Ft.nnz, B->ftmap));
    int hbad = 0;
    CSX_HIP(hipMemcpyAsync(&hbad, bad, sizeof(int), hipMemcpyDeviceToHost, s));
    CSX_HIP(hipStreamSynchronize(s));
    if (hbad) return CSX_EINVAL;
    // the schedule: a group is a diagonal block
    CSX_TRY(refactor_build(&B->Dq, pinv_h.data(), L, U, blk, &B->R));
    CSX_TRY(download_i32(B->Lp, L->p, (size_t)n + 1));
    CSX_TRY(download_i32(B->Up, U->p, (size_t)n + 1));
    CSX_TRY(B->Fx.alloc((size_t)F->nnz));
    CSX_TRY(B->Lx.alloc((size_t)L->nnz));
    CSX_TRY(B->Ux.alloc((size_t)U->nnz));
    CSX_TRY(B->flag.alloc(1));
    CSX_HIP(hipStreamSynchronize(s));
    P->rf = std::move(B);
    return CSX_OK;
}

}  // namespace csx

using namespace csx;

extern "C" int csx_btf_split(csx_handle_t hA, const int32_t *p, const int32_t *q, const int32_t *r, int32_t nb, int32_t *p_out,
                             int32_t *q_out, int32_t *r_out, int32_t *level, int32_t *nlevels, csx_handle_t *hD,
                             csx_handle_t *hF) {
    CSX_TRY(require_ready());
    Csc *A = csc(hA);
    if (!A || !A->x || A->m != A->n || !p || !q || !r || !p_out || !q_out || !r_out || !level || !nlevels || !hD || !hF)
        return CSX_EINVAL;
    const int32_t n = A->n;
    if (!is_perm(p, n) || !is_perm(q, n) || !is_blocks(r, nb, n)) return CSX_EINVAL;
    hipStream_t s = ctx().stream;
    std::vector<int32_t> Ap((size_t)n + 1), Ai((size_t)A->nnz);
    CSX_HIP(hipMemcpyAsync(Ap.data(), A->p, ((size_t)n + 1) * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (A->nnz) CSX_HIP(hipMemcpyAsync(Ai.data(), A->i, (size_t)A->nnz * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    CSX_HIP(hipStreamSynchronize(s));
    // block of every row and column of A in the given order
    std::vector<int32_t> rowblk((size_t)n), colblk((size_t)n);
    for (int32_t b = 0; b < nb; b++)
        for (int32_t k = r[b]; k < r[b + 1]; k++) {
            rowblk[p[k]] = b;
            colblk[q[k]] = b;
        }
    // edges block(row) -> block(column) of the entries outside the diagonal blocks, grouped by the row's block
    std::vector<int32_t> eptr((size_t)nb + 1, 0);
    for (int32_t j = 0; j < n; j++)
        for (int32_t t = Ap[j]; t < Ap[j + 1]; t++) {
            const int32_t bi = rowblk[Ai[t]], bj = colblk[j];
            if (bj < bi) return CSX_EINVAL;   // not block upper triangular in this order
            if (bj != bi) eptr[bi + 1]++;
        }
    for (int32_t b = 0; b < nb; b++) eptr[b + 1] += eptr[b];
    std::vector<int32_t> edst((size_t)eptr[nb]), fill(eptr.begin(), eptr.end() - 1);
    for (int32_t j = 0; j < n; j++)
        for (int32_t t = Ap[j]; t < Ap[j + 1]; t++) {
            const int32_t bi = rowblk[Ai[t]], bj = colblk[j];
            if (bj != bi) edst[fill[bi]++] = bj;
        }
    // level: 0 without entries outside the block, else 1 + the largest level reached; edges point to later blocks
    std::vector<int32_t> lev((size_t)nb, 0);
    int32_t L = nb ? 1 : 0;
    for (int32_t b = nb - 1; b >= 0; b--) {
        int32_t v = 0;
        for (int32_t t = eptr[b]; t < eptr[b + 1]; t++) v = std::max(v, lev[edst[t]] + 1);
        lev[b] = v;
        L = std::max(L, v + 1);
    }
    // blocks by level, highest first (a block's F reaches lower levels only: later blocks), dmperm's order inside a level
    std::vector<int32_t> order((size_t)nb);
    for (int32_t b = 0; b < nb; b++) order[b] = b;
    std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) { return lev[x] > lev[y]; });
    std::vector<int32_t> pinv_new((size_t)n), blk_new((size_t)n);
    int32_t k = 0;
    r_out[0] = 0;
    for (int32_t nbk = 0; nbk < nb; nbk++) {
        const int32_t b = order[nbk];
        for (int32_t t = r[b]; t < r[b + 1]; t++, k++) {
            p_out[k] = p[t];
            q_out[k] = q[t];
            pinv_new[p[t]] = k;
            blk_new[k] = nbk;
        }
        r_out[nbk + 1] = k;
        level[nbk] = lev[b];
    }
    *nlevels = L;
    csx_handle_t hC = 0;
    CSX_TRY(csx_permute(hA, pinv_new.data(), q_out, 1, &hC));
    std::unique_ptr<Csc> D(new Csc()), F(new Csc());
    const int st = split_device(csc(hC), blk_new, D.get(), F.get());
    csx_free(hC);
    CSX_TRY(st);
    *hD = put(K_CSC, D.release());
    *hF = put(K_CSC, F.release());
    return CSX_OK;
}

extern "C" int csx_btf_plan(csx_handle_t hL, csx_handle_t hU, csx_handle_t hF, const int32_t *pinv, const int32_t *p,
                            const int32_t *q, const int32_t *r, const int32_t *level, int32_t nb, csx_handle_t *out) {
    CSX_TRY(require_ready());
    Csc *L = csc(hL), *U = csc(hU), *F = csc(hF);
    if (!L || !U || !F || !L->x || !U->x || !F->x || !pinv || !p || !q || !r || !level || !out) return CSX_EINVAL;
    const int32_t n = L->n;
    if (L->m != n || U->m != n || U->n != n || F->m != n || F->n != n) return CSX_EINVAL;
    if (!is_perm(pinv, n) || !is_perm(p, n) || !is_perm(q, n) || !is_blocks(r, nb, n)) return CSX_EINVAL;
    int32_t nlev = 0;
    for (int32_t b = 0; b < nb; b++) {
        if (level[b] < 0 || level[b] >= nb || (b && level[b] > level[b - 1])) return CSX_EINVAL;
        nlev = std::max(nlev, level[b] + 1);
    }
    // pivots stay inside their block
    for (int32_t b = 0; b < nb; b++)
        for (int32_t i = r[b]; i < r[b + 1]; i++)
            if (pinv[i] < r[b] || pinv[i] >= r[b + 1]) return CSX_EINVAL;
    hipStream_t s = ctx().stream;
    std::unique_ptr<BtfPlan> P(new BtfPlan());
    P->n = n;
    P->nb = nb;
    P->nlevels = nlev;
    std::vector<int32_t> r0h((size_t)n), r1h((size_t)n), levh((size_t)n);
    for (int32_t b = 0; b < nb; b++) {
        P->max_block = std::max(P->max_block, r[b + 1] - r[b]);
        for (int32_t i = r[b]; i < r[b + 1]; i++) {
            r0h[i] = r[b];
            r1h[i] = r[b + 1];
            levh[i] = level[b];
        }
    }
    // blocks grouped by level, level 0 first
    std::vector<int32_t> small_h;
    P->small_ptr.assign(1, 0);
    P->small_rows.assign((size_t)nlev, 0);
    P->large_of_level.assign((size_t)nlev, {});
    // levels fall along the block order (checked above): level l is one run of blocks, found walking from the end
    int32_t run_end = nb;
    for (int32_t l = 0; l < nlev; l++) {
        int32_t run_begin = run_end;
        while (run_begin > 0 && level[run_begin - 1] == l) run_begin--;
        for (int32_t b = run_begin; b < run_end; b++) {
            const int32_t nr = r[b + 1] - r[b];
            if (nr <= BTF_SMALL) {
                small_h.push_back(b);
                P->small_rows[l] = std::max(P->small_rows[l], nr);
            } else {
                P->large_of_level[l].push_back((int32_t)P->large.size());
                P->large.emplace_back(new BtfLarge());
                P->large.back()->r0 = r[b];
                P->large.back()->nr = nr;
            }
        }
        P->small_ptr.push_back((int32_t)small_h.size());
        run_end = run_begin;
    }
    DevBuf<int32_t> row_r0, row_r1, row_lev;
    DevBuf<int> bad;
    CSX_TRY(upload(row_r0, r0h));
    CSX_TRY(upload(row_r1, r1h));
    CSX_TRY(upload(row_lev, levh));
    CSX_TRY(bad.alloc(1));
    CSX_HIP(hipMemsetAsync(bad, 0, sizeof(int), s));
    CSX_TRY(upload(P->p, p, (size_t)n));
    CSX_TRY(upload(P->q, q, (size_t)n));
    CSX_TRY(upload(P->pinv, pinv, (size_t)n));
    CSX_TRY(upload(P->r, r, (size_t)nb + 1));
    CSX_TRY(upload(P->small, small_h));
    CSX_TRY(strip(L, false, false, row_r0, row_r1, bad, P->Lp, P->Li, P->Lx, P->Ld));
    CSX_TRY(strip(U, true, false, row_r0, row_r1, bad, P->Up, P->Ui, P->Ux, P->Ud));
    CSX_TRY(transpose_device(F, true, &P->Ft));
    if (n) hipLaunchKernelGGL(k_btf_check_f, dim3(grid_for(n)), dim3(256), 0, s, n, P->Ft.p, P->Ft.i, row_r1, row_lev, bad);
    int hbad = 0;
    CSX_HIP(hipMemcpyAsync(&hbad, bad, sizeof(int), hipMemcpyDeviceToHost, s));
    CSX_HIP(hipStreamSynchronize(s));
    if (hbad) return CSX_EINVAL;
    P->lnz = L->nnz;
    P->unz = U->nnz;
    P->fnz = F->nnz;
    P->hL = hL;
    P->hU = hU;
    P->hF = hF;
    P->r_h.assign(r, r + nb + 1);
    P->level_h.assign(level, level + nb);
    for (const std::unique_ptr<BtfLarge> &G : P->large) {
        CSX_TRY(block_factor(L, G->r0, G->nr, &G->L));
        CSX_TRY(block_factor(U, G->r0, G->nr, &G->U));
        CSX_TRY(tri_analyse_raw(&G->L, CSX_TRI_L, &G->pl));
        CSX_TRY(tri_analyse_raw(&G->U, CSX_TRI_U, &G->pu));
    }
    CSX_HIP(hipStreamSynchronize(s));
    *out = put(K_BTFPLAN, P.release());
    return CSX_OK;
}

extern "C" int csx_btf_solve(csx_handle_t h, csx_handle_t hB, csx_handle_t hW, int32_t nrhs) {
    CSX_TRY(require_ready());
    BtfPlan *P = (BtfPlan *)get(h, K_BTFPLAN);
    Vec *B = vec(hB), *W = vec(hW);
    if (!P || !B || !W || B == W || nrhs < 1) return CSX_EINVAL;
    const int64_t need = (int64_t)P->n * nrhs;
    if (B->len < need || W->len < need) return CSX_EINVAL;
    return btf_solve(P, (const double *)B->d, (double *)W->d, (double *)B->d, nrhs);
}

extern "C" int csx_btf_solve_trans(csx_handle_t h, csx_handle_t hB, csx_handle_t hW, int32_t nrhs) {
    CSX_TRY(require_ready());
    BtfPlan *P = (BtfPlan *)get(h, K_BTFPLAN);
    Vec *B = vec(hB), *W = vec(hW);
    if (!P || !B || !W || B == W || nrhs < 1) return CSX_EINVAL;
    const int64_t need = (int64_t)P->n * nrhs;
    if (B->len < need || W->len < need) return CSX_EINVAL;
    CSX_TRY(btf_trans_plan(P));
    return btf_solve_trans(P, (const double *)B->d, (double *)W->d, (double *)B->d, nrhs);
}

// the cuts and strides of the btf solve and of the refactor kernel, for the tests (no device needed)
extern "C" int csx_btf_limits(int32_t *out) {
    if (!out) return CSX_EINVAL;
    const int32_t v[6] = {BTF_SMALL, RF_MAX, RF_WAVES, BTF_TILE, TERM_CHUNK, TERM_GROUP};
    for (int k = 0; k < 6; k++) out[k] = v[k];
    return CSX_OK;
}

extern "C" int csx_btf_info(csx_handle_t h, int64_t *info) {
    CSX_TRY(require_ready());
    BtfPlan *P = (BtfPlan *)get(h, K_BTFPLAN);
    if (!P || !info) return CSX_EINVAL;
    int64_t launches = 1;
    for (int32_t l = 0; l < P->nlevels; l++) launches += (P->small_ptr[l + 1] > P->small_ptr[l]) ? 1 : 0;
    info[0] = P->nb;
    info[1] = P->nlevels;
    info[2] = P->max_block;
    info[3] = P->lnz;
    info[4] = P->unz;
    info[5] = P->fnz;
    info[6] = (int64_t)P->large.size();
    info[7] = launches;   // the solve's own launches; every large block adds one plus those of its two triangular plans
    return CSX_OK;
}

extern "C" int csx_btf_refactor(csx_handle_t h, csx_handle_t hA, csx_handle_t hA2, csx_handle_t hD, int *ok, double *ratio,
                                int64_t *cols) {
    CSX_TRY(require_ready());
    BtfPlan *P = (BtfPlan *)get(h, K_BTFPLAN);
    if (!P || !ok || !ratio) return CSX_EINVAL;
    Csc *L = csc(P->hL), *U = csc(P->hU), *F = csc(P->hF);
    if (!L || !U || !F || !L->x || !U->x || !F->x || L->n != P->n || U->n != P->n || F->n != P->n || L->nnz != P->lnz ||
        U->nnz != P->unz || F->nnz != P->fnz)
        return CSX_EINVAL;
    Csc *D = hD ? csc(hD) : nullptr;
    if (hD && (!D || !D->x || D->n != P->n)) return CSX_EINVAL;
    if (!P->rf) {
        Csc *A = csc(hA);
        if (!A) return CSX_EINVAL;
        CSX_TRY(btf_refactor_prepare(P, A, L, U, F));
    }
    BtfRefactor *B = P->rf.get();
    if (D && D->nnz != B->Dq.nnz) return CSX_EINVAL;
    const double *x2 = nullptr;
    CSX_TRY(rf_values(hA2, P->n, P->n, B->anz, B->p0, B->i0, B->flag, &x2));
    if (!x2) {
        *ok = -1;   // another pattern: nothing changes
        return CSX_OK;
    }
    hipStream_t s = ctx().stream;
    CSX_TRY(rf_gather(B->Dq.nnz, B->dmap, x2, B->Dq.x));
    CSX_TRY(rf_gather(F->nnz, B->fmap, x2, B->Fx));
    CSX_TRY(refactor_run(B->R, &B->Dq, B->Dq.x, L, U, B->Lx, B->Ux, ok, ratio));
    refactor_counts(B->R, cols);
    if (!*ok) return CSX_OK;
    // the large blocks' own factors and triangular plans from the new values, into temporaries: an error here leaves
    // everything as it was
    const int64_t nlarge = (int64_t)P->large.size();
    std::vector<std::unique_ptr<Csc>> nL((size_t)nlarge), nU((size_t)nlarge);
    std::vector<TriPlan *> npl((size_t)nlarge, nullptr), npu((size_t)nlarge, nullptr);
    struct PlansGuard {   // frees the temporaries' plans unless they were committed
        std::vector<TriPlan *> &a, &b;
        ~PlansGuard() {
            for (TriPlan *t : a) destroy(t);
            for (TriPlan *t : b) destroy(t);
        }
    } guard{npl, npu};
    if (nlarge) {
        Csc vL, vU;   // views of the new values on the factors' patterns (arrays not owned)
        vL.owns = vU.owns = false;
        vL.m = vL.n = vU.m = vU.n = P->n;
        vL.nnz = L->nnz;
        vU.nnz = U->nnz;
        vL.p = L->p;
        vL.i = L->i;
        vL.x = B->Lx;
        vU.p = U->p;
        vU.i = U->i;
        vU.x = B->Ux;
        for (int64_t g = 0; g < nlarge; g++) {
            const BtfLarge *G = P->large[g].get();
            nL[g].reset(new Csc());
            nU[g].reset(new Csc());
            CSX_TRY(block_factor(&vL, G->r0, G->nr, nL[g].get()));
            CSX_TRY(block_factor(&vU, G->r0, G->nr, nU[g].get()));
            CSX_TRY(tri_analyse_raw(nL[g].get(), CSX_TRI_L, &npl[g]));
            CSX_TRY(tri_analyse_raw(nU[g].get(), CSX_TRI_U, &npu[g]));
        }
    }
    // commit: the factors, F and D, then everything the solves read (copies and gathers on the stream)
    const auto d2d = [&](double *dst, const double *src, int64_t cnt) {
        return cnt > 0 ? hipMemcpyAsync(dst, src, (size_t)cnt * sizeof(double), hipMemcpyDeviceToDevice, s) : hipSuccess;
    };
    CSX_HIP(d2d(L->x, B->Lx, L->nnz));
    CSX_HIP(d2d(U->x, B->Ux, U->nnz));
    CSX_HIP(d2d(F->x, B->Fx, F->nnz));
    if (D) CSX_HIP(d2d(D->x, B->Dq.x, D->nnz));
    const int32_t n = P->n;
    CSX_TRY(rf_gather(std::max<int64_t>(0, (int64_t)P->lnz - n), B->lxmap, L->x, P->Lx));
    CSX_TRY(rf_gather(n, B->ldmap, L->x, P->Ld));
    CSX_TRY(rf_gather(std::max<int64_t>(0, (int64_t)P->unz - n), B->uxmap, U->x, P->Ux));
    CSX_TRY(rf_gather(n, B->udmap, U->x, P->Ud));
    CSX_TRY(rf_gather(P->Ft.nnz, B->ftmap, F->x, P->Ft.x));
    for (int64_t g = 0; g < nlarge; g++) {
        BtfLarge *G = P->large[g].get();
        // (the same patterns: the new arrays take the old ones' place, the old ones go with the temporaries)
        std::swap(G->L.p, nL[g]->p);
        std::swap(G->L.i, nL[g]->i);
        std::swap(G->L.x, nL[g]->x);
        std::swap(G->U.p, nU[g]->p);
        std::swap(G->U.i, nU[g]->i);
        std::swap(G->U.x, nU[g]->x);
        for (TriPlan **T : {&G->pl, &G->pu, &G->put, &G->plt}) {
            destroy(*T);
            *T = nullptr;
        }
        G->pl = npl[g];
        G->pu = npu[g];
        npl[g] = npu[g] = nullptr;
    }
    P->trans_ready = false;   // the transposed programs are made again, from the new values, by the next transposed solve
    for (Csc *M : {L, U, F, D})
        if (M) {
            M->rows.reset();
            M->tiled.reset();
        }
    CSX_HIP(hipStreamSynchronize(s));
    return CSX_OK;
}

extern "C" int csx_btf_refactor_dx(csx_handle_t h, double *Dx) {
    CSX_TRY(require_ready());
    BtfPlan *P = (BtfPlan *)get(h, K_BTFPLAN);
    if (!P || !P->rf || !Dx) return CSX_EINVAL;
    hipStream_t s = ctx().stream;
    if (P->rf->Dq.nnz)
        CSX_HIP(hipMemcpyAsync(Dx, P->rf->Dq.x, (size_t)P->rf->Dq.nnz * sizeof(double), hipMemcpyDeviceToHost, s));
    CSX_HIP(hipStreamSynchronize(s));
    return CSX_OK;
}
