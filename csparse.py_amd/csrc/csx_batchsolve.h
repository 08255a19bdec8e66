// The two sweeps of a batched solve in the reference's operation order, over the height levels of a LevelFactor: what
// csx_slu_batch.hip, csx_ldl_batch.hip and csx_hqr_batch.hip share of a solve.  The kernels take raw
// pointers -- a pattern (Lp, Li), its row view (row_ptr, row_col, row_pos), a member-major value plane (stride lnz) -- and know
// nothing of the factorisation the plane came from.
//   k_slb_level / k_slb_run <rows or dots, division>   a wide level is one launch of a thread per (row, member, right-hand side),
//                    a run of narrow levels one launch of a workgroup per member with a wave per (row, right-hand side) -- F's
//                    schedule, so len(schedule) launches a sweep for any B
//   batch_sweep / batch_sweep_upper   one sweep of a lower / an upper factor, launched (batch_sweep_as); both are templates on
//                    what they sweep, so a translation unit holds the kernels of its own sweeps and no others
//   k_batch_permute  the solve's permutations, gather or scatter; with the flags it fills a failed member's columns with NaN
// The division of a row has three modes.  Two are the runtime argument `div` of the instantiations <ROWS, false>: none (unit L),
// or AFTER the chain by the plane's own diagonal val[Lp[j]] (Ut).  The third is the template parameter PRE: BEFORE the chain by
// dd[member n + j], the D step of an L D L' solve fused into the backward sweep: s = x_j / d_j, then the chain, then the store.
// The backward chain of row j reads only x_i with i > j, all finished (divided, swept) in earlier levels, and x_j / d_j is rounded
// once before the first subtraction: the bits of "X[j, :] /= d[j] for all j, then cs_ltsolve".  The division must NOT move to
// the end of the forward sweep instead: a later row k > j of cs_lsolve reads x_j, and it must read the undivided one.
// Two more template parameters, independent of the gather kind, serve an UPPER factor whose diagonal is the last stored entry of
// its column (the R of csx_hqr_batch.hip).  LAST: the diagonal is val[Lp[j + 1] - 1], and a dot runs over the
// entries BEFORE it.  ASC: a run walks its levels ascending; the default is the gather kind's own direction (rows ascending,
// dots descending), and R turns both round: the rows of cs_usolve from the top level down, the dots of cs_utsolve from the
// leaves up.  A row view always ends with the diagonal, whichever end of the row that is: for R the columns of a row descend.
// The defaults are the instantiations the LU and LDL' batches launch, with the code they always had.
#pragma once
#include "csx_levelwalk.h"

#pragma clang fp contract(off)

namespace csx {

constexpr int SLB_THREADS = 256;   // threads of a workgroup of the solve kernels: the (row, column) pairs a wide level's workgroup takes
constexpr int SLB_FETCH = 4;       // terms of a chain that a thread of a wide level fetches together, then applies one after the other
constexpr int SLB_RUN_WAVES = 16;  // waves of a walker's workgroup: (row, right-hand side) pairs it takes at a time, a wave each
constexpr int SLB_RUN_FETCH = 64;  // terms of a chain that a walker's wave fetches together, a lane each

// X is n x K row-major, K = B r; column c belongs to member c / r.  val: the member-major values of the factor the sweep reads
// (stride lnz); div: divide by the diagonal val[Lp[j]] (Ut) or not (unit L); PRE: d is the member's pivots, x_j / d[j] first.

// x_j = ((x_j - v1 x_k1) - v2 x_k2) - ... over row j's entries off the diagonal in the row view's order (k ascending for a lower
// factor, descending for an upper one), then / d_j
template <bool PRE, bool LAST = false>
__device__ __forceinline__ void slb_row(int32_t j, int64_t c, int64_t K, const int32_t *__restrict__ Lp,
                                        const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ row_col,
                                        const int32_t *__restrict__ row_pos, const double *__restrict__ v, bool div,
                                        const double *__restrict__ d, double *X) {
    double s = X[(int64_t)j * K + c];
    if (PRE) s = s / d[j];
    const int32_t qe = row_ptr[j + 1] - 1;   // the row view ends with the diagonal
    for (int32_t q0 = row_ptr[j]; q0 < qe; q0 += SLB_FETCH) {
        double a_[SLB_FETCH], x_[SLB_FETCH];
#pragma unroll
        for (int u = 0; u < SLB_FETCH; u++) {
            const int32_t q = q0 + u < qe ? q0 + u : q0;
            a_[u] = v[row_pos[q]];
            x_[u] = X[(int64_t)row_col[q] * K + c];
        }
#pragma unroll
        for (int u = 0; u < SLB_FETCH; u++)
            if (q0 + u < qe) {
                const double t = a_[u] * x_[u];
                s = s - t;
            }
    }
    if (div) s = s / v[LAST ? Lp[j + 1] - 1 : Lp[j]];
    X[(int64_t)j * K + c] = s;
}

// x_j = ((x_j - v1 x_i1) - v2 x_i2) - ... over column j's stored entries off the diagonal (below it and after it in storage, or
// LAST: above it and before it) in storage order, then / d_j
template <bool PRE, bool LAST = false>
__device__ __forceinline__ void slb_dot(int32_t j, int64_t c, int64_t K, const int32_t *__restrict__ Lp, const int32_t *__restrict__ Li,
                                        const double *__restrict__ v, bool div, const double *__restrict__ d, double *X) {
    double s = X[(int64_t)j * K + c];
    if (PRE) s = s / d[j];
    const int32_t pe = LAST ? Lp[j + 1] - 1 : Lp[j + 1];
    for (int32_t p0 = LAST ? Lp[j] : Lp[j] + 1; p0 < pe; p0 += SLB_FETCH) {
        double a_[SLB_FETCH], x_[SLB_FETCH];
#pragma unroll
        for (int u = 0; u < SLB_FETCH; u++) {
            const int32_t p = p0 + u < pe ? p0 + u : p0;
            a_[u] = v[p];
            x_[u] = X[(int64_t)Li[p] * K + c];
        }
#pragma unroll
        for (int u = 0; u < SLB_FETCH; u++)
            if (p0 + u < pe) {
                const double t = a_[u] * x_[u];
                s = s - t;
            }
    }
    if (div) s = s / v[LAST ? Lp[j + 1] - 1 : Lp[j]];
    X[(int64_t)j * K + c] = s;
}

// a wide level: one thread per (row of the level, column of X), the columns fastest.  dd, dn: the pivots of all members and
// their stride (PRE only; they come last so that the other instantiations read their arguments where they always did)
template <bool ROWS, bool PRE, bool LAST = false>
__global__ __launch_bounds__(SLB_THREADS) void k_slb_level(const int32_t *__restrict__ cols, int32_t count, int64_t K, int32_t r,
                                                           int64_t lnz, const int32_t *__restrict__ Lp, const int32_t *__restrict__ Li,
                                                           const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ row_col,
                                                           const int32_t *__restrict__ row_pos, const double *__restrict__ val, int div,
                                                           double *X, const double *__restrict__ dd, int64_t dn) {
    const int64_t t = (int64_t)blockIdx.x * SLB_THREADS + threadIdx.x;
    if (t >= (int64_t)count * K) return;
    const int64_t i = t / K, c = t - i * K;
    const double *v = val + (c / r) * lnz;
    const double *d = PRE ? dd + (c / r) * dn : nullptr;
    if (ROWS) slb_row<PRE, LAST>(cols[i], c, K, Lp, row_ptr, row_col, row_pos, v, div != 0, d, X);
    else slb_dot<PRE, LAST>(cols[i], c, K, Lp, Li, v, div != 0, d, X);
}

// One WAVE's (row, column of X) of a narrow level, where a chain is long (the top of a nested-dissection tree) and there are few
// of them: the 64 lanes fetch 64 terms of the chain together and each forms one product -- a product is rounded on its own,
// whoever forms it -- then the products are applied one after the other in the chain's order, every lane keeping the same sum.
template <bool ROWS, bool PRE, bool LAST = false>
__device__ __forceinline__ void slb_wave_chain(int32_t j, int64_t c, int64_t K, int lane, const int32_t *__restrict__ Lp,
                                               const int32_t *__restrict__ Li, const int32_t *__restrict__ row_ptr,
                                               const int32_t *__restrict__ row_col, const int32_t *__restrict__ row_pos,
                                               const double *__restrict__ v, bool div, const double *__restrict__ d, double *X) {
    const int32_t q0 = __builtin_amdgcn_readfirstlane(ROWS ? row_ptr[j] : LAST ? Lp[j] : Lp[j] + 1);
    const int32_t qe = __builtin_amdgcn_readfirstlane(ROWS || LAST ? (ROWS ? row_ptr : Lp)[j + 1] - 1 : Lp[j + 1]);
    double s = X[(int64_t)j * K + c];
    if (PRE) s = s / d[j];
    for (int32_t b = q0; b < qe; b += 64) {
        const int32_t q = b + lane;
        double t = 0.0;
        if (q < qe) {
            const double a = ROWS ? v[row_pos[q]] : v[q];
            const int32_t k = ROWS ? row_col[q] : Li[q];
            t = a * X[(int64_t)k * K + c];
        }
        const int32_t terms = qe - b < 64 ? qe - b : 64;
        for (int32_t u = 0; u < terms; u++) {
            const double tu = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(t), u),
                                               __builtin_amdgcn_readlane(__double2loint(t), u));
            s = s - tu;
        }
    }
    if (div) s = s / v[LAST ? Lp[j + 1] - 1 : Lp[j]];
    if (lane == 0) X[(int64_t)j * K + c] = s;
}

// a run of narrow levels: the workgroup of member blockIdx.x walks [l0, l1) -- ASC: ascending (the rows of a lower factor, the
// dots of an upper one), else descending --
// with a barrier per level; its SLB_RUN_WAVES waves take the (row of the level, right-hand side) pairs one each at a time
// (slb_wave_chain).  The trip counts are the level pointers and r, the same for every wave, so every wave reaches every barrier.
template <bool ROWS, bool PRE, bool LAST = false, bool ASC = ROWS>
__global__ __launch_bounds__(64 * SLB_RUN_WAVES) void k_slb_run(const int32_t *__restrict__ cols, const int32_t *__restrict__ level_ptr,
                                                         int32_t l0, int32_t l1, int64_t K, int32_t r, int64_t lnz,
                                                         const int32_t *__restrict__ Lp, const int32_t *__restrict__ Li,
                                                         const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ row_col,
                                                         const int32_t *__restrict__ row_pos, const double *__restrict__ val, int div,
                                                         double *X, const double *__restrict__ dd, int64_t dn) {
    const int64_t m = blockIdx.x;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const double *v = val + m * lnz;
    const double *d = PRE ? dd + m * dn : nullptr;
    for (int32_t s = 0; s < l1 - l0; s++) {
        const int32_t l = ASC ? l0 + s : l1 - 1 - s;
        const int32_t b = level_ptr[l], cnt = level_ptr[l + 1] - b;
        for (int32_t t = w; t < cnt * r; t += SLB_RUN_WAVES) {
            const int32_t i = t / r;
            const int32_t j = __builtin_amdgcn_readfirstlane(cols[b + i]);
            slb_wave_chain<ROWS, PRE, LAST>(j, m * r + (t - i * r), K, lane, Lp, Li, row_ptr, row_col, row_pos, v, div != 0, d, X);
        }
        __syncthreads();
    }
}

// dst[i, :] = src[p[i], :] (scatter 0) or dst[p[i], :] = src[i, :] (scatter 1) over `rows` rows, p null: the identity; with flags,
// NaN in the columns of a member that broke down (its flag words are 3 apart in every batch)
static __global__ __launch_bounds__(256) void k_batch_permute(int64_t rows, int64_t K, int32_t r, const int32_t *__restrict__ p, int scatter,
                                                              const int *__restrict__ flags, const double *__restrict__ src,
                                                              double *__restrict__ dst) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= rows * K) return;
    const int64_t i = t / K, c = t - i * K, pi = p ? (int64_t)p[i] : i;
    const bool ok = !flags || flags[3 * (c / r)] == WALK_NONE;
    const double v = ok ? src[(scatter ? i : pi) * K + c] : __longlong_as_double(0x7ff8000000000000ll);
    dst[(scatter ? pi : i) * K + c] = v;
}

// ---- host -------------------------------------------------------------------------------------------------------------------

// The pattern a sweep reads (all device pointers, borrowed) and the members on it
struct BatchPattern {
    const int32_t *Lp, *Li, *row_ptr, *row_col, *row_pos;
    int64_t n, lnz;
    int32_t B;
};

// One sweep over F's schedule on the context's stream, as the instantiation <ROWS, PRE, LAST> walked ascending (ASC) or
// descending: len(F->schedule) launches.  The arguments are batch_sweep's.
template <bool ROWS, bool PRE, bool LAST, bool ASC>
int batch_sweep_as(const LevelFactor *F, const BatchPattern &P, const double *val, bool div, const double *dd, int32_t r, double *X) {
    hipStream_t s = ctx().stream;
    const std::vector<int32_t> &lp = F->level_ptr_h;
    const int64_t K = (int64_t)P.B * r;
    const size_t nl = F->schedule.size();
    for (size_t t = 0; t < nl; t++) {
        const LevelLaunch &Ln = F->schedule[ASC ? t : nl - 1 - t];
        if (Ln.wide) {
            const int32_t cnt = lp[(size_t)Ln.l0 + 1] - lp[(size_t)Ln.l0];
            const unsigned blocks = (unsigned)(((int64_t)cnt * K + SLB_THREADS - 1) / SLB_THREADS);
            const int32_t *cols = F->level_cols.get() + lp[(size_t)Ln.l0];
            hipLaunchKernelGGL((k_slb_level<ROWS, PRE, LAST>), dim3(blocks), dim3(SLB_THREADS), 0, s, cols, cnt, K, r, P.lnz, P.Lp, P.Li,
                               P.row_ptr, P.row_col, P.row_pos, val, div ? 1 : 0, X, dd, P.n);
        } else {
            hipLaunchKernelGGL((k_slb_run<ROWS, PRE, LAST, ASC>), dim3((unsigned)P.B), dim3(64 * SLB_RUN_WAVES), 0, s,
                               F->level_cols.get(), F->level_ptr.get(), Ln.l0, Ln.l1, K, r, P.lnz, P.Lp, P.Li, P.row_ptr, P.row_col,
                               P.row_pos, val, div ? 1 : 0, X, dd, P.n);
        }
    }
    CSX_LAUNCH_CHECK();
    return CSX_OK;
}

// A sweep of a LOWER factor with the diagonal first in its column: ROWS: the rows ascending (cs_lsolve), else the dots descending
// (cs_ltsolve) of the value plane val, r right-hand sides a member; div: / val[Lp[j]] after the chain; PRE (dots only): dd is the
// members' pivots (stride P.n) to divide by BEFORE the chain (see the head of this file), and there is no other division.
// (A template, so that a file holds only the kernels of the sweeps it calls.)
template <bool ROWS, bool PRE = false>
int batch_sweep(const LevelFactor *F, const BatchPattern &P, const double *val, bool div, const double *dd, int32_t r, double *X) {
    static_assert(!(ROWS && PRE), "the division before the chain belongs to the backward sweep");
    if ((dd && (ROWS || div)) || PRE != (dd != nullptr)) return CSX_EINVAL;
    return batch_sweep_as<ROWS, PRE, false, ROWS>(F, P, val, div, dd, r, X);
}

// A sweep of an UPPER factor with the diagonal last in its column, always divided by it: ROWS: the rows from the top level down
// (cs_usolve: P's row view holds row i's columns descending, the diagonal last), else the dots from the leaves up (cs_utsolve).
template <bool ROWS>
int batch_sweep_upper(const LevelFactor *F, const BatchPattern &P, const double *val, int32_t r, double *X) {
    return batch_sweep_as<ROWS, false, true, !ROWS>(F, P, val, true, nullptr, r, X);
}

// whether one launch takes K = B r columns of an n-row block (a walker counts rows x r in 32 bits)
inline bool batch_solve_fits(int64_t n, int64_t K) { return K <= 0x7fffffffll / WALK_WAVES && n * K <= 0x7fffffffll * SLB_THREADS; }

// the device block of at least `need` doubles behind a vector handle, or null
inline double *batch_block(csx_handle_t h, int64_t need) {
    Vec *v = vec(h);
    return v && v->d && v->len >= need ? (double *)v->d : nullptr;
}

}  // namespace csx
