// sparseinv: Z = inv(L L') on the pattern of the Cholesky factor L, by the Takahashi recurrence.
//
// The contract (L: diagonal first and positive, rows ascending; d = L(j,j); S_j = the rows of column j below the diagonal in
// storage order; Zs(a, b) = the stored Z(max(a,b), min(a,b))):
//     for j = n-1 .. 0:
//         for i in S_j:   s = 0;  for k in S_j in storage order: s = s + L(k,j) * Zs(i,k);   Z(i,j) = (-s) / d
//         s = 0;  for k in S_j in storage order: s = s + L(k,j) * Z(k,j);                    Z(j,j) = (1/d - s) / d
// with every product and every sum rounded on its own.  Z.x is byte-equal to that loop.
//
// Why the bits are the loop's: an entry of Z is ONE ordered sum of products whose operands are entries of L and entries of Z
// in columns that are ancestors of j in the elimination tree (S_j is a clique of the filled graph, so the pair {i,k} is stored
// in column min(i,k), a member of S_j, and S_j lies on j's path to the root).  Whoever runs column j after its ancestors sees
// the loop's operands; one lane forms each sum in storage order with contraction off and true divisions.
//
// Schedule.  Columns of one depth of the elimination forest (roots 0) are independent: one launch per depth, roots first.
// Depths come from pointer jumping on parent[j] = the row of the second entry of column j, the columns are sorted by depth
// with the library's stable sort (ascending inside a depth), and the lists stay on the matrix (Csc::inv; the pattern's, so
// they outlive csx_updown_block).  |S_j| <= depth(j), so the longest column of a depth picks that launch's shape.  A run of
// depths of one column each with at most SI_WIDE_ROWS rows (all of a chain of short columns) is walked by one workgroup inside
// one launch ("sparseinv.walk", on by default).
//
// Kernels.  k_si_group<G>: G = 8 / 16 / 32 / 64 lanes per column, lane r owns row S_j[r] and its sum.  Zs(i,k) is found in
// column a = min(i,k) at offset |r - t| from its diagonal when column a holds exactly the tail of S_j (cliques, supernodes:
// one compare), by bisection of column a otherwise; a pair that is not there raises the flag.  A lane looks up eight terms at a
// time and then adds them in order.  The diagonal's sum takes the lanes' results by shuffles.  k_si_block<B>: one workgroup
// per column for 64 < |S_j| <= SI_WIDE_ROWS and for the walk; rows strided over the threads, the diagonal's products through
// LDS and summed by one thread in order.  k_si_wide: longer columns, one wave per row (see there), then k_si_block for the
// diagonals alone.
#include <algorithm>

#include "csx_internal.h"

namespace csx {

namespace {

struct SiInfo {
    int32_t depths = 0, widest = 0;
    int64_t terms = 0;
    double kernel_ms = 0.0;
};
SiInfo g_si_info;

// flag bits of the validation
constexpr int SI_EMPTY = 1, SI_DIAG_FIRST = 2, SI_ROWS = 4, SI_DIAG_VALUE = 8, SI_PTR = 16, SI_PAIR = 32;

// per column: pointers monotone, the column non-empty, its first entry the diagonal, positive and finite
__global__ __launch_bounds__(256) void k_si_check_cols(int32_t n, int32_t nnz, const int32_t *__restrict__ Lp,
                                                       const int32_t *__restrict__ Li, const double *__restrict__ Lx, int *flag) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const int32_t b = Lp[j], e = Lp[j + 1];
    if ((j == 0 && b != 0) || (j == n - 1 && e != nnz) || b < 0 || e > nnz || e < b) {
        atomicOr(flag, SI_PTR);
        return;
    }
    if (e == b) {
        atomicOr(flag, SI_EMPTY);
        return;
    }
    if (Li[b] != (int32_t)j) {
        atomicOr(flag, SI_DIAG_FIRST);
        return;
    }
    const double d = Lx[b];
    if (!(d > 0.0) || !(d <= 1.79769313486231570815e308)) atomicOr(flag, SI_DIAG_VALUE);
}

// per entry: the row in range, and above the row before it unless the entry opens a column (the diagonal of column Li[q],
// which k_si_check_cols holds to Li[Lp[j]] == j)
__global__ __launch_bounds__(256) void k_si_check_rows(int32_t n, int32_t nnz, const int32_t *__restrict__ Lp,
                                                       const int32_t *__restrict__ Li, int *flag) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nnz) return;
    const int32_t r = Li[q];
    if (r < 0 || r >= n) {
        atomicOr(flag, SI_ROWS);
        return;
    }
    if (q == 0) return;
    if (!(r > Li[q - 1]) && Lp[r] != (int32_t)q) atomicOr(flag, SI_ROWS);
}

// parent and |S_j| of every column; the pointer-jumping state starts as (parent, one step)
__global__ __launch_bounds__(256) void k_si_parent(int32_t n, const int32_t *__restrict__ Lp, const int32_t *__restrict__ Li,
                                                   int32_t *__restrict__ anc, int32_t *__restrict__ dep,
                                                   unsigned long long *terms) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long mine = 0;
    if (j < n) {
        const int32_t b = Lp[j], m = Lp[j + 1] - b - 1;
        anc[j] = m > 0 ? Li[b + 1] : -1;
        dep[j] = m > 0 ? 1 : 0;
        mine = (unsigned long long)m * (unsigned long long)m;
    }
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o, 64);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(terms, mine);
}

// dep[j] = the steps from j to anc[j] (to the root once anc[j] == -1); one round doubles the reach
__global__ __launch_bounds__(256) void k_si_jump(int32_t n, const int32_t *__restrict__ anc, const int32_t *__restrict__ dep,
                                                 int32_t *__restrict__ anc2, int32_t *__restrict__ dep2) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const int32_t a = anc[j];
    if (a < 0) {
        anc2[j] = -1;
        dep2[j] = dep[j];
    } else {
        anc2[j] = anc[a];
        dep2[j] = dep[j] + dep[a];
    }
}

__global__ __launch_bounds__(256) void k_si_iota_max(int32_t n, const int32_t *__restrict__ dep, uint32_t *__restrict__ col,
                                                     int32_t *maxdep) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int32_t mine = 0;
    if (j < n) {
        col[j] = (uint32_t)j;
        mine = dep[j];
    }
    for (int o = 32; o > 0; o >>= 1) mine = max(mine, __shfl_xor(mine, o, 64));
    if ((threadIdx.x & 63) == 0) atomicMax(maxdep, mine);
}

// rows[d] = the largest |S_j| among the columns of depth d
__global__ __launch_bounds__(256) void k_si_rows_of_depth(int32_t n, const int32_t *__restrict__ Lp, const int32_t *__restrict__ dep,
                                                          int32_t *rows) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    atomicMax(&rows[dep[j]], Lp[j + 1] - Lp[j] - 1);
}

#pragma clang fp contract(off)

constexpr int SI_BATCH = 8;   // terms whose lookups a lane has in flight together

// the position of Z(row, col), row > col, col's entries at [b, e), by bisection; b itself (in range) when it is not stored
__device__ __noinline__ int32_t si_bisect(const int32_t *__restrict__ Li, int32_t b, int32_t e, int32_t row, int *flag) {
    int32_t lo = b + 1, hi = e;
    while (lo < hi) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        if (Li[mid] < row) lo = mid + 1;
        else hi = mid;
    }
    if (lo < e && Li[lo] == row) return lo;
    atomicOr(flag, SI_PAIR);   // not a Cholesky pattern: the call fails, nothing out of range was read
    return b;
}

// Z(S_j[r], j) = (-sum_t L(S_j[t], j) * Zs(S_j[r], S_j[t])) / d, the sum in storage order.  With i = S_j[r] and k = S_j[t],
// Zs(i,k) lies in column k at row i for t < r and in column i at row k for t >= r (t == r: the diagonal of column i), |r - t|
// entries below that column's diagonal when the column holds exactly the tail of S_j -- one compare -- and wherever bisection
// finds it otherwise.  The lookups of SI_BATCH terms are issued together (they do not depend on one another; the sum does):
// a lane that walks a long column alone is bound by the latency of these loads, not by their number.
__device__ __forceinline__ double si_row(const int32_t *__restrict__ Lp, const int32_t *__restrict__ Li,
                                         const double *__restrict__ Lx, const double *Zx, int32_t pj, int32_t m, int32_t r, double d,
                                         int *flag) {
    const int32_t i = Li[pj + 1 + r];
    double s = 0.0;
    for (int32_t t0 = 0; t0 < m; t0 += SI_BATCH) {
        int32_t k[SI_BATCH], b[SI_BATCH], e[SI_BATCH], pos[SI_BATCH];
        double l[SI_BATCH], z[SI_BATCH];
#pragma unroll
        for (int u = 0; u < SI_BATCH; u++) {
            const int32_t t = min(t0 + u, m - 1);   // (past the end: the last term again, not added)
            k[u] = Li[pj + 1 + t];
            l[u] = Lx[pj + 1 + t];
        }
#pragma unroll
        for (int u = 0; u < SI_BATCH; u++) {
            const int32_t col = min(t0 + u, m - 1) < r ? k[u] : i;
            b[u] = Lp[col];
            e[u] = Lp[col + 1];
        }
#pragma unroll
        for (int u = 0; u < SI_BATCH; u++) {
            const int32_t t = min(t0 + u, m - 1);
            const int32_t g = t < r ? r - t : t - r;
            pos[u] = b[u] + min(g, e[u] - b[u] - 1);
            k[u] = Li[pos[u]] == (t < r ? i : k[u]) ? -1 : (t < r ? i : k[u]);   // -1: found; else the row to look for
        }
#pragma unroll
        for (int u = 0; u < SI_BATCH; u++)
            if (k[u] >= 0) pos[u] = si_bisect(Li, b[u], e[u], k[u], flag);
#pragma unroll
        for (int u = 0; u < SI_BATCH; u++) z[u] = Zx[pos[u]];
#pragma unroll
        for (int u = 0; u < SI_BATCH; u++)
            if (t0 + u < m) s = s + l[u] * z[u];
    }
    return (-s) / d;
}

// G lanes per column of the list [c0, c0 + cnt): every column has at most G rows below its diagonal
template <int G>
__global__ __launch_bounds__(256) void k_si_group(const int32_t *__restrict__ list, int32_t c0, int32_t cnt,
                                                  const int32_t *__restrict__ Lp, const int32_t *__restrict__ Li,
                                                  const double *__restrict__ Lx, double *Zx, int *flag) {
    const int64_t g = ((int64_t)blockIdx.x * 256 + threadIdx.x) / G;
    const int32_t r = (int32_t)(threadIdx.x % G);
    const bool has = g < cnt;
    const int32_t j = has ? list[c0 + g] : 0;
    const int32_t pj = has ? Lp[j] : 0;
    const int32_t m = has ? Lp[j + 1] - pj - 1 : 0;
    const double d = has ? Lx[pj] : 1.0;
    double z = 0.0;
    if (r < m) {
        z = si_row(Lp, Li, Lx, Zx, pj, m, r, d, flag);
        Zx[pj + 1 + r] = z;
    }
    int32_t mmax = m;   // the wave's longest column: every lane stays in the loop of shuffles
    for (int o = 32; o > 0; o >>= 1) mmax = max(mmax, __shfl_xor(mmax, o, 64));
    double s = 0.0;
    for (int32_t t = 0; t < mmax; t++) {
        const double zt = __shfl(z, t, G);
        if (t < m) s = s + Lx[pj + 1 + t] * zt;
    }
    if (has && r == 0) Zx[pj] = (1.0 / d - s) / d;
}

constexpr int SI_WIDE_CHUNK = 512;   // products a wave of k_si_wide holds in LDS at a time
constexpr int SI_WIDE_ROWS = 128;    // a depth whose longest column has more rows below the diagonal goes to k_si_wide

// One WAVE per row of a long column (four rows to a workgroup, `rowblocks` workgroups to a column): a lone lane would walk the
// row's |S_j| lookups a batch at a time; here the lanes look the terms up side by side, the products wait in LDS, and lane 0
// adds them in storage order.  The diagonal follows in a launch of its own (k_si_block, SI_DIAGONALS).
__global__ __launch_bounds__(256) void k_si_wide(const int32_t *__restrict__ list, int32_t c0, int32_t rowblocks,
                                                 const int32_t *__restrict__ Lp, const int32_t *__restrict__ Li,
                                                 const double *__restrict__ Lx, double *Zx, int *flag) {
    __shared__ double prod[4][SI_WIDE_CHUNK];
    const int32_t w = (int32_t)(threadIdx.x >> 6), lane = (int32_t)(threadIdx.x & 63);
    const int32_t j = list[c0 + (int32_t)(blockIdx.x / (unsigned)rowblocks)];
    const int32_t r = (int32_t)(blockIdx.x % (unsigned)rowblocks) * 4 + w;
    const int32_t pj = Lp[j];
    const int32_t m = Lp[j + 1] - pj - 1;   // the same for the four waves: they meet at every barrier
    const bool has = r < m;
    const int32_t i = has ? Li[pj + 1 + r] : 0;
    double s = 0.0;
    for (int32_t base = 0; base < m; base += SI_WIDE_CHUNK) {
        const int32_t cn = min(SI_WIDE_CHUNK, m - base);
        if (has) {
            for (int32_t u = lane; u < cn; u += 64) {
                const int32_t t = base + u;
                const int32_t k = Li[pj + 1 + t];
                const int32_t col = t < r ? k : i, row = t < r ? i : k;
                const int32_t b = Lp[col], e = Lp[col + 1];
                int32_t pos = b + min(t < r ? r - t : t - r, e - b - 1);
                if (Li[pos] != row) pos = si_bisect(Li, b, e, row, flag);
                prod[w][u] = Lx[pj + 1 + t] * Zx[pos];
            }
        }
        __syncthreads();
        if (has && lane == 0)
            for (int32_t u = 0; u < cn; u++) s = s + prod[w][u];
        __syncthreads();
    }
    if (has && lane == 0) Zx[pj + 1 + r] = (-s) / Lx[pj];
}

// what a launch of k_si_block does
enum SiBlockMode : int {
    SI_COLUMNS = 0,     // workgroup b: column list[c0 + b], rows and diagonal
    SI_WALK = 1,        // one workgroup: the columns [c0, c0 + cnt) one after the other (a run of depths of one column each:
                        // every column may read what the one before it wrote)
    SI_DIAGONALS = 2    // workgroup b: the diagonal of column list[c0 + b] alone, its rows are k_si_wide's
};

template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void k_si_block(const int32_t *__restrict__ list, int32_t c0, int32_t cnt, int mode,
                                                    const int32_t *__restrict__ Lp, const int32_t *__restrict__ Li,
                                                    const double *__restrict__ Lx, double *Zx, int *flag) {
    __shared__ double prod[BLOCK];
    const int32_t tid = (int32_t)threadIdx.x;
    const bool walk = mode == SI_WALK;
    const int32_t first = walk ? c0 : c0 + (int32_t)blockIdx.x;
    const int32_t last = walk ? c0 + cnt : first + 1;
    for (int32_t c = first; c < last; c++) {
        const int32_t j = list[c];
        const int32_t pj = Lp[j];
        const int32_t m = Lp[j + 1] - pj - 1;
        const double d = Lx[pj];
        if (mode != SI_DIAGONALS) {
            for (int32_t r = tid; r < m; r += BLOCK) Zx[pj + 1 + r] = si_row(Lp, Li, Lx, Zx, pj, m, r, d, flag);
            __syncthreads();
        }
        double s = 0.0;
        for (int32_t b = 0; b < m; b += BLOCK) {
            if (b + tid < m) prod[tid] = Lx[pj + 1 + b + tid] * Zx[pj + 1 + b + tid];
            __syncthreads();
            if (tid == 0) {
                const int32_t cntb = min(BLOCK, m - b);
                for (int32_t u = 0; u < cntb; u++) s = s + prod[u];
            }
            __syncthreads();
        }
        if (tid == 0) Zx[pj] = (1.0 / d - s) / d;
        if (walk) {
            __threadfence();
            __syncthreads();
        }
    }
}

#pragma clang fp contract(fast)

__global__ __launch_bounds__(256) void k_si_diag(int32_t n, const int32_t *__restrict__ p, const double *__restrict__ x,
                                                 double *__restrict__ out) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const int32_t b = p[j];
    out[j] = b < p[j + 1] ? x[b] : 0.0;
}

inline unsigned blocks_of(int64_t count, int per) { return (unsigned)((count + per - 1) / per); }

// depth of every column, the columns listed by depth: built once per pattern (L passed the structure checks)
int si_schedule(Csc *L) {
    if (L->inv) return CSX_OK;
    const int32_t n = L->n;
    hipStream_t s = ctx().stream;
    const unsigned nb = blocks_of(n, 256);
    DevBuf<int32_t> anc, dep, anc2, dep2, maxdep, rows;
    DevBuf<unsigned long long> terms;
    CSX_TRY(anc.alloc((size_t)n));
    CSX_TRY(dep.alloc((size_t)n));
    CSX_TRY(anc2.alloc((size_t)n));
    CSX_TRY(dep2.alloc((size_t)n));
    CSX_TRY(maxdep.alloc(1));
    CSX_TRY(terms.alloc(1));
    CSX_HIP(hipMemsetAsync(maxdep, 0, sizeof(int32_t), s));
    CSX_HIP(hipMemsetAsync(terms, 0, sizeof(unsigned long long), s));
    hipLaunchKernelGGL(k_si_parent, dim3(nb), dim3(256), 0, s, n, L->p, L->i, anc.get(), dep.get(), terms.get());
    int32_t *a = anc, *d = dep, *a2 = anc2, *d2 = dep2;
    for (int64_t reach = 1; reach < n; reach *= 2) {   // parent[j] > j: a path has fewer than n steps
        hipLaunchKernelGGL(k_si_jump, dim3(nb), dim3(256), 0, s, n, a, d, a2, d2);
        std::swap(a, a2);
        std::swap(d, d2);
    }
    DevBuf<uint32_t> col, skey, scol;
    CSX_TRY(col.alloc((size_t)n));
    hipLaunchKernelGGL(k_si_iota_max, dim3(nb), dim3(256), 0, s, n, d, col.get(), maxdep.get());
    CSX_LAUNCH_CHECK();
    std::vector<int32_t> h;
    CSX_TRY(download_i32(h, maxdep, 1));
    const int32_t nd = h[0] + 1;
    unsigned long long hterms = 0;
    CSX_HIP(hipMemcpyAsync(&hterms, terms, sizeof(hterms), hipMemcpyDeviceToHost, s));
    std::unique_ptr<InvSchedule> S(new InvSchedule());
    CSX_TRY(skey.alloc((size_t)n));
    CSX_TRY(S->cols.alloc((size_t)n));
    CSX_TRY(stable_sort_by_key((const uint32_t *)d, col, nullptr, n, (uint32_t)nd, skey, (uint32_t *)S->cols.get(), nullptr));
    DevBuf<int32_t> ptr;
    CSX_TRY(ptr.alloc((size_t)nd + 1));
    CSX_TRY(boundaries_from_sorted(skey, n, nd, ptr));
    CSX_TRY(rows.alloc((size_t)nd));
    CSX_HIP(hipMemsetAsync(rows, 0, (size_t)nd * sizeof(int32_t), s));
    hipLaunchKernelGGL(k_si_rows_of_depth, dim3(nb), dim3(256), 0, s, n, L->p, d, rows.get());
    CSX_LAUNCH_CHECK();
    CSX_TRY(download_i32(S->ptr, ptr, (size_t)nd + 1));
    CSX_TRY(download_i32(S->rows, rows, (size_t)nd));
    S->ndepths = nd;
    S->terms = (int64_t)hterms;
    for (int32_t t = 0; t < nd; t++) S->widest = std::max(S->widest, S->ptr[(size_t)t + 1] - S->ptr[(size_t)t]);
    L->inv = std::move(S);
    return CSX_OK;
}

template <int G>
void si_launch_group(const InvSchedule *S, int32_t c0, int32_t cnt, const Csc *L, double *Zx, int *flag) {
    hipLaunchKernelGGL(k_si_group<G>, dim3(blocks_of((int64_t)cnt * G, 256)), dim3(256), 0, ctx().stream, S->cols.get(), c0, cnt, L->p,
                       L->i, L->x, Zx, flag);
}

void si_launch_block(const InvSchedule *S, int32_t c0, int32_t cnt, SiBlockMode mode, int32_t rows, const Csc *L, double *Zx, int *flag) {
    const dim3 grid(mode == SI_WALK ? 1u : (unsigned)cnt);
    hipStream_t s = ctx().stream;
    if (rows <= 64)
        hipLaunchKernelGGL(k_si_block<64>, grid, dim3(64), 0, s, S->cols.get(), c0, cnt, (int)mode, L->p, L->i, L->x, Zx, flag);
    else
        hipLaunchKernelGGL(k_si_block<256>, grid, dim3(256), 0, s, S->cols.get(), c0, cnt, (int)mode, L->p, L->i, L->x, Zx, flag);
}

// a depth of long columns: a wave per row, then the diagonals
void si_launch_wide(const InvSchedule *S, int32_t c0, int32_t cnt, int32_t rows, const Csc *L, double *Zx, int *flag) {
    const int32_t rowblocks = (rows + 3) / 4;
    hipLaunchKernelGGL(k_si_wide, dim3((unsigned)((int64_t)cnt * rowblocks)), dim3(256), 0, ctx().stream, S->cols.get(), c0, rowblocks,
                       L->p, L->i, L->x, Zx, flag);
    si_launch_block(S, c0, cnt, SI_DIAGONALS, rows, L, Zx, flag);
}

const char *si_what(int bits) {
    if (bits & SI_PTR) return "column pointers are not monotone from 0 to nnz";
    if (bits & SI_EMPTY) return "a column is empty";
    if (bits & SI_DIAG_FIRST) return "the first entry of a column is not its diagonal";
    if (bits & SI_ROWS) return "row indices are not strictly ascending below the diagonal and < n";
    if (bits & SI_DIAG_VALUE) return "a diagonal entry is not positive and finite";
    return "the pattern is not that of a Cholesky factor (an entry Z(i,k), i and k in one column of L, is not stored)";
}

}  // namespace

}  // namespace csx

using namespace csx;

extern "C" int csx_chol_inverse(csx_handle_t hL, csx_handle_t *out) {
    CSX_TRY(require_ready());
    Csc *L = csc(hL);
    if (!L || !out) {
        set_error("csx_chol_inverse: not a matrix handle");
        return CSX_EINVAL;
    }
    if (L->m != L->n) {
        set_error("csx_chol_inverse: L is %d-by-%d, not square", L->m, L->n);
        return CSX_EINVAL;
    }
    if (!L->x) {
        set_error("csx_chol_inverse: L has no values");
        return CSX_EINVAL;
    }
    const int32_t n = L->n, nnz = L->nnz;
    hipStream_t s = ctx().stream;
    g_si_info = SiInfo{};
    if (n > 0 && nnz < n) {
        set_error("csx_chol_inverse: %s", si_what(SI_EMPTY));
        return CSX_EINVAL;
    }
    DevBuf<int> flag;
    CSX_TRY(flag.alloc(1));
    CSX_HIP(hipMemsetAsync(flag, 0, sizeof(int), s));
    std::vector<int32_t> hflag(1, 0);
    if (n > 0) {
        // the column checks first: the row check relies on every column opening with its diagonal
        hipLaunchKernelGGL(k_si_check_cols, dim3(blocks_of(n, 256)), dim3(256), 0, s, n, nnz, L->p, L->i, L->x, flag.get());
        CSX_LAUNCH_CHECK();
        CSX_TRY(download_i32(hflag, (const int32_t *)flag.get(), 1));
        if (!hflag[0]) {
            hipLaunchKernelGGL(k_si_check_rows, dim3(blocks_of(nnz, 256)), dim3(256), 0, s, n, nnz, L->p, L->i, flag.get());
            CSX_LAUNCH_CHECK();
            CSX_TRY(download_i32(hflag, (const int32_t *)flag.get(), 1));
        }
        if (hflag[0]) {
            set_error("csx_chol_inverse: %s", si_what(hflag[0]));
            return CSX_EINVAL;
        }
    }
    csx_handle_t hZ = 0;
    CSX_TRY(csx_csc_alloc(n, n, nnz, 1, &hZ));
    Csc *Z = csc(hZ);
    struct Guard {   // no Z unless the call succeeds
        csx_handle_t h;
        ~Guard() {
            if (h) csx_free(h);
        }
    } guard{hZ};
    CSX_HIP(hipMemcpyAsync(Z->p, L->p, ((size_t)n + 1) * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    if (nnz) CSX_HIP(hipMemcpyAsync(Z->i, L->i, (size_t)nnz * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    if (n > 0) {
        CSX_TRY(si_schedule(L));
        const InvSchedule *S = L->inv.get();
        const bool walk = ctx().opt.sparseinv_walk != 0;
        hipEvent_t e0, e1;
        CSX_HIP(hipEventCreate(&e0));
        if (hipEventCreate(&e1) != hipSuccess) {
            (void)hipEventDestroy(e0);
            set_error("csx_chol_inverse: hipEventCreate failed");
            return CSX_ERUNTIME;
        }
        struct EvGuard {
            hipEvent_t a, b;
            ~EvGuard() {
                (void)hipEventDestroy(a);
                (void)hipEventDestroy(b);
            }
        } evguard{e0, e1};
        CSX_HIP(hipEventRecord(e0, s));
        for (int32_t t = 0; t < S->ndepths;) {
            const int32_t c0 = S->ptr[(size_t)t], cnt = S->ptr[(size_t)t + 1] - c0;
            int32_t rows = S->rows[(size_t)t], u = t + 1;
            if (walk && cnt == 1 && rows <= SI_WIDE_ROWS) {   // a run of depths of one short column each: one workgroup walks it
                while (u < S->ndepths && S->ptr[(size_t)u + 1] - S->ptr[(size_t)u] == 1 && S->rows[(size_t)u] <= SI_WIDE_ROWS)
                    rows = std::max(rows, S->rows[(size_t)u++]);
            }
            if (u - t > 1) si_launch_block(S, c0, u - t, SI_WALK, rows, L, Z->x, flag);
            else if (rows <= 8) si_launch_group<8>(S, c0, cnt, L, Z->x, flag);
            else if (rows <= 16) si_launch_group<16>(S, c0, cnt, L, Z->x, flag);
            else if (rows <= 32) si_launch_group<32>(S, c0, cnt, L, Z->x, flag);
            else if (rows <= 64) si_launch_group<64>(S, c0, cnt, L, Z->x, flag);
            else if (rows <= SI_WIDE_ROWS) si_launch_block(S, c0, cnt, SI_COLUMNS, rows, L, Z->x, flag);
            else si_launch_wide(S, c0, cnt, rows, L, Z->x, flag);
            t = u;
        }
        CSX_HIP(hipEventRecord(e1, s));
        CSX_LAUNCH_CHECK();
        CSX_TRY(download_i32(hflag, (const int32_t *)flag.get(), 1));
        float ms = 0.0f;
        CSX_HIP(hipEventElapsedTime(&ms, e0, e1));
        if (hflag[0]) {
            set_error("csx_chol_inverse: %s", si_what(hflag[0]));
            return CSX_EINVAL;
        }
        g_si_info.depths = S->ndepths;   // (a call that fails reports zeros, whichever check refused it)
        g_si_info.widest = S->widest;
        g_si_info.terms = S->terms;
        g_si_info.kernel_ms = ms;
    }
    guard.h = 0;
    *out = hZ;
    return CSX_OK;
}

extern "C" int csx_chol_inverse_info(int32_t *depths, int32_t *widest, int64_t *terms, double *kernel_ms) {
    if (depths) *depths = g_si_info.depths;
    if (widest) *widest = g_si_info.widest;
    if (terms) *terms = g_si_info.terms;
    if (kernel_ms) *kernel_ms = g_si_info.kernel_ms;
    return CSX_OK;
}

extern "C" int csx_csc_diag(csx_handle_t hM, csx_handle_t hout) {
    CSX_TRY(require_ready());
    Csc *M = csc(hM);
    Vec *o = vec(hout);
    if (!M || !M->x || !o || o->len < M->n) {
        set_error("csx_csc_diag: needs a matrix with values and a vector of at least n entries");
        return CSX_EINVAL;
    }
    if (M->n == 0) return CSX_OK;
    hipLaunchKernelGGL(k_si_diag, dim3(blocks_of(M->n, 256)), dim3(256), 0, ctx().stream, M->n, M->p, M->x, (double *)o->d);
    CSX_LAUNCH_CHECK();
    return CSX_OK;
}
