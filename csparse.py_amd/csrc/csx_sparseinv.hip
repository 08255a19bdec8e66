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
//
// Column policies.  The same schedule, lookups and four kernel shapes serve three factorisations on a Cholesky
// pattern; a policy K says where the pivot of a column lives and how a finished sum becomes an entry:
//     SI_CHOL  Z = inv(L L'):   d = L(j,j);   Z(i,j) = (-s) / d;                       Z(j,j) = (1/d - s) / d
//     SI_LDL   Z = inv(L D L'): d = d[j];     Z(i,j) = -s;                             Z(j,j) = 1/d - s        (L(j,j) never read)
//     SI_LU    Z = inv(L U):    d = Ut(j,j);  ZL(i,j) = -sL, ZU(i,j) = (-sU) / d;      ZL(j,j) = ZU(j,j) = 1/d - s,
// where for SI_LU  sL = sum_k L(k,j) Z(i,k),  sU = sum_k Ut(k,j) Z(k,i)  and  s = sum_k L(k,j) ZU(k,j).  Z(i,k) and Z(k,i) share
// ONE slot of the pattern (column min(i,k), row max(i,k)): ZL holds the entry below the diagonal, ZU the one above it, so one
// position lookup serves both sums and the two arrays swap roles where the term index passes the row's own (t = r).
#include <algorithm>

#include "csx_internal.h"

namespace csx {

namespace {

enum SiKind : int { SI_CHOL = 0, SI_LDL = 1, SI_LU = 2 };

struct SiInfo {
    int kind = SI_CHOL;
    int32_t depths = 0, widest = 0;
    int64_t terms = 0;
    double kernel_ms = 0.0;
};
SiInfo g_si_info;

// flag bits of the validation
constexpr int SI_EMPTY = 1, SI_DIAG_FIRST = 2, SI_ROWS = 4, SI_DIAG_VALUE = 8, SI_PTR = 16, SI_PAIR = 32, SI_PATTERN = 64, SI_INDEX = 128;

// per column: pointers monotone, the column non-empty, its first entry the diagonal; the pivot of the policy positive
// (SI_CHOL: Dx = L.x, the first entry of the column) or non-zero (SI_LDL: Dx = d, entry j; SI_LU: Dx = Ut.x, the first entry of
// the column) and finite
__global__ __launch_bounds__(256) void k_si_check_cols(int32_t n, int32_t nnz, int kind, const int32_t *__restrict__ Lp,
                                                       const int32_t *__restrict__ Li, const double *__restrict__ Dx, int *flag) {
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
    const double d = Dx[kind == SI_LDL ? (int32_t)j : b];
    const bool ok = kind == SI_CHOL ? d > 0.0 : d != 0.0;
    if (!ok || !(fabs(d) <= 1.79769313486231570815e308)) atomicOr(flag, SI_DIAG_VALUE);
}

// SI_LU: Ut on L's pattern, entry for entry (n and nnz were compared on the host)
__global__ __launch_bounds__(256) void k_si_same_pattern(int32_t n, int32_t nnz, const int32_t *__restrict__ Lp,
                                                         const int32_t *__restrict__ Li, const int32_t *__restrict__ Up,
                                                         const int32_t *__restrict__ Ui, int *flag) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool differ = false;
    if (q <= n) differ = Lp[q] != Up[q];
    if (q < nnz) differ = differ || Li[q] != Ui[q];
    if (differ) atomicOr(flag, SI_PATTERN);
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

// the pivot of column j (entries from pj) under the policy K: L(j,j), d[j] or Ut(j,j)
template <int K>
__device__ __forceinline__ double si_pivot(const double *__restrict__ Lx, const double *__restrict__ Dx, int32_t j, int32_t pj) {
    if constexpr (K == SI_CHOL) return Lx[pj];
    else if constexpr (K == SI_LDL) return Dx[j];
    else return Dx[pj];
}

// Z(S_j[r], j) = (-sum_t L(S_j[t], j) * Zs(S_j[r], S_j[t])) / d, the sum in storage order.  With i = S_j[r] and k = S_j[t],
// Zs(i,k) lies in column k at row i for t < r and in column i at row k for t >= r (t == r: the diagonal of column i), |r - t|
// entries below that column's diagonal when the column holds exactly the tail of S_j -- one compare -- and wherever bisection
// finds it otherwise.  The lookups of SI_BATCH terms are issued together (they do not depend on one another; the sum does):
// a lane that walks a long column alone is bound by the latency of these loads, not by their number.
//
// The policy K: SI_CHOL and SI_LDL form the one sum s and return zl = (-s) / d resp. -s.  SI_LU forms two sums over the same
// lookups: sL takes L(k,j) * Z(i,k) and sU takes Ut(k,j) * Z(k,i), where Z(i,k) is ZL[pos] and Z(k,i) is ZU[pos] for t < r and the
// other way round for t >= r (at t == r both are the diagonal of column i); zl = -sL, zu = (-sU) / d.  Two value loads and two
// separately rounded multiply-adds a term, one lookup.
template <int K>
__device__ __forceinline__ void si_row(const int32_t *__restrict__ Lp, const int32_t *__restrict__ Li,
                                       const double *__restrict__ Lx, const double *__restrict__ Dx, const double *Zx,
                                       const double *Zu, int32_t pj, int32_t m, int32_t r, double d, int *flag, double &zl,
                                       double &zu) {
    const int32_t i = Li[pj + 1 + r];
    double s = 0.0, su = 0.0;
    for (int32_t t0 = 0; t0 < m; t0 += SI_BATCH) {
        int32_t k[SI_BATCH], b[SI_BATCH], e[SI_BATCH], pos[SI_BATCH];
        double l[SI_BATCH], z[SI_BATCH];
        double ut[K == SI_LU ? SI_BATCH : 1], w[K == SI_LU ? SI_BATCH : 1];
#pragma unroll
        for (int u = 0; u < SI_BATCH; u++) {
            const int32_t t = min(t0 + u, m - 1);   // (past the end: the last term again, not added)
            k[u] = Li[pj + 1 + t];
            if constexpr (K != SI_LU) l[u] = Lx[pj + 1 + t];
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
        for (int u = 0; u < SI_BATCH; u++) {
            z[u] = Zx[pos[u]];
            if constexpr (K == SI_LU) {
                w[u] = Zu[pos[u]];
                l[u] = Lx[pj + 1 + min(t0 + u, m - 1)];   // (the two factors after the lookups: not held across them)
                ut[u] = Dx[pj + 1 + min(t0 + u, m - 1)];
            }
        }
#pragma unroll
        for (int u = 0; u < SI_BATCH; u++) {
            if constexpr (K == SI_LU) {
                const bool below = t0 + u < r;   // Z(i,k) below the diagonal: in ZL, and Z(k,i) in ZU
                if (t0 + u < m) {
                    s = s + l[u] * (below ? z[u] : w[u]);
                    su = su + ut[u] * (below ? w[u] : z[u]);
                }
            } else {
                if (t0 + u < m) s = s + l[u] * z[u];
            }
        }
    }
    if constexpr (K == SI_CHOL) zl = (-s) / d;
    else zl = -s;
    if constexpr (K == SI_LU) zu = (-su) / d;
}

// the diagonal of a column from the finished sum s = sum_k L(k,j) * Z(k,j) (SI_LU: Z(k,j) read from ZU)
template <int K>
__device__ __forceinline__ double si_diag(double d, double s) {
    if constexpr (K == SI_CHOL) return (1.0 / d - s) / d;
    else return 1.0 / d - s;
}

// G lanes per column of the list [c0, c0 + cnt): every column has at most G rows below its diagonal
// (SI_LU: the diagonal's sum takes the lanes' ZU results)
template <int K, int G>
__global__ __launch_bounds__(256) void k_si_group(const int32_t *__restrict__ list, int32_t c0, int32_t cnt,
                                                  const int32_t *__restrict__ Lp, const int32_t *__restrict__ Li,
                                                  const double *__restrict__ Lx, const double *__restrict__ Dx, double *Zx,
                                                  double *Zu, int *flag) {
    const int64_t g = ((int64_t)blockIdx.x * 256 + threadIdx.x) / G;
    const int32_t r = (int32_t)(threadIdx.x % G);
    const bool has = g < cnt;
    const int32_t j = has ? list[c0 + g] : 0;
    const int32_t pj = has ? Lp[j] : 0;
    const int32_t m = has ? Lp[j + 1] - pj - 1 : 0;
    const double d = has ? si_pivot<K>(Lx, Dx, j, pj) : 1.0;
    double z = 0.0, zu = 0.0;
    if (r < m) {
        si_row<K>(Lp, Li, Lx, Dx, Zx, Zu, pj, m, r, d, flag, z, zu);
        Zx[pj + 1 + r] = z;
        if constexpr (K == SI_LU) Zu[pj + 1 + r] = zu;
    }
    int32_t mmax = m;   // the wave's longest column: every lane stays in the loop of shuffles
    for (int o = 32; o > 0; o >>= 1) mmax = max(mmax, __shfl_xor(mmax, o, 64));
    double s = 0.0;
    for (int32_t t = 0; t < mmax; t++) {
        const double zt = __shfl(K == SI_LU ? zu : z, t, G);
        if (t < m) s = s + Lx[pj + 1 + t] * zt;
    }
    if (has && r == 0) {
        const double zd = si_diag<K>(d, s);
        Zx[pj] = zd;
        if constexpr (K == SI_LU) Zu[pj] = zd;
    }
}

constexpr int SI_WIDE_CHUNK = 512;   // products a wave of k_si_wide holds in LDS at a time
constexpr int SI_WIDE_ROWS = 128;    // a depth whose longest column has more rows below the diagonal goes to k_si_wide

// One WAVE per row of a long column (four rows to a workgroup, `rowblocks` workgroups to a column): a lone lane would walk the
// row's |S_j| lookups a batch at a time; here the lanes look the terms up side by side, the products wait in LDS, and lane 0
// adds them in storage order.  The diagonal follows in a launch of its own (k_si_block, SI_DIAGONALS).
// SI_LU keeps both product streams in LDS (2 x 4 x 512 doubles = 32 KB a workgroup); lane 0 adds L's products in order while
// lane 1 adds U's, so the serial tail of a row stays |S_j| adds.
template <int K>
__global__ __launch_bounds__(256) void k_si_wide(const int32_t *__restrict__ list, int32_t c0, int32_t rowblocks,
                                                 const int32_t *__restrict__ Lp, const int32_t *__restrict__ Li,
                                                 const double *__restrict__ Lx, const double *__restrict__ Dx, double *Zx,
                                                 double *Zu, int *flag) {
    constexpr int NS = K == SI_LU ? 2 : 1;   // product streams
    __shared__ double prod[NS][4][SI_WIDE_CHUNK];
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
                if constexpr (K == SI_LU) {
                    const double zl = Zx[pos], zu = Zu[pos];
                    prod[0][w][u] = Lx[pj + 1 + t] * (t < r ? zl : zu);
                    prod[1][w][u] = Dx[pj + 1 + t] * (t < r ? zu : zl);
                } else {
                    prod[0][w][u] = Lx[pj + 1 + t] * Zx[pos];
                }
            }
        }
        __syncthreads();
        if (has && lane < NS)
            for (int32_t u = 0; u < cn; u++) s = s + prod[lane][w][u];
        __syncthreads();
    }
    if constexpr (K == SI_CHOL) {
        if (has && lane == 0) Zx[pj + 1 + r] = (-s) / Lx[pj];
    } else {
        if (has && lane == 0) Zx[pj + 1 + r] = -s;
        if constexpr (K == SI_LU)
            if (has && lane == 1) Zu[pj + 1 + r] = (-s) / Dx[pj];
    }
}

// what a launch of k_si_block does
enum SiBlockMode : int {
    SI_COLUMNS = 0,     // workgroup b: column list[c0 + b], rows and diagonal
    SI_WALK = 1,        // one workgroup: the columns [c0, c0 + cnt) one after the other (a run of depths of one column each:
                        // every column may read what the one before it wrote)
    SI_DIAGONALS = 2    // workgroup b: the diagonal of column list[c0 + b] alone, its rows are k_si_wide's
};

template <int K, int BLOCK>
__global__ __launch_bounds__(BLOCK) void k_si_block(const int32_t *__restrict__ list, int32_t c0, int32_t cnt, int mode,
                                                    const int32_t *__restrict__ Lp, const int32_t *__restrict__ Li,
                                                    const double *__restrict__ Lx, const double *__restrict__ Dx, double *Zx,
                                                    double *Zu, int *flag) {
    __shared__ double prod[BLOCK];
    const int32_t tid = (int32_t)threadIdx.x;
    const bool walk = mode == SI_WALK;
    const int32_t first = walk ? c0 : c0 + (int32_t)blockIdx.x;
    const int32_t last = walk ? c0 + cnt : first + 1;
    for (int32_t c = first; c < last; c++) {
        const int32_t j = list[c];
        const int32_t pj = Lp[j];
        const int32_t m = Lp[j + 1] - pj - 1;
        const double d = si_pivot<K>(Lx, Dx, j, pj);
        const double *Zd = K == SI_LU ? Zu : Zx;   // where the diagonal's sum reads Z(k,j)
        if (mode != SI_DIAGONALS) {
            for (int32_t r = tid; r < m; r += BLOCK) {
                double z = 0.0, zu = 0.0;
                si_row<K>(Lp, Li, Lx, Dx, Zx, Zu, pj, m, r, d, flag, z, zu);
                Zx[pj + 1 + r] = z;
                if constexpr (K == SI_LU) Zu[pj + 1 + r] = zu;
            }
            __syncthreads();
        }
        double s = 0.0;
        for (int32_t b = 0; b < m; b += BLOCK) {
            if (b + tid < m) prod[tid] = Lx[pj + 1 + b + tid] * Zd[pj + 1 + b + tid];
            __syncthreads();
            if (tid == 0) {
                const int32_t cntb = min(BLOCK, m - b);
                for (int32_t u = 0; u < cntb; u++) s = s + prod[u];
            }
            __syncthreads();
        }
        if (tid == 0) {
            const double zd = si_diag<K>(d, s);
            Zx[pj] = zd;
            if constexpr (K == SI_LU) Zu[pj] = zd;
        }
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

// csx_inverse_at: out[t] = Z(a, b), a = rmap[rows[t]], b = cmap[cols[t]] (null map: the identity), read off the pattern: a > b from
// column b of the lower array, a < b from column a of the upper array, a == b the first entry of column a.  A pair that is not
// stored gives NaN and is counted; an index outside [0, n) raises the flag (nothing is read for it).  Every position read lies
// inside [0, nnz): the column's range is clamped to it.
__global__ __launch_bounds__(256) void k_si_gather(int64_t count, int32_t n, int32_t nnz, const int32_t *__restrict__ rows,
                                                   const int32_t *__restrict__ cols, const int32_t *__restrict__ rmap,
                                                   const int32_t *__restrict__ cmap, const int32_t *__restrict__ Zp,
                                                   const int32_t *__restrict__ Zi, const double *__restrict__ Zl,
                                                   const double *__restrict__ Zu, double *__restrict__ out,
                                                   unsigned long long *missing, int *flag) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count) return;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    int32_t a = rows[t], b = cols[t];
    bool ok = (uint32_t)a < (uint32_t)n && (uint32_t)b < (uint32_t)n;
    if (ok) {
        if (rmap) a = rmap[a];
        if (cmap) b = cmap[b];
        ok = (uint32_t)a < (uint32_t)n && (uint32_t)b < (uint32_t)n;
    }
    if (!ok) {
        atomicOr(flag, SI_INDEX);
        out[t] = nan;
        return;
    }
    const int32_t col = min(a, b), row = max(a, b);
    const int32_t cb = max(Zp[col], 0), ce = min(Zp[col + 1], nnz);
    int32_t pos = -1;
    if (cb < ce && Zi[cb] == col) {   // the diagonal opens the column
        if (a == b) {
            pos = cb;
        } else {
            int32_t lo = cb + 1, hi = ce;
            while (lo < hi) {
                const int32_t mid = lo + ((hi - lo) >> 1);
                if (Zi[mid] < row) lo = mid + 1;
                else hi = mid;
            }
            if (lo < ce && Zi[lo] == row) pos = lo;
        }
    }
    if (pos < 0) {
        atomicAdd(missing, 1ull);
        out[t] = nan;
        return;
    }
    out[t] = (a >= b ? Zl : Zu)[pos];
}

// what the launches of one call read and write (Dx: nothing, d or Ut.x; Zu: ZU of SI_LU, else null)
struct SiRun {
    const InvSchedule *S;
    const Csc *L;
    const double *Dx;
    double *Zx, *Zu;
    int *flag;
};

template <int K, int G>
void si_launch_group(const SiRun &R, int32_t c0, int32_t cnt) {
    hipLaunchKernelGGL((k_si_group<K, G>), dim3(blocks_of((int64_t)cnt * G, 256)), dim3(256), 0, ctx().stream, R.S->cols.get(), c0, cnt,
                       R.L->p, R.L->i, R.L->x, R.Dx, R.Zx, R.Zu, R.flag);
}

template <int K>
void si_launch_block(const SiRun &R, int32_t c0, int32_t cnt, SiBlockMode mode, int32_t rows) {
    const dim3 grid(mode == SI_WALK ? 1u : (unsigned)cnt);
    hipStream_t s = ctx().stream;
    if (rows <= 64)
        hipLaunchKernelGGL((k_si_block<K, 64>), grid, dim3(64), 0, s, R.S->cols.get(), c0, cnt, (int)mode, R.L->p, R.L->i, R.L->x, R.Dx,
                           R.Zx, R.Zu, R.flag);
    else
        hipLaunchKernelGGL((k_si_block<K, 256>), grid, dim3(256), 0, s, R.S->cols.get(), c0, cnt, (int)mode, R.L->p, R.L->i, R.L->x,
                           R.Dx, R.Zx, R.Zu, R.flag);
}

// a depth of long columns: a wave per row, then the diagonals
template <int K>
void si_launch_wide(const SiRun &R, int32_t c0, int32_t cnt, int32_t rows) {
    const int32_t rowblocks = (rows + 3) / 4;
    hipLaunchKernelGGL(k_si_wide<K>, dim3((unsigned)((int64_t)cnt * rowblocks)), dim3(256), 0, ctx().stream, R.S->cols.get(), c0,
                       rowblocks, R.L->p, R.L->i, R.L->x, R.Dx, R.Zx, R.Zu, R.flag);
    si_launch_block<K>(R, c0, cnt, SI_DIAGONALS, rows);
}

// one launch per depth, roots first; the selection is the same for every policy
template <int K>
void si_run(const SiRun &R, bool walk) {
    const InvSchedule *S = R.S;
    for (int32_t t = 0; t < S->ndepths;) {
        const int32_t c0 = S->ptr[(size_t)t], cnt = S->ptr[(size_t)t + 1] - c0;
        int32_t rows = S->rows[(size_t)t], u = t + 1;
        if (walk && cnt == 1 && rows <= SI_WIDE_ROWS) {   // a run of depths of one short column each: one workgroup walks it
            while (u < S->ndepths && S->ptr[(size_t)u + 1] - S->ptr[(size_t)u] == 1 && S->rows[(size_t)u] <= SI_WIDE_ROWS)
                rows = std::max(rows, S->rows[(size_t)u++]);
        }
        if (u - t > 1) si_launch_block<K>(R, c0, u - t, SI_WALK, rows);
        else if (rows <= 8) si_launch_group<K, 8>(R, c0, cnt);
        else if (rows <= 16) si_launch_group<K, 16>(R, c0, cnt);
        else if (rows <= 32) si_launch_group<K, 32>(R, c0, cnt);
        else if (rows <= 64) si_launch_group<K, 64>(R, c0, cnt);
        else if (rows <= SI_WIDE_ROWS) si_launch_block<K>(R, c0, cnt, SI_COLUMNS, rows);
        else si_launch_wide<K>(R, c0, cnt, rows);
        t = u;
    }
}

const char *si_what(int bits, int kind) {
    if (bits & SI_PATTERN) return "Ut is not on the pattern of L (its column pointers or row indices differ)";
    if (bits & SI_PTR) return "column pointers are not monotone from 0 to nnz";
    if (bits & SI_EMPTY) return "a column is empty";
    if (bits & SI_DIAG_FIRST) return "the first entry of a column is not its diagonal";
    if (bits & SI_ROWS) return "row indices are not strictly ascending below the diagonal and < n";
    if (bits & SI_DIAG_VALUE)
        return kind == SI_CHOL  ? "a diagonal entry is not positive and finite"
               : kind == SI_LDL ? "an entry of d is zero or not finite"
                                : "a pivot Ut(j,j) is zero or not finite";
    return "the pattern is not that of a Cholesky factor (an entry Z(i,k), i and k in one column of L, is not stored)";
}

// The body of csx_chol_inverse, csx_ldl_inverse and csx_slu_inverse.  L: square with values (the caller checked); Dx: the
// policy's pivots (null for SI_CHOL: they are L's); U: Ut of SI_LU, else null; outU: where ZU's handle goes (SI_LU).
int si_inverse(int kind, const char *who, Csc *L, const double *Dx, const Csc *U, csx_handle_t *outL, csx_handle_t *outU) {
    const int32_t n = L->n, nnz = L->nnz;
    hipStream_t s = ctx().stream;
    g_si_info = SiInfo{};
    g_si_info.kind = kind;
    if (n > 0 && nnz < n) {
        set_error("%s: %s", who, si_what(SI_EMPTY, kind));
        return CSX_EINVAL;
    }
    DevBuf<int> flag;
    CSX_TRY(flag.alloc(1));
    CSX_HIP(hipMemsetAsync(flag, 0, sizeof(int), s));
    std::vector<int32_t> hflag(1, 0);
    if (n > 0) {
        if (kind == SI_LU && (U->p != L->p || U->i != L->i)) {   // Ut on L's pattern, before anything is read through it
            hipLaunchKernelGGL(k_si_same_pattern, dim3(blocks_of(std::max<int64_t>(nnz, (int64_t)n + 1), 256)), dim3(256), 0, s, n, nnz,
                               L->p, L->i, U->p, U->i, flag.get());
            CSX_LAUNCH_CHECK();
            CSX_TRY(download_i32(hflag, (const int32_t *)flag.get(), 1));
        }
        // the column checks next: the row check relies on every column opening with its diagonal
        if (!hflag[0]) {
            hipLaunchKernelGGL(k_si_check_cols, dim3(blocks_of(n, 256)), dim3(256), 0, s, n, nnz, kind, L->p, L->i,
                               kind == SI_CHOL ? L->x : Dx, flag.get());
            CSX_LAUNCH_CHECK();
            CSX_TRY(download_i32(hflag, (const int32_t *)flag.get(), 1));
        }
        if (!hflag[0]) {
            hipLaunchKernelGGL(k_si_check_rows, dim3(blocks_of(nnz, 256)), dim3(256), 0, s, n, nnz, L->p, L->i, flag.get());
            CSX_LAUNCH_CHECK();
            CSX_TRY(download_i32(hflag, (const int32_t *)flag.get(), 1));
        }
        if (hflag[0]) {
            set_error("%s: %s", who, si_what(hflag[0], kind));
            return CSX_EINVAL;
        }
    }
    struct Guard {   // no Z unless the call succeeds
        csx_handle_t h = 0;
        ~Guard() {
            if (h) csx_free(h);
        }
    } guard[2];
    Csc *Z[2] = {nullptr, nullptr};
    for (int a = 0; a < (kind == SI_LU ? 2 : 1); a++) {
        CSX_TRY(csx_csc_alloc(n, n, nnz, 1, &guard[a].h));
        Z[a] = csc(guard[a].h);
        CSX_HIP(hipMemcpyAsync(Z[a]->p, L->p, ((size_t)n + 1) * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
        if (nnz) CSX_HIP(hipMemcpyAsync(Z[a]->i, L->i, (size_t)nnz * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    }
    if (n > 0) {
        CSX_TRY(si_schedule(L));
        const InvSchedule *S = L->inv.get();
        const bool walk = ctx().opt.sparseinv_walk != 0;
        hipEvent_t e0, e1;
        CSX_HIP(hipEventCreate(&e0));
        if (hipEventCreate(&e1) != hipSuccess) {
            (void)hipEventDestroy(e0);
            set_error("%s: hipEventCreate failed", who);
            return CSX_ERUNTIME;
        }
        struct EvGuard {
            hipEvent_t a, b;
            ~EvGuard() {
                (void)hipEventDestroy(a);
                (void)hipEventDestroy(b);
            }
        } evguard{e0, e1};
        const SiRun R{S, L, Dx, Z[0]->x, Z[1] ? Z[1]->x : nullptr, flag.get()};
        CSX_HIP(hipEventRecord(e0, s));
        if (kind == SI_CHOL) si_run<SI_CHOL>(R, walk);
        else if (kind == SI_LDL) si_run<SI_LDL>(R, walk);
        else si_run<SI_LU>(R, walk);
        CSX_HIP(hipEventRecord(e1, s));
        CSX_LAUNCH_CHECK();
        CSX_TRY(download_i32(hflag, (const int32_t *)flag.get(), 1));
        float ms = 0.0f;
        CSX_HIP(hipEventElapsedTime(&ms, e0, e1));
        if (hflag[0]) {
            set_error("%s: %s", who, si_what(hflag[0], kind));
            return CSX_EINVAL;
        }
        g_si_info.depths = S->ndepths;   // (a call that fails reports zeros, whichever check refused it)
        g_si_info.widest = S->widest;
        g_si_info.terms = S->terms;
        g_si_info.kernel_ms = ms;
    }
    *outL = guard[0].h;
    guard[0].h = 0;
    if (kind == SI_LU) {
        *outU = guard[1].h;
        guard[1].h = 0;
    }
    return CSX_OK;
}

// a square matrix with values, or null and the error set
Csc *si_factor(const char *who, const char *name, csx_handle_t h) {
    Csc *L = csc(h);
    if (!L) {
        set_error("%s: %s is not a matrix handle", who, name);
        return nullptr;
    }
    if (L->m != L->n) {
        set_error("%s: %s is %d-by-%d, not square", who, name, L->m, L->n);
        return nullptr;
    }
    if (!L->x) {
        set_error("%s: %s has no values", who, name);
        return nullptr;
    }
    return L;
}

}  // namespace

}  // namespace csx

using namespace csx;

extern "C" int csx_chol_inverse(csx_handle_t hL, csx_handle_t *out) {
    CSX_TRY(require_ready());
    if (!out) {
        set_error("csx_chol_inverse: not a matrix handle");
        return CSX_EINVAL;
    }
    Csc *L = si_factor("csx_chol_inverse", "L", hL);
    if (!L) {
        g_si_info = SiInfo{};
        return CSX_EINVAL;
    }
    return si_inverse(SI_CHOL, "csx_chol_inverse", L, nullptr, nullptr, out, nullptr);
}

extern "C" int csx_ldl_inverse(csx_handle_t hL, csx_handle_t hd, csx_handle_t *out) {
    CSX_TRY(require_ready());
    g_si_info = SiInfo{};
    g_si_info.kind = SI_LDL;
    if (!out) {
        set_error("csx_ldl_inverse: no place for Z");
        return CSX_EINVAL;
    }
    Csc *L = si_factor("csx_ldl_inverse", "L", hL);
    if (!L) return CSX_EINVAL;
    Vec *d = vec(hd);
    if (!d || (L->n > 0 && !d->d)) {
        set_error("csx_ldl_inverse: d is not a vector handle");
        return CSX_EINVAL;
    }
    if (d->len < L->n) {
        set_error("csx_ldl_inverse: d has %lld entries, L has %d columns", (long long)d->len, L->n);
        return CSX_EINVAL;
    }
    return si_inverse(SI_LDL, "csx_ldl_inverse", L, (const double *)d->d, nullptr, out, nullptr);
}

extern "C" int csx_slu_inverse(csx_handle_t hL, csx_handle_t hU, csx_handle_t *outL, csx_handle_t *outU) {
    CSX_TRY(require_ready());
    g_si_info = SiInfo{};
    g_si_info.kind = SI_LU;
    if (!outL || !outU) {
        set_error("csx_slu_inverse: no place for ZL and ZUt");
        return CSX_EINVAL;
    }
    Csc *L = si_factor("csx_slu_inverse", "L", hL);
    if (!L) return CSX_EINVAL;
    Csc *U = si_factor("csx_slu_inverse", "Ut", hU);
    if (!U) return CSX_EINVAL;
    if (U->n != L->n || U->nnz != L->nnz) {
        set_error("csx_slu_inverse: Ut is of order %d with %d entries, L of order %d with %d: not one pattern", U->n, U->nnz, L->n,
                  L->nnz);
        return CSX_EINVAL;
    }
    return si_inverse(SI_LU, "csx_slu_inverse", L, U->x, U, outL, outU);
}

extern "C" int csx_inverse_at(csx_handle_t hZL, csx_handle_t hZU, csx_handle_t hrmap, csx_handle_t hcmap, int64_t count,
                              const int32_t *rows, const int32_t *cols, csx_handle_t hout, int64_t *missing) {
    CSX_TRY(require_ready());
    Csc *ZL = si_factor("csx_inverse_at", "ZL", hZL);
    if (!ZL) return CSX_EINVAL;
    Csc *ZU = ZL;
    if (hZU) {
        ZU = si_factor("csx_inverse_at", "ZUt", hZU);
        if (!ZU) return CSX_EINVAL;
        if (ZU->n != ZL->n || ZU->nnz != ZL->nnz) {
            set_error("csx_inverse_at: ZL and ZUt are not on one pattern");
            return CSX_EINVAL;
        }
    }
    const int32_t n = ZL->n;
    Vec *rmap = hrmap ? ivec(hrmap) : nullptr, *cmap = hcmap ? ivec(hcmap) : nullptr;
    Vec *out = vec(hout);
    if ((hrmap && (!rmap || rmap->len < n)) || (hcmap && (!cmap || cmap->len < n))) {
        set_error("csx_inverse_at: a map is not an int vector of at least n entries");
        return CSX_EINVAL;
    }
    if (count < 0 || !out || out->len < count || (count > 0 && (!rows || !cols))) {
        set_error("csx_inverse_at: needs count >= 0, rows, cols and an output vector of at least count entries");
        return CSX_EINVAL;
    }
    if (missing) *missing = 0;
    if (count == 0) return CSX_OK;
    hipStream_t s = ctx().stream;
    DevBuf<int32_t> drows, dcols;
    DevBuf<unsigned long long> dmiss;
    DevBuf<int> flag;
    CSX_TRY(upload(drows, rows, (size_t)count));
    CSX_TRY(upload(dcols, cols, (size_t)count));
    CSX_TRY(dmiss.alloc(1));
    CSX_TRY(flag.alloc(1));
    CSX_HIP(hipMemsetAsync(dmiss, 0, sizeof(unsigned long long), s));
    CSX_HIP(hipMemsetAsync(flag, 0, sizeof(int), s));
    hipLaunchKernelGGL(k_si_gather, dim3(blocks_of(count, 256)), dim3(256), 0, s, count, n, ZL->nnz, drows.get(), dcols.get(),
                       rmap ? (const int32_t *)rmap->d : nullptr, cmap ? (const int32_t *)cmap->d : nullptr, ZL->p, ZL->i, ZL->x,
                       ZU->x, (double *)out->d, dmiss.get(), flag.get());
    CSX_LAUNCH_CHECK();
    std::vector<int32_t> hflag;
    CSX_TRY(download_i32(hflag, (const int32_t *)flag.get(), 1));
    unsigned long long hmiss = 0;
    CSX_HIP(hipMemcpyAsync(&hmiss, dmiss, sizeof(hmiss), hipMemcpyDeviceToHost, s));
    CSX_HIP(hipStreamSynchronize(s));
    if (hflag[0]) {
        set_error("csx_inverse_at: an index in rows, cols or a map is outside [0, %d)", n);
        return CSX_EINVAL;
    }
    if (missing) *missing = (int64_t)hmiss;
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
