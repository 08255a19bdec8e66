// Assembly and reshaping around the hot path: the callers either side of
// cs_multiply / cs_transpose that are the same device primitives in other clothes.
//
//   cs_compress (csparse.py:647-673)  triplets -> CSC: the reference's counting sort by column, stable in
//                                     triplet order = one stable radix sort by column key (csx_sort.hip)
//   cs_add      (csparse.py:163-192)  alpha A + beta B, column pattern in first-touch order over
//                                     [A(:,j) then B(:,j)]:  C = [A B] * [alpha I; beta I]  through the
//                                     SpGEMM kernels, whose column order IS the reference's cs_scatter order
//   cs_dupl     (csparse.py:1035-1065) sum duplicates, first occurrence keeps its place:  C = A * I
//   cs_dropzeros / cs_droptol (csparse.py:1019-1031, 1002-1014; cs_fkeep :1172-1196)  order-preserving
//                                     compaction: per-column counts (ballots), scan, fill
//   cs_permute  (csparse.py:1666-1693) C = P A Q: columns gathered by q, rows renamed by pinv, order kept
//   cs_symperm  (csparse.py:2220-2255) upper triangle of P A P': entries i <= j renamed, bucketed by their
//                                     new column max(i2, j2) in (j, p) order = filter + stable radix sort
//
// p[] and i[] of every result are bit-identical to the reference's; x[] too wherever a value is copied or
// is the sum of at most two terms (cs_add of matrices without duplicates), otherwise sums are in arrival
// order and agree to rounding.
#include <cstring>
#include <vector>

#include "csx_internal.h"

namespace csx {

int multiply_device(const Csc *A, const Csc *B, Csc *C);   // csx_spgemm.hip

static inline unsigned blocks_for(int64_t n) { return (unsigned)((n + 255) / 256); }

static bool is_permutation(const int32_t *p, int32_t n) {
    std::vector<char> seen((size_t)n, 0);
    for (int32_t k = 0; k < n; k++) {
        if (p[k] < 0 || p[k] >= n || seen[(size_t)p[k]]) return false;
        seen[(size_t)p[k]] = 1;
    }
    return true;
}

// ---- cs_add / cs_dupl helpers --------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_cat_ptr(int32_t n, const int32_t *__restrict__ Ap, const int32_t *__restrict__ Bp,
                                                 int32_t *__restrict__ p) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j <= n) p[j] = Ap[j];
    if (j >= 1 && j <= n) p[n + j] = Ap[n] + Bp[j];
}

// S = [alpha I; beta I]  (2n x n), or the n x n identity when stacked == 0
__global__ __launch_bounds__(256) void k_selector(int32_t n, int stacked, double alpha, double beta, int32_t *__restrict__ p,
                                                  int32_t *__restrict__ i, double *__restrict__ x) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j > n) return;
    const int per = stacked ? 2 : 1;
    p[j] = (int32_t)(per * j);
    if (j == n) return;
    i[per * j] = (int32_t)j;
    if (x) x[per * j] = alpha;
    if (stacked) {
        i[2 * j + 1] = (int32_t)(n + j);
        if (x) x[2 * j + 1] = beta;
    }
}

static int add_device(const Csc *A, const Csc *B, double alpha, double beta, Csc *C) {
    hipStream_t s = ctx().stream;
    const int32_t n = A->n;
    const bool values = A->x && B->x;
    const int64_t tot = (int64_t)A->nnz + B->nnz;
    if (tot > 0x7FFFFFFFll || 2 * (int64_t)n > 0x7FFFFFFFll) return CSX_EINVAL;
    Csc cat, S;
    cat.m = A->m;
    cat.n = 2 * n;
    cat.nnz = (int32_t)tot;
    S.m = 2 * n;
    S.n = n;
    S.nnz = 2 * n;
    CSX_TRY(dalloc(&cat.p, (size_t)2 * n + 1));
    CSX_TRY(dalloc(&cat.i, (size_t)tot));
    if (values) CSX_TRY(dalloc(&cat.x, (size_t)tot));
    CSX_TRY(dalloc(&S.p, (size_t)n + 1));
    CSX_TRY(dalloc(&S.i, (size_t)2 * n));
    if (values) CSX_TRY(dalloc(&S.x, (size_t)2 * n));
    hipLaunchKernelGGL(k_cat_ptr, dim3(blocks_for((int64_t)n + 1)), dim3(256), 0, s, n, A->p, B->p, cat.p);
    hipLaunchKernelGGL(k_selector, dim3(blocks_for((int64_t)n + 1)), dim3(256), 0, s, n, 1, alpha, beta, S.p, S.i, S.x);
    if (A->nnz) CSX_HIP(hipMemcpyAsync(cat.i, A->i, (size_t)A->nnz * 4, hipMemcpyDeviceToDevice, s));
    if (B->nnz) CSX_HIP(hipMemcpyAsync(cat.i + A->nnz, B->i, (size_t)B->nnz * 4, hipMemcpyDeviceToDevice, s));
    if (values && A->nnz) CSX_HIP(hipMemcpyAsync(cat.x, A->x, (size_t)A->nnz * 8, hipMemcpyDeviceToDevice, s));
    if (values && B->nnz) CSX_HIP(hipMemcpyAsync(cat.x + A->nnz, B->x, (size_t)B->nnz * 8, hipMemcpyDeviceToDevice, s));
    return multiply_device(&cat, &S, C);   // (synchronises: cat and S go back to the pool with nothing queued on them)
}

static int dupl_device(const Csc *A, Csc *C) {
    hipStream_t s = ctx().stream;
    Csc I;
    I.m = I.n = A->n;
    I.nnz = A->n;
    CSX_TRY(dalloc(&I.p, (size_t)A->n + 1));
    CSX_TRY(dalloc(&I.i, (size_t)A->n));
    if (A->x) CSX_TRY(dalloc(&I.x, (size_t)A->n));
    hipLaunchKernelGGL(k_selector, dim3(blocks_for((int64_t)A->n + 1)), dim3(256), 0, s, A->n, 0, 1.0, 0.0, I.p, I.i, I.x);
    return multiply_device(A, &I, C);
}

// ---- order-preserving filters --------------------------------------------------------------------------
enum { KEEP_NONZERO = 0, KEEP_ABOVE_TOL = 1, KEEP_UPPER = 2 };

__device__ __forceinline__ bool keep_entry(int mode, double tol, int32_t i, int32_t j, double a) {
    if (mode == KEEP_NONZERO) return a != 0;
    if (mode == KEEP_ABOVE_TOL) return fabs(a) > tol;
    return i <= j;
}

// one wave per column; FILL = false: cnt[j] = kept entries; FILL = true: write them at optr[j] in order.
// For KEEP_UPPER the outputs are the renamed (row, column-key) pairs of cs_symperm instead of (row, value).
template <bool FILL>
__global__ __launch_bounds__(256) void k_filter(int32_t n, int mode, double tol, const int32_t *__restrict__ Ap,
                                                const int32_t *__restrict__ Ai, const double *__restrict__ Ax,
                                                const int32_t *__restrict__ pinv, int32_t *__restrict__ cnt,
                                                const int32_t *__restrict__ optr, int32_t *__restrict__ oi,
                                                double *__restrict__ ox, uint32_t *__restrict__ okey) {
    const int lane = threadIdx.x & 63;
    const int64_t j = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (j >= n) return;
    const int32_t b = Ap[j], e = Ap[j + 1];
    int32_t run = FILL ? optr[j] : 0;
    const int32_t j2 = (mode == KEEP_UPPER && pinv) ? pinv[j] : (int32_t)j;
    for (int32_t p0 = b; p0 < e; p0 += 64) {
        const int32_t p = p0 + lane;
        bool keep = false;
        int32_t i = 0;
        double a = 1.0;
        if (p < e) {
            i = Ai[p];
            if (Ax) a = Ax[p];
            keep = keep_entry(mode, tol, i, (int32_t)j, a);
        }
        const unsigned long long bal = __ballot(keep);
        if (FILL && keep) {
            const int32_t q = run + __popcll(bal & ((1ull << lane) - 1ull));
            if (mode == KEEP_UPPER) {
                const int32_t i2 = pinv ? pinv[i] : i;
                oi[q] = i2 < j2 ? i2 : j2;
                okey[q] = (uint32_t)(i2 > j2 ? i2 : j2);
            } else {
                oi[q] = i;
            }
            if (ox) ox[q] = a;
        }
        run += __popcll(bal);
    }
    if (!FILL && lane == 0) cnt[j] = run;
}

static int drop_device(const Csc *A, int mode, double tol, Csc *C) {
    hipStream_t s = ctx().stream;
    const int32_t n = A->n;
    C->m = A->m;
    C->n = n;
    C->owns = true;
    DevBuf<int32_t> cnt;
    int64_t total = 0;
    CSX_TRY(cnt.alloc((size_t)n + 1));
    CSX_TRY(dalloc(&C->p, (size_t)n + 1));
    if (n) hipLaunchKernelGGL(k_filter<false>, dim3(blocks_for((int64_t)n * 64)), dim3(256), 0, s, n, mode, tol, A->p, A->i, A->x,
                              nullptr, cnt, nullptr, nullptr, nullptr, nullptr);
    CSX_TRY(scan_exclusive_i32(cnt, C->p, n, &total));
    C->nnz = (int32_t)total;
    CSX_TRY(dalloc(&C->i, (size_t)total));
    if (A->x) CSX_TRY(dalloc(&C->x, (size_t)total));
    if (n)
        hipLaunchKernelGGL(k_filter<true>, dim3(blocks_for((int64_t)n * 64)), dim3(256), 0, s, n, mode, tol, A->p, A->i, A->x, nullptr,
                           nullptr, C->p, C->i, C->x, nullptr);
    CSX_HIP(hipStreamSynchronize(s));
    return CSX_OK;
}

static int symperm_device(const Csc *A, const int32_t *pinv_h, bool values, Csc *C) {
    hipStream_t s = ctx().stream;
    const int32_t n = A->n;
    const bool with_values = values && A->x;
    C->m = C->n = n;
    C->owns = true;
    DevBuf<int32_t> pinv, cnt, optr, ri;
    DevBuf<uint32_t> key, skey;
    DevBuf<double> rx;
    int64_t total = 0;
    if (pinv_h) CSX_TRY(upload(pinv, pinv_h, (size_t)n));
    CSX_TRY(cnt.alloc((size_t)n + 1));
    CSX_TRY(optr.alloc((size_t)n + 1));
    CSX_TRY(dalloc(&C->p, (size_t)n + 1));
    if (n) hipLaunchKernelGGL(k_filter<false>, dim3(blocks_for((int64_t)n * 64)), dim3(256), 0, s, n, (int)KEEP_UPPER, 0.0, A->p, A->i,
                              nullptr, pinv, cnt, nullptr, nullptr, nullptr, nullptr);
    CSX_TRY(scan_exclusive_i32(cnt, optr, n, &total));
    C->nnz = (int32_t)total;
    CSX_TRY(dalloc(&C->i, (size_t)total));
    if (with_values) CSX_TRY(dalloc(&C->x, (size_t)total));
    CSX_TRY(ri.alloc((size_t)total));
    CSX_TRY(key.alloc((size_t)total));
    CSX_TRY(skey.alloc((size_t)total));
    if (with_values) CSX_TRY(rx.alloc((size_t)total));
    if (total > 0) {
        hipLaunchKernelGGL(k_filter<true>, dim3(blocks_for((int64_t)n * 64)), dim3(256), 0, s, n, (int)KEEP_UPPER, 0.0, A->p, A->i,
                           with_values ? A->x : nullptr, pinv, nullptr, optr, ri, rx, key);
        CSX_TRY(stable_sort_by_key(key, (const uint32_t *)ri.get(), rx, total, (uint32_t)n, skey, (uint32_t *)C->i, C->x));
        CSX_TRY(boundaries_from_sorted(skey, total, n, C->p));
    } else {
        CSX_HIP(hipMemsetAsync(C->p, 0, ((size_t)n + 1) * sizeof(int32_t), s));
    }
    CSX_HIP(hipStreamSynchronize(s));
    return CSX_OK;
}

// ---- cs_permute ----------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_perm_len(int32_t n, const int32_t *__restrict__ Ap, const int32_t *__restrict__ q,
                                                  int32_t *__restrict__ len) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const int32_t j = q ? q[k] : (int32_t)k;
    len[k] = Ap[j + 1] - Ap[j];
}

__global__ __launch_bounds__(256) void k_perm_fill(int32_t n, const int32_t *__restrict__ Ap, const int32_t *__restrict__ Ai,
                                                   const double *__restrict__ Ax, const int32_t *__restrict__ pinv,
                                                   const int32_t *__restrict__ q, const int32_t *__restrict__ Cp,
                                                   int32_t *__restrict__ Ci, double *__restrict__ Cx) {
    const int lane = threadIdx.x & 63;
    const int64_t k = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (k >= n) return;
    const int32_t j = q ? q[k] : (int32_t)k;
    const int32_t b = Ap[j], len = Ap[j + 1] - b, o = Cp[k];
    for (int32_t t = lane; t < len; t += 64) {
        const int32_t i = Ai[b + t];
        Ci[o + t] = pinv ? pinv[i] : i;
        if (Cx) Cx[o + t] = Ax[b + t];
    }
}

static int permute_device(const Csc *A, const int32_t *pinv_h, const int32_t *q_h, bool values, Csc *C) {
    hipStream_t s = ctx().stream;
    const int32_t n = A->n;
    const bool with_values = values && A->x;
    C->m = A->m;
    C->n = n;
    C->nnz = A->nnz;
    C->owns = true;
    DevBuf<int32_t> pinv, q, len;
    if (pinv_h) CSX_TRY(upload(pinv, pinv_h, (size_t)A->m));
    if (q_h) CSX_TRY(upload(q, q_h, (size_t)n));
    CSX_TRY(len.alloc((size_t)n + 1));
    CSX_TRY(dalloc(&C->p, (size_t)n + 1));
    CSX_TRY(dalloc(&C->i, (size_t)A->nnz));
    if (with_values) CSX_TRY(dalloc(&C->x, (size_t)A->nnz));
    if (n) hipLaunchKernelGGL(k_perm_len, dim3(blocks_for(n)), dim3(256), 0, s, n, A->p, q, len);
    CSX_TRY(scan_exclusive_i32(len, C->p, n, nullptr));
    if (n)
        hipLaunchKernelGGL(k_perm_fill, dim3(blocks_for((int64_t)n * 64)), dim3(256), 0, s, n, A->p, A->i, with_values ? A->x : nullptr,
                           pinv, q, C->p, C->i, C->x);
    CSX_HIP(hipStreamSynchronize(s));
    return CSX_OK;
}

// ---- cs_compress ---------------------------------------------------------------------------------------
static int compress_device(int32_t m, int32_t n, int64_t nz, const int32_t *Ti, const int32_t *Tj, const double *Tx, Csc *C) {
    hipStream_t s = ctx().stream;
    C->m = m;
    C->n = n;
    C->nnz = (int32_t)nz;
    C->owns = true;
    CSX_TRY(dalloc(&C->p, (size_t)n + 1));
    CSX_TRY(dalloc(&C->i, (size_t)nz));
    if (Tx) CSX_TRY(dalloc(&C->x, (size_t)nz));
    if (nz == 0) {
        CSX_HIP(hipMemsetAsync(C->p, 0, ((size_t)n + 1) * sizeof(int32_t), s));
        CSX_HIP(hipStreamSynchronize(s));
        return CSX_OK;
    }
    DevBuf<int32_t> di, dj;
    DevBuf<uint32_t> skey;
    DevBuf<double> dx;
    CSX_TRY(upload(di, Ti, (size_t)nz));
    CSX_TRY(upload(dj, Tj, (size_t)nz));
    if (Tx) CSX_TRY(upload(dx, Tx, (size_t)nz));
    CSX_TRY(skey.alloc((size_t)nz));
    CSX_TRY(stable_sort_by_key((const uint32_t *)dj.get(), (const uint32_t *)di.get(), dx, nz, (uint32_t)n, skey, (uint32_t *)C->i,
                               C->x));
    CSX_TRY(boundaries_from_sorted(skey, nz, n, C->p));
    CSX_HIP(hipStreamSynchronize(s));
    return CSX_OK;
}

// ---- column block (sharding a matrix by columns) ---------------------------------------------
__global__ __launch_bounds__(256) void k_shift_ptr(int32_t count, const int32_t *__restrict__ Ap, int32_t first,
                                                   int32_t *__restrict__ p) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j <= count) p[j] = Ap[first + j] - Ap[first];
}

int col_block_device(const Csc *A, int32_t first, int32_t count, Csc *C) {
    hipStream_t s = ctx().stream;
    int32_t ends[2] = {0, 0};
    CSX_HIP(hipMemcpyAsync(&ends[0], A->p + first, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    CSX_HIP(hipMemcpyAsync(&ends[1], A->p + first + count, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    CSX_HIP(hipStreamSynchronize(s));
    const int32_t nnz = ends[1] - ends[0];
    C->m = A->m;
    C->n = count;
    C->nnz = nnz;
    C->owns = true;
    CSX_TRY(dalloc(&C->p, (size_t)count + 1));
    CSX_TRY(dalloc(&C->i, (size_t)nnz));
    if (A->x) CSX_TRY(dalloc(&C->x, (size_t)nnz));
    hipLaunchKernelGGL(k_shift_ptr, dim3(blocks_for((int64_t)count + 1)), dim3(256), 0, s, count, A->p, first, C->p);
    if (nnz) CSX_HIP(hipMemcpyAsync(C->i, A->i + ends[0], (size_t)nnz * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    if (nnz && A->x) CSX_HIP(hipMemcpyAsync(C->x, A->x + ends[0], (size_t)nnz * sizeof(double), hipMemcpyDeviceToDevice, s));
    CSX_HIP(hipStreamSynchronize(s));
    return CSX_OK;
}

// ---- cs_norm (csparse.py:1647-1663): largest column sum of |a| -------------------------------------------
// One thread per column, entries added in storage order: every column sum, hence the maximum, has the
// reference's bits.  Non-negative doubles order like their bit patterns, so the maximum is an integer atomic.
__global__ __launch_bounds__(256) void k_norm1(int32_t n, const int32_t *__restrict__ Ap, const double *__restrict__ Ax,
                                               unsigned long long *best) {
#pragma clang fp contract(off)
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    double sum = 0.0;
    for (int32_t p = Ap[j]; p < Ap[j + 1]; p++) sum += fabs(Ax[p]);
    if (sum == sum) atomicMax(best, (unsigned long long)__double_as_longlong(sum));
    else atomicMax(best + 1, 1ull);   // a NaN column: max(best, NaN) in the reference keeps `best`; remembered only for the caller
}

template <class F>
static int make_csc(csx_handle_t *out, F &&build) {
    std::unique_ptr<Csc> C(new Csc());
    CSX_TRY(build(C.get()));
    *out = put(K_CSC, C.release());
    return CSX_OK;
}

}  // namespace csx

using namespace csx;

extern "C" int csx_compress(int32_t m, int32_t n, int64_t nz, const int32_t *Ti, const int32_t *Tj, const double *Tx,
                            csx_handle_t *out) {
    CSX_TRY(require_ready());
    if (m < 0 || n < 0 || nz < 0 || nz > 0x7FFFFFFFll || !out || (nz > 0 && (!Ti || !Tj))) return CSX_EINVAL;
    for (int64_t k = 0; k < nz; k++)
        if (Tj[k] < 0 || Tj[k] >= n || Ti[k] < 0 || Ti[k] >= m) return CSX_EINVAL;   // the reference would raise IndexError
    return make_csc(out, [&](Csc *C) { return compress_device(m, n, nz, Ti, Tj, Tx, C); });
}

extern "C" int csx_add(csx_handle_t hA, csx_handle_t hB, double alpha, double beta, csx_handle_t *out) {
    CSX_TRY(require_ready());
    Csc *A = csc(hA), *B = csc(hB);
    if (!A || !B || !out || A->m != B->m || A->n != B->n) return CSX_EINVAL;
    return make_csc(out, [&](Csc *C) { return add_device(A, B, alpha, beta, C); });
}

extern "C" int csx_dupl(csx_handle_t hA, csx_handle_t *out) {
    CSX_TRY(require_ready());
    Csc *A = csc(hA);
    if (!A || !out) return CSX_EINVAL;
    return make_csc(out, [&](Csc *C) { return dupl_device(A, C); });
}

extern "C" int csx_drop(csx_handle_t hA, int mode, double tol, csx_handle_t *out) {
    CSX_TRY(require_ready());
    Csc *A = csc(hA);
    if (!A || !out || !A->x || (mode != KEEP_NONZERO && mode != KEEP_ABOVE_TOL)) return CSX_EINVAL;
    return make_csc(out, [&](Csc *C) { return drop_device(A, mode, tol, C); });
}

extern "C" int csx_permute(csx_handle_t hA, const int32_t *pinv, const int32_t *q, int values, csx_handle_t *out) {
    CSX_TRY(require_ready());
    Csc *A = csc(hA);
    if (!A || !out) return CSX_EINVAL;
    if (pinv)
        for (int32_t k = 0; k < A->m; k++)
            if (pinv[k] < 0) return CSX_EINVAL;
    if (q)
        for (int32_t k = 0; k < A->n; k++)
            if (q[k] < 0 || q[k] >= A->n) return CSX_EINVAL;
    return make_csc(out, [&](Csc *C) { return permute_device(A, pinv, q, values != 0, C); });
}

extern "C" int csx_symperm(csx_handle_t hA, const int32_t *pinv, int values, csx_handle_t *out) {
    CSX_TRY(require_ready());
    Csc *A = csc(hA);
    if (!A || !out || A->m != A->n) return CSX_EINVAL;
    if (pinv && !is_permutation(pinv, A->n)) return CSX_EINVAL;
    return make_csc(out, [&](Csc *C) { return symperm_device(A, pinv, values != 0, C); });
}

extern "C" int csx_csc_col_block(csx_handle_t hA, int32_t first, int32_t count, csx_handle_t *out) {
    CSX_TRY(require_ready());
    Csc *A = csc(hA);
    if (!A || !out || first < 0 || count < 0 || (int64_t)first + count > A->n) return CSX_EINVAL;
    return make_csc(out, [&](Csc *C) { return col_block_device(A, first, count, C); });
}

extern "C" int csx_norm1(csx_handle_t hA, double *out) {
    CSX_TRY(require_ready());
    Csc *A = csc(hA);
    if (!A || !out || !A->x) return CSX_EINVAL;
    hipStream_t s = ctx().stream;
    DevBuf<unsigned long long> d;
    unsigned long long h[2] = {0, 0};
    CSX_TRY(d.alloc(2));
    CSX_HIP(hipMemsetAsync(d, 0, 2 * sizeof(unsigned long long), s));
    if (A->n > 0) hipLaunchKernelGGL(k_norm1, dim3(blocks_for(A->n)), dim3(256), 0, s, A->n, A->p, A->x, d);
    CSX_HIP(hipMemcpyAsync(h, d, sizeof h, hipMemcpyDeviceToHost, s));
    CSX_HIP(hipStreamSynchronize(s));
    double v;
    std::memcpy(&v, &h[0], sizeof v);
    *out = v;
    return CSX_OK;
}
