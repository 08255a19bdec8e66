// Multiply plan (the definition is the comment of csx_multiply_plan in include/csx.h): the patterns of A and B
// stay from step to step, only their values change.  Which products A.x[ia] B.x[ib] land in which entry of C = cs_multiply(A, B)
// and in which order the reference adds them is found once, on the host, by the reference's own two loops on the indices
// (csx_host.cpp: csx_multiply_plan_host).  A step is then ONE launch over the values:
//
//     C.x[s] = ((b0 a0) + b1 a1) + b2 a2 + ...      over (ia, ib) = pair[sp[s] .. sp[s + 1]), the first term assigned
//
// -- the reference's bits: every product rounded on its own and never fused with the addition that follows, no atomics, no
// hash table, no reassociation.  Two classes of work, one kernel, shaped like k_assemble (csx_assemble_plan.hip):
//   * short slots: one lane per slot; adjacent lanes read adjacent stretches of pair (8-byte loads), the gathers of up to four
//     products are in flight together, the multiplies and additions follow in order;
//   * long slots (more than `thr` products, Options::multiply_long): one WAVE per slot.  The wave loads 64 pairs per step --
//     coalesced on pair, the 128 gathers in flight together, the next step's already issued -- every lane forms its own term
//     (exact: a term is a single rounding whoever computes it), and the terms are added in index order through v_readlane,
//     every lane keeping the same running sum.  The blocks of the long slots come FIRST in the grid.
// C = A diag(d) B is by definition cs_multiply(A, B2) with B2.x[p] = d[B.i[p]] * B.x[p]: an elementwise kernel over nnz(B)
// writes B2.x into a scratch vector of the plan and the same fold reads it in place of B.x.
#include <algorithm>
#include <chrono>

#include "csx_internal.h"

// every multiply below is rounded before the addition that takes it (the build's default contracts a * b + c into one FMA)
#pragma clang fp contract(off)

namespace csx {

int32_t multiply_slot_stats(int32_t nnz, const int32_t *sp, int32_t thr, std::vector<int32_t> *longs);

constexpr int MUL_WAVES = 4;   // waves per workgroup; a long slot takes one of them

struct MulPlan {
    int32_t m = 0, k = 0, n = 0, anz = 0, bnz = 0, nnz = 0, products = 0;
    int32_t thr = 0, max_len = 0, nlong = 0;
    DevBuf<int32_t> p, i;       // the pattern of C
    DevBuf<int32_t> sp, pair;   // slot pointers; (ia, ib) of every product, grouped by slot
    DevBuf<int32_t> longs;      // the long slots, ascending
    DevBuf<int32_t> bi;         // B.i (the scale reads it; Bx may come as a bare vector)
    DevBuf<double> b2;          // d[B.i[p]] * B.x[p], made by the first scaled step, kept
    int64_t build_us = 0;
    hipEvent_t e0 = nullptr, e1 = nullptr;   // around the last step
    bool timed = false;
    MulPlan() = default;
    MulPlan(const MulPlan &) = delete;
    MulPlan &operator=(const MulPlan &) = delete;
    ~MulPlan() {
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
    }
};

void destroy(MulPlan *P) { delete P; }

__device__ __forceinline__ double mp_readlane_f64(double v, int k) {   // k: the same in every lane
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), k);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), k);
    return __hiloint2double(hi, lo);
}

__global__ __launch_bounds__(256) void k_multiply_scale(int32_t bnz, const int32_t *__restrict__ Bi, const double *__restrict__ Bx,
                                                        const double *__restrict__ d, double *__restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t < bnz) out[t] = d[Bi[t]] * Bx[t];
}

__global__ __launch_bounds__(64 * MUL_WAVES) void k_multiply_fold(int32_t nnz, int32_t thr, int32_t nlong,
                                                                  const int32_t *__restrict__ longs,
                                                                  const int32_t *__restrict__ sp, const int2 *__restrict__ pair,
                                                                  const double *__restrict__ Ax, const double *__restrict__ Bx,
                                                                  double *__restrict__ out) {
    const int32_t long_blocks = (nlong + MUL_WAVES - 1) / MUL_WAVES;
    if ((int32_t)blockIdx.x < long_blocks) {
        const int lane = threadIdx.x & 63;
        // (the wave's own number, told to the compiler as the scalar it is: the slot's bounds and the fold's counters stay scalar)
        const int32_t w = (int32_t)blockIdx.x * MUL_WAVES + __builtin_amdgcn_readfirstlane((int32_t)(threadIdx.x >> 6));
        if (w >= nlong) return;
        const int32_t s = longs[w], a = sp[s], e = sp[s + 1];
        double v = 0.0;
        if ((int64_t)a + lane < e) {
            const int2 q = pair[a + lane];
            v = Bx[q.y] * Ax[q.x];
        }
        double acc = 0.0;
        for (int64_t b = a; b < e; b += 64) {   // (64-bit: a slot may end within a step of 2^31 - 1)
            const int64_t tn = b + 64 + lane;
            double vn = 0.0;
            if (tn < e) {   // the next step's loads fly while this step adds
                const int2 q = pair[tn];
                vn = Bx[q.y] * Ax[q.x];
            }
            const int cnt = (int)min((int64_t)64, e - b);
            const double first = mp_readlane_f64(v, 0);
            acc = b == a ? first : acc + first;   // the first term of a slot is assigned
            if (cnt == 64) {
#pragma unroll
                for (int k = 1; k < 64; k++) acc = acc + mp_readlane_f64(v, k);
            } else {
                for (int k = 1; k < cnt; k++) acc = acc + mp_readlane_f64(v, k);
            }
            v = vn;
        }
        if (lane == 0) out[s] = acc;
        return;
    }
    const int64_t s = (int64_t)(blockIdx.x - long_blocks) * (64 * MUL_WAVES) + threadIdx.x;
    if (s >= nnz) return;
    const int32_t a = sp[s], e = sp[s + 1];
    if (e - a > thr) return;   // a wave's
    const int2 q = pair[a];
    double acc = Bx[q.y] * Ax[q.x];
    int64_t t = (int64_t)a + 1;
    for (; t + 4 <= e; t += 4) {
        const int2 q0 = pair[t], q1 = pair[t + 1], q2 = pair[t + 2], q3 = pair[t + 3];
        const double a0 = Ax[q0.x], a1 = Ax[q1.x], a2 = Ax[q2.x], a3 = Ax[q3.x];
        const double b0 = Bx[q0.y], b1 = Bx[q1.y], b2 = Bx[q2.y], b3 = Bx[q3.y];
        const double t0 = b0 * a0, t1 = b1 * a1, t2 = b2 * a2, t3 = b3 * a3;
        acc = acc + t0;
        acc = acc + t1;
        acc = acc + t2;
        acc = acc + t3;
    }
    for (; t < e; t++) {
        const int2 qt = pair[t];
        const double term = Bx[qt.y] * Ax[qt.x];
        acc = acc + term;
    }
    out[s] = acc;
}

// out[0 .. nnz) <- the fold of Ax, Bx (Bx scaled by d first when d is given); queued on the context's stream between the
// plan's two events
static int multiply_launch(MulPlan *P, const double *Ax, const double *Bx, const double *d, double *out) {
    hipStream_t s = ctx().stream;
    if (d && P->bnz > 0 && !P->b2.get()) CSX_TRY(P->b2.alloc((size_t)P->bnz));
    CSX_HIP(hipEventRecord(P->e0, s));
    if (P->nnz > 0) {
        if (d) {
            hipLaunchKernelGGL(k_multiply_scale, dim3((unsigned)(((int64_t)P->bnz + 255) / 256)), dim3(256), 0, s, P->bnz,
                               P->bi.get(), Bx, d, P->b2.get());
            Bx = P->b2.get();
        }
        const int64_t blocks = (P->nlong + MUL_WAVES - 1) / MUL_WAVES + ((int64_t)P->nnz + 64 * MUL_WAVES - 1) / (64 * MUL_WAVES);
        hipLaunchKernelGGL(k_multiply_fold, dim3((unsigned)blocks), dim3(64 * MUL_WAVES), 0, s, P->nnz, P->thr, P->nlong,
                           P->longs.get(), P->sp.get(), (const int2 *)P->pair.get(), Ax, Bx, out);
        CSX_LAUNCH_CHECK();
    }
    CSX_HIP(hipEventRecord(P->e1, s));
    P->timed = true;
    return CSX_OK;
}

// The values an operand handle stands for: a CSC handle with values and the operand's shape and entry count (its pattern is NOT
// compared), or a vector of exactly nz doubles.  null: neither.
static const double *operand_values(csx_handle_t h, int32_t rows, int32_t cols, int32_t nz) {
    if (Csc *M = csc(h)) return (M->x && M->m == rows && M->n == cols && M->nnz == nz) ? M->x : nullptr;
    if (Vec *v = vec(h)) return v->len == nz ? (const double *)v->d : nullptr;
    return nullptr;
}

// Ax, Bx, d of a step, checked; d stays null when hd is 0
static int multiply_inputs(const MulPlan *P, csx_handle_t hAx, csx_handle_t hBx, csx_handle_t hd, const double **Ax,
                           const double **Bx, const double **d) {
    *Ax = operand_values(hAx, P->m, P->k, P->anz);
    *Bx = operand_values(hBx, P->k, P->n, P->bnz);
    *d = nullptr;
    if (!*Ax || !*Bx) return CSX_EINVAL;
    if (hd) {
        Vec *v = vec(hd);
        if (!v || v->len < P->k) return CSX_EINVAL;
        *d = (const double *)v->d;
    }
    return CSX_OK;
}

}  // namespace csx

using namespace csx;

extern "C" int csx_multiply_plan(csx_handle_t hA, csx_handle_t hB, csx_handle_t *out) {
    CSX_TRY(require_ready());
    Csc *A = csc(hA), *B = csc(hB);
    if (!A || !B || !out || A->n != B->m) {
        set_error("csx_multiply_plan: needs two CSC matrices with A.n == B.m");
        return CSX_EINVAL;
    }
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<int32_t> Ap, Ai, Bp, Bi;
    CSX_TRY(download_i32(Ap, A->p, (size_t)A->n + 1));
    CSX_TRY(download_i32(Ai, A->i, (size_t)A->nnz));
    CSX_TRY(download_i32(Bp, B->p, (size_t)B->n + 1));
    CSX_TRY(download_i32(Bi, B->i, (size_t)B->nnz));
    int64_t nnz = 0, products = 0;
    if (Ap[A->n] != A->nnz || Bp[B->n] != B->nnz ||
        csx_multiply_plan_count(A->m, A->n, B->n, Ap.data(), Ai.data(), Bp.data(), Bi.data(), &nnz, &products) != CSX_OK) {
        set_error("csx_multiply_plan: an operand's pointers or row indices are out of range");
        return CSX_EINVAL;
    }
    if (products > INT32_MAX) {
        set_error("csx_multiply_plan: %lld products do not fit the plan's int32 pointers", (long long)products);
        return CSX_EINVAL;
    }
    std::vector<int32_t> Cp((size_t)B->n + 1), Ci((size_t)nnz), sp((size_t)nnz + 1), pair(2 * (size_t)products);
    CSX_TRY(csx_multiply_plan_host(A->m, A->n, B->n, Ap.data(), Ai.data(), Bp.data(), Bi.data(), Cp.data(), Ci.data(), sp.data(),
                                   pair.data()));
    std::unique_ptr<MulPlan> P(new MulPlan());
    P->m = A->m;
    P->k = A->n;
    P->n = B->n;
    P->anz = A->nnz;
    P->bnz = B->nnz;
    P->nnz = (int32_t)nnz;
    P->products = (int32_t)products;
    P->thr = ctx().opt.multiply_long;
    std::vector<int32_t> longs;
    P->max_len = multiply_slot_stats(P->nnz, sp.data(), P->thr, &longs);
    P->nlong = (int32_t)longs.size();
    P->build_us = std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
    CSX_TRY(upload(P->p, Cp));
    CSX_TRY(upload(P->i, Ci));
    CSX_TRY(upload(P->sp, sp));
    CSX_TRY(upload(P->pair, pair));
    CSX_TRY(upload(P->longs, longs));
    CSX_TRY(upload(P->bi, Bi));
    CSX_HIP(hipEventCreate(&P->e0));
    CSX_HIP(hipEventCreate(&P->e1));
    CSX_HIP(hipStreamSynchronize(ctx().stream));   // the host arrays go out of scope
    *out = put(K_MULPLAN, P.release());
    return CSX_OK;
}

extern "C" int csx_multiply_plan_run(csx_handle_t h, csx_handle_t hAx, csx_handle_t hBx, csx_handle_t hd, csx_handle_t hout) {
    CSX_TRY(require_ready());
    MulPlan *P = (MulPlan *)get(h, K_MULPLAN);
    if (!P) return CSX_EINVAL;
    const double *Ax, *Bx, *d;
    CSX_TRY(multiply_inputs(P, hAx, hBx, hd, &Ax, &Bx, &d));
    double *x = nullptr;
    Csc *C = nullptr;
    if (Vec *o = vec(hout)) {
        if (o->len < P->nnz) return CSX_EINVAL;
        x = (double *)o->d;
    } else {
        C = csc(hout);
        if (!C || !C->x || C->m != P->m || C->n != P->n || C->nnz != P->nnz) return CSX_EINVAL;
        x = C->x;
    }
    if (x == Ax || x == Bx || x == d) return CSX_EINVAL;   // out aliases no input
    CSX_TRY(multiply_launch(P, Ax, Bx, d, x));
    if (C) {
        C->rows.reset();    // the SpMV plans cached on the matrix hold copies of the old values
        C->tiled.reset();
    }
    return CSX_OK;
}

extern "C" int csx_multiply_plan_matrix(csx_handle_t h, csx_handle_t hAx, csx_handle_t hBx, csx_handle_t hd, csx_handle_t *out) {
    CSX_TRY(require_ready());
    MulPlan *P = (MulPlan *)get(h, K_MULPLAN);
    if (!P || !out) return CSX_EINVAL;
    const bool values = hAx || hBx;
    const double *Ax = nullptr, *Bx = nullptr, *d = nullptr;
    if (values) CSX_TRY(multiply_inputs(P, hAx, hBx, hd, &Ax, &Bx, &d));
    hipStream_t s = ctx().stream;
    std::unique_ptr<Csc> C(new Csc());
    C->m = P->m;
    C->n = P->n;
    C->nnz = P->nnz;
    CSX_TRY(dalloc(&C->p, (size_t)P->n + 1));
    CSX_TRY(dalloc(&C->i, (size_t)P->nnz));
    if (values) CSX_TRY(dalloc(&C->x, (size_t)P->nnz));
    CSX_HIP(hipMemcpyAsync(C->p, P->p.get(), ((size_t)P->n + 1) * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    if (P->nnz) CSX_HIP(hipMemcpyAsync(C->i, P->i.get(), (size_t)P->nnz * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    if (values) CSX_TRY(multiply_launch(P, Ax, Bx, d, C->x));
    *out = put(K_CSC, C.release());
    return CSX_OK;
}

extern "C" int csx_multiply_plan_info(csx_handle_t h, int64_t *info) {
    CSX_TRY(require_ready());
    MulPlan *P = (MulPlan *)get(h, K_MULPLAN);
    if (!P || !info) return CSX_EINVAL;
    info[0] = P->m;
    info[1] = P->n;
    info[2] = P->nnz;
    info[3] = P->products;
    info[4] = P->max_len;
    info[5] = P->nlong;
    info[6] = P->build_us;
    info[7] = 0;
    if (P->timed) {
        float ms = 0.f;
        CSX_HIP(hipEventSynchronize(P->e1));
        CSX_HIP(hipEventElapsedTime(&ms, P->e0, P->e1));
        info[7] = (int64_t)(1e3 * (double)ms + 0.5);
    }
    return CSX_OK;
}
