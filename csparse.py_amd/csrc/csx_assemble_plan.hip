// Assembly plan (the definition is the comment of csx_assemble_plan in include/csx.h): the triplets (Ti, Tj) of a
// matrix keep their places from step to step, only their values change.  Where every triplet lands in
// C = cs_dupl(cs_compress(T)) and in which order the duplicates of a slot are added is found once, on the host, by the
// reference's own two loops (csx_host.cpp: csx_assemble_plan_host).  A step is then ONE launch over the values:
//
//     C.x[s] = ((Tx[t0] + Tx[t1]) + Tx[t2]) + ...      over t = src[sp[s] .. sp[s + 1]), the first term assigned
//
// -- the reference's bits: no atomics, no reassociation, no multiply.  Three classes of work, one kernel:
//   * no duplicates at all (nz == nnz): a permuted copy out[s] = Tx[src[s]] that never reads sp (k_assemble_copy);
//   * short slots: one lane per slot; adjacent lanes read adjacent stretches of src, the gathers of up to four terms are in
//     flight together, the additions follow in order;
//   * long slots (more than `thr` terms, Options::assemble_long): one WAVE per slot.  A lane walking such a slot alone would
//     pay a chain of dependent random loads with 63 lanes idle.  The wave loads 64 sources per step -- coalesced on src, the
//     64 gathers in flight together, the next step's already issued -- and adds them in index order through v_readlane, every
//     lane keeping the same running sum.  The sum itself stays the serial chain the definition makes it.  The blocks of the
//     long slots come FIRST in the grid, so the longest chains start first and run beside the short slots.
#include <algorithm>
#include <chrono>

#include "csx_internal.h"

namespace csx {

int32_t assemble_slot_stats(int32_t nnz, const int32_t *sp, int32_t thr, std::vector<int32_t> *longs);

constexpr int ASM_WAVES = 4;   // waves per workgroup; a long slot takes one of them

struct AsmPlan {
    int32_t m = 0, n = 0, nz = 0, nnz = 0;
    int32_t thr = 0, max_dup = 0, nlong = 0;
    DevBuf<int32_t> p, i;       // the pattern of C
    DevBuf<int32_t> sp, src;    // slot pointers (null when nz == nnz: never read), triplets grouped by slot
    DevBuf<int32_t> longs;      // the long slots, ascending
    int64_t build_us = 0;
    hipEvent_t e0 = nullptr, e1 = nullptr;   // around the last launch
    bool timed = false;
    AsmPlan() = default;
    AsmPlan(const AsmPlan &) = delete;
    AsmPlan &operator=(const AsmPlan &) = delete;
    ~AsmPlan() {
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
    }
};

void destroy(AsmPlan *P) { delete P; }

__global__ __launch_bounds__(256) void k_assemble_copy(int32_t nnz, const int32_t *__restrict__ src,
                                                       const double *__restrict__ Tx, double *__restrict__ out) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s < nnz) out[s] = Tx[src[s]];
}

__device__ __forceinline__ double readlane_f64(double v, int k) {   // k: the same in every lane
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), k);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), k);
    return __hiloint2double(hi, lo);
}

__global__ __launch_bounds__(64 * ASM_WAVES) void k_assemble(int32_t nnz, int32_t thr, int32_t nlong,
                                                             const int32_t *__restrict__ longs,
                                                             const int32_t *__restrict__ sp, const int32_t *__restrict__ src,
                                                             const double *__restrict__ Tx, double *__restrict__ out) {
    const int32_t long_blocks = (nlong + ASM_WAVES - 1) / ASM_WAVES;
    if ((int32_t)blockIdx.x < long_blocks) {
        const int lane = threadIdx.x & 63;
        // (the wave's own number, told to the compiler as the scalar it is: the slot's bounds and the fold's counters stay scalar)
        const int32_t w = (int32_t)blockIdx.x * ASM_WAVES + __builtin_amdgcn_readfirstlane((int32_t)(threadIdx.x >> 6));
        if (w >= nlong) return;
        const int32_t s = longs[w], a = sp[s], e = sp[s + 1];
        double v = (int64_t)a + lane < e ? Tx[src[a + lane]] : 0.0;
        double acc = 0.0;
        for (int64_t b = a; b < e; b += 64) {   // (64-bit: a slot may end within a step of 2^31 - 1)
            const int64_t tn = b + 64 + lane;
            const double vn = tn < e ? Tx[src[tn]] : 0.0;   // the next step's gathers fly while this step adds
            const int cnt = (int)min((int64_t)64, e - b);
            const double first = readlane_f64(v, 0);
            acc = b == a ? first : acc + first;   // the first term of a slot is assigned
            if (cnt == 64) {
#pragma unroll
                for (int k = 1; k < 64; k++) acc = acc + readlane_f64(v, k);
            } else {
                for (int k = 1; k < cnt; k++) acc = acc + readlane_f64(v, k);
            }
            v = vn;
        }
        if (lane == 0) out[s] = acc;
        return;
    }
    const int64_t s = (int64_t)(blockIdx.x - long_blocks) * (64 * ASM_WAVES) + threadIdx.x;
    if (s >= nnz) return;
    const int32_t a = sp[s], e = sp[s + 1];
    if (e - a > thr) return;   // a wave's
    double acc = Tx[src[a]];
    int64_t t = (int64_t)a + 1;
    for (; t + 4 <= e; t += 4) {
        const int32_t i0 = src[t], i1 = src[t + 1], i2 = src[t + 2], i3 = src[t + 3];
        const double v0 = Tx[i0], v1 = Tx[i1], v2 = Tx[i2], v3 = Tx[i3];
        acc = acc + v0;
        acc = acc + v1;
        acc = acc + v2;
        acc = acc + v3;
    }
    for (; t < e; t++) acc = acc + Tx[src[t]];
    out[s] = acc;
}

// out[0 .. nnz) <- the fold of Tx; queued on the context's stream between the plan's two events
static int assemble_launch(AsmPlan *P, const double *Tx, double *out) {
    hipStream_t s = ctx().stream;
    CSX_HIP(hipEventRecord(P->e0, s));
    if (P->nnz > 0) {
        if (P->nz == P->nnz) {
            hipLaunchKernelGGL(k_assemble_copy, dim3((unsigned)(((int64_t)P->nnz + 255) / 256)), dim3(256), 0, s, P->nnz,
                               P->src.get(), Tx, out);
        } else {
            const int64_t blocks = (P->nlong + ASM_WAVES - 1) / ASM_WAVES + ((int64_t)P->nnz + 64 * ASM_WAVES - 1) / (64 * ASM_WAVES);
            hipLaunchKernelGGL(k_assemble, dim3((unsigned)blocks), dim3(64 * ASM_WAVES), 0, s, P->nnz, P->thr, P->nlong,
                               P->longs.get(), P->sp.get(), P->src.get(), Tx, out);
        }
        CSX_LAUNCH_CHECK();
    }
    CSX_HIP(hipEventRecord(P->e1, s));
    P->timed = true;
    return CSX_OK;
}

}  // namespace csx

using namespace csx;

extern "C" int csx_assemble_plan(int32_t m, int32_t n, int64_t nz, const int32_t *Ti, const int32_t *Tj, csx_handle_t *out) {
    CSX_TRY(require_ready());
    if (!out || m < 0 || n < 0 || nz < 0 || nz > INT32_MAX) return CSX_EINVAL;
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<int32_t> Cp((size_t)n + 1), Ci((size_t)nz), sp((size_t)nz + 1), src((size_t)nz);
    int32_t nnz = 0;
    CSX_TRY(csx_assemble_plan_host(m, n, nz, Ti, Tj, Cp.data(), Ci.data(), sp.data(), src.data(), &nnz));
    std::unique_ptr<AsmPlan> P(new AsmPlan());
    P->m = m;
    P->n = n;
    P->nz = (int32_t)nz;
    P->nnz = nnz;
    P->thr = ctx().opt.assemble_long;
    std::vector<int32_t> longs;
    P->max_dup = assemble_slot_stats(nnz, sp.data(), P->thr, &longs);
    P->nlong = (int32_t)longs.size();
    P->build_us = std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
    CSX_TRY(upload(P->p, Cp));
    CSX_TRY(upload(P->i, Ci.data(), (size_t)nnz));
    CSX_TRY(upload(P->src, src));
    if (nz != nnz) CSX_TRY(upload(P->sp, sp.data(), (size_t)nnz + 1));
    CSX_TRY(upload(P->longs, longs));
    CSX_HIP(hipEventCreate(&P->e0));
    CSX_HIP(hipEventCreate(&P->e1));
    CSX_HIP(hipStreamSynchronize(ctx().stream));   // the host arrays go out of scope
    *out = put(K_ASMPLAN, P.release());
    return CSX_OK;
}

extern "C" int csx_assemble(csx_handle_t h, csx_handle_t hTx, csx_handle_t hout) {
    CSX_TRY(require_ready());
    AsmPlan *P = (AsmPlan *)get(h, K_ASMPLAN);
    Vec *tx = vec(hTx);
    if (!P || !tx || tx->len < P->nz) return CSX_EINVAL;
    if (Vec *o = vec(hout)) {
        if (o == tx || o->d == tx->d || o->len < P->nnz) return CSX_EINVAL;
        return assemble_launch(P, (const double *)tx->d, (double *)o->d);
    }
    Csc *A = csc(hout);
    if (!A || !A->x || A->m != P->m || A->n != P->n || A->nnz != P->nnz) return CSX_EINVAL;
    CSX_TRY(assemble_launch(P, (const double *)tx->d, A->x));
    A->rows.reset();    // the SpMV plans cached on the matrix hold copies of the old values
    A->tiled.reset();
    return CSX_OK;
}

extern "C" int csx_assemble_matrix(csx_handle_t h, csx_handle_t hTx, csx_handle_t *out) {
    CSX_TRY(require_ready());
    AsmPlan *P = (AsmPlan *)get(h, K_ASMPLAN);
    Vec *tx = hTx ? vec(hTx) : nullptr;
    if (!P || !out || (hTx && (!tx || tx->len < P->nz))) return CSX_EINVAL;
    hipStream_t s = ctx().stream;
    std::unique_ptr<Csc> C(new Csc());
    C->m = P->m;
    C->n = P->n;
    C->nnz = P->nnz;
    CSX_TRY(dalloc(&C->p, (size_t)P->n + 1));
    CSX_TRY(dalloc(&C->i, (size_t)P->nnz));
    if (tx) CSX_TRY(dalloc(&C->x, (size_t)P->nnz));
    CSX_HIP(hipMemcpyAsync(C->p, P->p.get(), ((size_t)P->n + 1) * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    if (P->nnz) CSX_HIP(hipMemcpyAsync(C->i, P->i.get(), (size_t)P->nnz * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    if (tx) CSX_TRY(assemble_launch(P, (const double *)tx->d, C->x));
    *out = put(K_CSC, C.release());
    return CSX_OK;
}

extern "C" int csx_assemble_plan_info(csx_handle_t h, int64_t *info) {
    CSX_TRY(require_ready());
    AsmPlan *P = (AsmPlan *)get(h, K_ASMPLAN);
    if (!P || !info) return CSX_EINVAL;
    info[0] = P->nz;
    info[1] = P->nnz;
    info[2] = P->max_dup;
    info[3] = P->nlong;
    info[4] = P->build_us;
    info[5] = 0;
    if (P->timed) {
        float ms = 0.f;
        CSX_HIP(hipEventSynchronize(P->e1));
        CSX_HIP(hipEventElapsedTime(&ms, P->e0, P->e1));
        info[5] = (int64_t)(1e3 * (double)ms + 0.5);
    }
    return CSX_OK;
}
