// The ordered fold shared by the plans that put new values into a fixed pattern (assembly_plan; multiply_plan,
// §18; add_plan, §19).  Every stored slot s of C is a serial, never-reassociated sum over a list fixed when the plan is built:
//
//     out[s] = ((term(t0) + term(t0 + 1)) + term(t0 + 2)) + ...      over t = sp[s] .. sp[s + 1], the first term assigned
//
// -- no atomics, no reassociation.  What a term is, is the plan's (a struct passed to the kernel by value): Tx[src[t]] for
// assembly, Bx[pair[t].y] * Ax[pair[t].x] rounded on its own for the product, c_r * x_r[..] rounded on its own for the sum.  Two
// classes of work, one kernel:
//   * short slots: one lane per slot; adjacent lanes read adjacent stretches of the plan's lists, the loads of up to four terms
//     are in flight together (Term::four), the additions follow in order;
//   * long slots (more than `thr` terms): one WAVE per slot.  A lane walking such a slot alone would pay a chain of dependent
//     random loads with 63 lanes idle.  The wave loads 64 terms per step -- coalesced on the plan's lists, the gathers in flight
//     together, the next step's already issued -- every lane forms its own term (exact: a term is a single rounding whoever
//     computes it), and the terms are added in index order through v_readlane, every lane keeping the same running sum.  The
//     sum itself stays the serial chain the definition makes it.  The blocks of the long slots come FIRST in the grid, so the
//     longest chains start first and run beside the short slots.
// FoldCore is the host side the plans share: the pattern of C, the slot pointers, the long list, the two events of a step.
#pragma once
#include <algorithm>
#include <chrono>

#include "csx_internal.h"

// no addition of a fold is contracted with the multiply of a term (the build's default turns a * b + c into one FMA); the
// files that define a term with a multiply keep it under the same pragma
#pragma clang fp contract(off)

namespace csx {

constexpr int FOLD_WAVES = 4;   // waves per workgroup; a long slot takes one of them

__device__ __forceinline__ double readlane_f64(double v, int k) {   // k: the same in every lane
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), k);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), k);
    return __hiloint2double(hi, lo);
}

// Term: __restrict__ pointers by value; double operator()(int64_t t): term t; void four(int64_t t, double v[4]): terms
// t .. t + 3 with their index loads issued first, then the gathers, then whatever arithmetic a term has.
template <class Term>
__global__ __launch_bounds__(64 * FOLD_WAVES) void k_fold(int32_t nnz, int32_t thr, int32_t nlong,
                                                          const int32_t *__restrict__ longs, const int32_t *__restrict__ sp,
                                                          Term term, double *__restrict__ out) {
    const int32_t long_blocks = (nlong + FOLD_WAVES - 1) / FOLD_WAVES;
    if ((int32_t)blockIdx.x < long_blocks) {
        const int lane = threadIdx.x & 63;
        // (the wave's own number, told to the compiler as the scalar it is: the slot's bounds and the fold's counters stay scalar)
        const int32_t w = (int32_t)blockIdx.x * FOLD_WAVES + __builtin_amdgcn_readfirstlane((int32_t)(threadIdx.x >> 6));
        if (w >= nlong) return;
        const int32_t s = longs[w], a = sp[s], e = sp[s + 1];
        double v = (int64_t)a + lane < e ? term(a + lane) : 0.0;
        double acc = 0.0;
        for (int64_t b = a; b < e; b += 64) {   // (64-bit: a slot may end within a step of 2^31 - 1)
            const int64_t tn = b + 64 + lane;
            const double vn = tn < e ? term(tn) : 0.0;   // the next step's loads fly while this step adds
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
    const int64_t s = (int64_t)(blockIdx.x - long_blocks) * (64 * FOLD_WAVES) + threadIdx.x;
    if (s >= nnz) return;
    const int32_t a = sp[s], e = sp[s + 1];
    if (e - a > thr) return;   // a wave's
    double acc = term(a);
    int64_t t = (int64_t)a + 1;
    for (; t + 4 <= e; t += 4) {
        double v[4];
        term.four(t, v);
        acc = acc + v[0];
        acc = acc + v[1];
        acc = acc + v[2];
        acc = acc + v[3];
    }
    for (; t < e; t++) acc = acc + term(t);
    out[s] = acc;
}

// the longest slot; *longs: the slots of more than thr terms, ascending
inline int32_t fold_slot_stats(int32_t nnz, const int32_t *sp, int32_t thr, std::vector<int32_t> *longs) {
    int32_t longest = 0;
    for (int32_t s = 0; s < nnz; s++) {
        const int32_t len = sp[s + 1] - sp[s];
        longest = std::max(longest, len);
        if (len > thr) longs->push_back(s);
    }
    return longest;
}

// What a plan of ordered folds keeps, whatever its terms are.  The plan makes it before its host work (build_us counts from
// there), fills m, n, nnz, p and i, and calls set_slots once.
struct FoldCore {
    int32_t m = 0, n = 0, nnz = 0;
    int32_t thr = 0, longest = 0, nlong = 0;
    DevBuf<int32_t> p, i;       // the pattern of C
    DevBuf<int32_t> sp;         // slot pointers (null for a plan that never folds)
    DevBuf<int32_t> longs;      // the long slots, ascending
    int64_t build_us = 0;       // the host build: from the core's making to the slot statistics
    hipEvent_t e0 = nullptr, e1 = nullptr;   // around the last step
    bool timed = false;
    const std::chrono::steady_clock::time_point made = std::chrono::steady_clock::now();
    FoldCore() = default;
    FoldCore(const FoldCore &) = delete;
    FoldCore &operator=(const FoldCore &) = delete;
    ~FoldCore() {
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
    }

    // The slots of the plan (host sp[0 .. nnz]) under the threshold `long_thr`: statistics, long list, build_us, then the
    // uploads (sp only when `folds`) and the two events.  The caller synchronises before its host arrays go.
    int set_slots(const int32_t *sp_h, int32_t long_thr, bool folds = true) {
        thr = long_thr;
        std::vector<int32_t> longs_h;
        longest = fold_slot_stats(nnz, sp_h, thr, &longs_h);
        nlong = (int32_t)longs_h.size();
        build_us = std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - made).count();
        if (folds) CSX_TRY(upload(sp, sp_h, (size_t)nnz + 1));
        CSX_TRY(upload(longs, longs_h));
        CSX_HIP(hipEventCreate(&e0));
        CSX_HIP(hipEventCreate(&e1));
        return CSX_OK;
    }

    // a step is everything a plan queues on the context's stream between begin() and end(); a step of no launch is timed too
    int begin() {
        CSX_HIP(hipEventRecord(e0, ctx().stream));
        return CSX_OK;
    }
    int end() {
        CSX_HIP(hipEventRecord(e1, ctx().stream));
        timed = true;
        return CSX_OK;
    }

    // out[0 .. nnz) <- the fold of the terms (nnz > 0); queued on the context's stream
    template <class Term>
    int launch(Term term, double *out) {
        const int64_t blocks = (nlong + FOLD_WAVES - 1) / FOLD_WAVES + ((int64_t)nnz + 64 * FOLD_WAVES - 1) / (64 * FOLD_WAVES);
        hipLaunchKernelGGL(k_fold<Term>, dim3((unsigned)blocks), dim3(64 * FOLD_WAVES), 0, ctx().stream, nnz, thr, nlong,
                           longs.get(), sp.get(), term, out);
        CSX_LAUNCH_CHECK();
        return CSX_OK;
    }

    // *us: the last step between its two events, 0 before the first (waits for that step)
    int kernel_us(int64_t *us) {
        *us = 0;
        if (timed) {
            float ms = 0.f;
            CSX_HIP(hipEventSynchronize(e1));
            CSX_HIP(hipEventElapsedTime(&ms, e0, e1));
            *us = (int64_t)(1e3 * (double)ms + 0.5);
        }
        return CSX_OK;
    }

    // Where a step writes: a vector of at least nnz doubles (*C null), or a CSC handle with the plan's m, n, nnz and values
    // (*C: that matrix; fold_wrote(*C) after the step).  CSX_EINVAL for anything else.  Aliasing is the caller's to check.
    int target(csx_handle_t hout, double **x, Csc **C) const {
        *C = nullptr;
        if (Vec *o = vec(hout)) {
            if (o->len < nnz) return CSX_EINVAL;
            *x = (double *)o->d;
            return CSX_OK;
        }
        Csc *A = csc(hout);
        if (!A || !A->x || A->m != m || A->n != n || A->nnz != nnz) return CSX_EINVAL;
        *C = A;
        *x = A->x;
        return CSX_OK;
    }
};

// The values an operand handle of a step stands for: a CSC handle with values and the operand's shape and entry count (its pattern
// is NOT compared), or a vector of exactly nz doubles.  null: neither.
inline const double *fold_operand_values(csx_handle_t h, int32_t rows, int32_t cols, int32_t nz) {
    if (Csc *M = csc(h)) return (M->x && M->m == rows && M->n == cols && M->nnz == nz) ? M->x : nullptr;
    if (Vec *v = vec(h)) return v->len == nz ? (const double *)v->d : nullptr;
    return nullptr;
}

// after a step has written C's values in place (C may be null: the step wrote a vector)
inline void fold_wrote(Csc *C) {
    if (!C) return;
    C->rows.reset();    // the SpMV plans cached on the matrix hold copies of the old values
    C->tiled.reset();
}

}  // namespace csx
