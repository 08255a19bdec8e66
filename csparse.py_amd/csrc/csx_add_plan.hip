// Add plan (the definition is the comment of csx_add_plan in include/csx.h): the patterns of the operands
// A_0 .. A_{k-1} of C = c_0 A_0 + c_1 A_1 + ... stay from step to step, only their values and the coefficients change.  Which
// entries land in which slot of the reference's chain of cs_add and in which order the chain adds them is found once, on the
// host, by the reference's own loops on the indices (csx_host.cpp: csx_add_plan_host).  A step is then ONE launch over the values:
//
//     C.x[s] = ((c x) + c' x') + c'' x'' + ...      over the entries src[sp[s] .. sp[s + 1]), the first term assigned
//
// -- the reference's bits: every c x rounded on its own and never fused with the addition that follows, no atomics, no
// reassociation.  Two classes of step, decided when the plan is built:
//   * aligned: every operand has exactly C's pattern in C's order (K + sigma M).  No index is read at all: a streaming kernel
//     out[s] = (c_0 x_0[s] + c_1 x_1[s]) + ..., 16-byte loads and stores, a grid sized to the chip; 8 (k + 1) nnz bytes.
//   * general: the ordered fold of csx_fold.h (k_fold: a lane per short slot, a wave per slot of more than Options::add_long
//     terms) with the term c_r * x_r[src[t] - off[r]], r the operand that holds position src[t] of the concatenated values.
#include "csx_fold.h"

// every multiply below is rounded before the addition that takes it (the build's default contracts a * b + c into one FMA)
#pragma clang fp contract(off)

namespace csx {

constexpr int ADD_MAX = 8;   // operands of one plan

struct AddPlan {
    FoldCore core;              // core.longest: the most terms of one slot (info's max_terms); core.sp null when aligned
    int32_t k = 0, terms = 0;
    int32_t off[ADD_MAX + 1] = {0};   // off[r]: the first position of operand r in the concatenated values; off[k] = terms
    bool aligned = false;
    int64_t room = 0;           // the nzmax the reference's chain leaves: entries of the last cs_add's two operands
    DevBuf<int32_t> src;        // positions grouped by slot (null when aligned)
};

void destroy(AddPlan *P) { delete P; }

struct AddArgs {   // the values and coefficients of a step; slots k .. 7 repeat slot 0 and are never used
    const double *x[ADD_MAX];
    double c[ADD_MAX];
};

// The aligned step.  W = 2: every pointer is 16-byte aligned, a lane moves two slots per load; W = 1: 8-byte accesses.
template <int K, int W>
__global__ __launch_bounds__(256) void k_add_aligned(int32_t nnz, AddArgs a, double *__restrict__ out) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    const int64_t first = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (W == 2) {
        const int64_t pairs = nnz >> 1;
        for (int64_t q = first; q < pairs; q += stride) {
            double2 v[K];
#pragma unroll
            for (int r = 0; r < K; r++) v[r] = ((const double2 *)a.x[r])[q];   // all k loads in flight together
            double2 acc;
            acc.x = a.c[0] * v[0].x;
            acc.y = a.c[0] * v[0].y;
#pragma unroll
            for (int r = 1; r < K; r++) {
                const double tx = a.c[r] * v[r].x, ty = a.c[r] * v[r].y;
                acc.x = acc.x + tx;
                acc.y = acc.y + ty;
            }
            ((double2 *)out)[q] = acc;
        }
        if (!(nnz & 1) || first != 0) return;
    }
    // W = 1: every slot; W = 2: the odd last slot, by one lane
    for (int64_t s = W == 2 ? (int64_t)nnz - 1 : first; s < nnz; s += stride) {
        double v[K];
#pragma unroll
        for (int r = 0; r < K; r++) v[r] = a.x[r][s];
        double acc = a.c[0] * v[0];
#pragma unroll
        for (int r = 1; r < K; r++) {
            const double t = a.c[r] * v[r];
            acc = acc + t;
        }
        out[s] = acc;
    }
}

// Term t of the general fold: position g = src[t] of the concatenated values belongs to the last operand r with off[r] <= g.
// The operand is found by a fixed chain of compares and selects over the eight slots (every index below is a constant after
// unrolling: the arrays stay in the kernel's argument registers; a dynamic index would put them in scratch memory).
struct AddTerm {
    const int32_t *__restrict__ src;
    int32_t off[ADD_MAX];   // off[r] of the plan; INT32_MAX for r >= k (no position reaches it: terms <= INT32_MAX)
    AddArgs a;
    __device__ __forceinline__ const double *pick(int32_t g, double *c) const {
        const double *p = a.x[0];
        double cc = a.c[0];
        int32_t base = 0;
#pragma unroll
        for (int r = 1; r < ADD_MAX; r++) {
            const bool in = g >= off[r];
            p = in ? a.x[r] : p;
            cc = in ? a.c[r] : cc;
            base = in ? off[r] : base;
        }
        *c = cc;
        return p + (g - base);
    }
    __device__ __forceinline__ double operator()(int64_t t) const {
        double c;
        const double *p = pick(src[t], &c);
        return c * *p;
    }
    __device__ __forceinline__ void four(int64_t t, double v[4]) const {
        const int32_t g0 = src[t], g1 = src[t + 1], g2 = src[t + 2], g3 = src[t + 3];
        double c0, c1, c2, c3;
        const double *p0 = pick(g0, &c0), *p1 = pick(g1, &c1), *p2 = pick(g2, &c2), *p3 = pick(g3, &c3);
        const double x0 = *p0, x1 = *p1, x2 = *p2, x3 = *p3;
        v[0] = c0 * x0, v[1] = c1 * x1, v[2] = c2 * x2, v[3] = c3 * x3;
    }
};

template <int W>
static void aligned_launch(int k, unsigned blocks, int32_t nnz, const AddArgs &a, double *out) {
    hipStream_t s = ctx().stream;
    switch (k) {
    case 2: hipLaunchKernelGGL((k_add_aligned<2, W>), dim3(blocks), dim3(256), 0, s, nnz, a, out); break;
    case 3: hipLaunchKernelGGL((k_add_aligned<3, W>), dim3(blocks), dim3(256), 0, s, nnz, a, out); break;
    case 4: hipLaunchKernelGGL((k_add_aligned<4, W>), dim3(blocks), dim3(256), 0, s, nnz, a, out); break;
    case 5: hipLaunchKernelGGL((k_add_aligned<5, W>), dim3(blocks), dim3(256), 0, s, nnz, a, out); break;
    case 6: hipLaunchKernelGGL((k_add_aligned<6, W>), dim3(blocks), dim3(256), 0, s, nnz, a, out); break;
    case 7: hipLaunchKernelGGL((k_add_aligned<7, W>), dim3(blocks), dim3(256), 0, s, nnz, a, out); break;
    default: hipLaunchKernelGGL((k_add_aligned<8, W>), dim3(blocks), dim3(256), 0, s, nnz, a, out); break;
    }
}

// out[0 .. nnz) <- the step on the values x[0 .. k) with the coefficients coef; queued on the context's stream between the
// plan's two events
static int add_launch(AddPlan *P, const double *coef, const double *const *x, double *out) {
    FoldCore &c = P->core;
    AddArgs a;
    for (int r = 0; r < ADD_MAX; r++) {
        a.x[r] = x[r < P->k ? r : 0];
        a.c[r] = coef[r < P->k ? r : 0];
    }
    CSX_TRY(c.begin());
    if (c.nnz > 0) {
        if (P->aligned) {
            uintptr_t bits = (uintptr_t)out;
            for (int r = 0; r < P->k; r++) bits |= (uintptr_t)x[r];
            const bool wide = (bits & 15) == 0;
            const int64_t work = wide ? std::max<int64_t>(c.nnz >> 1, 1) : c.nnz;   // a lane's iterations over the whole grid
            const int64_t cap = (int64_t)std::max(ctx().cus, 1) * 8;               // 8 workgroups of 256 per CU, the rest by stride
            const unsigned blocks = (unsigned)std::min<int64_t>((work + 255) / 256, cap);
            if (wide) aligned_launch<2>(P->k, blocks, c.nnz, a, out);
            else aligned_launch<1>(P->k, blocks, c.nnz, a, out);
            CSX_LAUNCH_CHECK();
        } else {
            AddTerm term;
            term.src = P->src.get();
            for (int r = 0; r < ADD_MAX; r++) term.off[r] = r < P->k ? P->off[r] : INT32_MAX;
            term.a = a;
            CSX_TRY(c.launch(term, out));
        }
    }
    return c.end();
}

// x[0 .. k) of a step, checked
static int add_inputs(const AddPlan *P, const double *coef, const csx_handle_t *hX, const double **x) {
    if (!coef || !hX) return CSX_EINVAL;
    for (int r = 0; r < P->k; r++) {
        x[r] = fold_operand_values(hX[r], P->core.m, P->core.n, P->off[r + 1] - P->off[r]);
        if (!x[r]) return CSX_EINVAL;
    }
    return CSX_OK;
}

}  // namespace csx

using namespace csx;

extern "C" int csx_add_plan(int32_t k, const csx_handle_t *operands, csx_handle_t *out) {
    CSX_TRY(require_ready());
    if (k < 2 || k > ADD_MAX || !operands || !out) {
        set_error("csx_add_plan: needs 2 to 8 operands");
        return CSX_EINVAL;
    }
    const Csc *A[ADD_MAX];
    for (int r = 0; r < k; r++) {
        A[r] = csc(operands[r]);
        if (!A[r] || A[r]->m != A[0]->m || A[r]->n != A[0]->n) {
            set_error("csx_add_plan: needs CSC matrices of one shape");
            return CSX_EINVAL;
        }
    }
    std::unique_ptr<AddPlan> P(new AddPlan());   // (build_us counts from here)
    FoldCore &c = P->core;
    const int32_t m = A[0]->m, n = A[0]->n;
    std::vector<int32_t> hp[ADD_MAX], hi[ADD_MAX];
    const int32_t *Ap[ADD_MAX], *Ai[ADD_MAX];
    int64_t terms = 0;
    for (int r = 0; r < k; r++) {
        int same = -1;   // the same handle again (A + A): its arrays are downloaded once
        for (int q = 0; q < r && same < 0; q++)
            if (A[q] == A[r]) same = q;
        if (same < 0) {
            CSX_TRY(download_i32(hp[r], A[r]->p, (size_t)n + 1));
            CSX_TRY(download_i32(hi[r], A[r]->i, (size_t)A[r]->nnz));
            if (hp[r][n] != A[r]->nnz) {
                set_error("csx_add_plan: an operand's pointers do not end at its entry count");
                return CSX_EINVAL;
            }
        }
        Ap[r] = hp[same < 0 ? r : same].data();
        Ai[r] = hi[same < 0 ? r : same].data();
        P->off[r] = (int32_t)terms;   // (checked below before it is used)
        terms += A[r]->nnz;
    }
    if (terms > INT32_MAX) {
        set_error("csx_add_plan: %lld terms do not fit the plan's int32 pointers", (long long)terms);
        return CSX_EINVAL;
    }
    P->off[k] = (int32_t)terms;
    P->k = k;
    P->terms = (int32_t)terms;
    std::vector<int32_t> Cp((size_t)n + 1), Ci((size_t)terms), sp((size_t)terms + 1), src((size_t)terms);
    if (csx_add_plan_host(m, n, k, Ap, Ai, Cp.data(), Ci.data(), sp.data(), src.data(), &c.nnz) != CSX_OK) {
        set_error("csx_add_plan: an operand's pointers or row indices are out of range");
        return CSX_EINVAL;
    }
    c.m = m;
    c.n = n;
    // aligned: every operand has exactly C's pattern in C's order -- slot s is the entries s of A_0, A_1, ... and nothing else
    bool aligned = terms == (int64_t)k * c.nnz;
    for (int32_t s = 0; aligned && s < c.nnz; s++)
        for (int r = 0; r < k; r++)
            if (src[(size_t)k * s + r] != P->off[r] + s) {
                aligned = false;
                break;
            }
    P->aligned = aligned;
    // what the chain's last cs_add allocates: the entries of its first operand (A_0 for k = 2, else the sum so far: the slots
    // opened by an operand before the last) plus those of the last operand
    int64_t before = A[0]->nnz;
    if (k > 2) {
        before = 0;
        for (int32_t s = 0; s < c.nnz; s++) before += src[sp[s]] < P->off[k - 1];
    }
    P->room = before + A[k - 1]->nnz;
    // (an aligned plan folds nothing: no slot is a wave's, whatever the threshold)
    CSX_TRY(c.set_slots(sp.data(), aligned ? INT32_MAX : ctx().opt.add_long, !aligned));
    CSX_TRY(upload(c.p, Cp));
    CSX_TRY(upload(c.i, Ci.data(), (size_t)c.nnz));
    if (!aligned) CSX_TRY(upload(P->src, src));
    CSX_HIP(hipStreamSynchronize(ctx().stream));   // the host arrays go out of scope
    *out = put(K_ADDPLAN, P.release());
    return CSX_OK;
}

extern "C" int csx_add_plan_run(csx_handle_t h, const double *coef, const csx_handle_t *hX, csx_handle_t hout) {
    CSX_TRY(require_ready());
    AddPlan *P = (AddPlan *)get(h, K_ADDPLAN);
    if (!P) return CSX_EINVAL;
    const double *x[ADD_MAX];
    CSX_TRY(add_inputs(P, coef, hX, x));
    double *o = nullptr;
    Csc *C = nullptr;
    CSX_TRY(P->core.target(hout, &o, &C));
    for (int r = 0; r < P->k; r++)
        if (o == x[r]) return CSX_EINVAL;   // out aliases no input
    CSX_TRY(add_launch(P, coef, x, o));
    fold_wrote(C);
    return CSX_OK;
}

extern "C" int csx_add_plan_matrix(csx_handle_t h, const double *coef, const csx_handle_t *hX, csx_handle_t *out) {
    CSX_TRY(require_ready());
    AddPlan *P = (AddPlan *)get(h, K_ADDPLAN);
    if (!P || !out) return CSX_EINVAL;
    const double *x[ADD_MAX];
    if (hX) CSX_TRY(add_inputs(P, coef, hX, x));
    const FoldCore &c = P->core;
    std::unique_ptr<Csc> C;
    CSX_TRY(csc_copy_pattern(c.m, c.n, c.nnz, c.p, c.i, hX != nullptr, &C));
    if (hX) CSX_TRY(add_launch(P, coef, x, C->x));
    *out = put(K_CSC, C.release());
    return CSX_OK;
}

extern "C" int csx_add_plan_info(csx_handle_t h, int64_t *info) {
    CSX_TRY(require_ready());
    AddPlan *P = (AddPlan *)get(h, K_ADDPLAN);
    if (!P || !info) return CSX_EINVAL;
    info[0] = P->k;
    info[1] = P->core.m;
    info[2] = P->core.n;
    info[3] = P->core.nnz;
    info[4] = P->terms;
    info[5] = P->core.longest;
    info[6] = P->core.nlong;
    info[7] = P->aligned ? 1 : 0;
    info[8] = P->core.build_us;
    CSX_TRY(P->core.kernel_us(&info[9]));
    info[10] = P->room;
    return CSX_OK;
}
