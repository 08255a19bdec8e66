// Multiply plan (the definition is the comment of csx_multiply_plan in include/csx.h): the patterns of A and B
// stay from step to step, only their values change.  Which products A.x[ia] B.x[ib] land in which entry of C = cs_multiply(A, B)
// and in which order the reference adds them is found once, on the host, by the reference's own two loops on the indices
// (csx_host.cpp: csx_multiply_plan_host).  A step is then ONE launch over the values:
//
//     C.x[s] = ((b0 a0) + b1 a1) + b2 a2 + ...      over (ia, ib) = pair[sp[s] .. sp[s + 1]), the first term assigned
//
// -- the reference's bits: every product rounded on its own and never fused with the addition that follows, no atomics, no
// hash table, no reassociation.  It is the ordered fold of csx_fold.h (k_fold: a lane per short slot, a wave per slot of more
// than Options::multiply_long products) with the term Bx[pair[t].y] * Ax[pair[t].x]: adjacent lanes read adjacent stretches
// of pair (8-byte loads), the pairs and gathers of up to four products of a lane, or of the 64 of a wave's step, are in flight
// together, and every lane forms its own term (exact: a term is a single rounding whoever computes it).
// C = A diag(d) B is by definition cs_multiply(A, B2) with B2.x[p] = d[B.i[p]] * B.x[p]: an elementwise kernel over nnz(B)
// writes B2.x into a scratch vector of the plan and the same fold reads it in place of B.x.
#include "csx_fold.h"

// every multiply below is rounded before the addition that takes it (the build's default contracts a * b + c into one FMA)
#pragma clang fp contract(off)

namespace csx {

struct MulPlan {
    FoldCore core;              // core.longest: the most products of one slot (info's max_products)
    int32_t k = 0, anz = 0, bnz = 0, products = 0;
    DevBuf<int32_t> pair;       // (ia, ib) of every product, grouped by slot
    DevBuf<int32_t> bi;         // B.i (the scale reads it; Bx may come as a bare vector)
    DevBuf<double> b2;          // d[B.i[p]] * B.x[p], made by the first scaled step, kept
};

void destroy(MulPlan *P) { delete P; }

__global__ __launch_bounds__(256) void k_multiply_scale(int32_t bnz, const int32_t *__restrict__ Bi, const double *__restrict__ Bx,
                                                        const double *__restrict__ d, double *__restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t < bnz) out[t] = d[Bi[t]] * Bx[t];
}

struct MulTerm {   // term t of the fold: the product pair[t] = (ia, ib), rounded on its own
    const int2 *__restrict__ pair;
    const double *__restrict__ Ax;
    const double *__restrict__ Bx;
    __device__ __forceinline__ double operator()(int64_t t) const {
        const int2 q = pair[t];
        return Bx[q.y] * Ax[q.x];
    }
    __device__ __forceinline__ void four(int64_t t, double v[4]) const {
        const int2 q0 = pair[t], q1 = pair[t + 1], q2 = pair[t + 2], q3 = pair[t + 3];
        const double a0 = Ax[q0.x], a1 = Ax[q1.x], a2 = Ax[q2.x], a3 = Ax[q3.x];
        const double b0 = Bx[q0.y], b1 = Bx[q1.y], b2 = Bx[q2.y], b3 = Bx[q3.y];
        v[0] = b0 * a0, v[1] = b1 * a1, v[2] = b2 * a2, v[3] = b3 * a3;
    }
};

// out[0 .. nnz) <- the fold of Ax, Bx (Bx scaled by d first when d is given); queued on the context's stream between the
// plan's two events
static int multiply_launch(MulPlan *P, const double *Ax, const double *Bx, const double *d, double *out) {
    FoldCore &c = P->core;
    if (d && P->bnz > 0 && !P->b2.get()) CSX_TRY(P->b2.alloc((size_t)P->bnz));
    CSX_TRY(c.begin());
    if (c.nnz > 0) {
        if (d) {
            hipLaunchKernelGGL(k_multiply_scale, dim3((unsigned)(((int64_t)P->bnz + 255) / 256)), dim3(256), 0, ctx().stream,
                               P->bnz, P->bi.get(), Bx, d, P->b2.get());
            Bx = P->b2.get();
        }
        CSX_TRY(c.launch(MulTerm{(const int2 *)P->pair.get(), Ax, Bx}, out));
    }
    return c.end();
}

// Ax, Bx, d of a step, checked; d stays null when hd is 0
static int multiply_inputs(const MulPlan *P, csx_handle_t hAx, csx_handle_t hBx, csx_handle_t hd, const double **Ax,
                           const double **Bx, const double **d) {
    *Ax = fold_operand_values(hAx, P->core.m, P->k, P->anz);
    *Bx = fold_operand_values(hBx, P->k, P->core.n, P->bnz);
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
    std::unique_ptr<MulPlan> P(new MulPlan());   // (build_us counts from here)
    FoldCore &c = P->core;
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
    c.m = A->m;
    P->k = A->n;
    c.n = B->n;
    P->anz = A->nnz;
    P->bnz = B->nnz;
    c.nnz = (int32_t)nnz;
    P->products = (int32_t)products;
    CSX_TRY(c.set_slots(sp.data(), ctx().opt.multiply_long));
    CSX_TRY(upload(c.p, Cp));
    CSX_TRY(upload(c.i, Ci));
    CSX_TRY(upload(P->pair, pair));
    CSX_TRY(upload(P->bi, Bi));
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
    CSX_TRY(P->core.target(hout, &x, &C));
    if (x == Ax || x == Bx || x == d) return CSX_EINVAL;   // out aliases no input
    CSX_TRY(multiply_launch(P, Ax, Bx, d, x));
    fold_wrote(C);
    return CSX_OK;
}

extern "C" int csx_multiply_plan_matrix(csx_handle_t h, csx_handle_t hAx, csx_handle_t hBx, csx_handle_t hd, csx_handle_t *out) {
    CSX_TRY(require_ready());
    MulPlan *P = (MulPlan *)get(h, K_MULPLAN);
    if (!P || !out) return CSX_EINVAL;
    const bool values = hAx || hBx;
    const double *Ax = nullptr, *Bx = nullptr, *d = nullptr;
    if (values) CSX_TRY(multiply_inputs(P, hAx, hBx, hd, &Ax, &Bx, &d));
    const FoldCore &c = P->core;
    std::unique_ptr<Csc> C;
    CSX_TRY(csc_copy_pattern(c.m, c.n, c.nnz, c.p, c.i, values, &C));
    if (values) CSX_TRY(multiply_launch(P, Ax, Bx, d, C->x));
    *out = put(K_CSC, C.release());
    return CSX_OK;
}

extern "C" int csx_multiply_plan_info(csx_handle_t h, int64_t *info) {
    CSX_TRY(require_ready());
    MulPlan *P = (MulPlan *)get(h, K_MULPLAN);
    if (!P || !info) return CSX_EINVAL;
    info[0] = P->core.m;
    info[1] = P->core.n;
    info[2] = P->core.nnz;
    info[3] = P->products;
    info[4] = P->core.longest;
    info[5] = P->core.nlong;
    info[6] = P->core.build_us;
    return P->core.kernel_us(&info[7]);
}
