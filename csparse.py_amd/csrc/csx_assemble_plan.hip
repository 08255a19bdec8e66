// Assembly plan (the definition is the comment of csx_assemble_plan in include/csx.h): the triplets (Ti, Tj) of a
// matrix keep their places from step to step, only their values change.  Where every triplet lands in
// C = cs_dupl(cs_compress(T)) and in which order the duplicates of a slot are added is found once, on the host, by the
// reference's own two loops (csx_host.cpp: csx_assemble_plan_host).  A step is then ONE launch over the values:
//
//     C.x[s] = ((Tx[t0] + Tx[t1]) + Tx[t2]) + ...      over t = src[sp[s] .. sp[s + 1]), the first term assigned
//
// -- the reference's bits: no atomics, no reassociation, no multiply.  Either
//   * no duplicates at all (nz == nnz): a permuted copy out[s] = Tx[src[s]] that never reads sp (k_assemble_copy), or
//   * the ordered fold of csx_fold.h (k_fold: a lane per short slot, a wave per slot of more than Options::assemble_long
//     terms) with the term Tx[src[t]]: adjacent lanes read adjacent stretches of src, the gathers of up to four terms of a
//     lane, or of the 64 of a wave's step, are in flight together.
#include "csx_fold.h"

namespace csx {

struct AsmPlan {
    FoldCore core;          // core.longest: the most triplets of one slot (info's max_dup); core.sp null when nz == nnz
    int32_t nz = 0;
    DevBuf<int32_t> src;    // triplets grouped by slot
};

void destroy(AsmPlan *P) { delete P; }

__global__ __launch_bounds__(256) void k_assemble_copy(int32_t nnz, const int32_t *__restrict__ src,
                                                       const double *__restrict__ Tx, double *__restrict__ out) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s < nnz) out[s] = Tx[src[s]];
}

struct AsmTerm {   // term t of the fold: Tx[src[t]]
    const int32_t *__restrict__ src;
    const double *__restrict__ Tx;
    __device__ __forceinline__ double operator()(int64_t t) const { return Tx[src[t]]; }
    __device__ __forceinline__ void four(int64_t t, double v[4]) const {
        const int32_t i0 = src[t], i1 = src[t + 1], i2 = src[t + 2], i3 = src[t + 3];
        v[0] = Tx[i0], v[1] = Tx[i1], v[2] = Tx[i2], v[3] = Tx[i3];
    }
};

// out[0 .. nnz) <- the fold of Tx; queued on the context's stream between the plan's two events
static int assemble_launch(AsmPlan *P, const double *Tx, double *out) {
    FoldCore &c = P->core;
    CSX_TRY(c.begin());
    if (c.nnz > 0) {
        if (P->nz == c.nnz) {
            hipLaunchKernelGGL(k_assemble_copy, dim3((unsigned)(((int64_t)c.nnz + 255) / 256)), dim3(256), 0, ctx().stream, c.nnz,
                               P->src.get(), Tx, out);
            CSX_LAUNCH_CHECK();
        } else {
            CSX_TRY(c.launch(AsmTerm{P->src.get(), Tx}, out));
        }
    }
    return c.end();
}

// The pull-back of the fold: every triplet of slot s takes g[s] (a copy of bits).  A lane per slot; sp null: no duplicates.
__global__ __launch_bounds__(256) void k_assemble_pullback(int32_t nnz, const int32_t *__restrict__ sp,
                                                           const int32_t *__restrict__ src, const double *__restrict__ g,
                                                           double *__restrict__ out) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= nnz) return;
    const double v = g[s];
    if (!sp) {
        out[src[s]] = v;
        return;
    }
    for (int32_t u = sp[s], e = sp[s + 1]; u < e; u++) out[src[u]] = v;
}

}  // namespace csx

using namespace csx;

extern "C" int csx_assemble_pullback(csx_handle_t h, csx_handle_t hg, csx_handle_t hout) {
    CSX_TRY(require_ready());
    AsmPlan *P = (AsmPlan *)get(h, K_ASMPLAN);
    Vec *g = vec(hg), *o = vec(hout);
    if (!P || !g || !o || g->len < P->core.nnz || o->len < P->nz) return CSX_EINVAL;
    const uintptr_t gb = (uintptr_t)g->d, ge = gb + (uintptr_t)P->core.nnz * sizeof(double);
    const uintptr_t ob = (uintptr_t)o->d, oe = ob + (uintptr_t)P->nz * sizeof(double);
    if (P->nz > 0 && gb < oe && ob < ge) return CSX_EINVAL;
    if (P->core.nnz == 0) return CSX_OK;
    hipLaunchKernelGGL(k_assemble_pullback, dim3((unsigned)(((int64_t)P->core.nnz + 255) / 256)), dim3(256), 0, ctx().stream,
                       P->core.nnz, P->core.sp.get(), P->src.get(), (const double *)g->d, (double *)o->d);
    CSX_LAUNCH_CHECK();
    return CSX_OK;
}

extern "C" int csx_assemble_plan(int32_t m, int32_t n, int64_t nz, const int32_t *Ti, const int32_t *Tj, csx_handle_t *out) {
    CSX_TRY(require_ready());
    if (!out || m < 0 || n < 0 || nz < 0 || nz > INT32_MAX) return CSX_EINVAL;
    std::unique_ptr<AsmPlan> P(new AsmPlan());   // (build_us counts from here)
    FoldCore &c = P->core;
    std::vector<int32_t> Cp((size_t)n + 1), Ci((size_t)nz), sp((size_t)nz + 1), src((size_t)nz);
    CSX_TRY(csx_assemble_plan_host(m, n, nz, Ti, Tj, Cp.data(), Ci.data(), sp.data(), src.data(), &c.nnz));
    c.m = m;
    c.n = n;
    P->nz = (int32_t)nz;
    CSX_TRY(c.set_slots(sp.data(), ctx().opt.assemble_long, nz != c.nnz));
    CSX_TRY(upload(c.p, Cp));
    CSX_TRY(upload(c.i, Ci.data(), (size_t)c.nnz));
    CSX_TRY(upload(P->src, src));
    CSX_HIP(hipStreamSynchronize(ctx().stream));   // the host arrays go out of scope
    *out = put(K_ASMPLAN, P.release());
    return CSX_OK;
}

extern "C" int csx_assemble(csx_handle_t h, csx_handle_t hTx, csx_handle_t hout) {
    CSX_TRY(require_ready());
    AsmPlan *P = (AsmPlan *)get(h, K_ASMPLAN);
    Vec *tx = vec(hTx);
    if (!P || !tx || tx->len < P->nz) return CSX_EINVAL;
    if (Vec *o = vec(hout))
        if (o == tx || o->d == tx->d) return CSX_EINVAL;
    double *x = nullptr;
    Csc *C = nullptr;
    CSX_TRY(P->core.target(hout, &x, &C));
    CSX_TRY(assemble_launch(P, (const double *)tx->d, x));
    fold_wrote(C);
    return CSX_OK;
}

extern "C" int csx_assemble_matrix(csx_handle_t h, csx_handle_t hTx, csx_handle_t *out) {
    CSX_TRY(require_ready());
    AsmPlan *P = (AsmPlan *)get(h, K_ASMPLAN);
    Vec *tx = hTx ? vec(hTx) : nullptr;
    if (!P || !out || (hTx && (!tx || tx->len < P->nz))) return CSX_EINVAL;
    const FoldCore &c = P->core;
    std::unique_ptr<Csc> C;
    CSX_TRY(csc_copy_pattern(c.m, c.n, c.nnz, c.p, c.i, tx != nullptr, &C));
    if (tx) CSX_TRY(assemble_launch(P, (const double *)tx->d, C->x));
    *out = put(K_CSC, C.release());
    return CSX_OK;
}

extern "C" int csx_assemble_plan_info(csx_handle_t h, int64_t *info) {
    CSX_TRY(require_ready());
    AsmPlan *P = (AsmPlan *)get(h, K_ASMPLAN);
    if (!P || !info) return CSX_EINVAL;
    info[0] = P->nz;
    info[1] = P->core.nnz;
    info[2] = P->core.longest;
    info[3] = P->core.nlong;
    info[4] = P->core.build_us;
    return P->core.kernel_us(&info[5]);
}
