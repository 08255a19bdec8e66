// Cholesky refactor (the definition is the comment of csx_chol_refactor in include/csx.h): new values for a
// factor L of cs_chol with everything the analysis found kept.  The plan holds A's pattern and, by route,
//   general: the CholAnalysis of csx_chol.hip (row view, entry map, forest partition, level lists, supernode groups, band
//            decision) -- made from L itself, so no S is needed;
//   forest:  the CliqueForest of csx_cholclique.hip (A's elimination forest is cliques or small sparse trees on consecutive
//            columns).
// A refactor writes the new factor into a scratch array of lnz doubles with the launches csx_chol itself makes and copies it
// over L.x only when no pivot failed: L.x keeps its address (the solve plans borrow it) and a matrix that is not positive
// definite changes nothing.
#include <algorithm>
#include <chrono>

#include "csx_internal.h"
#include "csx_sweep.h"
#include "csx_cholclique.h"

namespace csx {

// what the last csx_chol_refactor did (csx_chol_refactor_info)
static bool g_rf_valid = false;
static double g_rf_numeric_ms = 0.0, g_rf_call_ms = 0.0;

// The values of A into the slots of L through the kept entry map: one coalesced pass over the slots with a gather from Ax.
// No searches, no atomics: which entry wins a slot was settled when the map was made.
__global__ __launch_bounds__(256) void k_chol_scatter(int64_t lnz, const int32_t *__restrict__ win, const double *__restrict__ Ax,
                                                      double *__restrict__ Lx) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < lnz; q += stride) {
        const int32_t w = win[q];
        Lx[q] = w >= 0 ? Ax[w] : 0.0;
    }
}

int chol_scatter(int64_t lnz, const int32_t *win, const double *Ax, double *Lx) {
    if (lnz <= 0) return CSX_OK;
    const int64_t most = (int64_t)std::max(ctx().cus, 1) * 16;   // workgroups: enough to fill the device, the rest by stride
    const int64_t blocks = std::min<int64_t>((lnz + 255) / 256, most);
    hipLaunchKernelGGL(k_chol_scatter, dim3((unsigned)blocks), dim3(256), 0, ctx().stream, lnz, win, Ax, Lx);
    CSX_LAUNCH_CHECK();
    return CSX_OK;
}

// One wave per column of L (Lp checked on the host): the diagonal first, rows strictly ascending below it and inside the
// matrix; parent[j] = the row of the column's second entry (the elimination tree, as csx_updown_block reads it).
__global__ __launch_bounds__(256) void k_chol_shape(int32_t n, const int32_t *__restrict__ Lp, const int32_t *__restrict__ Li,
                                                    int32_t *__restrict__ parent, int *bad) {
    const int lane = threadIdx.x & 63;
    const int64_t j = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (j >= n) return;
    const int32_t b = Lp[j], e = Lp[j + 1];
    if (lane == 0) {
        if (Li[b] != (int32_t)j) *bad = 1;
        parent[j] = e - b > 1 ? Li[b + 1] : -1;
    }
    for (int32_t p = b + 1 + lane; p < e; p += 64) {
        const int32_t r = Li[p];
        if (r <= Li[p - 1] || r >= n) *bad = 1;
    }
}

struct CholRefPlan {
    csx_handle_t hL = 0;
    int32_t n = 0, anz = 0, lnz = 0;
    DevBuf<int32_t> p0, i0;              // A's pattern: every A2 is checked against it, and the forest route reads it
    CholAnalysis *An = nullptr;          // general route
    std::unique_ptr<CliqueForest> F;     // forest route
    bool made = false;                   // the scratch arrays exist (the first refactor makes them)
    DevBuf<double> Lx;                   // scratch: committed only when every pivot passed
    DevBuf<int32_t> Li;                  // forest route: where the block kernel stores the row indices it derives (L.i is not written)
    DevBuf<int> flag;
    hipEvent_t ev_a = nullptr, ev_b = nullptr;
    CholRefPlan() = default;
    CholRefPlan(const CholRefPlan &) = delete;
    CholRefPlan &operator=(const CholRefPlan &) = delete;
    ~CholRefPlan() {
        destroy(An);
        if (ev_a) (void)hipEventDestroy(ev_a);
        if (ev_b) (void)hipEventDestroy(ev_b);
    }
};

void destroy(CholRefPlan *P) { delete P; }

static int chol_refactor_plan(Csc *A, Csc *L, const int32_t *pinv, CholRefPlan *P) {
    hipStream_t s = ctx().stream;
    const int32_t n = A->n;
    P->n = n;
    P->anz = A->nnz;
    P->lnz = L->nnz;
    if (!A->trusted) CSX_TRY(csc_validate(A));
    if (pinv) {   // must be a permutation of 0..n-1
        std::vector<char> seen((size_t)n, 0);
        for (int32_t j = 0; j < n; j++) {
            if (pinv[j] < 0 || pinv[j] >= n || seen[(size_t)pinv[j]]) {
                set_error("csx_chol_refactor_plan: pinv is not a permutation");
                return CSX_EINVAL;
            }
            seen[(size_t)pinv[j]] = 1;
        }
    }
    CSX_TRY(rf_keep_pattern(A, P->p0, P->i0));
    CSX_TRY(P->flag.alloc(1));
    CSX_HIP(hipEventCreate(&P->ev_a));
    CSX_HIP(hipEventCreate(&P->ev_b));
    if (n == 0) return CSX_OK;
    // L's shape: column pointers on the host (they are the counts cp of the schedule), rows and the tree on the device
    std::vector<int32_t> Lp_h, parent_h;
    CSX_TRY(download_i32(Lp_h, L->p, (size_t)n + 1));
    bool shaped = Lp_h[0] == 0 && Lp_h[(size_t)n] == L->nnz;
    for (int32_t j = 0; shaped && j < n; j++) shaped = Lp_h[(size_t)j + 1] > Lp_h[(size_t)j];
    DevBuf<int32_t> d_parent;
    if (shaped) {
        CSX_TRY(d_parent.alloc((size_t)n));
        CSX_HIP(hipMemsetAsync(P->flag, 0, sizeof(int), s));
        hipLaunchKernelGGL(k_chol_shape, dim3((unsigned)(((int64_t)n + 3) / 4)), dim3(256), 0, s, n, L->p, L->i, d_parent.get(),
                           P->flag.get());
        CSX_LAUNCH_CHECK();
        int bad = 0;
        CSX_HIP(hipMemcpyAsync(&bad, P->flag.get(), sizeof(int), hipMemcpyDeviceToHost, s));
        CSX_TRY(download_i32(parent_h, d_parent, (size_t)n));
        shaped = !bad;
    }
    if (!shaped) {
        set_error("csx_chol_refactor_plan: L is not Cholesky-shaped (diagonal first, rows ascending)");
        return CSX_EINVAL;
    }
    // forest route: clique_forest_route's (a finding of this plan's own: the matrix's cached one goes with csx_csc_invalidate), and
    // L's columns are the forest's
    {
        ForestRoute R;   // (a finding that is not taken is let go before the general analysis)
        CSX_TRY(clique_forest_route(A, pinv != nullptr, false, &R));
        if (R.F && R.F->lnz == (int64_t)L->nnz) {
            int differ = 0;
            CSX_TRY(rf_differ((int64_t)n + 1, L->p, R.F->cp.get(), P->flag.get(), &differ));
            if (differ) {
                set_error("csx_chol_refactor_plan: an upper entry of A has no slot in L (L is not the factor of A's pattern)");
                return CSX_EINVAL;
            }
            P->F = std::move(R.own);
            return CSX_OK;
        }
    }
    bool foreign = false;
    CSX_TRY(chol_analysis_of_factor(A, pinv, L, parent_h.data(), Lp_h.data(), &P->An, &foreign));
    if (foreign) {
        set_error("csx_chol_refactor_plan: an upper entry of A has no slot in L (L is not the factor of A's pattern)");
        return CSX_EINVAL;
    }
    return CSX_OK;
}

}  // namespace csx

using namespace csx;

extern "C" int csx_chol_refactor_plan(csx_handle_t hA, csx_handle_t hL, const int32_t *pinv, csx_handle_t *out) {
    CSX_TRY(require_ready());
    Csc *A = csc(hA), *L = csc(hL);   // (a factor whose rows are pending gets them here)
    if (!A || !L || !out || !L->x || A->m != A->n || L->m != L->n || L->n != A->n) return CSX_EINVAL;
    std::unique_ptr<CholRefPlan> P(new CholRefPlan());
    P->hL = hL;
    CSX_TRY(chol_refactor_plan(A, L, pinv, P.get()));
    *out = put(K_CHOLREFPLAN, P.release());
    return CSX_OK;
}

extern "C" int csx_chol_refactor(csx_handle_t h, csx_handle_t hA2, int *ok, int32_t *info) {
    CSX_TRY(require_ready());
    const auto t_call = std::chrono::steady_clock::now();
    CholRefPlan *P = (CholRefPlan *)get(h, K_CHOLREFPLAN);
    if (!P || !ok) return CSX_EINVAL;
    Csc *L = csc(P->hL);
    if (!L || !L->x || L->n != P->n || L->nnz != P->lnz) return CSX_EINVAL;
    if (info)
        for (int k = 0; k < 8; k++) info[k] = 0;
    const double *x2 = nullptr;
    CSX_TRY(rf_values(hA2, P->n, P->n, P->anz, P->p0, P->i0, P->flag, &x2));
    if (!x2) {
        *ok = -1;   // another pattern or length: nothing changes
        return CSX_OK;
    }
    hipStream_t s = ctx().stream;
    const bool first = !P->made;
    if (first) {
        DevBuf<double> lx;
        DevBuf<int32_t> li;
        CSX_TRY(lx.alloc((size_t)P->lnz));
        if (P->F) CSX_TRY(li.alloc((size_t)P->lnz));
        P->Lx = std::move(lx);
        P->Li = std::move(li);
        P->made = true;
    }
    bool notspd = false;
    CSX_HIP(hipEventRecord(P->ev_a, s));
    if (P->n == 0) {
        CSX_HIP(hipEventRecord(P->ev_b, s));
    } else if (P->F) {
        Csc A2v, Lv;   // views: the kept pattern with A2's values; L's columns with the scratch arrays
        A2v.owns = Lv.owns = false;
        A2v.m = A2v.n = Lv.m = Lv.n = P->n;
        A2v.nnz = P->anz;
        A2v.p = P->p0;
        A2v.i = P->i0;
        A2v.x = const_cast<double *>(x2);
        Lv.nnz = P->lnz;
        Lv.p = L->p;
        Lv.i = P->Li;
        Lv.x = P->Lx;
        int hflag = 0;
        // (ev_a: recorded above, for every route)
        CSX_TRY(clique_run_collect(clique_run_launch(&A2v, *P->F, &Lv, P->flag, 1, nullptr, nullptr, P->ev_b), P->flag, 1, &hflag, "csx_chol_refactor", &notspd));
    } else {
        CSX_TRY(chol_analysis_refactor(P->An, L, x2, P->Lx, P->ev_b, &notspd));
    }
    if (info) {
        info[0] = P->F ? 1 : 0;
        if (P->An) chol_analysis_info(P->An, info);
        info[6] = first ? 1 : 0;
    }
    *ok = notspd ? 0 : 1;
    if (!notspd) {
        if (P->lnz) CSX_HIP(hipMemcpyAsync(L->x, P->Lx.get(), (size_t)P->lnz * sizeof(double), hipMemcpyDeviceToDevice, s));
        L->rows.reset();    // (copies of the old values)
        L->tiled.reset();
    }
    CSX_HIP(hipStreamSynchronize(s));
    float ms = 0.0f;
    g_rf_numeric_ms = hipEventElapsedTime(&ms, P->ev_a, P->ev_b) == hipSuccess ? ms : 0.0;
    g_rf_call_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_call).count();
    g_rf_valid = true;
    return CSX_OK;
}

extern "C" int csx_chol_refactor_window(csx_handle_t h, int32_t *window) {
    CholRefPlan *P = (CholRefPlan *)get(h, K_CHOLREFPLAN);
    if (!P || !window) return CSX_EINVAL;
    *window = P->An ? chol_analysis_window(P->An) : 0;
    return CSX_OK;
}

extern "C" int csx_chol_refactor_info(double *numeric_ms, double *call_ms) {
    if (!g_rf_valid) return CSX_EINVAL;   // no csx_chol_refactor has completed yet
    if (numeric_ms) *numeric_ms = g_rf_numeric_ms;
    if (call_ms) *call_ms = g_rf_call_ms;
    return CSX_OK;
}
