// Refactor: new values for cs_lu's L and U with the pivots and the patterns kept -- the numeric part of a
// left-looking LU on a known schedule.  Column k, in pivot-row space: x = 0 on the rows of U(:,k) and L(:,k); x[pinv[i]] =
// A2(i, k) in storage order; for every entry J of U(:,k) but the last, in storage order: U.x = x[J], x[L.i[t]] -= L.x[t] x[J]
// over L(:,J) after its unit diagonal; the pivot x[k] goes last into U(:,k); L.x = x / pivot after the unit diagonal.
//
// The columns fall into groups that do not depend on one another (btf: the diagonal blocks; lusol: the connected components
// of the pattern of L + U).  A group of at most RF_MAX rows whose columns of A have no duplicate rows is refactored by ONE
// WAVE with x in LDS, its columns one after another, the entries of U(:,k) in storage order; at each J the wave reads x[J]
// once and the updates from L(:,J) are spread over the lanes (distinct rows: the bits do not depend on the lanes' order).
// The other groups run the same statements on the host (csx_host.cpp: lu_refactor_columns) while the launch runs.
#include <algorithm>
#include <cmath>
#include <numeric>

#include "csx_internal.h"
#include "csx_sweep.h"

namespace csx {

int lu_refactor_columns(int32_t n, const int32_t *cols, int32_t ncols, const int32_t *Ap, const int32_t *Ai,
                        const double *Ax, const int32_t *pinv, const int32_t *Lp, const int32_t *Li, double *Lx,
                        const int32_t *Up, const int32_t *Ui, double *Ux, double *x, int *ok, double *ratio);  // csx_host.cpp

// RF_MAX, RF_WAVES: csx_internal.h (csx_btf_limits hands them out)

struct Refactor {
    int32_t n = 0, ngroups = 0;
    int64_t dev_cols = 0, host_cols = 0;
    DevBuf<Tree> groups;          // device groups, biggest first: positions [first, first + count) of gnodes
    DevBuf<int32_t> gnodes, loc;  // columns of the device groups (ascending inside a group); position -> index in its group
    DevBuf<int32_t> aloc;         // per entry of A (factorisation's column order): loc[pinv[row]]
    DevBuf<int> gbad, bad;        // per device group / reduced
    DevBuf<double> gratio, ratio;
    // the host groups: their columns (ascending), runs of consecutive ones, and host copies of the patterns
    std::vector<int32_t> hcols;
    std::vector<std::pair<int32_t, int32_t>> runs;
    std::vector<int32_t> Ap, Ai, pinv, Lp, Li, Up, Ui;
    std::vector<double> ax, Lx, Ux, x;
    hipEvent_t ax_ready = nullptr;   // recorded after A's values come down for the host groups
    Refactor() = default;
    Refactor(const Refactor &) = delete;
    Refactor &operator=(const Refactor &) = delete;
    ~Refactor() {
        if (ax_ready) (void)hipEventDestroy(ax_ready);
    }
};

void destroy(Refactor *R) { delete R; }

static unsigned grid_for(int64_t count) { return (unsigned)std::max<int64_t>(1, (count + 255) / 256); }

// Cross-lane hand-over inside one wave through LDS: every LDS write issued before it has landed, and the compiler keeps
// the wave's LDS accesses on their side of it (the memory clobber).  The wave runs in lock step: no workgroup barrier.
__device__ __forceinline__ void wave_lds_sync() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
}

#pragma clang fp contract(off)   // multiply and subtract rounded separately, as the host loop and cs_lu
__global__ __launch_bounds__(64 * RF_WAVES) void k_refactor(const Tree *__restrict__ groups, int32_t ngroups,
                                                            const int32_t *__restrict__ gnodes,
                                                            const int32_t *__restrict__ loc, const int32_t *__restrict__ Ap,
                                                            const int32_t *__restrict__ aloc, const double *__restrict__ Ax,
                                                            const int32_t *__restrict__ Lp, const int32_t *__restrict__ Li,
                                                            double *Lx, const int32_t *__restrict__ Up,
                                                            const int32_t *__restrict__ Ui, double *__restrict__ Ux,
                                                            int *__restrict__ gbad, double *__restrict__ gratio) {
    __shared__ double xs[RF_WAVES][RF_MAX];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t g = (int64_t)blockIdx.x * RF_WAVES + w;
    if (g >= ngroups) return;
    double *x = xs[w];
    const Tree tr = groups[g];
    double rmin = 1.0;
    int bad = 0;
    for (int32_t c = 0; c < tr.count; c++) {
        const int32_t k = gnodes[tr.first + c];
        const int32_t u0 = Up[k], ue = Up[k + 1] - 1, l0 = Lp[k], le = Lp[k + 1];
        for (int32_t t = u0 + lane; t <= ue; t += 64) x[loc[Ui[t]]] = 0.0;
        for (int32_t t = l0 + lane; t < le; t += 64) x[loc[Li[t]]] = 0.0;
        wave_lds_sync();
        for (int32_t t = Ap[k] + lane; t < Ap[k + 1]; t += 64) x[aloc[t]] = Ax[t];
        wave_lds_sync();
        for (int32_t t = u0; t < ue; t++) {
            const int32_t J = Ui[t];
            const double xj = x[loc[J]];
            if (lane == 0) Ux[t] = xj;
            // L(:,J)'s values were written by this refactor, entry s by lane (s - Lp[J] - 1) % 64: the lane that reads it here
            for (int32_t s = Lp[J] + 1 + lane; s < Lp[J + 1]; s += 64) {
                const int32_t r = loc[Li[s]];
                const double prod = Lx[s] * xj;
                x[r] = x[r] - prod;
            }
            wave_lds_sync();
        }
        const double piv = x[loc[k]];
        double big = fabs(piv);
        for (int32_t s = l0 + 1 + lane; s < le; s += 64) big = fmax(big, fabs(x[loc[Li[s]]]));
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) big = fmax(big, __shfl_xor(big, off));
        if (lane == 0) {
            Ux[ue] = piv;
            Lx[l0] = 1.0;
        }
        for (int32_t s = l0 + 1 + lane; s < le; s += 64) Lx[s] = x[loc[Li[s]]] / piv;
        wave_lds_sync();   // the next column zeroes slots read above
        if (piv == 0.0 || !__builtin_isfinite(piv)) {
            bad = 1;
            break;
        }
        rmin = fmin(rmin, fabs(piv) / big);
    }
    if (lane == 0) {
        gbad[g] = bad;
        gratio[g] = rmin;
    }
}
#pragma clang fp contract(fast)

// bad = any group's flag, ratio = the smallest group ratio (one workgroup; min and max do not depend on the order)
__global__ __launch_bounds__(256) void k_refactor_reduce(int32_t ngroups, const int *__restrict__ gbad,
                                                         const double *__restrict__ gratio, int *bad, double *ratio) {
    __shared__ int sb[256];
    __shared__ double sr[256];
    int b = 0;
    double r = 1.0;
    for (int32_t g = threadIdx.x; g < ngroups; g += 256) {
        b |= gbad[g];
        r = fmin(r, gratio[g]);
    }
    sb[threadIdx.x] = b;
    sr[threadIdx.x] = r;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) {
            sb[threadIdx.x] |= sb[threadIdx.x + h];
            sr[threadIdx.x] = fmin(sr[threadIdx.x], sr[threadIdx.x + h]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        *bad = sb[0];
        *ratio = sr[0];
    }
}

__global__ __launch_bounds__(256) void k_rf_gather(int64_t cnt, const int32_t *__restrict__ map, const double *__restrict__ src,
                                                   double *__restrict__ dst) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < cnt) dst[t] = src[map[t]];
}

__global__ __launch_bounds__(256) void k_rf_iota(int64_t cnt, double *__restrict__ x) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < cnt) x[t] = (double)t;
}

__global__ __launch_bounds__(256) void k_rf_to_index(int64_t cnt, const double *__restrict__ x, int32_t *__restrict__ map) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < cnt) map[t] = (int32_t)x[t];
}

__global__ __launch_bounds__(256) void k_rf_differ(int64_t cnt, const int32_t *__restrict__ a, const int32_t *__restrict__ b,
                                                   int *differ) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < cnt && a[t] != b[t]) *differ = 1;
}

int rf_gather(int64_t cnt, const int32_t *map, const double *src, double *dst) {
    if (cnt > 0) hipLaunchKernelGGL(k_rf_gather, dim3(grid_for(cnt)), dim3(256), 0, ctx().stream, cnt, map, src, dst);
    CSX_LAUNCH_CHECK();
    return CSX_OK;
}

// a new matrix handle: A's pattern, x[t] = t (exact in binary64): run through the pattern builders, its values say where
// every entry of the result came from
int rf_index_copy(const Csc *A, csx_handle_t *out) {
    std::unique_ptr<Csc> C;
    CSX_TRY(csc_copy_pattern(A->m, A->n, A->nnz, A->p, A->i, true, &C));
    if (A->nnz) {
        hipLaunchKernelGGL(k_rf_iota, dim3(grid_for(A->nnz)), dim3(256), 0, ctx().stream, (int64_t)A->nnz, C->x);
        CSX_LAUNCH_CHECK();
    }
    *out = put(K_CSC, C.release());
    return CSX_OK;
}

// map[t] = x[t] of an index-valued result
int rf_index_map(const double *x, int64_t cnt, DevBuf<int32_t> &map) {
    CSX_TRY(map.alloc((size_t)cnt));
    if (cnt > 0) hipLaunchKernelGGL(k_rf_to_index, dim3(grid_for(cnt)), dim3(256), 0, ctx().stream, cnt, x, map.get());
    CSX_LAUNCH_CHECK();
    return CSX_OK;
}

// A's pattern kept for the check of every A2 (pointers and row indices)
int rf_keep_pattern(const Csc *A, DevBuf<int32_t> &p, DevBuf<int32_t> &i) {
    hipStream_t s = ctx().stream;
    CSX_TRY(p.alloc((size_t)A->n + 1));
    CSX_TRY(i.alloc((size_t)A->nnz));
    CSX_HIP(hipMemcpyAsync(p, A->p, ((size_t)A->n + 1) * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    if (A->nnz) CSX_HIP(hipMemcpyAsync(i, A->i, (size_t)A->nnz * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    return CSX_OK;
}

// *differ: a[0 .. cnt) is not b[0 .. cnt), or a2[0 .. cnt2) is not b2[0 .. cnt2) (cnt2 may be 0).  flag: one int of device
// scratch.  Synchronises.
int rf_differ(int64_t cnt, const int32_t *a, const int32_t *b, int *flag, int *differ, int64_t cnt2, const int32_t *a2,
              const int32_t *b2) {
    hipStream_t s = ctx().stream;
    CSX_HIP(hipMemsetAsync(flag, 0, sizeof(int), s));
    if (cnt) hipLaunchKernelGGL(k_rf_differ, dim3(grid_for(cnt)), dim3(256), 0, s, cnt, a, b, flag);
    if (cnt2) hipLaunchKernelGGL(k_rf_differ, dim3(grid_for(cnt2)), dim3(256), 0, s, cnt2, a2, b2, flag);
    CSX_LAUNCH_CHECK();
    CSX_HIP(hipMemcpyAsync(differ, flag, sizeof(int), hipMemcpyDeviceToHost, s));
    CSX_HIP(hipStreamSynchronize(s));
    return CSX_OK;
}

// The values of A2 (a matrix with the kept pattern, or a vector of nnz values): *x; *x = nullptr (CSX_OK) when A2's pattern or
// length differs from A's; CSX_EINVAL for a handle that is neither or a matrix without values.  flag: one int of scratch.
int rf_values(csx_handle_t hA2, int32_t m, int32_t n, int32_t nnz, const int32_t *p0, const int32_t *i0, int *flag,
              const double **x) {
    if (Csc *A2 = csc(hA2)) {
        *x = nullptr;
        if (!A2->x) return CSX_EINVAL;
        if (A2->m != m || A2->n != n || A2->nnz != nnz) return CSX_OK;
        if (!A2->trusted) CSX_TRY(csc_validate(A2));
        int differ = 0;
        CSX_TRY(rf_differ((int64_t)n + 1, A2->p, p0, flag, &differ, nnz, A2->i, i0));
        if (!differ) *x = A2->x;
        return CSX_OK;
    }
    Vec *v = vec(hA2);
    if (!v) return CSX_EINVAL;
    *x = v->len == nnz ? (const double *)v->d : nullptr;
    return CSX_OK;
}

// The schedule of a refactor.  A: the matrix in the factorisation's column order (pattern, device); pinv (host, n); L, U:
// cs_lu's factors (device); gid (host, n, or empty): the group of every position (btf: its block), empty = the connected
// components of L + U.  CSX_EINVAL when the factors do not have cs_lu's shape or A(:,k) has a row outside L(:,k) + U(:,k).
int refactor_build(const Csc *A, const int32_t *pinv_h, const Csc *L, const Csc *U, const std::vector<int32_t> &gid_in,
                   Refactor **out) {
    const int32_t n = A->n;
    if (A->m != n || L->n != n || L->m != n || U->n != n || U->m != n) return CSX_EINVAL;
    std::unique_ptr<Refactor> R(new Refactor());
    R->n = n;
    std::vector<int32_t> Ap, Ai, Lp, Li, Up, Ui;
    CSX_TRY(download_i32(Ap, A->p, (size_t)n + 1));
    CSX_TRY(download_i32(Ai, A->i, (size_t)A->nnz));
    CSX_TRY(download_i32(Lp, L->p, (size_t)n + 1));
    CSX_TRY(download_i32(Li, L->i, (size_t)L->nnz));
    CSX_TRY(download_i32(Up, U->p, (size_t)n + 1));
    CSX_TRY(download_i32(Ui, U->i, (size_t)U->nnz));
    std::vector<int32_t> pinv(pinv_h, pinv_h + n), mark((size_t)n, -1);
    for (int32_t i = 0; i < n; i++) {
        if (pinv[i] < 0 || pinv[i] >= n || mark[pinv[i]] >= 0) return CSX_EINVAL;
        mark[pinv[i]] = n;
    }
    // the groups: given, or the connected components of the pattern of L + U (union-find, the smaller root kept)
    std::vector<int32_t> gid;
    if (gid_in.empty()) {
        std::vector<int32_t> par((size_t)n);
        std::iota(par.begin(), par.end(), 0);
        auto find = [&](int32_t v) {
            while (par[v] != v) v = par[v] = par[par[v]];
            return v;
        };
        auto unite = [&](int32_t a, int32_t b) {
            a = find(a);
            b = find(b);
            if (a != b) par[std::max(a, b)] = std::min(a, b);
        };
        for (int32_t k = 0; k < n; k++) {
            for (int32_t t = Lp[k]; t < Lp[k + 1]; t++)
                if (Li[t] >= 0 && Li[t] < n) unite(k, Li[t]);
            for (int32_t t = Up[k]; t < Up[k + 1]; t++)
                if (Ui[t] >= 0 && Ui[t] < n) unite(k, Ui[t]);
        }
        gid.resize((size_t)n);
        for (int32_t k = 0; k < n; k++) gid[k] = find(k);   // the root is the group's smallest position
    } else {
        gid = gid_in;
    }
    // checks: cs_lu's shape, every entry inside its column's group, A(:,k)'s rows among L(:,k) + U(:,k); duplicates
    std::vector<char> dup_group((size_t)n, 0);
    std::vector<int32_t> amark((size_t)n, -1);
    if (Ap[0] != 0 || Lp[0] != 0 || Up[0] != 0) return CSX_EINVAL;
    for (int32_t k = 0; k < n; k++) {
        if (Ap[k + 1] < Ap[k] || Lp[k + 1] <= Lp[k] || Up[k + 1] <= Up[k]) return CSX_EINVAL;
        if (Li[Lp[k]] != k || Ui[Up[k + 1] - 1] != k) return CSX_EINVAL;
        const int32_t gk = gid[k];
        if (gk < 0 || gk >= n) return CSX_EINVAL;
        for (int32_t t = Lp[k]; t < Lp[k + 1]; t++) {
            if (Li[t] < k || Li[t] >= n || gid[Li[t]] != gk) return CSX_EINVAL;
            mark[Li[t]] = k;
        }
        for (int32_t t = Up[k]; t < Up[k + 1]; t++) {
            if (Ui[t] < 0 || Ui[t] > k || gid[Ui[t]] != gk) return CSX_EINVAL;
            mark[Ui[t]] = k;
        }
        for (int32_t t = Ap[k]; t < Ap[k + 1]; t++) {
            if (Ai[t] < 0 || Ai[t] >= n || mark[pinv[Ai[t]]] != k) return CSX_EINVAL;
            if (amark[Ai[t]] == k) dup_group[gk] = 1;
            amark[Ai[t]] = k;
        }
    }
    // positions of every group, ascending; the device takes groups of at most RF_MAX rows without duplicate entries
    std::vector<int32_t> cnt((size_t)n + 1, 0), locv((size_t)n, 0);
    for (int32_t k = 0; k < n; k++) locv[k] = cnt[gid[k]]++;
    std::vector<int32_t> start((size_t)n + 1, 0);
    std::vector<Tree> trees;
    int32_t dev_total = 0;
    for (int32_t g = 0; g < n; g++) {
        if (cnt[g] == 0) continue;
        if (cnt[g] <= RF_MAX && !dup_group[g]) {
            start[g] = dev_total;
            trees.push_back(Tree{dev_total, cnt[g]});
            dev_total += cnt[g];
        } else {
            start[g] = -1;
        }
    }
    std::vector<int32_t> gnodes((size_t)dev_total), aloc((size_t)Ap[n]);
    for (int32_t k = 0; k < n; k++) {
        if (start[gid[k]] >= 0) {
            gnodes[start[gid[k]] + locv[k]] = k;
        } else {
            if (!R->runs.empty() && R->runs.back().second == k) R->runs.back().second = k + 1;
            else R->runs.push_back({k, k + 1});
            R->hcols.push_back(k);
        }
    }
    for (int32_t k = 0; k < n; k++)
        for (int32_t t = Ap[k]; t < Ap[k + 1]; t++) aloc[t] = locv[pinv[Ai[t]]];
    R->dev_cols = dev_total;
    R->host_cols = (int64_t)R->hcols.size();
    R->ngroups = (int32_t)trees.size();
    CSX_TRY(upload(R->gnodes, gnodes));
    CSX_TRY(upload(R->loc, locv));
    CSX_TRY(upload(R->aloc, aloc));
    CSX_TRY(R->gbad.alloc((size_t)std::max<int32_t>(R->ngroups, 1)));
    CSX_TRY(R->gratio.alloc((size_t)std::max<int32_t>(R->ngroups, 1)));
    CSX_TRY(R->bad.alloc(1));
    CSX_TRY(R->ratio.alloc(1));
    if (R->ngroups) {
        DevBuf<Tree> tr;
        CSX_TRY(upload(tr, trees));
        CSX_TRY(trees_biggest_first(tr, R->ngroups, RF_MAX, &R->groups));
    }
    if (!R->hcols.empty()) {
        R->Ap = std::move(Ap);
        R->Ai = std::move(Ai);
        R->pinv = std::move(pinv);
        R->Lp = std::move(Lp);
        R->Li = std::move(Li);
        R->Up = std::move(Up);
        R->Ui = std::move(Ui);
        R->ax.resize(R->Ai.size());
        R->Lx.resize(R->Li.size());
        R->Ux.resize(R->Ui.size());
        R->x.assign((size_t)n, 0.0);
        CSX_HIP(hipEventCreateWithFlags(&R->ax_ready, hipEventDisableTiming));
    }
    CSX_HIP(hipStreamSynchronize(ctx().stream));
    *out = R.release();
    return CSX_OK;
}

// Lx, Ux (device, nnz(L) / nnz(U)) <- the refactor of the values Ax (device, A's column order) on the factors' patterns
// (L, U: the ones refactor_build saw).  Synchronises; *ok, *ratio as csx_lu_refactor_host.
int refactor_run(Refactor *R, const Csc *A, const double *Ax, const Csc *L, const Csc *U, double *Lx, double *Ux, int *ok,
                 double *ratio) {
    hipStream_t s = ctx().stream;
    // the host groups' copy of A's values is queued ahead of the launch: the host loop then runs while the device groups do
    if (!R->hcols.empty()) {
        CSX_HIP(hipMemcpyAsync(R->ax.data(), Ax, R->ax.size() * sizeof(double), hipMemcpyDeviceToHost, s));
        CSX_HIP(hipEventRecord(R->ax_ready, s));
    }
    if (R->ngroups) {
        hipLaunchKernelGGL(k_refactor, dim3((unsigned)((R->ngroups + RF_WAVES - 1) / RF_WAVES)), dim3(64 * RF_WAVES), 0, s,
                           R->groups.get(), R->ngroups, R->gnodes.get(), R->loc.get(), A->p, R->aloc.get(), Ax, L->p, L->i,
                           Lx, U->p, U->i, Ux, R->gbad.get(), R->gratio.get());
        CSX_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_refactor_reduce, dim3(1), dim3(256), 0, s, R->ngroups, R->gbad.get(), R->gratio.get(),
                           R->bad.get(), R->ratio.get());
        CSX_LAUNCH_CHECK();
    }
    int hok = 1;
    double hratio = 1.0;
    if (!R->hcols.empty()) {
        CSX_HIP(hipEventSynchronize(R->ax_ready));
        CSX_TRY(lu_refactor_columns(R->n, R->hcols.data(), (int32_t)R->hcols.size(), R->Ap.data(), R->Ai.data(), R->ax.data(),
                                    R->pinv.data(), R->Lp.data(), R->Li.data(), R->Lx.data(), R->Up.data(), R->Ui.data(),
                                    R->Ux.data(), R->x.data(), &hok, &hratio));
        if (hok)   // (disjoint from what the kernel writes: other groups' columns)
            for (const auto &run : R->runs) {
                const int32_t a = R->Lp[run.first], e = R->Lp[run.second];
                const int32_t ua = R->Up[run.first], ueo = R->Up[run.second];
                if (e > a) CSX_HIP(hipMemcpyAsync(Lx + a, R->Lx.data() + a, (size_t)(e - a) * sizeof(double), hipMemcpyHostToDevice, s));
                if (ueo > ua)
                    CSX_HIP(hipMemcpyAsync(Ux + ua, R->Ux.data() + ua, (size_t)(ueo - ua) * sizeof(double), hipMemcpyHostToDevice, s));
            }
    }
    int dbad = 0;
    double dratio = 1.0;
    if (R->ngroups) {
        CSX_HIP(hipMemcpyAsync(&dbad, R->bad.get(), sizeof(int), hipMemcpyDeviceToHost, s));
        CSX_HIP(hipMemcpyAsync(&dratio, R->ratio.get(), sizeof(double), hipMemcpyDeviceToHost, s));
    }
    CSX_HIP(hipStreamSynchronize(s));
    *ok = hok && !dbad;
    *ratio = std::fmin(hratio, dratio);
    return CSX_OK;
}

void refactor_counts(const Refactor *R, int64_t *cols) {
    if (!cols) return;
    cols[0] = R ? R->dev_cols : 0;
    cols[1] = R ? R->host_cols : 0;
}

// ------------------------------------------------------------------------------------------------- lusol side --

struct LuRefPlan {
    csx_handle_t hL = 0, hU = 0;
    int32_t n = 0, anz = 0;
    DevBuf<int32_t> p0, i0;   // A's pattern: every A2 is checked against it
    DevBuf<int32_t> qmap;     // entry t of A(:, q) is entry qmap[t] of A
    Csc Aq;                   // A(:, q): the pattern the refactor walks (x: the gathered values of the current A2)
    DevBuf<double> Lx, Ux;    // scratch: committed only when every pivot passed
    DevBuf<int> flag;
    Refactor *R = nullptr;
    LuRefPlan() = default;
    LuRefPlan(const LuRefPlan &) = delete;
    LuRefPlan &operator=(const LuRefPlan &) = delete;
    ~LuRefPlan() { destroy(R); }
};

void destroy(LuRefPlan *P) { delete P; }

}  // namespace csx

using namespace csx;

extern "C" int csx_lu_refactor_plan(csx_handle_t hL, csx_handle_t hU, csx_handle_t hA, const int32_t *q, const int32_t *pinv,
                                    csx_handle_t *out) {
    CSX_TRY(require_ready());
    Csc *L = csc(hL), *U = csc(hU), *A = csc(hA);
    if (!L || !U || !A || !L->x || !U->x || !pinv || !out || A->m != A->n || L->n != A->n) return CSX_EINVAL;
    const int32_t n = A->n;
    if (q) {
        std::vector<char> seen((size_t)n, 0);
        for (int32_t k = 0; k < n; k++) {
            if (q[k] < 0 || q[k] >= n || seen[q[k]]) return CSX_EINVAL;
            seen[q[k]] = 1;
        }
    }
    std::unique_ptr<LuRefPlan> P(new LuRefPlan());
    P->hL = hL;
    P->hU = hU;
    P->n = n;
    P->anz = A->nnz;
    CSX_TRY(rf_keep_pattern(A, P->p0, P->i0));
    // A(:, q) of an index-valued copy of A: its pattern is the refactor's, its values the gather map
    csx_handle_t hI = 0, hQ = 0;
    CSX_TRY(rf_index_copy(A, &hI));
    int st = csx_permute(hI, nullptr, q, 1, &hQ);
    csx_free(hI);
    CSX_TRY(st);
    Csc *Q = csc(hQ);
    st = rf_index_map(Q->x, Q->nnz, P->qmap);
    if (st == CSX_OK) {
        P->Aq.m = Q->m;
        P->Aq.n = Q->n;
        P->Aq.nnz = Q->nnz;
        std::swap(P->Aq.p, Q->p);
        std::swap(P->Aq.i, Q->i);
        std::swap(P->Aq.x, Q->x);   // (reused as the gathered values)
        CSX_HIP(hipStreamSynchronize(ctx().stream));
    }
    csx_free(hQ);
    CSX_TRY(st);
    CSX_TRY(refactor_build(&P->Aq, pinv, L, U, {}, &P->R));
    CSX_TRY(P->flag.alloc(1));
    *out = put(K_LUREFPLAN, P.release());
    return CSX_OK;
}

extern "C" int csx_lu_refactor(csx_handle_t h, csx_handle_t hA2, int *ok, double *ratio, int64_t *cols) {
    CSX_TRY(require_ready());
    LuRefPlan *P = (LuRefPlan *)get(h, K_LUREFPLAN);
    if (!P || !ok || !ratio) return CSX_EINVAL;
    Csc *L = csc(P->hL), *U = csc(P->hU);
    if (!L || !U || !L->x || !U->x || L->n != P->n || U->n != P->n) return CSX_EINVAL;
    const double *x2 = nullptr;
    CSX_TRY(rf_values(hA2, P->n, P->n, P->anz, P->p0, P->i0, P->flag, &x2));
    if (!x2) {
        *ok = -1;   // another pattern: nothing changes
        return CSX_OK;
    }
    hipStream_t s = ctx().stream;
    if (!P->Lx.get()) {
        CSX_TRY(P->Lx.alloc((size_t)L->nnz));
        CSX_TRY(P->Ux.alloc((size_t)U->nnz));
    }
    CSX_TRY(rf_gather(P->anz, P->qmap, x2, P->Aq.x));
    CSX_TRY(refactor_run(P->R, &P->Aq, P->Aq.x, L, U, P->Lx, P->Ux, ok, ratio));
    refactor_counts(P->R, cols);
    if (!*ok) return CSX_OK;
    if (L->nnz) CSX_HIP(hipMemcpyAsync(L->x, P->Lx, (size_t)L->nnz * sizeof(double), hipMemcpyDeviceToDevice, s));
    if (U->nnz) CSX_HIP(hipMemcpyAsync(U->x, P->Ux, (size_t)U->nnz * sizeof(double), hipMemcpyDeviceToDevice, s));
    for (Csc *M : {L, U}) {
        M->rows.reset();
        M->tiled.reset();
    }
    CSX_HIP(hipStreamSynchronize(s));
    return CSX_OK;
}
