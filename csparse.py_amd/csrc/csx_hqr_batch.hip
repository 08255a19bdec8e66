// Many value sets on the analysis of one Householder QR (the definition is the comment of csx_hqr_batch_factor in
// include/csx.h).  An HqrBatch BORROWS an HqrFactor -- the patterns of V and R, the slot views, the entry maps, the height levels
// of the column elimination tree, the launch schedule, the permutations -- and owns B value sets: Vx (B x vnz doubles,
// member-major: member m's column k is the contiguous piece hqr_column expects), Rx (B x rnz), beta (B x n), flags (B x 3),
// stats (B x 3).  It never writes the factor's V.x / R.x / beta or its scratch, and keeps its own launch counters.  What a batch
// of any factorisation is -- the object's common part, the guards, the frame of a run (the flag and stat words set, every member's
// values through winV / winR, of duplicates the map's) -- is csx_valuebatch.h; this file holds what is QR's:
//   HqrBatchColumn  the batch policy of the level walk (csx_levelwalk.h: k_level_batch, k_run_batch): Vx by vnz, Rx by rnz, beta
//                    by n, flags by 3, then HqrColumn::column -- hqr_column itself, the host rule's bits
//   k_hqb_stats      hqr_stats_column per (column, member)
//   the solve        cs_qrsol's two sequences on an m2 x (B r) block: k_hqb_happly_level / k_hqb_happly, csx_qr.hip's two
//                    kernels with the value plane and beta chosen per lane, and csx_batchsolve.h's sweeps of an upper factor
//                    whose diagonal is stored last -- the rows of R from the top level down (cs_usolve), its dots from the
//                    leaves up (cs_utsolve).  R(i, j) != 0 makes i a descendant of j in the column elimination tree, so the
//                    factor's own levels and schedule order both.
// There is NO scratch-then-commit: a member with a non-finite diagonal of R is marked failed (ok[m] = 0, its values mean nothing)
// where the single factor keeps its old values.
#include <cmath>

#include "csx_hqr.h"
#include "csx_internal.h"
#include "csx_valuebatch.h"

#pragma clang fp contract(off)

namespace csx {

constexpr int HQB_LANES = 64;   // columns of X a workgroup of the reflection kernels takes, a lane each (csx_qr.hip's chunk)

struct HqrBatch : ValueBatch {
    static constexpr Kind KIND = K_HQRBATCH, FACTOR_KIND = K_HQRFACTOR;
    DevBuf<double> Vx, Rx, beta;
    int64_t solve_launches = 0;
    // flags per member: the smallest column with a non-finite diagonal, the columns updated in place, one spare word (the stride
    // of every batch); stats: hqr_stats_column's three words, min |r_kk| the first
    HqrBatch() : ValueBatch("csx_hqr_batch", 3, 0) {}
    HqrFactor *factor() const { return static_cast<HqrFactor *>(F); }
};

void destroy(HqrBatch *b) { delete b; }

// ---- factor ------------------------------------------------------------------------------------------------------------------

// The batch policy: the member's own Vx (stride vnz), Rx (stride rnz), beta (stride n) and flags (stride 3); the rest is shared.
struct HqrBatchColumn {
    using Args = ColumnArgs<const int32_t *__restrict__, const int32_t *__restrict__, double *, const int32_t *__restrict__,
                            const int32_t *__restrict__, double *, double *, const int32_t *__restrict__, const int32_t *__restrict__,
                            const int32_t *__restrict__, int *, int64_t, int64_t, int64_t>;
    static __device__ __forceinline__ void column(int32_t k, int32_t member, int w, int lane, const int32_t *Vp, const int32_t *Vi,
                                                  double *Vx, const int32_t *Rp, const int32_t *Ri, double *Rx, double *beta,
                                                  const int32_t *Sp, const int32_t *Srow, const int32_t *Sdst, int *flags, int64_t vnz,
                                                  int64_t rnz, int64_t n) {
        HqrColumn::column(k, w, lane, Vp, Vi, Vx + member * vnz, Rp, Ri, Rx + member * rnz, beta + member * n, Sp, Srow, Sdst,
                          flags + 3 * (int64_t)member);
    }
};

__global__ __launch_bounds__(256) void k_hqb_stats(int32_t n, int64_t rnz, const int32_t *__restrict__ Rp, const double *__restrict__ Rx,
                                                   unsigned long long *st) {
    const int64_t m = blockIdx.y;
    hqr_stats_column((int64_t)blockIdx.x * blockDim.x + threadIdx.x, threadIdx.x & 63, n, Rp, Rx + m * rnz, st + 3 * m);
}

// ---- solve: the reflections -----------------------------------------------------------------------------------------------------
// csx_qr.hip's two kernels with a lane per column c of X (K = B r of them) instead of per right-hand side of one factor: the lane
// reads its member's value plane Vx + (c / r) vnz and beta + (c / r) n, and runs the reference's loops -- the dot product in
// storage order, product and sum rounded separately, tau *= beta, x(i) -= v(i) tau.  The pattern and with it the levels are shared.

__global__ __launch_bounds__(HQB_LANES) void k_hqb_happly(int32_t n, const int32_t *__restrict__ Vp, const int32_t *__restrict__ Vi,
                                                          const double *__restrict__ Vx, const double *__restrict__ beta, double *X,
                                                          int64_t K, int32_t r, int64_t vnz, int transpose) {
    const int64_t c = (int64_t)blockIdx.x * HQB_LANES + threadIdx.x;
    if (c >= K) return;
    const double *vx = Vx + (c / r) * vnz, *bt = beta + (c / r) * n;
    for (int32_t t = 0; t < n; t++) {
        const int32_t k = transpose ? t : n - 1 - t;
        const int32_t pb = Vp[k], pe = Vp[k + 1];
        double tau = 0.0;
        for (int32_t p = pb; p < pe; p++) {
            const double prod = vx[p] * X[(int64_t)Vi[p] * K + c];
            tau = tau + prod;
        }
        tau = tau * bt[k];
        for (int32_t p = pb; p < pe; p++) {
            const double prod = vx[p] * tau;
            X[(int64_t)Vi[p] * K + c] = X[(int64_t)Vi[p] * K + c] - prod;
        }
    }
}

// one level: workgroup = (reflection cols[c0 + blockIdx.x / chunks], chunk of HQB_LANES columns of X)
__global__ __launch_bounds__(HQB_LANES) void k_hqb_happly_level(const int32_t *__restrict__ cols, int32_t c0, int32_t c1,
                                                                const int32_t *__restrict__ Vp, const int32_t *__restrict__ Vi,
                                                                const double *__restrict__ Vx, const double *__restrict__ beta,
                                                                double *X, int64_t K, int32_t r, int64_t vnz, int64_t n,
                                                                int32_t chunks) {
    const int32_t w = (int32_t)blockIdx.x;
    const int32_t ci = c0 + w / chunks;
    const int64_t c = (int64_t)(w % chunks) * HQB_LANES + threadIdx.x;
    if (ci >= c1 || c >= K) return;
    const int32_t k = cols[ci];
    const double *vx = Vx + (c / r) * vnz;
    const int32_t pb = Vp[k], pe = Vp[k + 1];
    double tau = 0.0;
    for (int32_t p = pb; p < pe; p++) {
        const double prod = vx[p] * X[(int64_t)Vi[p] * K + c];
        tau = tau + prod;
    }
    tau = tau * beta[(c / r) * n + k];
    for (int32_t p = pb; p < pe; p++) {
        const double prod = vx[p] * tau;
        X[(int64_t)Vi[p] * K + c] = X[(int64_t)Vi[p] * K + c] - prod;
    }
}

// ---- host -------------------------------------------------------------------------------------------------------------------

static HqrFactor *hqb_factor(const char *who, csx_handle_t hF) {
    HqrFactor *F = (HqrFactor *)get(hF, K_HQRFACTOR);
    if (!F) set_error("%s: F is not a factor of csx_hqr_factor (or has been freed)", who);
    return F;
}

// The row view of R's pattern with its map to storage positions: row i holds (column, position) of its entries with the columns
// DESCENDING, so the diagonal (the smallest column of a row of an upper factor) comes last -- the order in which cs_usolve's
// column loop reaches row i.  Built on the first csx_hqr_batch_solve on F and kept there (R's pattern never changes);
// synchronises.
static int hqb_row_view(HqrFactor *F, const Csc *R) {
    if (F->r_rows) return CSX_OK;
    const size_t n = (size_t)F->n;
    std::vector<int32_t> p, i, rp, rc, rpos;
    CSX_TRY(download_i32(p, R->p, n + 1));
    CSX_TRY(download_i32(i, R->i, (size_t)F->rnz));
    if ((n > 0 ? p[n] : 0) != F->rnz || !row_view(F->n, p.data(), i.data(), true, rp, rc, rpos)) return CSX_EINVAL;
    for (size_t r = 0; r < n; r++)   // every row ends with its diagonal, which is the last entry of column r
        if (rp[r + 1] == rp[r] || rc[(size_t)rp[r + 1] - 1] != (int32_t)r || rpos[(size_t)rp[r + 1] - 1] != p[r + 1] - 1) return CSX_EINVAL;
    CSX_TRY(upload(F->rrp, rp));
    CSX_TRY(upload(F->rrc, rc));
    CSX_TRY(upload(F->rrpos, rpos));
    CSX_HIP(hipStreamSynchronize(ctx().stream));   // (the host lists go out of scope)
    F->r_rows = true;
    return CSX_OK;
}

// every member's factor of V into the batch's arrays; ok[m] = 1 where no diagonal of member m's R is non-finite.  One
// synchronisation.
static int hqb_run(HqrBatch *b, const double *V, int *ok) {
    hipStream_t s = ctx().stream;
    HqrFactor *F = b->factor();
    const Csc *Vm = csc(F->hV), *R = csc(F->hR);
    if (!Vm || !R) return CSX_EINVAL;
    const int32_t n = F->n, B = b->B;
    const int64_t vnz = F->vnz, rnz = F->rnz;
    CSX_TRY(batch_begin(b, nullptr, nullptr));
    batch_scatter(b, V, vnz, F->winV.get(), b->Vx.get(), rnz, F->winR.get(), b->Rx.get());
    walk_levels_batch<HqrBatchColumn>(F, B, &b->level_launches, &b->run_launches, HqrBatchColumn::Args(), Vm->p, Vm->i, b->Vx, R->p,
                                      R->i, b->Rx, b->beta, F->sp, F->srow, F->sdst, b->flags, vnz, rnz, (int64_t)n);
    if (n > 0)
        hipLaunchKernelGGL(k_hqb_stats, dim3((unsigned)(((int64_t)n + 255) / 256), (unsigned)B), dim3(256), 0, s, n, rnz, R->p,
                           b->Rx.get(), b->stats.get());
    return batch_end(b, ok);
}

// Q' W (transpose) or Q W on the m2 x K block W with every member's V.x and beta: csx_happly's launches, whatever B is
static int hqb_happly(HqrBatch *b, Csc *V, double *W, int64_t K, int32_t r, int transpose) {
    hipStream_t s = ctx().stream;
    const HqrFactor *F = b->factor();
    if (V->n == 0) return CSX_OK;
    CSX_TRY(house_levels(V));
    const HouseLevels *H = V->house.get();
    const int32_t chunks = (int32_t)((K + HQB_LANES - 1) / HQB_LANES);
    if (H->nlevels > HAPPLY_MAX_LEVELS || H->nlevels == V->n) {   // csx_happly's rule: nothing to run side by side, one launch
        hipLaunchKernelGGL(k_hqb_happly, dim3((unsigned)chunks), dim3(HQB_LANES), 0, s, V->n, V->p, V->i, b->Vx.get(), b->beta.get(), W,
                           K, r, (int64_t)F->vnz, transpose);
        b->solve_launches++;
        CSX_LAUNCH_CHECK();
        return CSX_OK;
    }
    for (int32_t t = 0; t < H->nlevels; t++) {
        const int32_t l = transpose ? t : H->nlevels - 1 - t;   // Q' x: reflections ascending; Q x: descending
        const int32_t c0 = H->ptr[(size_t)l], c1 = H->ptr[(size_t)l + 1];
        hipLaunchKernelGGL(k_hqb_happly_level, dim3((unsigned)((int64_t)(c1 - c0) * chunks)), dim3(HQB_LANES), 0, s, H->cols.get(), c0,
                           c1, V->p, V->i, b->Vx.get(), b->beta.get(), W, K, r, (int64_t)F->vnz, (int64_t)F->n, chunks);
        b->solve_launches++;
    }
    CSX_LAUNCH_CHECK();
    return CSX_OK;
}

}  // namespace csx

using namespace csx;

extern "C" int csx_hqr_batch_limits(int32_t *out) {   // (no device needed)
    CSX_TRY(batch_limits(out));
    out[6] = HQB_LANES;
    out[7] = HAPPLY_MAX_LEVELS;
    return CSX_OK;
}

extern "C" int csx_hqr_batch_factor(csx_handle_t hF, csx_handle_t hV, int32_t B, csx_handle_t *out, int *ok) {
    CSX_TRY(require_ready());
    if (out) *out = 0;
    HqrFactor *F = hqb_factor("csx_hqr_batch_factor", hF);
    if (!F || !out || !ok) return CSX_EINVAL;
    if (!batch_members_ok("csx_hqr_batch_factor", B)) return CSX_EINVAL;
    const double *V = batch_values("csx_hqr_batch_factor", hV, F->anz, B);
    if (!V) return CSX_EINVAL;
    std::unique_ptr<HqrBatch> b(new HqrBatch());
    CSX_TRY(b->Vx.alloc((size_t)B * (size_t)F->vnz));
    CSX_TRY(b->Rx.alloc((size_t)B * (size_t)F->rnz));
    CSX_TRY(b->beta.alloc((size_t)B * (size_t)F->n));
    CSX_TRY(batch_alloc_common(b.get(), F, hF, B));
    CSX_TRY(hqb_run(b.get(), V, ok));
    *out = put(K_HQRBATCH, b.release());
    return CSX_OK;
}

extern "C" int csx_hqr_batch_refactor(csx_handle_t h, csx_handle_t hV, int *ok) {
    CSX_TRY(require_ready());
    HqrBatch *b = batch_get<HqrBatch>(h);
    if (!b || !ok) return CSX_EINVAL;
    const double *V = batch_values("csx_hqr_batch_refactor", hV, b->F->anz, b->B);
    return V ? hqb_run(b, V, ok) : CSX_EINVAL;
}

extern "C" int csx_hqr_batch_solve(csx_handle_t h, csx_handle_t hXin, csx_handle_t hXout, int32_t r, int second) {
    CSX_TRY(require_ready());
    HqrBatch *b = batch_get<HqrBatch>(h);
    if (!b || r < 1) return CSX_EINVAL;
    HqrFactor *F = b->factor();
    Csc *V = csc(F->hV), *R = csc(F->hR);
    if (!V || !R) return CSX_EINVAL;
    const int64_t m = F->m, n = F->n, m2 = F->m2, K = (int64_t)b->B * r;
    const int64_t rows_in = second ? n : m, rows_out = second ? m : n;
    if (!batch_solve_fits(m2, K) || (n + 1) * ((K + HQB_LANES - 1) / HQB_LANES) > 0x7fffffffll) {
        set_error("csx_hqr_batch_solve: B r = %lld columns are more than one launch takes", (long long)K);
        return CSX_EINVAL;
    }
    const double *Xin = batch_block(hXin, rows_in * K);
    double *Xout = batch_block(hXout, rows_out * K);
    if (!Xin || !Xout || Xin == Xout) {
        set_error("csx_hqr_batch_solve: X is not a block of %lld x B r = %lld doubles and the result one of %lld x %lld, apart",
                  (long long)rows_in, (long long)K, (long long)rows_out, (long long)K);
        return CSX_EINVAL;
    }
    b->solve_launches = 0;
    if (m2 == 0 || rows_out == 0) return CSX_OK;
    for (int32_t mm = 0; mm < b->B; mm++)   // the reference divides by it: what the single solver's triangular solve answers
        if (b->hflags[(size_t)3 * mm] == WALK_NONE && b->hstats[(size_t)3 * mm + 2]) {
            set_error("csx_hqr_batch_solve: R of member %d has an exact zero on its diagonal", (int)mm);
            return CSX_EZEROPIVOT;
        }
    CSX_TRY(hqb_row_view(F, R));
    hipStream_t s = ctx().stream;
    DevBuf<double> W;
    CSX_TRY(W.alloc((size_t)(m2 * K)));
    CSX_HIP(hipMemsetAsync(W.get(), 0, (size_t)(m2 * K) * sizeof(double), s));   // the fictitious rows stay zero
    const BatchPattern P = {R->p, R->i, F->rrp.get(), F->rrc.get(), F->rrpos.get(), n, F->rnz, b->B};
    const int32_t *q = F->perm_q.get(), *pinv = F->perm_p.get();
    auto permute = [&](int64_t rows, const int32_t *p, int scatter, const int *flags, const double *src, double *dst) {
        if (rows == 0) return;
        hipLaunchKernelGGL(k_batch_permute, dim3((unsigned)((rows * K + 255) / 256)), dim3(256), 0, s, rows, K, r, p, scatter, flags, src,
                           dst);
        b->solve_launches++;
    };
    if (!second) {   // W[pinv[i], :] = X[i, :], Q' W, R \ W, out[q[k], :] = W[k, :]
        permute(m, pinv, 1, nullptr, Xin, W.get());
        CSX_TRY(hqb_happly(b, V, W.get(), K, r, 1));
        CSX_TRY(batch_sweep_upper<true>(F, P, b->Rx.get(), r, W.get()));
        b->solve_launches += (int64_t)F->schedule.size();
        permute(n, q, 1, b->flags.get(), W.get(), Xout);
    } else {         // W[k, :] = X[q[k], :], R' \ W, Q W, out[i, :] = W[pinv[i], :]
        permute(n, q, 0, nullptr, Xin, W.get());
        CSX_TRY(batch_sweep_upper<false>(F, P, b->Rx.get(), r, W.get()));
        b->solve_launches += (int64_t)F->schedule.size();
        CSX_TRY(hqb_happly(b, V, W.get(), K, r, 0));
        permute(m, pinv, 0, b->flags.get(), W.get(), Xout);
    }
    CSX_LAUNCH_CHECK();
    CSX_HIP(hipStreamSynchronize(s));   // W goes out of scope
    return CSX_OK;
}

extern "C" int csx_hqr_batch_info(csx_handle_t h, int64_t *shared, int64_t *members) {
    CSX_TRY(require_ready());
    HqrBatch *b = batch_get<HqrBatch>(h);
    if (!b || !shared || !members) return CSX_EINVAL;
    const HqrFactor *F = b->factor();
    shared[0] = F->m;
    shared[1] = F->n;
    shared[2] = F->m2;
    shared[3] = F->vnz;
    shared[4] = F->rnz;
    shared[5] = F->levels();
    shared[6] = b->level_launches + b->run_launches;
    shared[7] = b->level_launches;
    shared[8] = b->run_launches;
    shared[9] = b->kernel_us;
    shared[10] = b->B;
    shared[11] = b->solve_launches;
    for (int32_t m = 0; m < b->B; m++) {
        const int *f = &b->hflags[(size_t)3 * m];
        members[3 * m + 0] = f[0] == WALK_NONE ? -1 : f[0];
        members[3 * m + 1] = f[1];
        members[3 * m + 2] = (int64_t)b->hstats[(size_t)3 * m + 2];
    }
    return CSX_OK;
}

extern "C" int csx_hqr_batch_stats(csx_handle_t h, double *out) {
    CSX_TRY(require_ready());
    HqrBatch *b = batch_get<HqrBatch>(h);
    if (!b || !out) return CSX_EINVAL;
    batch_stats(b, 0, 2, out);
    return CSX_OK;
}

extern "C" int csx_hqr_batch_member(csx_handle_t h, int32_t m, double *Vx_out, double *Rx_out, double *beta_out) {
    CSX_TRY(require_ready());
    HqrBatch *b = batch_get<HqrBatch>(h);
    if (!b || m < 0 || m >= b->B || !Vx_out || !Rx_out || !beta_out) return CSX_EINVAL;
    CSX_TRY(batch_member(b->Vx, m, (size_t)b->factor()->vnz, Vx_out));
    CSX_TRY(batch_member(b->Rx, m, (size_t)b->factor()->rnz, Rx_out));
    CSX_TRY(batch_member(b->beta, m, (size_t)b->F->n, beta_out));
    CSX_HIP(hipStreamSynchronize(ctx().stream));
    return CSX_OK;
}

// out[m n + k] = R_m(k, k): gathered on the device, one download
__global__ __launch_bounds__(256) void k_hqb_diag(int64_t n, int64_t rnz, int32_t B, const int32_t *__restrict__ Rp,
                                                  const double *__restrict__ Rx, double *__restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * B) return;
    const int64_t m = t / n, k = t - m * n;
    out[t] = Rx[m * rnz + Rp[k + 1] - 1];
}

extern "C" int csx_hqr_batch_r_diag(csx_handle_t h, double *out) {
    CSX_TRY(require_ready());
    HqrBatch *b = batch_get<HqrBatch>(h);
    if (!b || !out) return CSX_EINVAL;
    const Csc *R = csc(b->factor()->hR);
    if (!R) return CSX_EINVAL;
    hipStream_t s = ctx().stream;
    const int64_t n = b->F->n, all = n * b->B;
    if (all == 0) return CSX_OK;
    DevBuf<double> d;
    CSX_TRY(d.alloc((size_t)all));
    hipLaunchKernelGGL(k_hqb_diag, dim3((unsigned)((all + 255) / 256)), dim3(256), 0, s, n, (int64_t)b->factor()->rnz, b->B, R->p, b->Rx.get(),
                       d.get());
    CSX_LAUNCH_CHECK();
    CSX_HIP(hipMemcpyAsync(out, d.get(), (size_t)all * sizeof(double), hipMemcpyDeviceToHost, s));
    CSX_HIP(hipStreamSynchronize(s));
    return CSX_OK;
}
