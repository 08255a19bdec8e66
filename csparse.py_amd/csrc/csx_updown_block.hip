// updown_block: k rank-1 Cholesky updates / downdates L L' + sum_t sigma_t w_t w_t' in one pass over the union of their
// elimination-tree paths, L.x byte-equal to the loop `for t: if not cs_updown(L, sigma_t, C(:,t)): break`.
//
// Why the bits are the loop's: at a column j, term t of the loop sees L(:,j) after the terms before it that pass through j
// and before any term after it, and its own w_t and beta_t as its walk left them below j.  Here the columns of a tree are
// taken in ascending order (topological: parent[j] > j), and at each column the terms whose path holds it run in ascending
// order, each with the reference's operations (k_updown's, contraction off).  A term reads and writes only its own w_t and
// beta_t, so it sees the same operands as in the loop.
//
// Schedule.  A term's path lies in one tree of the elimination forest: the terms are grouped by the root of their path (a
// walk per term on the device, k_ud_terms).  Within a tree the terms are taken in ascending order, 64 at a time: CHUNK s of
// the call holds ranks [64 s, 64 s + 64) of every tree, bit (rank mod 64) of a 64-bit mask.  A chunk's walks mark the union
// of its paths (k_ud_walk: one atomic OR per path column; the first to mark a column lists it), the host sorts the union by
// (tree, column) -- nothing of length n leaves the device -- and every tree of the chunk is one workgroup (k_ud_block):
// trees share nothing, workgroups never wait on one another.  Chunks run in order: per tree that is the loop again.
//
// Per column j of a tree: (a) one lane runs the scalar chain of the terms in j's mask (alpha, beta2, the failure test, sqrt,
// delta, gamma, L(j,j)), L(j,j) and beta_t carried from term to term; (b) the lanes take the entries below the diagonal,
// each loading L(q) once, applying the mask's terms in order to it and to W(row, t), and storing it once; (c) a barrier.
// W holds w_t on the union rows only (every row of a union column is a union column of its tree): in LDS when it fits.
//
// Failure.  A downdate that is not positive definite at term t, column j: terms >= t of that tree stop (the later ones
// depend on t), terms < t go on (they do not).  The smallest failing t over all trees, taken with an atomic min, is the
// loop's first failing column.  Every chunk snapshots its union columns' values before it runs (k_ud_prep); after a failure
// the snapshots are put back, last chunk first, and, unless all-or-nothing is asked for, the chunks run again with terms
// [0, t] only: term t stops where the loop's stops, the terms before it apply in full.
#include <algorithm>
#include <climits>

#include "csx_internal.h"

namespace csx {

namespace {

struct UdGroup {        // one tree of the elimination forest in one chunk
    int32_t u0, ucnt;   // its union columns: [u0, u0 + ucnt) of the chunk's sorted lists, ascending
    int32_t t0, nterm;  // its terms in the chunk: [t0, t0 + nterm) of the chunk's term list; term t0 + b is mask bit b
    int64_t woff;       // W: ucnt x nterm doubles, row-major by union column, at woff of the chunk's scratch
    int32_t tree;       // index of the tree (over the whole call)
    int32_t pad;
};

constexpr int UD_BATCH = 16;      // terms whose W loads a lane issues together
constexpr int UD_LDS_W = 60 * 1024;   // bytes of W a workgroup may keep in LDS (with the kernel's own 3 KB: under 64 KB)

__device__ __forceinline__ int32_t ud_next(int32_t j, const int32_t *__restrict__ Lp, const int32_t *__restrict__ Li,
                                           const int32_t *__restrict__ parent) {
    if (parent) return parent[j];
    const int32_t p = Lp[j];
    return Lp[j + 1] - p > 1 ? Li[p + 1] : -1;
}

// the given tree against L's: parent[j] = the row of the second entry of column j, -1 when the column holds its diagonal only
__global__ __launch_bounds__(256) void k_ud_check_parent(int32_t n, const int32_t *__restrict__ Lp, const int32_t *__restrict__ Li,
                                                         const int32_t *__restrict__ parent, int *bad) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    if (parent[j] != ud_next((int32_t)j, Lp, Li, nullptr)) *bad = 1;
}

// per column t of C: f = its smallest row (-1: empty), the root of f's path and the path's length.  err bits: 1 a row out of
// range, 2 a row outside L(:, f)'s pattern (checked when pattern != 0), 4 L is not Cholesky-shaped along the path
__global__ __launch_bounds__(64) void k_ud_terms(int32_t k, int32_t n, const int32_t *__restrict__ Cp, const int32_t *__restrict__ Ci,
                                                 const int32_t *__restrict__ Lp, const int32_t *__restrict__ Li,
                                                 const int32_t *__restrict__ parent, int pattern, int32_t *__restrict__ f_out,
                                                 int32_t *__restrict__ root_out, int32_t *__restrict__ len_out, int *err) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= k) return;
    const int32_t b = Cp[t], e = Cp[t + 1];
    f_out[t] = root_out[t] = -1;
    len_out[t] = 0;
    if (b >= e) return;
    int32_t f = n;
    for (int32_t q = b; q < e; q++) {
        const int32_t r = Ci[q];
        if (r < 0 || r >= n) {
            atomicOr(err, 1);
            return;
        }
        f = min(f, r);
    }
    if (pattern) {   // every row of C(:,t) in L(:, f) (rows ascending): the update leaves L's pattern as it is
        const int32_t lb = Lp[f], le = Lp[f + 1];
        for (int32_t q = b; q < e; q++) {
            const int32_t r = Ci[q];
            int32_t lo = lb, hi = le;
            while (lo < hi) {
                const int32_t mid = lo + (hi - lo) / 2;
                if (Li[mid] < r) lo = mid + 1;
                else hi = mid;
            }
            if (lo >= le || Li[lo] != r) atomicOr(err, 2);
        }
    }
    int32_t j = f, len = 1;
    for (;;) {
        const int32_t nx = ud_next(j, Lp, Li, parent);
        if (nx == -1) break;
        if (nx <= j || nx >= n) {
            atomicOr(err, 4);
            break;
        }
        j = nx;
        len++;
    }
    f_out[t] = f;
    root_out[t] = j;
    len_out[t] = len;
}

// a chunk's walks: mark[j] |= the term's bit on every path column; the first to mark a column lists it (ucol, and the group)
__global__ __launch_bounds__(64) void k_ud_walk(int32_t nt, const int32_t *__restrict__ tf, const int32_t *__restrict__ tbit,
                                                const int32_t *__restrict__ tgroup, const int32_t *__restrict__ Lp,
                                                const int32_t *__restrict__ Li, const int32_t *__restrict__ parent,
                                                unsigned long long *mark, int32_t *cnt, int32_t *__restrict__ ucol,
                                                int32_t *__restrict__ ugrp) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nt) return;
    const unsigned long long bit = 1ull << tbit[i];
    const int32_t g = tgroup[i];
    for (int32_t j = tf[i]; j != -1; j = ud_next(j, Lp, Li, parent)) {
        if (atomicOr(&mark[j], bit) == 0ull) {
            const int32_t at = atomicAdd(cnt, 1);
            ucol[at] = j;
            ugrp[at] = g;
        }
    }
}

// the listed columns' masks and lengths; mark goes back to 0 for the next chunk
__global__ __launch_bounds__(256) void k_ud_collect(const int32_t *cnt, const int32_t *__restrict__ ucol, unsigned long long *mark,
                                                    unsigned long long *__restrict__ umask, int32_t *__restrict__ ulen,
                                                    const int32_t *__restrict__ Lp) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= *cnt) return;
    const int32_t j = ucol[i];
    umask[i] = mark[j];
    mark[j] = 0ull;
    ulen[i] = Lp[j + 1] - Lp[j];
}

// pos[j] = the place of union column j in its tree's list
__global__ __launch_bounds__(256) void k_ud_pos(int32_t U, const int32_t *__restrict__ ucol, const int32_t *__restrict__ uloc,
                                                int32_t *__restrict__ pos) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < U) pos[ucol[i]] = uloc[i];
}

// is r union column u of group G?  (pos is not cleared between calls: a stale entry fails the comparison)
__device__ __forceinline__ bool ud_member(const UdGroup &G, int32_t u, int32_t r, const int32_t *__restrict__ ucol) {
    return u >= 0 && u < G.ucnt && ucol[G.u0 + u] == r;
}

// one wave per union column: the snapshot of its values and the W row of every entry; err = 8 when an entry's row is not a
// later union column of the tree or the diagonal is not first (L is not Cholesky-shaped)
__global__ __launch_bounds__(256) void k_ud_prep(int32_t U, const int32_t *__restrict__ ucol, const int32_t *__restrict__ ugrp,
                                                 const int64_t *__restrict__ usoff, const UdGroup *__restrict__ groups,
                                                 const int32_t *__restrict__ pos, const int32_t *__restrict__ Lp,
                                                 const int32_t *__restrict__ Li, const double *__restrict__ Lx,
                                                 double *__restrict__ snap, int32_t *__restrict__ rowslot, int2 *__restrict__ upe,
                                                 int *err) {
    const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
    const int lane = threadIdx.x & (WAVE - 1);
    if (i >= U) return;
    const int32_t j = ucol[i], p = Lp[j], len = Lp[j + 1] - p;
    if (lane == 0) upe[i] = make_int2(p, p + len);
    const UdGroup G = groups[ugrp[i]];
    const int64_t o = usoff[i];
    for (int32_t e = lane; e < len; e += WAVE) {
        const int32_t r = Li[p + e];
        snap[o + e] = Lx[p + e];
        int32_t u = 0;
        if (e == 0) {
            if (r != j) atomicOr(err, 8);
        } else {
            u = pos[r];
            if (r <= j || !ud_member(G, u, r, ucol)) atomicOr(err, 8);
        }
        rowslot[o + e] = u;
    }
}

// W(u, b) = C's entries of term t0 + b on its path, in storage order (a later duplicate row wins); W is zero before
__global__ __launch_bounds__(64) void k_ud_w_init(int32_t nt, const int32_t *__restrict__ tglob, const int32_t *__restrict__ tgroup,
                                                  const int32_t *__restrict__ tbit, const UdGroup *__restrict__ groups,
                                                  const int32_t *__restrict__ Cp, const int32_t *__restrict__ Ci,
                                                  const double *__restrict__ Cx, const int32_t *__restrict__ ucol,
                                                  const unsigned long long *__restrict__ umask, const int32_t *__restrict__ pos,
                                                  double *__restrict__ W) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nt) return;
    const int32_t t = tglob[i], b = tbit[i];
    const UdGroup G = groups[tgroup[i]];
    for (int32_t q = Cp[t]; q < Cp[t + 1]; q++) {
        const int32_t r = Ci[q], u = pos[r];
        if (ud_member(G, u, r, ucol) && ((umask[G.u0 + u] >> b) & 1ull))
            W[G.woff + (int64_t)u * G.nterm + b] = Cx[q];
    }
}

__global__ __launch_bounds__(256) void k_ud_restore(int32_t U, const int32_t *__restrict__ ucol, const int64_t *__restrict__ usoff,
                                                    const int32_t *__restrict__ Lp, const double *__restrict__ snap,
                                                    double *__restrict__ Lx) {
    const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
    const int lane = threadIdx.x & (WAVE - 1);
    if (i >= U) return;
    const int32_t j = ucol[i], p = Lp[j], len = Lp[j + 1] - p;
    for (int32_t e = lane; e < len; e += WAVE) Lx[p + e] = snap[usoff[i] + e];
}

#pragma clang fp contract(off)
// One workgroup per tree of the chunk (glist: biggest first).  limit: terms with a global index above it take no part (the
// replay after a failure).  tfail[tree]: the tree's failing term (INT_MAX: none yet); a tree that failed in an earlier chunk
// is skipped (its later terms come after the failing one).  fail_min: the smallest failing term of the call.
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void k_ud_block(const int32_t *__restrict__ glist, const UdGroup *__restrict__ groups,
                                                    const int2 *__restrict__ upe, const unsigned long long *__restrict__ umask,
                                                    const int64_t *__restrict__ usoff, const int32_t *__restrict__ rowslot,
                                                    const int32_t *__restrict__ tglob, const int32_t *__restrict__ tsig,
                                                    double *Lx, double *Wglob, int in_lds,
                                                    int32_t limit, int *tfail, int *fail_min, const int *err) {
    extern __shared__ double w_lds[];
    __shared__ double s_beta[64], s_alpha[64], s_delta[64], s_gamma[64], s_sig[64], s_w[64];
    __shared__ unsigned long long s_alive, s_mask;
    const UdGroup G = groups[glist[blockIdx.x]];
    if (*err || tfail[G.tree] != INT_MAX) return;
    const int tid = threadIdx.x;
    const int32_t T = G.nterm;
    double *W = Wglob + G.woff;
    if (in_lds) {
        for (int64_t q = tid; q < (int64_t)G.ucnt * T; q += BLOCK) w_lds[q] = W[q];
        W = w_lds;
    }
    if (tid < 64) {
        const bool live = tid < T && tglob[G.t0 + tid] <= limit;
        s_beta[tid] = 1.0;
        s_sig[tid] = tid < T ? (double)tsig[G.t0 + tid] : 1.0;
        const unsigned long long live_bits = __ballot(live);
        if (tid == 0) s_alive = live_bits;
    }
    __syncthreads();
    unsigned long long alive = s_alive;   // the terms still going: every lane's own copy, refreshed after each chain
    __syncthreads();                      // (before tid 0 can write s_alive again)
    for (int32_t u = 0; u < G.ucnt; u++) {
        // everything column u needs that no earlier column writes, in one round of loads: its place in L (upe, from the
        // schedule), its diagonal, the first entry below it per lane and that entry's W row
        const int2 pe = upe[G.u0 + u];
        const int32_t p = pe.x, e = pe.y;
        const unsigned long long mask = umask[G.u0 + u] & alive;
        const int64_t o = usoff[G.u0 + u] - p;
        const bool has0 = p + 1 + tid < e;
        const double ljj0 = Lx[p];
        const double lx0 = has0 ? Lx[p + 1 + tid] : 0.0;
        const int32_t rs0 = has0 ? rowslot[o + p + 1 + tid] : 0;
        if (mask == 0ull) continue;                                   // uniform: every lane holds the same `alive`
        // (a) the scalar chain of the mask's terms, in order
        if (tid < 64) {
            if ((mask >> tid) & 1ull) s_w[tid] = W[(int64_t)u * T + tid];
            if (tid == 0) {
                double ljj = ljj0;
                unsigned long long m = mask, done = 0ull, live = alive;
                while (m) {
                    const int b = __builtin_ctzll(m);
                    m &= m - 1;
                    const double wj = s_w[b], beta = s_beta[b], sigma = s_sig[b];
                    const double alpha = wj / ljj;
                    const double sa = sigma * alpha;
                    double beta2 = beta * beta + sa * alpha;
                    if (beta2 <= 0.0) {                               // not positive definite: term b and the later ones stop
                        const int tg = tglob[G.t0 + b];
                        tfail[G.tree] = tg;
                        atomicMin(fail_min, tg);
                        live &= (1ull << b) - 1ull;
                        break;
                    }
                    beta2 = sqrt(beta2);
                    const double delta = sigma > 0.0 ? beta / beta2 : beta2 / beta;
                    const double gamma = sa / (beta2 * beta);
                    const double dl = delta * ljj;
                    ljj = sigma > 0.0 ? dl + gamma * wj : dl + 0.0;
                    s_beta[b] = beta2;
                    s_alpha[b] = alpha;
                    s_delta[b] = delta;
                    s_gamma[b] = gamma;
                    done |= 1ull << b;
                }
                if (done) Lx[p] = ljj;
                s_mask = done;
                s_alive = live;
            }
        }
        lds_barrier();   // only LDS crosses it (s_alpha .. s_mask); the diagonal stored is read by no other lane
        // (b) the entries below the diagonal: L(q) loaded once, the terms applied in order, stored once
        const unsigned long long done = s_mask;
        alive = s_alive;   // (a lane reads it here only: tid 0 writes it again after the next barrier)
        if (done) {
            for (int32_t q = p + 1 + tid; q < e; q += BLOCK) {
                const bool first = q == p + 1 + tid;
                double lx = first ? lx0 : Lx[q];
                double *Wr = W + (int64_t)(first ? rs0 : rowslot[o + q]) * T;
                unsigned long long m = done;
                while (m) {   // up to UD_BATCH terms at a time: their W loads issue together (distinct slots)
                    int bs[UD_BATCH];
                    double w[UD_BATCH];
                    int c = 0;
#pragma unroll
                    for (int h = 0; h < UD_BATCH; h++) {
                        bs[h] = 0;
                        if (m) {
                            bs[h] = __builtin_ctzll(m);
                            m &= m - 1;
                            c = h + 1;
                        }
                    }
#pragma unroll
                    for (int h = 0; h < UD_BATCH; h++)
                        if (h < c) w[h] = Wr[bs[h]];
#pragma unroll
                    for (int h = 0; h < UD_BATCH; h++) {
                        if (h < c) {
                            const int b = bs[h];
                            const double w1 = w[h];
                            const double w2 = w1 - s_alpha[b] * lx;
                            w[h] = w2;
                            lx = s_delta[b] * lx + s_gamma[b] * (s_sig[b] > 0.0 ? w1 : w2);
                        }
                    }
#pragma unroll
                    for (int h = 0; h < UD_BATCH; h++)
                        if (h < c) Wr[bs[h]] = w[h];
                }
                Lx[q] = lx;
            }
        }
        if (in_lds) lds_barrier();   // W rows of the next columns, s_mask, s_alpha ... are rewritten
        else __syncthreads();        // (W in global memory: its stores must be seen by the chain of the next columns)
    }
}
#pragma clang fp contract(fast)

// one chunk's schedule, kept for the replay and the restore
struct UdChunk {
    int32_t U = 0, nt = 0, ngroups = 0;
    int64_t snap_len = 0, wlen = 0;
    DevBuf<int32_t> ucol, ugrp, uloc, rowslot, glist, tf, tbit, tgroup, tglob, tsig;
    DevBuf<unsigned long long> umask;
    DevBuf<int64_t> usoff;
    DevBuf<UdGroup> groups;
    DevBuf<double> snap, W;
    DevBuf<int2> upe;   // (Lp[j], Lp[j + 1]) of every union column, in the sorted order
    // launches: (first entry of glist, count, BLOCK, LDS bytes)
    struct Launch {
        int32_t first, count, block;
        size_t lds;
    };
    std::vector<Launch> launches;
};

struct UdInfo {
    int32_t chunks = 0, union_columns = 0, groups = 0;
    int32_t classes[4] = {0, 0, 0, 0};   // groups launched in the first pass, by (block == 256) + 2 * (W in LDS)
    int32_t replayed = 0;                // 1 when the [0, tf] replay ran
    double kernel_ms = 0.0;
};
UdInfo g_ud_info;

// W = C's columns on their paths, then the chunk's block launches (events e0 / e1 around them).  pos: scattered again when
// another chunk has used it since this one's was
int ud_run_chunk(UdChunk &ch, const Csc *C, const Csc *L, int32_t *pos, bool scatter_pos, int32_t limit, int *tfail,
                 int *fail_min, const int *err, hipEvent_t e0, hipEvent_t e1) {
    hipStream_t s = ctx().stream;
    if (scatter_pos) {
        hipLaunchKernelGGL(k_ud_pos, dim3((unsigned)((ch.U + 255) / 256)), dim3(256), 0, s, ch.U, ch.ucol, ch.uloc, pos);
        CSX_LAUNCH_CHECK();
    }
    if (ch.wlen) CSX_HIP(hipMemsetAsync(ch.W, 0, (size_t)ch.wlen * sizeof(double), s));
    hipLaunchKernelGGL(k_ud_w_init, dim3((unsigned)((ch.nt + 63) / 64)), dim3(64), 0, s, ch.nt, ch.tglob, ch.tgroup, ch.tbit,
                       ch.groups, C->p, C->i, C->x, ch.ucol, ch.umask, pos, ch.W);
    CSX_LAUNCH_CHECK();
    CSX_HIP(hipEventRecord(e0, s));
    for (const UdChunk::Launch &l : ch.launches) {
        if (l.block == 64)
            hipLaunchKernelGGL(k_ud_block<64>, dim3((unsigned)l.count), dim3(64), l.lds, s, ch.glist + l.first, ch.groups, ch.upe,
                               ch.umask, ch.usoff, ch.rowslot, ch.tglob, ch.tsig, L->x, ch.W, l.lds ? 1 : 0, limit, tfail,
                               fail_min, err);
        else
            hipLaunchKernelGGL(k_ud_block<256>, dim3((unsigned)l.count), dim3(256), l.lds, s, ch.glist + l.first, ch.groups, ch.upe,
                               ch.umask, ch.usoff, ch.rowslot, ch.tglob, ch.tsig, L->x, ch.W, l.lds ? 1 : 0, limit, tfail,
                               fail_min, err);
        CSX_LAUNCH_CHECK();
    }
    CSX_HIP(hipEventRecord(e1, s));
    return CSX_OK;
}

int ud_restore(const UdChunk &ch, const Csc *L) {
    if (!ch.U) return CSX_OK;
    hipLaunchKernelGGL(k_ud_restore, dim3((unsigned)(((int64_t)ch.U * WAVE + 255) / 256)), dim3(256), 0, ctx().stream, ch.U, ch.ucol,
                       ch.usoff, L->p, ch.snap, L->x);
    CSX_LAUNCH_CHECK();
    return CSX_OK;
}

template <class T>
int ud_download(std::vector<T> &h, const T *d, size_t count) {
    h.resize(count);
    if (count) CSX_HIP(hipMemcpyAsync(h.data(), d, count * sizeof(T), hipMemcpyDeviceToHost, ctx().stream));
    CSX_HIP(hipStreamSynchronize(ctx().stream));
    return CSX_OK;
}

// Chunk s's terms (ranks [64 s, 64 s + 64) of every tree), their walks, the union sorted by (tree, column), its snapshot and
// W rows.  trees[g] = the terms of tree g, ascending.
int ud_build_chunk(UdChunk &ch, int32_t s, const std::vector<std::vector<int32_t>> &trees, const std::vector<int32_t> &hf,
                   const std::vector<int32_t> &hlen, const int32_t *sigma, const Csc *L, const int32_t *d_parent,
                   unsigned long long *mark, int32_t *pos, int *err) {
    hipStream_t st = ctx().stream;
    std::vector<int32_t> tf, tbit, tgroup, tglob, tsig;
    std::vector<UdGroup> groups;
    int64_t cap = 0;
    for (size_t g = 0; g < trees.size(); g++) {
        const int32_t cnt = (int32_t)trees[g].size();
        if (cnt <= 64 * s) continue;
        UdGroup G{};
        G.tree = (int32_t)g;
        G.t0 = (int32_t)tf.size();
        G.nterm = std::min(cnt - 64 * s, 64);
        for (int32_t b = 0; b < G.nterm; b++) {
            const int32_t t = trees[g][(size_t)(64 * s + b)];
            tf.push_back(hf[(size_t)t]);
            tbit.push_back(b);
            tgroup.push_back((int32_t)groups.size());
            tglob.push_back(t);
            tsig.push_back(sigma[t]);
            cap += hlen[(size_t)t];
        }
        groups.push_back(G);
    }
    ch.nt = (int32_t)tf.size();
    ch.ngroups = (int32_t)groups.size();
    if (cap > INT32_MAX) return CSX_EINVAL;
    DevBuf<int32_t> d_tf, d_ucol, d_ugrp, d_ulen, d_cnt;
    DevBuf<unsigned long long> d_umask;
    CSX_TRY(upload(d_tf, tf));
    CSX_TRY(upload(ch.tbit, tbit));
    CSX_TRY(upload(ch.tgroup, tgroup));
    CSX_TRY(upload(ch.tglob, tglob));
    CSX_TRY(upload(ch.tsig, tsig));
    CSX_TRY(d_ucol.alloc((size_t)cap));
    CSX_TRY(d_ugrp.alloc((size_t)cap));
    CSX_TRY(d_ulen.alloc((size_t)cap));
    CSX_TRY(d_umask.alloc((size_t)cap));
    CSX_TRY(d_cnt.alloc(1));
    CSX_HIP(hipMemsetAsync(d_cnt, 0, sizeof(int32_t), st));
    hipLaunchKernelGGL(k_ud_walk, dim3((unsigned)((ch.nt + 63) / 64)), dim3(64), 0, st, ch.nt, d_tf, ch.tbit, ch.tgroup, L->p, L->i,
                       d_parent, mark, d_cnt, d_ucol, d_ugrp);
    CSX_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_ud_collect, dim3((unsigned)((cap + 255) / 256)), dim3(256), 0, st, d_cnt, d_ucol, mark, d_umask, d_ulen, L->p);
    CSX_LAUNCH_CHECK();
    std::vector<int32_t> hcnt;
    CSX_TRY(ud_download(hcnt, d_cnt.get(), 1));
    const int32_t U = hcnt[0];
    std::vector<int32_t> ucol, ugrp, ulen;
    std::vector<unsigned long long> umask;
    ucol.resize((size_t)U);
    ugrp.resize((size_t)U);
    ulen.resize((size_t)U);
    umask.resize((size_t)U);
    if (U) {
        CSX_HIP(hipMemcpyAsync(ucol.data(), d_ucol, (size_t)U * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        CSX_HIP(hipMemcpyAsync(ugrp.data(), d_ugrp, (size_t)U * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        CSX_HIP(hipMemcpyAsync(ulen.data(), d_ulen, (size_t)U * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        CSX_HIP(hipMemcpyAsync(umask.data(), d_umask, (size_t)U * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    }
    CSX_HIP(hipStreamSynchronize(st));
    // the union by (tree, column): a tree's columns ascending are an order its paths can be walked in
    std::vector<int32_t> ord((size_t)U);
    for (int32_t i = 0; i < U; i++) ord[(size_t)i] = i;
    std::sort(ord.begin(), ord.end(), [&](int32_t a, int32_t b) {
        return ugrp[(size_t)a] != ugrp[(size_t)b] ? ugrp[(size_t)a] < ugrp[(size_t)b] : ucol[(size_t)a] < ucol[(size_t)b];
    });
    std::vector<int32_t> s_ucol((size_t)U), s_ugrp((size_t)U), s_uloc((size_t)U);
    std::vector<unsigned long long> s_umask((size_t)U);
    std::vector<int64_t> s_usoff((size_t)U);
    std::vector<int32_t> maxlen(groups.size(), 0);
    int64_t soff = 0;
    for (int32_t i = 0; i < U; i++) {
        const int32_t a = ord[(size_t)i], g = ugrp[(size_t)a];
        UdGroup &G = groups[(size_t)g];
        if (G.ucnt == 0) G.u0 = i;
        s_ucol[(size_t)i] = ucol[(size_t)a];
        s_ugrp[(size_t)i] = g;
        s_uloc[(size_t)i] = G.ucnt++;
        s_umask[(size_t)i] = umask[(size_t)a];
        s_usoff[(size_t)i] = soff;
        soff += ulen[(size_t)a];
        maxlen[(size_t)g] = std::max(maxlen[(size_t)g], ulen[(size_t)a]);
    }
    int64_t woff = 0;
    for (UdGroup &G : groups) {
        G.woff = woff;
        woff += (int64_t)G.ucnt * G.nterm;
    }
    ch.U = U;
    ch.snap_len = soff;
    ch.wlen = woff;
    // launch classes: a wave per tree whose columns fit one (else 256 lanes), W in LDS where it fits; biggest first in each
    std::vector<int32_t> glist;
    for (int cls = 0; cls < 4; cls++) {
        const int block = (cls & 1) ? 256 : 64;
        const bool lds = (cls & 2) != 0;
        std::vector<int32_t> mine;
        size_t lds_bytes = 0;
        for (size_t g = 0; g < groups.size(); g++) {
            const size_t wb = (size_t)groups[g].ucnt * (size_t)groups[g].nterm * sizeof(double);
            if ((maxlen[g] > 64 ? 256 : 64) != block || (wb <= (size_t)UD_LDS_W) != lds) continue;
            mine.push_back((int32_t)g);
            lds_bytes = std::max(lds_bytes, wb);
        }
        if (mine.empty()) continue;
        std::stable_sort(mine.begin(), mine.end(), [&](int32_t a, int32_t b) {
            return (int64_t)groups[(size_t)a].ucnt * groups[(size_t)a].nterm > (int64_t)groups[(size_t)b].ucnt * groups[(size_t)b].nterm;
        });
        ch.launches.push_back({(int32_t)glist.size(), (int32_t)mine.size(), block, lds ? lds_bytes : 0});
        g_ud_info.classes[cls] += (int32_t)mine.size();
        glist.insert(glist.end(), mine.begin(), mine.end());
    }
    CSX_TRY(upload(ch.ucol, s_ucol));
    CSX_TRY(upload(ch.ugrp, s_ugrp));
    CSX_TRY(upload(ch.uloc, s_uloc));
    CSX_TRY(upload(ch.umask, s_umask));
    CSX_TRY(upload(ch.usoff, s_usoff));
    CSX_TRY(upload(ch.groups, groups));
    CSX_TRY(upload(ch.glist, glist));
    CSX_TRY(ch.snap.alloc((size_t)soff));
    CSX_TRY(ch.rowslot.alloc((size_t)soff));
    CSX_TRY(ch.upe.alloc((size_t)U));
    CSX_TRY(ch.W.alloc((size_t)woff));
    hipLaunchKernelGGL(k_ud_pos, dim3((unsigned)((U + 255) / 256)), dim3(256), 0, st, U, ch.ucol, ch.uloc, pos);
    CSX_LAUNCH_CHECK();
    // the snapshot: this chunk's union columns as the chunks before it left them
    hipLaunchKernelGGL(k_ud_prep, dim3((unsigned)(((int64_t)U * WAVE + 255) / 256)), dim3(256), 0, st, U, ch.ucol, ch.ugrp, ch.usoff,
                       ch.groups, pos, L->p, L->i, L->x, ch.snap, ch.rowslot, ch.upe, err);
    CSX_LAUNCH_CHECK();
    return CSX_OK;
}

}  // namespace

}  // namespace csx

using namespace csx;

extern "C" int csx_updown_block(csx_handle_t hL, csx_handle_t hC, const int32_t *sigma, const int32_t *parent, int flags,
                                int32_t *applied) {
    CSX_TRY(require_ready());
    Csc *L = csc(hL);
    Csc *C = csc(hC);
    if (!L || !C || !L->x || !C->x || L->m != L->n || C->m != L->n || !applied || (C->n > 0 && !sigma)) return CSX_EINVAL;
    const int32_t n = L->n, k = C->n;
    for (int32_t t = 0; t < k; t++)
        if (sigma[t] != 1 && sigma[t] != -1) return CSX_EINVAL;
    g_ud_info = UdInfo{};
    *applied = k;
    if (k == 0 || n == 0) return CSX_OK;                  // no terms; or n = 0, where every column is empty
    hipStream_t s = ctx().stream;
    // flags[0] error bits (k_ud_terms, k_ud_prep), [1] the given parent differs from L's tree, [2] the smallest failing term
    DevBuf<int> d_flags;
    CSX_TRY(d_flags.alloc(3));
    const int flags0[3] = {0, 0, INT_MAX};
    CSX_HIP(hipMemcpyAsync(d_flags, flags0, sizeof(flags0), hipMemcpyHostToDevice, s));
    int *err = d_flags.get(), *fail_min = d_flags.get() + 2;
    DevBuf<int32_t> d_parent;
    if (parent) {
        CSX_TRY(upload(d_parent, parent, (size_t)n));
        hipLaunchKernelGGL(k_ud_check_parent, dim3((unsigned)(((int64_t)n + 255) / 256)), dim3(256), 0, s, n, L->p, L->i, d_parent,
                           d_flags.get() + 1);
        CSX_LAUNCH_CHECK();
    }
    DevBuf<int32_t> d_f, d_root, d_len;
    CSX_TRY(d_f.alloc((size_t)k));
    CSX_TRY(d_root.alloc((size_t)k));
    CSX_TRY(d_len.alloc((size_t)k));
    hipLaunchKernelGGL(k_ud_terms, dim3((unsigned)((k + 63) / 64)), dim3(64), 0, s, k, n, C->p, C->i, L->p, L->i,
                       parent ? d_parent.get() : nullptr, (flags & 2) ? 1 : 0, d_f, d_root, d_len, err);
    CSX_LAUNCH_CHECK();
    std::vector<int32_t> hflags, hf, hroot, hlen;
    CSX_TRY(ud_download(hflags, d_flags.get(), 2));
    if (hflags[1]) {                                      // (before the walks: with a wrong tree they may not end)
        *applied = -2;
        return CSX_OK;
    }
    if (hflags[0] & 5) return CSX_EINVAL;                 // a row out of range; L not Cholesky-shaped
    if ((flags & 2) && (hflags[0] & 2)) {
        *applied = -1;
        return CSX_OK;
    }
    CSX_TRY(ud_download(hf, d_f.get(), (size_t)k));
    CSX_TRY(ud_download(hroot, d_root.get(), (size_t)k));
    CSX_TRY(ud_download(hlen, d_len.get(), (size_t)k));
    // the terms by tree (root of their path), ascending in each; empty columns change nothing
    std::vector<int32_t> ord;
    for (int32_t t = 0; t < k; t++)
        if (hf[(size_t)t] >= 0) ord.push_back(t);
    if (ord.empty()) return CSX_OK;
    std::stable_sort(ord.begin(), ord.end(), [&](int32_t a, int32_t b) { return hroot[(size_t)a] < hroot[(size_t)b]; });
    std::vector<std::vector<int32_t>> trees;
    for (size_t q = 0; q < ord.size(); q++) {
        if (q == 0 || hroot[(size_t)ord[q]] != hroot[(size_t)ord[q - 1]]) trees.emplace_back();
        trees.back().push_back(ord[q]);
    }
    int32_t nchunks = 0;
    for (const auto &tr : trees) nchunks = std::max(nchunks, (int32_t)((tr.size() + 63) / 64));
    DevBuf<unsigned long long> mark;
    DevBuf<int32_t> pos;
    CSX_TRY(mark.alloc((size_t)n));
    CSX_TRY(pos.alloc((size_t)n));
    CSX_HIP(hipMemsetAsync(mark, 0, (size_t)n * sizeof(unsigned long long), s));
    std::vector<int> tfail0(trees.size(), INT_MAX);
    DevBuf<int> tfail;
    CSX_TRY(upload(tfail, tfail0));
    std::vector<UdChunk> chunks((size_t)nchunks);
    std::vector<hipEvent_t> evs;
    struct EvGuard {
        std::vector<hipEvent_t> &e;
        ~EvGuard() {
            for (hipEvent_t x : e) (void)hipEventDestroy(x);
        }
    } guard{evs};
    auto event_pair = [&](hipEvent_t *a, hipEvent_t *b) -> int {
        CSX_HIP(hipEventCreate(a));
        evs.push_back(*a);
        CSX_HIP(hipEventCreate(b));
        evs.push_back(*b);
        return CSX_OK;
    };
    for (int32_t c = 0; c < nchunks; c++) {
        UdChunk &ch = chunks[(size_t)c];
        CSX_TRY(ud_build_chunk(ch, c, trees, hf, hlen, sigma, L, parent ? d_parent.get() : nullptr, mark, pos, err));
        hipEvent_t e0, e1;
        CSX_TRY(event_pair(&e0, &e1));
        CSX_TRY(ud_run_chunk(ch, C, L, pos, false, INT_MAX, tfail, fail_min, err, e0, e1));
        g_ud_info.union_columns += ch.U;
        g_ud_info.groups += ch.ngroups;
    }
    std::vector<int32_t> res;
    CSX_TRY(ud_download(res, d_flags.get(), 3));
    const bool bad_shape = (res[0] & 8) != 0;
    const int32_t tf = res[2];
    if (bad_shape || tf != INT_MAX) {                     // put every chunk's union columns back, last chunk first
        for (int32_t c = nchunks - 1; c >= 0; c--) CSX_TRY(ud_restore(chunks[(size_t)c], L));
    }
    int status = CSX_OK;
    if (bad_shape) {
        status = CSX_EINVAL;
    } else if (tf != INT_MAX) {
        *applied = tf;
        if (!(flags & 1)) {                               // the loop's partial state: terms [0, tf] again, tf stopping where it stops
            g_ud_info.replayed = 1;
            CSX_TRY(upload(tfail, tfail0));
            CSX_HIP(hipMemcpyAsync(fail_min, &flags0[2], sizeof(int), hipMemcpyHostToDevice, s));
            for (int32_t c = 0; c < nchunks; c++) {
                hipEvent_t e0, e1;
                CSX_TRY(event_pair(&e0, &e1));
                CSX_TRY(ud_run_chunk(chunks[(size_t)c], C, L, pos, true, tf, tfail, fail_min, err, e0, e1));
            }
        }
    }
    CSX_HIP(hipStreamSynchronize(s));
    for (size_t q = 0; q + 1 < evs.size(); q += 2) {
        float ms = 0.0f;
        CSX_HIP(hipEventElapsedTime(&ms, evs[q], evs[q + 1]));
        g_ud_info.kernel_ms += ms;
    }
    g_ud_info.chunks = nchunks;
    if (status == CSX_OK && !(tf != INT_MAX && (flags & 1))) {
        // the factor's values changed: plans cached on it are stale
        L->rows.reset();
        L->tiled.reset();
    }
    return status;
}

extern "C" int csx_updown_block_info(int32_t *chunks, int32_t *union_columns, int32_t *groups, double *kernel_ms) {
    if (chunks) *chunks = g_ud_info.chunks;
    if (union_columns) *union_columns = g_ud_info.union_columns;
    if (groups) *groups = g_ud_info.groups;
    if (kernel_ms) *kernel_ms = g_ud_info.kernel_ms;
    return CSX_OK;
}

extern "C" int csx_updown_block_classes(int32_t counts[4], int32_t *replayed) {
    if (counts)
        for (int c = 0; c < 4; c++) counts[c] = g_ud_info.classes[c];
    if (replayed) *replayed = g_ud_info.replayed;
    return CSX_OK;
}
