// The Dulmage-Mendelsohn family on the device: cs_maxtrans (csparse.py:1527), cs_scc (:1992) and cs_dmperm (:905).
//
// The reference's copies do not run, so what is kept is CSparse's definition of the result, not
// its search order.  Everything here is level-synchronous: one thread per column (or row, or vertex) checks a level
// stamp and, if it is on the frontier, walks its entries.  Nothing depends on the order in which atomics arrive:
//   - a row claimed by several columns keeps the one of smallest priority key (atomicMin on a 64-bit key whose low
//     half is the column itself), so the claimant decodes from the key;
//   - set marks are idempotent stores of one value;
//   - degree counters reach zero exactly once (atomicSub), whatever the order of the decrements.
// Priority keys: (hash << 32) | index, with hash = index (seed 0), n-1-index (seed -1) or the upper half of
// splitmix64(splitmix64(seed) + index) otherwise.  cs_randperm is the order of these keys (csparse.py does the same
// in numpy).
//
// Round loops: each round is a few kernels ending in k_advance, which sets ctl->stop when the round added nothing.
// The host queues rounds in batches and reads ctl once per batch; queued kernels return at once after stop.  No loop
// runs more than m + n + 1 rounds, and the colouring of the SCC step no more than 2 (m + n + 1) rounds over all its
// iterations (CSX_ERUNTIME with a message past either).  All work space is allocated before the loops.
#include "csx_internal.h"

namespace csx {

namespace {

constexpr uint64_t KEY_NONE = ~0ull;

struct Ctl {
    int stop;    // the loop is over: queued kernels return
    int level;   // current level of the round
    int any;     // something joined the next frontier this round
    int found;   // matching: a free row was reached this level
    int done;    // matching: no augmenting path is left
    int pad[3];
};

__host__ __device__ inline uint64_t splitmix64(uint64_t z) {
    z += 0x9e3779b97f4a7c15ull;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

// priority key of index k out of n: smaller claims first; the low half is k itself
__device__ inline uint64_t pkey(uint64_t sh, int64_t seed, int32_t k, int32_t n) {
    uint32_t h;
    if (seed == 0) h = (uint32_t)k;
    else if (seed == -1) h = (uint32_t)(n - 1 - k);
    else h = (uint32_t)(splitmix64(sh + (uint64_t)(uint32_t)k) >> 32);
    return ((uint64_t)h << 32) | (uint32_t)k;
}

inline dim3 grid_of(int64_t n) { return dim3((unsigned)std::max<int64_t>(1, (n + 255) / 256)); }

__global__ void k_fill(int32_t *a, int64_t n, int32_t v) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) a[k] = v;
}
__global__ void k_fill64(uint64_t *a, int64_t n, uint64_t v) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) a[k] = v;
}
__global__ void k_iota(uint32_t *a, int64_t n) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) a[k] = (uint32_t)k;
}

__global__ void k_advance(Ctl *ctl) {
    if (ctl->stop) return;
    if (!ctl->any) ctl->stop = 1;
    else {
        ctl->level++;
        ctl->any = 0;
    }
}

// Queue rounds in batches, read the control block once per batch.  issue() queues one round ending in k_advance.
template <class F>
int run_rounds(Ctl *ctl, Ctl *h, int64_t bound, const char *what, F issue) {
    hipStream_t s = ctx().stream;
    int64_t queued = 0;
    for (;;) {
        const int batch = queued < 4 ? 1 : (queued < 64 ? 8 : 64);
        for (int b = 0; b < batch; b++) CSX_TRY(issue());
        queued += batch;
        CSX_HIP(hipMemcpyAsync(h, ctl, sizeof(Ctl), hipMemcpyDeviceToHost, s));
        CSX_HIP(hipStreamSynchronize(s));
        if (h->stop) return CSX_OK;
        if (h->level > bound) {
            set_error("%s: no fixed point after %lld rounds (bound m + n + 1)", what, (long long)bound);
            return CSX_ERUNTIME;
        }
    }
}

// ---------------------------------------------------------------- matching --

// zero-free diagonal: column j holds row j for every j < min(m, n)
__global__ void k_diag_check(int32_t k, const int32_t *__restrict__ Ap, const int32_t *__restrict__ Ai, int *missing) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= k) return;
    for (int32_t q = Ap[j]; q < Ap[j + 1]; q++)
        if (Ai[q] == (int32_t)j) return;
    *missing = 1;
}
__global__ void k_diag_set(int32_t k, int32_t *jm, int32_t *im) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < k) jm[j] = im[j] = (int32_t)j;
}

// greedy round: every unmatched column bids for its first unmatched row in row priority, a row keeps the bid of
// smallest column key
__global__ void k_greedy_bid(int32_t m, int32_t n, const int32_t *__restrict__ Ap, const int32_t *__restrict__ Ai,
                             const int32_t *__restrict__ jm, const int32_t *__restrict__ im, int64_t seed, uint64_t sh,
                             uint64_t *rbid) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n || im[j] >= 0) return;
    uint64_t best = KEY_NONE;
    for (int32_t q = Ap[j]; q < Ap[j + 1]; q++) {
        const int32_t i = Ai[q];
        if (jm[i] < 0) {
            const uint64_t kk = pkey(sh, seed, i, m);
            best = kk < best ? kk : best;
        }
    }
    if (best != KEY_NONE) atomicMin((unsigned long long *)&rbid[(uint32_t)best], (unsigned long long)pkey(sh, seed, (int32_t)j, n));
}
__global__ void k_greedy_take(int32_t m, uint64_t *rbid, int32_t *jm, int32_t *im) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const uint64_t b = rbid[i];
    if (b == KEY_NONE) return;
    rbid[i] = KEY_NONE;
    const int32_t j = (int32_t)(uint32_t)b;
    jm[i] = j;
    im[j] = (int32_t)i;
}

// augmentation phase: multi-source BFS along alternating paths from every unmatched column
__global__ void k_aug_seed(int32_t n, const int32_t *__restrict__ im, int32_t *cfr, int32_t *croot) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const bool root = im[j] < 0;
    cfr[j] = root ? 0 : -1;
    if (root) croot[j] = (int32_t)j;
}
__global__ void k_aug_expand(int32_t m, int32_t n, const int32_t *__restrict__ Ap, const int32_t *__restrict__ Ai,
                             const int32_t *__restrict__ cfr, const int32_t *__restrict__ rvis, int32_t phase,
                             int64_t seed, uint64_t sh, uint64_t *rbid, const Ctl *ctl) {
    if (ctl->stop) return;
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n || cfr[j] != ctl->level) return;
    const unsigned long long key = pkey(sh, seed, (int32_t)j, n);
    for (int32_t q = Ap[j]; q < Ap[j + 1]; q++) {
        const int32_t i = Ai[q];
        if (rvis[i] != phase) atomicMin((unsigned long long *)&rbid[i], key);
    }
}
__global__ void k_aug_resolve(int32_t m, uint64_t *rbid, int32_t *rvis, int32_t phase, int32_t *rpar,
                              const int32_t *__restrict__ jm, int32_t *cfr, int32_t *croot, uint64_t *rend, int64_t seed,
                              uint64_t sh, Ctl *ctl) {
    if (ctl->stop) return;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const uint64_t b = rbid[i];
    if (b == KEY_NONE) return;
    rbid[i] = KEY_NONE;
    const int32_t j = (int32_t)(uint32_t)b;
    rvis[i] = phase;
    rpar[i] = j;
    const int32_t r = croot[j];
    const int32_t j2 = jm[i];
    if (j2 < 0) {
        atomicMin((unsigned long long *)&rend[r], (unsigned long long)pkey(sh, seed, (int32_t)i, m));
        ctl->found = 1;
    } else {
        cfr[j2] = ctl->level + 1;
        croot[j2] = r;
        ctl->any = 1;
    }
}
// flip the chosen path of every root (the paths are vertex-disjoint: rows are claimed once per phase)
__global__ void k_aug_flip(int32_t n, int32_t m, uint64_t *rend, const int32_t *__restrict__ rpar, int32_t *jm,
                           int32_t *im, const Ctl *ctl) {
    if (ctl->stop || !ctl->found) return;
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const uint64_t b = rend[r];
    if (b == KEY_NONE) return;
    rend[r] = KEY_NONE;
    int32_t i = (int32_t)(uint32_t)b;
    for (int32_t step = 0; step <= m; step++) {
        const int32_t j = rpar[i];
        const int32_t prev = im[j];
        im[j] = i;
        jm[i] = j;
        if (prev < 0) break;
        i = prev;
    }
}
__global__ void k_aug_advance(Ctl *ctl) {
    if (ctl->stop) return;
    if (ctl->found) ctl->stop = 1;
    else if (!ctl->any) {
        ctl->stop = 1;
        ctl->done = 1;
    } else {
        ctl->level++;
        ctl->any = 0;
    }
}

// ------------------------------------------------------ coarse decomposition --

__global__ void k_c1_seed(int32_t n, const int32_t *__restrict__ im, int32_t *colset, int32_t *cfr) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const bool un = im[j] < 0;
    colset[j] = un ? 0 : -1;
    cfr[j] = un ? 0 : -1;
}
// unmatched columns -> rows -> their matched columns: R1 and C1 (mark 1)
__global__ void k_c1_expand(int32_t n, const int32_t *__restrict__ Ap, const int32_t *__restrict__ Ai,
                            const int32_t *__restrict__ jm, int32_t *rowset, int32_t *colset, int32_t *cfr, Ctl *ctl) {
    if (ctl->stop) return;
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int32_t L = ctl->level;
    if (j >= n || cfr[j] != L) return;
    for (int32_t q = Ap[j]; q < Ap[j + 1]; q++) {
        const int32_t i = Ai[q];
        if (rowset[i] >= 0) continue;
        rowset[i] = 1;
        const int32_t j2 = jm[i];
        if (j2 < 0 || colset[j2] >= 0) continue;
        colset[j2] = 1;
        cfr[j2] = L + 1;
        ctl->any = 1;
    }
}
__global__ void k_c2_seed(int32_t m, const int32_t *__restrict__ jm, int32_t *rowset, int32_t *rfr) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const bool un = jm[i] < 0;
    if (un) rowset[i] = 0;
    rfr[i] = un ? 0 : -1;
}
// unmatched rows -> columns (row view) -> their matched rows: C3 and R3 (mark 3)
__global__ void k_c2_expand(int32_t m, const int32_t *__restrict__ Tp, const int32_t *__restrict__ Ti,
                            const int32_t *__restrict__ im, int32_t *rowset, int32_t *colset, int32_t *rfr, Ctl *ctl) {
    if (ctl->stop) return;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int32_t L = ctl->level;
    if (i >= m || rfr[i] != L) return;
    for (int32_t q = Tp[i]; q < Tp[i + 1]; q++) {
        const int32_t j = Ti[q];
        if (colset[j] >= 0) continue;
        colset[j] = 3;
        const int32_t i2 = im[j];
        if (i2 < 0 || rowset[i2] >= 0) continue;
        rowset[i2] = 3;
        rfr[i2] = L + 1;
        ctl->any = 1;
    }
}
// column class 0 (C0), 1 (C1), 2 (C2: matched, reached by neither search), 3 (C3); counts per class, summed per
// wave first (one atomic per wave and class instead of one per column on four addresses)
__global__ void k_col_class(int32_t n, const int32_t *__restrict__ colset, uint32_t *cls, int *cnt) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t k = 4u;
    if (j < n) {
        const int32_t c = colset[j];
        k = c < 0 ? 2u : (uint32_t)c;
        cls[j] = k;
    }
    for (uint32_t c = 0; c < 4; c++) {
        const int w = __popcll(__ballot(k == c));
        if ((threadIdx.x & 63) == 0 && w) atomicAdd(&cnt[c], w);
    }
}
// p[k - cc1] = row matched to q[k] for k >= cc1
__global__ void k_rows_of_cols(int32_t n, int32_t cc1, const uint32_t *__restrict__ q, const int32_t *__restrict__ im,
                               int32_t *p) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x + cc1;
    if (k < n) p[k - cc1] = im[q[k]];
}
__global__ void k_unmatched_flag(int32_t m, const int32_t *__restrict__ jm, int32_t *flag) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < m) flag[i] = jm[i] < 0 ? 1 : 0;
}
__global__ void k_unmatched_put(int32_t m, int32_t base, const int32_t *__restrict__ jm, const int32_t *__restrict__ pos,
                                int32_t *p) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < m && jm[i] < 0) p[base + pos[i]] = (int32_t)i;
}

// --------------------------------------------------------------------- SCC --
// Graph on nv vertices: vertex v is column cv[v] and row rv[v] (cs_scc: both v; cs_dmperm: a column of C2 and its
// matched row).  vc / vr map columns / rows back to vertices (-1: not in the graph).  An entry (i, j) is the edge
// vr[i] -> vc[j]: its block comes no later.  Predecessors of v are the rows of column cv[v] (A); successors are the
// columns of row rv[v] (the row view T).  Self loops are ignored.
struct Graph {
    int32_t nv;
    const int32_t *Ap, *Ai, *Tp, *Ti;
    const int32_t *cv, *rv, *vc, *vr;
};

#define FOR_PRED(G, v, u)                                                              \
    for (int32_t _q = G.Ap[G.cv[v]], _e = G.Ap[G.cv[v] + 1]; _q < _e; _q++)            \
        if (int32_t u = G.vr[G.Ai[_q]]; u >= 0 && u != (int32_t)v)
#define FOR_SUCC(G, v, w)                                                              \
    for (int32_t _q = G.Tp[G.rv[v]], _e = G.Tp[G.rv[v] + 1]; _q < _e; _q++)            \
        if (int32_t w = G.vc[G.Ti[_q]]; w >= 0 && w != (int32_t)v)

// forward trim (Kahn from the sources): flev = peel level, -1 if not peeled
__global__ void k_s_indeg(Graph G, int32_t *deg, int32_t *flev) {
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= G.nv) return;
    int32_t d = 0;
    FOR_PRED(G, v, u) { (void)u; d++; }
    deg[v] = d;
    flev[v] = d == 0 ? 0 : -1;
}
__global__ void k_s_ftrim(Graph G, int32_t *deg, int32_t *flev, Ctl *ctl) {
    if (ctl->stop) return;
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int32_t L = ctl->level;
    if (v >= G.nv || flev[v] != L) return;
    FOR_SUCC(G, v, w) {
        if (atomicSub(&deg[w], 1) == 1) {
            flev[w] = L + 1;
            ctl->any = 1;
        }
    }
}
// backward trim (Kahn from the sinks) among the vertices the forward trim left
__global__ void k_s_outdeg(Graph G, const int32_t *__restrict__ flev, int32_t *deg, int32_t *blev) {
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= G.nv) return;
    if (flev[v] >= 0) {
        blev[v] = -1;
        return;
    }
    int32_t d = 0;
    FOR_SUCC(G, v, w) { (void)w; d++; }
    deg[v] = d;
    blev[v] = d == 0 ? 0 : -1;
}
__global__ void k_s_btrim(Graph G, const int32_t *__restrict__ flev, int32_t *deg, int32_t *blev, Ctl *ctl) {
    if (ctl->stop) return;
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int32_t L = ctl->level;
    if (v >= G.nv || blev[v] != L) return;
    FOR_PRED(G, v, u) {
        if (flev[u] >= 0) continue;
        if (atomicSub(&deg[u], 1) == 1) {
            blev[u] = L + 1;
            ctl->any = 1;
        }
    }
}
// peeled vertices are singleton components (comp = v); the rest (comp = -1) go to the colouring
__global__ void k_s_comp_init(Graph G, const int32_t *__restrict__ flev, const int32_t *__restrict__ blev, int32_t *comp,
                              int *stats) {
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= G.nv) return;
    comp[v] = (flev[v] >= 0 || blev[v] >= 0) ? (int32_t)v : -1;
    if (flev[v] >= 0) atomicMax(&stats[0], flev[v]);
    if (blev[v] >= 0) atomicMax(&stats[1], blev[v]);
    if (comp[v] < 0) atomicAdd(&stats[3], 1);
}
// colouring: colour = largest colour key of a live vertex that reaches v (max-label propagation); then each colour's
// root collects the vertices of its colour that reach it (backward search inside the colour) -- that is the root's SCC.
// The key of vertex v is (hash(v) << 32) | v, not v itself: with plain ids, a chain of components whose edges run from
// high ids to low ids (a block lower triangular matrix in natural order) takes one colour, loses one component per
// colouring and costs a quadratic number of rounds; with hashed keys the components that win their colour are spread
// along any chain, and each colouring cuts it into pieces.
__device__ inline uint64_t color_key(int32_t v) {
    return ((splitmix64(0x5cc0u + (uint64_t)(uint32_t)v) >> 32) << 32) | (uint32_t)v;
}
__global__ void k_col_init(Graph G, const int32_t *__restrict__ comp, uint64_t *color, Ctl *ctl) {
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= G.nv) return;
    color[v] = color_key((int32_t)v);
    if (comp[v] < 0) ctl->any = 1;
}
__global__ void k_col_prop(Graph G, const int32_t *__restrict__ comp, uint64_t *color, Ctl *ctl) {
    if (ctl->stop) return;
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= G.nv || comp[v] >= 0) return;
    uint64_t c = color[v];
    const uint64_t c0 = c;
    FOR_PRED(G, v, u) {
        if (comp[u] < 0) {
            const uint64_t cu = color[u];
            c = cu > c ? cu : c;
        }
    }
    if (c > c0) {
        color[v] = c;
        ctl->any = 1;
    }
}
__global__ void k_col_roots(Graph G, int32_t *comp, const uint64_t *__restrict__ color, int32_t *bfr) {
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= G.nv) return;
    const bool root = comp[v] < 0 && color[v] == color_key((int32_t)v);
    if (root) comp[v] = (int32_t)v;
    bfr[v] = root ? 0 : -1;
}
__global__ void k_col_back(Graph G, int32_t *comp, const uint64_t *__restrict__ color, int32_t *bfr, Ctl *ctl) {
    if (ctl->stop) return;
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int32_t L = ctl->level;
    if (v >= G.nv || bfr[v] != L) return;
    const uint64_t c = color[v];
    FOR_PRED(G, v, u) {
        if (comp[u] < 0 && color[u] == c) {
            comp[u] = (int32_t)(uint32_t)c;   // the root: the low half of its key
            bfr[u] = L + 1;
            ctl->any = 1;
        }
    }
}
// topological levels of the components of the middle (Kahn on the condensed graph; cdeg indexed by component root)
__global__ void k_m_deg(Graph G, const int32_t *__restrict__ flev, const int32_t *__restrict__ blev,
                        const int32_t *__restrict__ comp, int32_t *cdeg) {
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= G.nv || flev[v] >= 0 || blev[v] >= 0) return;
    int32_t d = 0;
    const int32_t c = comp[v];
    FOR_PRED(G, v, u) {
        if (flev[u] < 0 && blev[u] < 0 && comp[u] != c) d++;
    }
    if (d) atomicAdd(&cdeg[c], d);
}
__global__ void k_m_seed(Graph G, const int32_t *__restrict__ flev, const int32_t *__restrict__ blev,
                         const int32_t *__restrict__ comp, const int32_t *__restrict__ cdeg, int32_t *mlev) {
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= G.nv) return;
    const bool mid_root = flev[v] < 0 && blev[v] < 0 && comp[v] == (int32_t)v;
    mlev[v] = mid_root && cdeg[v] == 0 ? 0 : -1;
}
__global__ void k_m_step(Graph G, const int32_t *__restrict__ flev, const int32_t *__restrict__ blev,
                         const int32_t *__restrict__ comp, int32_t *cdeg, int32_t *mlev, Ctl *ctl) {
    if (ctl->stop) return;
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int32_t L = ctl->level;
    if (v >= G.nv || flev[v] >= 0 || blev[v] >= 0) return;
    const int32_t c = comp[v];
    if (mlev[c] != L) return;
    FOR_SUCC(G, v, w) {
        if (flev[w] >= 0 || blev[w] >= 0) continue;
        const int32_t cw = comp[w];
        if (cw != c && atomicSub(&cdeg[cw], 1) == 1) {
            mlev[cw] = L + 1;
            ctl->any = 1;
        }
    }
}
__global__ void k_m_max(Graph G, const int32_t *__restrict__ mlev, int *stats) {
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v < G.nv && mlev[v] >= 0) atomicMax(&stats[2], mlev[v]);
}
// block key: front peel level, then middle component level, then back peel level reversed
__global__ void k_s_key(Graph G, const int32_t *__restrict__ flev, const int32_t *__restrict__ blev,
                        const int32_t *__restrict__ comp, const int32_t *__restrict__ mlev, const int *stats,
                        const uint32_t *__restrict__ order, uint32_t *key) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= G.nv) return;
    const int32_t v = (int32_t)order[k];
    const int32_t F = stats[0] + 1, M = stats[2] + 1, B = stats[1];
    int32_t kk;
    if (flev[v] >= 0) kk = flev[v];
    else if (blev[v] >= 0) kk = F + M + (B - blev[v]);
    else kk = F + mlev[comp[v]];
    key[k] = (uint32_t)kk;
}
__global__ void k_s_heads(int32_t nv, const uint32_t *__restrict__ ps, const int32_t *__restrict__ comp, int32_t *head) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < nv) head[k] = (k == 0 || comp[ps[k]] != comp[ps[k - 1]]) ? 1 : 0;
}
__global__ void k_s_starts(int32_t nv, const int32_t *__restrict__ head, const int32_t *__restrict__ hscan, int32_t *rs) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < nv && head[k]) rs[hscan[k]] = (int32_t)k;
}

// the vertex maps of cs_dmperm's fine graph: vertex v is column q[cc2 + v] and row p[rr1 + v]
__global__ void k_fine_maps(int32_t nc, const uint32_t *__restrict__ q, int32_t cc2, const int32_t *__restrict__ p,
                            int32_t rr1, int32_t *cv, int32_t *rv, int32_t *vc, int32_t *vr) {
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nc) return;
    const int32_t j = (int32_t)q[cc2 + v], i = p[rr1 + v];
    cv[v] = j;
    rv[v] = i;
    vc[j] = (int32_t)v;
    vr[i] = (int32_t)v;
}
__global__ void k_fine_apply(int32_t nc, const uint32_t *__restrict__ ps, const int32_t *__restrict__ cv,
                             const int32_t *__restrict__ rv, uint32_t *q, int32_t cc2, int32_t *p, int32_t rr1) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nc) return;
    q[cc2 + k] = (uint32_t)cv[ps[k]];
    p[rr1 + k] = rv[ps[k]];
}

// What one csx_maxtrans / csx_scc / csx_dmperm call holds until it returns: the control block, the events, and the
// work arrays of maxtrans_device and scc_device
struct Work {
    DevBuf<Ctl> ctl;
    DevBuf<uint64_t> rbid, rend;                                  // maxtrans_device
    DevBuf<int32_t> cfr, croot, rvis, rpar;
    DevBuf<int32_t> deg, flev, blev, comp, bfr, mlev, head, hscan;   // scc_device
    DevBuf<uint64_t> color;
    DevBuf<uint32_t> iota, ord, key;
    DevBuf<int> stats;
    Ctl h{};
    hipEvent_t ev[6] = {};
    ~Work() {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};

// stage times of the last csx_dmperm / csx_maxtrans (ms): matching, augmentation, coarse, fine, total
double g_stage_ms[5] = {0, 0, 0, 0, 0};
// round counts of the last call: augmentation levels, augmentation phases, trim rounds, colouring rounds (propagation
// and backward search), block order rounds
int64_t g_rounds[5] = {0, 0, 0, 0, 0};

int reset_ctl(Ctl *ctl) {
    CSX_HIP(hipMemsetAsync(ctl, 0, sizeof(Ctl), ctx().stream));
    return CSX_OK;
}

// maximum matching; jm (m) and im (n) on the device
int maxtrans_device(const Csc *A, int64_t seed, int32_t *jm, int32_t *im, Work &W) {
    hipStream_t s = ctx().stream;
    const int32_t m = A->m, n = A->n, k = std::min(m, n);
    const uint64_t sh = splitmix64((uint64_t)seed);
    hipLaunchKernelGGL(k_fill, grid_of(m), dim3(256), 0, s, jm, (int64_t)m, -1);
    hipLaunchKernelGGL(k_fill, grid_of(n), dim3(256), 0, s, im, (int64_t)n, -1);
    CSX_LAUNCH_CHECK();
    if (m == 0 || n == 0 || A->nnz == 0) return CSX_OK;
    // zero-free diagonal: the diagonal is a matching of cardinality min(m, n)
    int *missing = &W.ctl.get()->pad[0];
    CSX_TRY(reset_ctl(W.ctl));
    hipLaunchKernelGGL(k_diag_check, grid_of(k), dim3(256), 0, s, k, A->p, A->i, missing);
    CSX_HIP(hipMemcpyAsync(&W.h, W.ctl, sizeof(Ctl), hipMemcpyDeviceToHost, s));
    CSX_HIP(hipStreamSynchronize(s));
    if (!W.h.pad[0]) {
        hipLaunchKernelGGL(k_diag_set, grid_of(k), dim3(256), 0, s, k, jm, im);
        CSX_LAUNCH_CHECK();
        CSX_HIP(hipEventRecord(W.ev[1], s));
        return CSX_OK;
    }
    CSX_TRY(W.rbid.alloc((size_t)m));
    CSX_TRY(W.rend.alloc((size_t)n));
    CSX_TRY(W.cfr.alloc((size_t)n));
    CSX_TRY(W.croot.alloc((size_t)n));
    CSX_TRY(W.rvis.alloc((size_t)m));
    CSX_TRY(W.rpar.alloc((size_t)m));
    uint64_t *rbid = W.rbid, *rend = W.rend;
    int32_t *cfr = W.cfr, *croot = W.croot, *rvis = W.rvis, *rpar = W.rpar;
    hipLaunchKernelGGL(k_fill64, grid_of(m), dim3(256), 0, s, rbid, (int64_t)m, KEY_NONE);
    hipLaunchKernelGGL(k_fill64, grid_of(n), dim3(256), 0, s, rend, (int64_t)n, KEY_NONE);
    hipLaunchKernelGGL(k_fill, grid_of(m), dim3(256), 0, s, rvis, (int64_t)m, -1);
    for (int r = 0; r < 4; r++) {   // greedy rounds
        hipLaunchKernelGGL(k_greedy_bid, grid_of(n), dim3(256), 0, s, m, n, A->p, A->i, jm, im, seed, sh, rbid);
        hipLaunchKernelGGL(k_greedy_take, grid_of(m), dim3(256), 0, s, m, rbid, jm, im);
    }
    CSX_LAUNCH_CHECK();
    CSX_HIP(hipEventRecord(W.ev[1], s));
    const int64_t bound = (int64_t)m + n + 1;
    for (int32_t phase = 0;; phase++) {
        if (phase > k) {
            set_error("csx_maxtrans: more than min(m, n) + 1 augmentation phases");
            return CSX_ERUNTIME;
        }
        CSX_TRY(reset_ctl(W.ctl));
        hipLaunchKernelGGL(k_aug_seed, grid_of(n), dim3(256), 0, s, n, im, cfr, croot);
        CSX_TRY(run_rounds(W.ctl, &W.h, bound, "csx_maxtrans augmentation", [&]() -> int {
            hipLaunchKernelGGL(k_aug_expand, grid_of(n), dim3(256), 0, s, m, n, A->p, A->i, cfr, rvis, phase, seed, sh,
                               rbid, W.ctl);
            hipLaunchKernelGGL(k_aug_resolve, grid_of(m), dim3(256), 0, s, m, rbid, rvis, phase, rpar, jm, cfr, croot,
                               rend, seed, sh, W.ctl);
            hipLaunchKernelGGL(k_aug_flip, grid_of(n), dim3(256), 0, s, n, m, rend, rpar, jm, im, W.ctl);
            hipLaunchKernelGGL(k_aug_advance, dim3(1), dim3(1), 0, s, W.ctl);
            CSX_LAUNCH_CHECK();
            return CSX_OK;
        }));
        g_rounds[0] += W.h.level + 1;
        g_rounds[1]++;
        if (W.h.done) break;
    }
    return CSX_OK;
}

// SCCs of G in block upper triangular order: ps (nv, vertex order), rs (nv + 1 slots, nb + 1 used), nb
int scc_device(const Graph &G, int64_t budget, uint32_t *ps, int32_t *rs, int32_t *nb_out, Work &W) {
    hipStream_t s = ctx().stream;
    const int32_t nv = G.nv;
    *nb_out = 0;
    if (nv == 0) return CSX_OK;
    const dim3 g = grid_of(nv), b(256);
    CSX_TRY(W.deg.alloc((size_t)nv));
    CSX_TRY(W.flev.alloc((size_t)nv));
    CSX_TRY(W.blev.alloc((size_t)nv));
    CSX_TRY(W.comp.alloc((size_t)nv));
    CSX_TRY(W.color.alloc((size_t)nv));
    CSX_TRY(W.bfr.alloc((size_t)nv));
    CSX_TRY(W.mlev.alloc((size_t)nv));
    CSX_TRY(W.head.alloc((size_t)nv + 1));
    CSX_TRY(W.hscan.alloc((size_t)nv + 1));
    CSX_TRY(W.iota.alloc((size_t)nv));
    CSX_TRY(W.ord.alloc((size_t)nv));
    CSX_TRY(W.key.alloc((size_t)nv));
    CSX_TRY(W.stats.alloc(4));
    int32_t *deg = W.deg, *flev = W.flev, *blev = W.blev, *comp = W.comp, *bfr = W.bfr, *mlev = W.mlev, *head = W.head,
            *hscan = W.hscan;
    uint64_t *color = W.color;
    uint32_t *iota = W.iota, *ord = W.ord, *key = W.key;
    int *stats = W.stats;
    CSX_HIP(hipMemsetAsync(stats, 0, 4 * sizeof(int), s));
    const int64_t bound = (int64_t)nv + 1;
    // trim: sources to the front, sinks to the back, in peel order
    hipLaunchKernelGGL(k_s_indeg, g, b, 0, s, G, deg, flev);
    CSX_TRY(reset_ctl(W.ctl));
    CSX_TRY(run_rounds(W.ctl, &W.h, bound, "csx_scc forward trim", [&]() -> int {
        hipLaunchKernelGGL(k_s_ftrim, g, b, 0, s, G, deg, flev, W.ctl);
        hipLaunchKernelGGL(k_advance, dim3(1), dim3(1), 0, s, W.ctl);
        CSX_LAUNCH_CHECK();
        return CSX_OK;
    }));
    g_rounds[2] += W.h.level + 1;
    hipLaunchKernelGGL(k_s_outdeg, g, b, 0, s, G, flev, deg, blev);
    CSX_TRY(reset_ctl(W.ctl));
    CSX_TRY(run_rounds(W.ctl, &W.h, bound, "csx_scc backward trim", [&]() -> int {
        hipLaunchKernelGGL(k_s_btrim, g, b, 0, s, G, flev, deg, blev, W.ctl);
        hipLaunchKernelGGL(k_advance, dim3(1), dim3(1), 0, s, W.ctl);
        CSX_LAUNCH_CHECK();
        return CSX_OK;
    }));
    g_rounds[2] += W.h.level + 1;
    hipLaunchKernelGGL(k_s_comp_init, g, b, 0, s, G, flev, blev, comp, stats);
    int hstats[4] = {0, 0, 0, 0};
    CSX_HIP(hipMemcpyAsync(hstats, stats, sizeof(hstats), hipMemcpyDeviceToHost, s));
    CSX_HIP(hipStreamSynchronize(s));
    if (hstats[3] > 0) {
        // colouring rounds on what the trim left; each takes at least the component of the largest live key.  One
        // budget of `budget` rounds covers every propagation and backward search of the call.  A chain of k
        // components costs about 0.8 k to 3.5 k rounds in all with hashed keys (a model of these rounds on the block
        // bidiagonal chain of tests/test_gpu_dmperm.py: 1 372 rounds for k = 400, 15 652 for k = 20 000), against a
        // budget of 2 (m + n + 1) >= 8 k; only an adversarial placement of keys along a chain can exhaust it, and then
        // the call fails with CSX_ERUNTIME instead of running on.
        int64_t spent = 0;
        auto over = [&]() -> int {
            set_error("csx_scc: the colouring needs more than %lld rounds (2 (m + n + 1)) in all", (long long)budget);
            return CSX_ERUNTIME;
        };
        for (;;) {
            CSX_TRY(reset_ctl(W.ctl));
            hipLaunchKernelGGL(k_col_init, g, b, 0, s, G, comp, color, W.ctl);
            CSX_HIP(hipMemcpyAsync(&W.h, W.ctl, sizeof(Ctl), hipMemcpyDeviceToHost, s));
            CSX_HIP(hipStreamSynchronize(s));
            if (!W.h.any) break;
            CSX_TRY(reset_ctl(W.ctl));
            CSX_TRY(run_rounds(W.ctl, &W.h, budget - spent, "csx_scc colour propagation", [&]() -> int {
                hipLaunchKernelGGL(k_col_prop, g, b, 0, s, G, comp, color, W.ctl);
                hipLaunchKernelGGL(k_advance, dim3(1), dim3(1), 0, s, W.ctl);
                CSX_LAUNCH_CHECK();
                return CSX_OK;
            }));
            spent += W.h.level + 1;
            if (spent > budget) return over();
            hipLaunchKernelGGL(k_col_roots, g, b, 0, s, G, comp, color, bfr);
            CSX_TRY(reset_ctl(W.ctl));
            CSX_TRY(run_rounds(W.ctl, &W.h, budget - spent, "csx_scc backward search", [&]() -> int {
                hipLaunchKernelGGL(k_col_back, g, b, 0, s, G, comp, color, bfr, W.ctl);
                hipLaunchKernelGGL(k_advance, dim3(1), dim3(1), 0, s, W.ctl);
                CSX_LAUNCH_CHECK();
                return CSX_OK;
            }));
            spent += W.h.level + 1;
            if (spent > budget) return over();
        }
        g_rounds[3] += spent;
        // topological levels of the middle's components
        CSX_HIP(hipMemsetAsync(deg, 0, (size_t)nv * sizeof(int32_t), s));
        hipLaunchKernelGGL(k_m_deg, g, b, 0, s, G, flev, blev, comp, deg);
        hipLaunchKernelGGL(k_m_seed, g, b, 0, s, G, flev, blev, comp, deg, mlev);
        CSX_TRY(reset_ctl(W.ctl));
        CSX_TRY(run_rounds(W.ctl, &W.h, bound, "csx_scc block order", [&]() -> int {
            hipLaunchKernelGGL(k_m_step, g, b, 0, s, G, flev, blev, comp, deg, mlev, W.ctl);
            hipLaunchKernelGGL(k_advance, dim3(1), dim3(1), 0, s, W.ctl);
            CSX_LAUNCH_CHECK();
            return CSX_OK;
        }));
        g_rounds[4] += W.h.level + 1;
        hipLaunchKernelGGL(k_m_max, g, b, 0, s, G, mlev, stats);
    } else {
        hipLaunchKernelGGL(k_fill, g, b, 0, s, mlev, (int64_t)nv, -1);
    }
    // vertices grouped by component (stable by component id), then blocks by key (stable)
    hipLaunchKernelGGL(k_iota, g, b, 0, s, iota, (int64_t)nv);
    CSX_TRY(stable_sort_by_key((const uint32_t *)comp, iota, nullptr, nv, (uint32_t)nv, nullptr, ord, nullptr));
    hipLaunchKernelGGL(k_s_key, g, b, 0, s, G, flev, blev, comp, mlev, stats, ord, key);
    CSX_HIP(hipMemcpyAsync(hstats, stats, sizeof(hstats), hipMemcpyDeviceToHost, s));
    CSX_HIP(hipStreamSynchronize(s));
    const uint32_t klim = (uint32_t)(hstats[0] + hstats[1] + hstats[2] + 3);
    CSX_TRY(stable_sort_by_key(key, ord, nullptr, nv, klim, nullptr, ps, nullptr));
    hipLaunchKernelGGL(k_s_heads, g, b, 0, s, nv, ps, comp, head);
    int64_t nb = 0;
    CSX_TRY(scan_exclusive_i32(head, hscan, nv, &nb));
    hipLaunchKernelGGL(k_s_starts, g, b, 0, s, nv, head, hscan, rs);
    CSX_HIP(hipMemcpyAsync(rs + nb, &nv, sizeof(int32_t), hipMemcpyHostToDevice, s));
    CSX_HIP(hipStreamSynchronize(s));
    *nb_out = (int32_t)nb;
    return CSX_OK;
}

// the row view of A (pattern): the cached one when A has values, else a temporary transpose
int row_view(Csc *A, Csc &tmp, const int32_t **Tp, const int32_t **Ti) {
    if (A->x) {
        CSX_TRY(build_row_gather(A));
        *Tp = A->rows->ptr;
        *Ti = A->rows->idx;
        return CSX_OK;
    }
    CSX_TRY(transpose_device(A, false, &tmp));
    *Tp = tmp.p;
    *Ti = tmp.i;
    return CSX_OK;
}

int begin(Work &W) {
    for (int64_t &r : g_rounds) r = 0;
    for (hipEvent_t &e : W.ev) CSX_HIP(hipEventCreate(&e));
    CSX_TRY(W.ctl.alloc(1));
    CSX_HIP(hipEventRecord(W.ev[0], ctx().stream));
    for (int k = 1; k < 5; k++) CSX_HIP(hipEventRecord(W.ev[k], ctx().stream));   // stages that do not run take 0 ms
    return CSX_OK;
}

int finish_times(Work &W, int last) {
    CSX_HIP(hipEventRecord(W.ev[5], ctx().stream));
    CSX_HIP(hipEventSynchronize(W.ev[5]));
    float t = 0.f;
    for (int k = 0; k < 4; k++) {
        const int a = k, b = k + 1 <= last ? k + 1 : last;
        g_stage_ms[k] = 0;
        if (b > a && hipEventElapsedTime(&t, W.ev[a], W.ev[b]) == hipSuccess) g_stage_ms[k] = t;
    }
    if (hipEventElapsedTime(&t, W.ev[0], W.ev[5]) == hipSuccess) g_stage_ms[4] = t;
    return CSX_OK;
}

int prepare(csx_handle_t hA, Csc **out) {
    CSX_TRY(require_ready());
    Csc *A = csc(hA);
    if (!A) return CSX_EINVAL;
    CSX_TRY(csc_validate(A));
    *out = A;
    return CSX_OK;
}

}  // namespace

}  // namespace csx

using namespace csx;

extern "C" int csx_maxtrans(csx_handle_t hA, int64_t seed, int32_t *jimatch, int32_t *sprank) {
    Csc *A = nullptr;
    CSX_TRY(prepare(hA, &A));
    if (!jimatch) return CSX_EINVAL;
    hipStream_t s = ctx().stream;
    const int32_t m = A->m, n = A->n;
    Work W;
    CSX_TRY(begin(W));
    DevBuf<int32_t> jim;
    CSX_TRY(jim.alloc((size_t)m + n));
    CSX_TRY(maxtrans_device(A, seed, jim, jim + m, W));
    CSX_HIP(hipEventRecord(W.ev[2], s));
    CSX_HIP(hipMemcpyAsync(jimatch, jim, ((size_t)m + n) * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    CSX_TRY(finish_times(W, 2));
    if (sprank) {
        int32_t r = 0;
        for (int32_t i = 0; i < m; i++) r += jimatch[i] >= 0;
        *sprank = r;
    }
    return CSX_OK;
}

extern "C" int csx_scc(csx_handle_t hA, int32_t *p, int32_t *r, int32_t *nb) {
    Csc *A = nullptr;
    CSX_TRY(prepare(hA, &A));
    if (!p || !r || !nb || A->m != A->n) return CSX_EINVAL;
    hipStream_t s = ctx().stream;
    const int32_t n = A->n;
    *nb = 0;
    r[0] = 0;
    if (n == 0) return CSX_OK;
    Work W;
    CSX_TRY(begin(W));
    Csc T;
    const int32_t *Tp = nullptr, *Ti = nullptr;
    CSX_TRY(row_view(A, T, &Tp, &Ti));
    DevBuf<int32_t> ident, rs;
    DevBuf<uint32_t> ps;
    CSX_TRY(ident.alloc((size_t)n));
    CSX_TRY(rs.alloc((size_t)n + 1));
    CSX_TRY(ps.alloc((size_t)n));
    hipLaunchKernelGGL(k_iota, grid_of(n), dim3(256), 0, s, (uint32_t *)ident.get(), (int64_t)n);
    Graph G{n, A->p, A->i, Tp, Ti, ident, ident, ident, ident};
    CSX_HIP(hipEventRecord(W.ev[3], s));
    int32_t nb1 = 0;
    CSX_TRY(scc_device(G, 2 * ((int64_t)A->m + A->n + 1), ps, rs, &nb1, W));
    CSX_HIP(hipEventRecord(W.ev[4], s));
    CSX_HIP(hipMemcpyAsync(p, ps, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    CSX_HIP(hipMemcpyAsync(r, rs, ((size_t)nb1 + 1) * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    CSX_TRY(finish_times(W, 4));
    *nb = nb1;
    return CSX_OK;
}

extern "C" int csx_dmperm(csx_handle_t hA, int64_t seed, int32_t *p, int32_t *q, int32_t *r, int32_t *s_, int32_t *nb,
                          int32_t *rr, int32_t *cc) {
    Csc *A = nullptr;
    CSX_TRY(prepare(hA, &A));
    if (!p || !q || !r || !s_ || !nb || !rr || !cc) return CSX_EINVAL;
    hipStream_t s = ctx().stream;
    const int32_t m = A->m, n = A->n;
    Work W;
    CSX_TRY(begin(W));
    DevBuf<int32_t> jm, im, colset, rowset, cfr, rfr, dp, flag, pos;
    DevBuf<uint32_t> cls, iota, dq;
    DevBuf<int> cnt;
    CSX_TRY(jm.alloc((size_t)m));
    CSX_TRY(im.alloc((size_t)n));
    CSX_TRY(colset.alloc((size_t)n));
    CSX_TRY(rowset.alloc((size_t)m));
    CSX_TRY(cfr.alloc((size_t)n));
    CSX_TRY(rfr.alloc((size_t)m));
    CSX_TRY(dp.alloc((size_t)m));
    CSX_TRY(flag.alloc((size_t)m + 1));
    CSX_TRY(pos.alloc((size_t)m + 1));
    CSX_TRY(cls.alloc((size_t)n));
    CSX_TRY(iota.alloc((size_t)n));
    CSX_TRY(dq.alloc((size_t)n));
    CSX_TRY(cnt.alloc(4));
    CSX_TRY(maxtrans_device(A, seed, jm, im, W));
    CSX_HIP(hipEventRecord(W.ev[2], s));
    // coarse decomposition (csparse.py's two cs_bfs calls)
    const int64_t bound = (int64_t)m + n + 1;
    Csc T;
    const int32_t *Tp = nullptr, *Ti = nullptr;
    hipLaunchKernelGGL(k_fill, grid_of(m), dim3(256), 0, s, rowset, (int64_t)m, -1);
    hipLaunchKernelGGL(k_c1_seed, grid_of(n), dim3(256), 0, s, n, im, colset, cfr);
    CSX_TRY(reset_ctl(W.ctl));
    CSX_TRY(run_rounds(W.ctl, &W.h, bound, "csx_dmperm search from unmatched columns", [&]() -> int {
        hipLaunchKernelGGL(k_c1_expand, grid_of(n), dim3(256), 0, s, n, A->p, A->i, jm, rowset, colset, cfr, W.ctl);
        hipLaunchKernelGGL(k_advance, dim3(1), dim3(1), 0, s, W.ctl);
        CSX_LAUNCH_CHECK();
        return CSX_OK;
    }));
    CSX_HIP(hipMemsetAsync(cnt, 0, 4 * sizeof(int), s));
    hipLaunchKernelGGL(k_unmatched_flag, grid_of(m), dim3(256), 0, s, m, jm, flag);
    int64_t n_unmatched_rows = 0;
    if (m > 0) CSX_TRY(scan_exclusive_i32(flag, pos, m, &n_unmatched_rows));
    if (m > 0 && n > 0 && A->nnz > 0) CSX_TRY(row_view(A, T, &Tp, &Ti));
    if (n_unmatched_rows > 0 && Tp) {
        hipLaunchKernelGGL(k_c2_seed, grid_of(m), dim3(256), 0, s, m, jm, rowset, rfr);
        CSX_TRY(reset_ctl(W.ctl));
        CSX_TRY(run_rounds(W.ctl, &W.h, bound, "csx_dmperm search from unmatched rows", [&]() -> int {
            hipLaunchKernelGGL(k_c2_expand, grid_of(m), dim3(256), 0, s, m, Tp, Ti, im, rowset, colset, rfr, W.ctl);
            hipLaunchKernelGGL(k_advance, dim3(1), dim3(1), 0, s, W.ctl);
            CSX_LAUNCH_CHECK();
            return CSX_OK;
        }));
    }
    hipLaunchKernelGGL(k_col_class, grid_of(n), dim3(256), 0, s, n, colset, cls, cnt);
    hipLaunchKernelGGL(k_iota, grid_of(n), dim3(256), 0, s, iota, (int64_t)n);
    CSX_LAUNCH_CHECK();
    if (n > 0) CSX_TRY(stable_sort_by_key(cls, iota, nullptr, n, 4, nullptr, dq, nullptr));
    int hc[4] = {0, 0, 0, 0};
    CSX_HIP(hipMemcpyAsync(hc, cnt, sizeof(hc), hipMemcpyDeviceToHost, s));
    CSX_HIP(hipStreamSynchronize(s));
    cc[0] = 0;
    cc[1] = hc[0];
    cc[2] = cc[1] + hc[1];
    cc[3] = cc[2] + hc[2];
    cc[4] = n;
    rr[0] = 0;
    rr[1] = hc[1];
    rr[2] = rr[1] + hc[2];
    rr[3] = rr[2] + hc[3];
    rr[4] = m;
    if (rr[3] + n_unmatched_rows != m || cc[4] != cc[3] + hc[3]) {
        set_error("csx_dmperm: coarse sets do not add up (m %d, n %d, sprank %d, unmatched rows %lld)", m, n, rr[3],
                  (long long)n_unmatched_rows);
        return CSX_ERUNTIME;
    }
    hipLaunchKernelGGL(k_rows_of_cols, grid_of(n - cc[1]), dim3(256), 0, s, n, cc[1], dq, im, dp);
    hipLaunchKernelGGL(k_unmatched_put, grid_of(m), dim3(256), 0, s, m, rr[3], jm, pos, dp);
    CSX_LAUNCH_CHECK();
    CSX_HIP(hipEventRecord(W.ev[3], s));
    // fine decomposition: SCCs of A(R2, C2), each column identified with its matched row
    const int32_t nc = cc[3] - cc[2];
    std::vector<int32_t> rs_h;
    int32_t nb1 = 0;
    if (nc > 0) {
        DevBuf<int32_t> cv, rv, vc, vr, rs;
        DevBuf<uint32_t> ps;
        CSX_TRY(cv.alloc((size_t)nc));
        CSX_TRY(rv.alloc((size_t)nc));
        CSX_TRY(vc.alloc((size_t)n));
        CSX_TRY(vr.alloc((size_t)m));
        CSX_TRY(rs.alloc((size_t)nc + 1));
        CSX_TRY(ps.alloc((size_t)nc));
        hipLaunchKernelGGL(k_fill, grid_of(n), dim3(256), 0, s, vc, (int64_t)n, -1);
        hipLaunchKernelGGL(k_fill, grid_of(m), dim3(256), 0, s, vr, (int64_t)m, -1);
        hipLaunchKernelGGL(k_fine_maps, grid_of(nc), dim3(256), 0, s, nc, dq, cc[2], dp, rr[1], cv, rv, vc, vr);
        CSX_LAUNCH_CHECK();
        Graph G{nc, A->p, A->i, Tp, Ti, cv, rv, vc, vr};
        CSX_TRY(scc_device(G, 2 * ((int64_t)A->m + A->n + 1), ps, rs, &nb1, W));
        hipLaunchKernelGGL(k_fine_apply, grid_of(nc), dim3(256), 0, s, nc, ps, cv, rv, dq, cc[2], dp, rr[1]);
        CSX_LAUNCH_CHECK();
        rs_h.resize((size_t)nb1 + 1);
        CSX_HIP(hipMemcpyAsync(rs_h.data(), rs, ((size_t)nb1 + 1) * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    }
    CSX_HIP(hipEventRecord(W.ev[4], s));
    CSX_HIP(hipMemcpyAsync(p, dp, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    CSX_HIP(hipMemcpyAsync(q, dq, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    CSX_TRY(finish_times(W, 4));
    // fine blocks (csparse.py:982-996): the leading coarse block, the SCCs of A(R2, C2), the trailing coarse block
    for (int32_t k = 0; k < m + 6; k++) r[k] = 0;
    for (int32_t k = 0; k < n + 6; k++) s_[k] = 0;
    int32_t nb2 = 0;
    if (cc[2] > 0) nb2++;
    for (int32_t k = 0; k < nb1; k++) {
        r[nb2] = rs_h[k] + rr[1];
        s_[nb2] = rs_h[k] + cc[2];
        nb2++;
    }
    if (rr[2] < m) {
        r[nb2] = rr[2];
        s_[nb2] = cc[3];
        nb2++;
    }
    r[nb2] = m;
    s_[nb2] = n;
    *nb = nb2;
    return CSX_OK;
}

extern "C" int csx_dmperm_times(double *ms) {
    if (!ms) return CSX_EINVAL;
    for (int k = 0; k < 5; k++) ms[k] = g_stage_ms[k];
    return CSX_OK;
}

extern "C" int csx_dmperm_rounds(int64_t *rounds) {
    if (!rounds) return CSX_EINVAL;
    for (int k = 0; k < 5; k++) rounds[k] = g_rounds[k];
    return CSX_OK;
}
