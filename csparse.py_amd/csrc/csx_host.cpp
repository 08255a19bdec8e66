// Host-side (CPU, C++) steps that feed the device hot path.  These are the
// integer / data-dependent phases the reference also runs before its hot loops:
//   csx_schol_host   cs_schol, natural order          (csparse.py:2051-2072)
//   symbolic_fill    pattern of L from cs_ereach walks (csparse.py:1094-1131, 606-617)
//   csx_lu_host      cs_lu with partial pivoting       (csparse.py:1370-1451, 2078-2113)
// They are written from the algorithms, not transcribed: the elimination tree
// uses the same ancestor path compression idea, the column counts come from the
// row-pattern walk (O(|L|)) that the numeric phase needs anyway.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#include "csx_internal.h"

namespace csx {

// Elimination tree of the symmetric matrix whose upper triangle is (Ap, Ai)
// (entries with row > col are ignored).  With a permutation, node ids are the
// permuted ones: entry (i, j) of A is entry (min, max) of (pinv[i], pinv[j]).
// up_ptr/up_idx receive the upper-triangular pattern of the permuted matrix by column.
void upper_pattern(int32_t n, const int32_t *Ap, const int32_t *Ai, const int32_t *pinv, std::vector<int32_t> &up_ptr,
                   std::vector<int32_t> &up_idx) {
    up_ptr.assign((size_t)n + 1, 0);
    for (int32_t j = 0; j < n; j++) {
        const int32_t j2 = pinv ? pinv[j] : j;
        for (int32_t p = Ap[j]; p < Ap[j + 1]; p++) {
            const int32_t i = Ai[p];
            if (i > j) continue;
            const int32_t i2 = pinv ? pinv[i] : i;
            up_ptr[(size_t)std::max(i2, j2) + 1]++;
        }
    }
    for (int32_t j = 0; j < n; j++) up_ptr[(size_t)j + 1] += up_ptr[(size_t)j];
    up_idx.resize((size_t)up_ptr[(size_t)n]);
    std::vector<int32_t> fill(up_ptr.begin(), up_ptr.end() - 1);
    for (int32_t j = 0; j < n; j++) {
        const int32_t j2 = pinv ? pinv[j] : j;
        for (int32_t p = Ap[j]; p < Ap[j + 1]; p++) {
            const int32_t i = Ai[p];
            if (i > j) continue;
            const int32_t i2 = pinv ? pinv[i] : i;
            up_idx[(size_t)fill[(size_t)std::max(i2, j2)]++] = std::min(i2, j2);
        }
    }
}

void etree_of_upper(int32_t n, const std::vector<int32_t> &up_ptr, const std::vector<int32_t> &up_idx,
                    std::vector<int32_t> &parent) {
    parent.assign((size_t)n, -1);
    std::vector<int32_t> anc((size_t)n, -1);
    for (int32_t k = 0; k < n; k++) {
        for (int32_t p = up_ptr[(size_t)k]; p < up_ptr[(size_t)k + 1]; p++) {
            int32_t i = up_idx[(size_t)p];
            while (i != -1 && i < k) {
                const int32_t next = anc[(size_t)i];
                anc[(size_t)i] = k;
                if (next == -1) parent[(size_t)i] = k;
                i = next;
            }
        }
    }
}

// the same from a full CSC pattern: only entries above the diagonal of each column take part
void etree_of_csc(int32_t n, const int32_t *Ap, const int32_t *Ai, int32_t *parent) {
    std::vector<int32_t> anc((size_t)n, -1);
    for (int32_t k = 0; k < n; k++) parent[k] = -1;
    for (int32_t k = 0; k < n; k++) {
        for (int32_t p = Ap[k]; p < Ap[k + 1]; p++) {
            int32_t i = Ai[p];
            while (i != -1 && i < k) {
                const int32_t next = anc[(size_t)i];
                anc[(size_t)i] = k;
                if (next == -1) parent[i] = k;
                i = next;
            }
        }
    }
}

// Row patterns of L below the diagonal: for row k the columns i < k with L(k,i) != 0 are
// the nodes on the etree paths from the entries of column k of the upper pattern up to k.
// visit(k, i) is called once per such pair, k ascending.
template <class Visit>
static void walk_row_patterns(int32_t n, const std::vector<int32_t> &up_ptr, const std::vector<int32_t> &up_idx,
                              const int32_t *parent, Visit visit) {
    std::vector<int32_t> mark((size_t)n, -1);
    for (int32_t k = 0; k < n; k++) {
        mark[(size_t)k] = k;
        for (int32_t p = up_ptr[(size_t)k]; p < up_ptr[(size_t)k + 1]; p++) {
            for (int32_t i = up_idx[(size_t)p]; i != -1 && i < k && mark[(size_t)i] != k; i = parent[i]) {
                mark[(size_t)i] = k;
                visit(k, i);
            }
        }
    }
}

// ---- a fill-reducing ordering that suits level scheduling: nested dissection --------------------------
// The reference's cs_amd does not run, so order = 1 has no answer to match; what the
// device wants from an ordering is a BUSHY elimination tree (wide levels), and nested dissection gives
// exactly that: split the graph of A + A' by a vertex separator, order the two halves first (recursively,
// they are independent subtrees) and the separator last.  Separators here are the middle level of a
// breadth-first level structure rooted at a pseudo-peripheral vertex (two sweeps) -- crude but O(nnz log n),
// deterministic, and good on the mesh-like matrices sparse Cholesky is used for.  Parts of <= ND_LEAF
// vertices, and parts whose level structure is too shallow to cut, are numbered in breadth-first order.
// perm[k] = the original index of the k-th row/column of P A P' (cs_amd's convention, csparse.py:214).
namespace {
constexpr int32_t ND_LEAF = 96;

struct NdGraph {
    int32_t n;
    std::vector<int32_t> ptr, adj;
};

void nd_build_graph(int32_t n, const int32_t *Ap, const int32_t *Ai, NdGraph &G) {
    G.n = n;
    G.ptr.assign((size_t)n + 1, 0);
    for (int32_t j = 0; j < n; j++)
        for (int32_t p = Ap[j]; p < Ap[j + 1]; p++) {
            const int32_t i = Ai[p];
            if (i == j) continue;
            G.ptr[(size_t)i + 1]++;
            G.ptr[(size_t)j + 1]++;
        }
    for (int32_t v = 0; v < n; v++) G.ptr[(size_t)v + 1] += G.ptr[(size_t)v];
    G.adj.assign((size_t)G.ptr[(size_t)n], 0);
    std::vector<int32_t> fill(G.ptr.begin(), G.ptr.end() - 1);
    for (int32_t j = 0; j < n; j++)
        for (int32_t p = Ap[j]; p < Ap[j + 1]; p++) {
            const int32_t i = Ai[p];
            if (i == j) continue;
            G.adj[(size_t)fill[(size_t)i]++] = j;
            G.adj[(size_t)fill[(size_t)j]++] = i;
        }
}

// breadth-first search inside the part `tag` (part[v] == tag); fills order[] / level_start[]; returns the number of
// levels.  part / mark are shared by the worker threads: a thread writes only vertices of the part it owns, and reads
// of other parts' entries only ever compare unequal (tags and stamps are unique), hence relaxed atomics.
using AtomicVec = std::unique_ptr<std::atomic<int32_t>[]>;
inline int32_t ld(const AtomicVec &a, int32_t i) { return a[(size_t)i].load(std::memory_order_relaxed); }
inline void st(AtomicVec &a, int32_t i, int32_t v) { a[(size_t)i].store(v, std::memory_order_relaxed); }

int32_t nd_bfs(const NdGraph &G, const AtomicVec &part, int32_t tag, int32_t root, AtomicVec &mark, int32_t stamp,
               std::vector<int32_t> &order, std::vector<int32_t> &level_start) {
    order.clear();
    level_start.clear();
    order.push_back(root);
    st(mark, root, stamp);
    size_t head = 0;
    while (head < order.size()) {
        level_start.push_back((int32_t)head);
        const size_t end = order.size();
        for (; head < end; head++) {
            const int32_t v = order[head];
            for (int32_t q = G.ptr[(size_t)v]; q < G.ptr[(size_t)v + 1]; q++) {
                const int32_t u = G.adj[(size_t)q];
                if (ld(part, u) == tag && ld(mark, u) != stamp) {
                    st(mark, u, stamp);
                    order.push_back(u);
                }
            }
        }
    }
    level_start.push_back((int32_t)order.size());
    return (int32_t)level_start.size() - 1;
}

struct NdJob {
    int32_t tag, out_lo;             // the part and where its vertices go in perm
    std::vector<int32_t> verts;
};

// The recursion as a pool of jobs: the two halves of a cut are independent, so after a few levels every worker has
// parts of its own.  The ordering does not depend on which thread takes which part (a part's numbering is a function
// of its vertex list and the graph alone).
struct NdPool {
    const NdGraph &G;
    int32_t *perm;
    AtomicVec part, mark;
    std::atomic<int32_t> next_tag{1}, stamp{0};
    std::mutex mu;
    std::condition_variable cv;
    std::vector<NdJob> jobs;
    int pending = 0;                 // jobs queued or being worked on

    NdPool(const NdGraph &g, int32_t *p) : G(g), perm(p) {
        part.reset(new std::atomic<int32_t>[(size_t)std::max(g.n, 1)]);
        mark.reset(new std::atomic<int32_t>[(size_t)std::max(g.n, 1)]);
        for (int32_t v = 0; v < g.n; v++) {
            st(part, v, 0);
            st(mark, v, -1);
        }
    }
    void push(NdJob &&j) {
        std::lock_guard<std::mutex> lock(mu);
        jobs.push_back(std::move(j));
        pending++;
        cv.notify_one();
    }
    bool pop(NdJob &j) {
        std::unique_lock<std::mutex> lock(mu);
        cv.wait(lock, [&] { return !jobs.empty() || pending == 0; });
        if (jobs.empty()) return false;
        j = std::move(jobs.back());
        jobs.pop_back();
        return true;
    }
    void finished() {
        std::lock_guard<std::mutex> lock(mu);
        if (--pending == 0) cv.notify_all();
    }
    void work() {
        std::vector<int32_t> order, level_start;
        NdJob job;
        while (pop(job)) {
            run(job, order, level_start);
            finished();
        }
    }
    void run(NdJob &job, std::vector<int32_t> &order, std::vector<int32_t> &level_start) {
        const int32_t sz = (int32_t)job.verts.size();
        if (sz == 0) return;
        // one connected component at a time: the rest goes back to the pool as its own part
        int32_t stp = ++stamp;
        nd_bfs(G, part, job.tag, job.verts[0], mark, stp, order, level_start);
        if ((int32_t)order.size() < sz) {
            NdJob rest;
            rest.tag = next_tag++;
            rest.out_lo = job.out_lo + (int32_t)order.size();
            for (int32_t v : job.verts)
                if (ld(mark, v) != stp) {
                    rest.verts.push_back(v);
                    st(part, v, rest.tag);
                }
            push(std::move(rest));
        }
        const int32_t csz = (int32_t)order.size();
        // pseudo-peripheral root: restart from a vertex of the last level (smallest degree), twice
        for (int sweep = 0; sweep < 2 && csz > ND_LEAF; sweep++) {
            const int32_t nl = (int32_t)level_start.size() - 1;
            int32_t far = order[(size_t)level_start[(size_t)nl - 1]];
            for (int32_t q = level_start[(size_t)nl - 1]; q < level_start[(size_t)nl]; q++) {
                const int32_t v = order[(size_t)q];
                if (G.ptr[(size_t)v + 1] - G.ptr[(size_t)v] < G.ptr[(size_t)far + 1] - G.ptr[(size_t)far]) far = v;
            }
            stp = ++stamp;
            nd_bfs(G, part, job.tag, far, mark, stp, order, level_start);
        }
        const int32_t nl = (int32_t)level_start.size() - 1;
        if (csz <= ND_LEAF || nl < 3) {   // leaf (or too shallow to cut): breadth-first numbering
            for (int32_t q = 0; q < csz; q++) perm[job.out_lo + q] = order[(size_t)q];
            return;
        }
        // separator = the level at which half of the component has been passed (never the first or last level)
        int32_t s = 1;
        while (s < nl - 2 && level_start[(size_t)s + 1] < csz / 2) s++;
        const int32_t a_end = level_start[(size_t)s], b_begin = level_start[(size_t)s + 1];
        // thin the separator: only the vertices of level s that touch level s + 1 have to be in it; the others
        // stay with the first half (every path into the second half leaves level s through such a vertex)
        const int32_t next_mark = -2 - stp;
        for (int32_t q = b_begin; q < level_start[(size_t)s + 2]; q++) st(mark, order[(size_t)q], next_mark);  // level s+1
        NdJob A, B;
        A.tag = next_tag++;
        B.tag = next_tag++;
        A.verts.assign(order.begin(), order.begin() + a_end);
        std::vector<int32_t> sep;
        for (int32_t q = a_end; q < b_begin; q++) {
            const int32_t v = order[(size_t)q];
            bool touches = false;
            for (int32_t e = G.ptr[(size_t)v]; e < G.ptr[(size_t)v + 1] && !touches; e++)
                touches = ld(mark, G.adj[(size_t)e]) == next_mark;
            if (touches) sep.push_back(v);
            else A.verts.push_back(v);
        }
        B.verts.assign(order.begin() + b_begin, order.end());
        A.out_lo = job.out_lo;
        B.out_lo = job.out_lo + (int32_t)A.verts.size();
        for (int32_t v : A.verts) st(part, v, A.tag);
        for (int32_t v : B.verts) st(part, v, B.tag);
        int32_t out = B.out_lo + (int32_t)B.verts.size();     // the separator goes last
        for (int32_t v : sep) {
            st(part, v, -1);
            perm[out++] = v;
        }
        push(std::move(A));
        push(std::move(B));
    }
};
}  // namespace

}  // namespace csx

using namespace csx;

extern "C" int csx_order_nd_host(int32_t n, const int32_t *Ap, const int32_t *Ai, int32_t *perm) {
    if (n < 0 || !Ap || (!Ai && Ap[n] > 0) || !perm) return CSX_EINVAL;
    for (int32_t j = 0; j < n; j++)
        for (int32_t p = Ap[j]; p < Ap[j + 1]; p++)
            if (Ai[p] < 0 || Ai[p] >= n) return CSX_EINVAL;
    if (n == 0) return CSX_OK;
    NdGraph G;
    nd_build_graph(n, Ap, Ai, G);
    NdPool pool(G, perm);
    {
        NdJob all;
        all.tag = 0;
        all.out_lo = 0;
        all.verts.resize((size_t)n);
        for (int32_t v = 0; v < n; v++) all.verts[(size_t)v] = v;
        pool.push(std::move(all));
    }
    // small problems: one thread (the pool costs more than it saves); else up to eight workers
    unsigned workers = 1;
    if (n >= 20000 || Ap[n] >= 200000) workers = std::min(8u, std::max(1u, std::thread::hardware_concurrency()));
    std::vector<std::thread> threads;
    for (unsigned t = 1; t < workers; t++) threads.emplace_back([&pool] { pool.work(); });
    pool.work();
    for (auto &t : threads) t.join();
    return CSX_OK;
}

namespace csx {

}  // namespace csx

using namespace csx;

// cs_counts (csparse.py:703-764, with cs_leaf :1280-1304 and the row lists of _init_ata :677-700): the column counts of
// chol(A) (ata = 0: A square, its upper triangle used) or of chol(A'A) (ata != 0: A m-by-n) from the elimination tree
// `parent` and its postorder `post` (both n entries, the caller's -- cs_etree / cs_post), without forming L.  For every node j
// in postorder the rows of the columns filed under j (ata: the rows whose leftmost column, by postorder rank, is j; else
// column j itself) are run through the skeleton test: A(i, j) counts where j is a leaf of row i's subtree, and the least
// common ancestor of two consecutive leaves loses the overlap; the deltas are then summed up the tree.
extern "C" int csx_counts_host(int32_t m, int32_t n, const int32_t *Ap, const int32_t *Ai, const int32_t *parent,
                               const int32_t *post, int ata, int32_t *colcount) {
    if (m < 0 || n < 0 || !Ap || (!Ai && Ap[n] > 0) || !parent || !post || !colcount) return CSX_EINVAL;
    if (!ata && m != n) return CSX_EINVAL;
    const int64_t nnz = Ap[n];
    for (int64_t p = 0; p < nnz; p++)
        if (Ai[p] < 0 || Ai[p] >= m) return CSX_EINVAL;
    {   // parent must be a forest on n nodes with parents above their children's... any value in [-1, n); post a permutation
        std::vector<char> seen((size_t)n, 0);
        for (int32_t k = 0; k < n; k++) {
            if (parent[k] < -1 || parent[k] >= n || post[k] < 0 || post[k] >= n || seen[(size_t)post[k]]) return CSX_EINVAL;
            seen[(size_t)post[k]] = 1;
        }
    }
    // the pattern of A' (row i of A lists its columns in ascending order): cs_transpose(A, False), csparse.py:721
    std::vector<int32_t> ATp((size_t)m + 1, 0), ATi((size_t)nnz);
    for (int64_t p = 0; p < nnz; p++) ATp[(size_t)Ai[p] + 1]++;
    for (int32_t i = 0; i < m; i++) ATp[(size_t)i + 1] += ATp[(size_t)i];
    {
        std::vector<int32_t> fill(ATp.begin(), ATp.end() - 1);
        for (int32_t k = 0; k < n; k++)
            for (int32_t p = Ap[k]; p < Ap[k + 1]; p++) ATi[(size_t)fill[(size_t)Ai[p]]++] = k;
    }
    std::vector<int32_t> first((size_t)n, -1), maxfirst((size_t)n, -1), prevleaf((size_t)n, -1), anc((size_t)n);
    int32_t *delta = colcount;
    for (int32_t k = 0; k < n; k++) {                 // first[j] = postorder rank of the first descendant of j
        int32_t j = post[k];
        delta[j] = first[(size_t)j] == -1 ? 1 : 0;    // 1 for a leaf
        int32_t guard = 0;
        while (j != -1 && first[(size_t)j] == -1) {
            first[(size_t)j] = k;
            j = parent[j];
            if (++guard > n) return CSX_EINVAL;       // a cycle in `parent`
        }
    }
    std::vector<int32_t> head, nxt;
    if (ata) {                                        // _init_ata: row i filed under the smallest postorder rank among its columns
        std::vector<int32_t> rank((size_t)n, 0);
        head.assign((size_t)n + 1, -1);
        nxt.assign((size_t)m, -1);
        for (int32_t k = 0; k < n; k++) rank[(size_t)post[k]] = k;
        for (int32_t i = 0; i < m; i++) {
            int32_t k = n;
            for (int32_t p = ATp[(size_t)i]; p < ATp[(size_t)i + 1]; p++) k = std::min(k, rank[(size_t)ATi[(size_t)p]]);
            nxt[(size_t)i] = head[(size_t)k];
            head[(size_t)k] = i;
        }
    }
    for (int32_t j = 0; j < n; j++) anc[(size_t)j] = j;
    for (int32_t k = 0; k < n; k++) {
        const int32_t j = post[k];
        if (parent[j] != -1) delta[parent[j]]--;      // j is not a root
        for (int32_t J = ata ? head[(size_t)k] : j; J != -1; J = ata ? nxt[(size_t)J] : -1) {
            for (int32_t p = ATp[(size_t)J]; p < ATp[(size_t)J + 1]; p++) {
                const int32_t i = ATi[(size_t)p];
                if (i <= j || first[(size_t)j] <= maxfirst[(size_t)i]) continue;      // cs_leaf: j is not a leaf of row i's subtree
                maxfirst[(size_t)i] = first[(size_t)j];
                const int32_t jprev = prevleaf[(size_t)i];
                prevleaf[(size_t)i] = j;
                delta[j]++;                           // A(i, j) is in the skeleton
                if (jprev != -1) {                    // a later leaf: the least common ancestor of the two loses the overlap
                    int32_t q = jprev;
                    while (q != anc[(size_t)q]) q = anc[(size_t)q];
                    for (int32_t s = jprev; s != q;) {
                        const int32_t sp = anc[(size_t)s];
                        anc[(size_t)s] = q;
                        s = sp;
                    }
                    delta[q]--;
                }
            }
        }
        if (parent[j] != -1) anc[(size_t)j] = parent[j];
    }
    for (int32_t j = 0; j < n; j++)
        if (parent[j] != -1) colcount[parent[j]] += colcount[j];
    return CSX_OK;
}

extern "C" int csx_schol_host(int32_t n, const int32_t *Ap, const int32_t *Ai, int32_t *parent, int32_t *cp) {
    if (n < 0 || !Ap || (!Ai && Ap[n] > 0) || !parent || !cp) return CSX_EINVAL;
    for (int32_t j = 0; j < n; j++)
        for (int32_t p = Ap[j]; p < Ap[j + 1]; p++)
            if (Ai[p] < 0 || Ai[p] >= n) return CSX_EINVAL;
    std::vector<int32_t> up_ptr, up_idx, par;
    upper_pattern(n, Ap, Ai, nullptr, up_ptr, up_idx);
    etree_of_upper(n, up_ptr, up_idx, par);
    std::vector<int32_t> count((size_t)n, 1);  // the diagonal
    walk_row_patterns(n, up_ptr, up_idx, par.data(), [&](int32_t, int32_t i) { count[(size_t)i]++; });
    int64_t run = 0;
    for (int32_t j = 0; j < n; j++) {
        parent[j] = par[(size_t)j];
        cp[j] = (int32_t)run;
        run += count[(size_t)j];
        if (run > 2147483647ll) return CSX_EINVAL;
    }
    cp[n] = (int32_t)run;
    return CSX_OK;
}

// ---- LU, left-looking, threshold partial pivoting, natural column order -----------------
// Output: L (unit diagonal first in each column, row indices in pivot order), U (diagonal last),
// pinv (row i of A is row pinv[i] of L U).  Arrays are malloc'ed; free with csx_host_free.
extern "C" int csx_lu_host(int32_t n, const int32_t *Ap, const int32_t *Ai, const double *Ax, double tol,
                           int32_t **Lp_out, int32_t **Li_out, double **Lx_out, int32_t **Up_out, int32_t **Ui_out,
                           double **Ux_out, int32_t *pinv) {
    if (n < 0 || !Ap || !Ai || !Ax || !Lp_out || !Li_out || !Lx_out || !Up_out || !Ui_out || !Ux_out || !pinv)
        return CSX_EINVAL;
    std::vector<int32_t> Lp((size_t)n + 1, 0), Up((size_t)n + 1, 0), Li, Ui;
    std::vector<double> Lx, Ux, x((size_t)n, 0.0);
    std::vector<int32_t> reach((size_t)n), stack((size_t)n), pos((size_t)n);
    std::vector<char> seen((size_t)n, 0);
    for (int32_t i = 0; i < n; i++) pinv[i] = -1;
    for (int32_t k = 0; k < n; k++) {
        Lp[(size_t)k] = (int32_t)Li.size();
        Up[(size_t)k] = (int32_t)Ui.size();
        // reach of A(:,k) in the graph of L (rows already pivotal map to columns of L): DFS,
        // topological order in reach[top..n-1]
        int32_t top = n;
        for (int32_t p = Ap[k]; p < Ap[k + 1]; p++) {
            if (seen[(size_t)Ai[p]]) continue;
            int32_t head = 0;
            stack[0] = Ai[p];
            while (head >= 0) {
                const int32_t j = stack[(size_t)head];
                const int32_t col = pinv[j];
                if (!seen[(size_t)j]) {
                    seen[(size_t)j] = 1;
                    pos[(size_t)head] = col < 0 ? 0 : Lp[(size_t)col];
                }
                bool done = true;
                const int32_t end = col < 0 ? 0 : (col == k ? (int32_t)Li.size() : Lp[(size_t)col + 1]);
                for (int32_t q = pos[(size_t)head]; q < end; q++) {
                    const int32_t i = Li[(size_t)q];
                    if (seen[(size_t)i]) continue;
                    pos[(size_t)head] = q;
                    stack[(size_t)++head] = i;
                    done = false;
                    break;
                }
                if (done) {
                    head--;
                    reach[(size_t)--top] = j;
                }
            }
        }
        for (int32_t p = top; p < n; p++) {
            seen[(size_t)reach[(size_t)p]] = 0;
            x[(size_t)reach[(size_t)p]] = 0.0;
        }
        for (int32_t p = Ap[k]; p < Ap[k + 1]; p++) x[(size_t)Ai[p]] = Ax[p];
        // sparse triangular solve x = L \ A(:,k) along the reach
        for (int32_t px = top; px < n; px++) {
            const int32_t j = reach[(size_t)px], col = pinv[j];
            if (col < 0) continue;
            x[(size_t)j] /= Lx[(size_t)Lp[(size_t)col]];
            const double xj = x[(size_t)j];
            for (int32_t q = Lp[(size_t)col] + 1; q < Lp[(size_t)col + 1]; q++) x[(size_t)Li[(size_t)q]] -= Lx[(size_t)q] * xj;
        }
        // pivot search among non-pivotal rows; pivotal rows go to U
        int32_t ipiv = -1;
        double a = -1.0;
        for (int32_t p = top; p < n; p++) {
            const int32_t i = reach[(size_t)p];
            if (pinv[i] < 0) {
                const double t = std::fabs(x[(size_t)i]);
                if (t > a) {
                    a = t;
                    ipiv = i;
                }
            } else {
                Ui.push_back(pinv[i]);
                Ux.push_back(x[(size_t)i]);
            }
        }
        if (ipiv == -1 || a <= 0) return CSX_ENOTSPD;  // singular: the reference returns None (csparse.py:1423)
        if (pinv[k] < 0 && std::fabs(x[(size_t)k]) >= a * tol) ipiv = k;
        const double pivot = x[(size_t)ipiv];
        Ui.push_back(k);
        Ux.push_back(pivot);
        pinv[ipiv] = k;
        Li.push_back(ipiv);
        Lx.push_back(1.0);
        for (int32_t p = top; p < n; p++) {
            const int32_t i = reach[(size_t)p];
            if (pinv[i] < 0) {
                Li.push_back(i);
                Lx.push_back(x[(size_t)i] / pivot);
            }
            x[(size_t)i] = 0.0;
        }
        // L's column k is complete only now; DFS above used Li.size() as its end while building
        Lp[(size_t)k + 1] = (int32_t)Li.size();
    }
    Lp[(size_t)n] = (int32_t)Li.size();
    Up[(size_t)n] = (int32_t)Ui.size();
    for (auto &r : Li) r = pinv[r];
    auto dup_i = [](const std::vector<int32_t> &v) {
        int32_t *p = (int32_t *)std::malloc((v.size() + 1) * sizeof(int32_t));
        if (!v.empty()) std::memcpy(p, v.data(), v.size() * sizeof(int32_t));
        return p;
    };
    auto dup_d = [](const std::vector<double> &v) {
        double *p = (double *)std::malloc((v.size() + 1) * sizeof(double));
        if (!v.empty()) std::memcpy(p, v.data(), v.size() * sizeof(double));
        return p;
    };
    *Lp_out = dup_i(Lp);
    *Li_out = dup_i(Li);
    *Lx_out = dup_d(Lx);
    *Up_out = dup_i(Up);
    *Ui_out = dup_i(Ui);
    *Ux_out = dup_d(Ux);
    return CSX_OK;
}

extern "C" void csx_host_free(void *p) { std::free(p); }

// ---- sparse Householder QR, numeric phase (csparse.py:1797-1870 with :1216-1261) -------------------------------
// Left-looking: column k of R and the Householder vector V(:,k) come from column q[k] of A after the earlier
// reflections that touch it have been applied.  Which ones touch it is read off the column elimination tree:
// every nonzero row i of the column starts a walk from leftmost[i] (the first column that has an entry in row i)
// towards the root; the walk stops at a column already collected for this k.  The collected columns, each path
// kept in root-ward order and later paths placed in front of earlier ones, are the nonzero pattern of R(:,k) in
// an order in which every reflection precedes its ancestors -- the order the reflections are applied in and the
// order the entries of R(:,k) are stored in (diagonal last).  V(:,k)'s pattern is the permuted rows of the column
// below k together with the patterns of the V columns whose tree parent is k.
//
// Symbolic input from cs_sqr: parent (column etree of A'A), pinv (row permutation, length m2), leftmost (length m),
// m2 (rows incl. fictitious ones), capacities vcap / rcap.  Output arrays are the caller's (sized by cs_sqr's counts).
extern "C" int csx_qr_host(int32_t m, int32_t n, int32_t m2, const int32_t *Ap, const int32_t *Ai, const double *Ax,
                           const int32_t *q, const int32_t *parent, const int32_t *pinv, const int32_t *leftmost,
                           int32_t vcap, int32_t rcap, int32_t *Vp, int32_t *Vi, double *Vx, int32_t *Rp, int32_t *Ri,
                           double *Rx, double *beta) {
    if (m < 0 || n < 0 || m2 < m || !Ap || !Ai || !Ax || !parent || !pinv || !leftmost || !Vp || !Vi || !Vx || !Rp ||
        !Ri || !Rx || !beta)
        return CSX_EINVAL;
    std::vector<int32_t> stamp((size_t)m2, -1);      // stamp[r] == k: row / column r already collected for column k
    std::vector<int32_t> order((size_t)n > 0 ? (size_t)n : 1), path((size_t)n > 0 ? (size_t)n : 1);
    std::vector<double> work((size_t)m2, 0.0);       // the column being reduced, in permuted row numbering
    int32_t vnz = 0, rnz = 0;
    // y <- (I - b v v') y for a stored reflection
    auto reflect = [&](int32_t col, double b) {
        double dot = 0.0;
        for (int32_t p = Vp[col]; p < Vp[col + 1]; p++) dot += Vx[p] * work[(size_t)Vi[p]];
        dot *= b;
        for (int32_t p = Vp[col]; p < Vp[col + 1]; p++) work[(size_t)Vi[p]] -= Vx[p] * dot;
    };
    for (int32_t k = 0; k < n; k++) {
        Rp[k] = rnz;
        Vp[k] = vnz;
        const int32_t vstart = vnz;
        if (vnz >= vcap) return CSX_EINVAL;
        stamp[(size_t)k] = k;                        // the diagonal position leads V(:,k)
        Vi[vnz++] = k;
        int32_t front = n;                           // order[front..n) = reflections to apply, children before parents
        const int32_t col = q ? q[k] : k;
        for (int32_t p = Ap[col]; p < Ap[col + 1]; p++) {
            int32_t len = 0;
            for (int32_t c = leftmost[Ai[p]]; stamp[(size_t)c] != k; c = parent[c]) {
                path[(size_t)len++] = c;
                stamp[(size_t)c] = k;
            }
            while (len > 0) order[(size_t)--front] = path[(size_t)--len];
            const int32_t r = pinv[Ai[p]];
            work[(size_t)r] = Ax[p];
            if (r > k && stamp[(size_t)r] < k) {     // a row below the diagonal not yet in V(:,k)'s pattern
                if (vnz >= vcap) return CSX_EINVAL;
                Vi[vnz++] = r;
                stamp[(size_t)r] = k;
            }
        }
        for (int32_t t = front; t < n; t++) {
            const int32_t c = order[(size_t)t];
            reflect(c, beta[c]);
            if (rnz >= rcap) return CSX_EINVAL;
            Ri[rnz] = c;
            Rx[rnz++] = work[(size_t)c];
            work[(size_t)c] = 0.0;
            if (parent[c] == k) {                    // V(:,c)'s rows below c pass on to V(:,k)
                for (int32_t p = Vp[c]; p < Vp[c + 1]; p++) {
                    const int32_t r = Vi[p];
                    if (stamp[(size_t)r] < k) {
                        if (vnz >= vcap) return CSX_EINVAL;
                        stamp[(size_t)r] = k;
                        Vi[vnz++] = r;
                    }
                }
            }
        }
        for (int32_t p = vstart; p < vnz; p++) {
            Vx[p] = work[(size_t)Vi[p]];
            work[(size_t)Vi[p]] = 0.0;
        }
        // Householder vector of Vx[vstart..vnz): afterwards (I - beta v v') x = s e1 (csparse.py:1238-1261)
        double tail2 = 0.0;
        for (int32_t p = vstart + 1; p < vnz; p++) tail2 += Vx[p] * Vx[p];
        const double head = Vx[vstart];
        double s, b;
        if (tail2 == 0.0) {
            s = std::fabs(head);
            b = head <= 0.0 ? 2.0 : 0.0;
            Vx[vstart] = 1.0;
        } else {
            s = std::sqrt(head * head + tail2);
            Vx[vstart] = head <= 0.0 ? head - s : -tail2 / (head + s);
            b = -1.0 / (s * Vx[vstart]);
        }
        if (rnz >= rcap) return CSX_EINVAL;
        Ri[rnz] = k;
        Rx[rnz++] = s;
        beta[k] = b;
    }
    Rp[n] = rnz;
    Vp[n] = vnz;
    return CSX_OK;
}

// x <- Q' x (transpose = 1: reflections 0 .. n-1 in order) or x <- Q x (transpose = 0: n-1 .. 0), csparse.py:1216-1235
extern "C" int csx_qr_apply_host(int32_t n, const int32_t *Vp, const int32_t *Vi, const double *Vx, const double *beta,
                                 int transpose, double *x) {
    if (n < 0 || !Vp || !Vi || !Vx || !beta || !x) return CSX_EINVAL;
    for (int32_t t = 0; t < n; t++) {
        const int32_t k = transpose ? t : n - 1 - t;
        double dot = 0.0;
        for (int32_t p = Vp[k]; p < Vp[k + 1]; p++) dot += Vx[p] * x[Vi[p]];
        dot *= beta[k];
        for (int32_t p = Vp[k]; p < Vp[k + 1]; p++) x[Vi[p]] -= Vx[p] * dot;
    }
    return CSX_OK;
}

// cs_sqr for QR with the natural column order (csparse.py:2187-2217): the column elimination tree (cs_etree of A'A,
// :1136-1169), its postorder (:1711-1742), the column counts of R = chol(A'A) (cs_counts with ata, :703-764 and
// :677-700) and cs_vcount (:2118-2184: leftmost[], the row permutation pinv, the rows of V, m2 with the
// fictitious rows of a structurally rank-deficient A).  Written from the algorithms; the same results as the
// Python versions in csparse.py, which stay as the list-level functions cs_etree / cs_post.
// parent, cp: n entries; pinv: m + n; leftmost: m.
extern "C" int csx_sqr_host(int32_t m, int32_t n, const int32_t *Ap, const int32_t *Ai, int32_t *parent, int32_t *cp,
                            int32_t *pinv, int32_t *leftmost, int32_t *m2_out, int64_t *vnz_out, int64_t *rnz_out) {
    if (m < 0 || n < 0 || !Ap || !Ai || !parent || !cp || !pinv || !leftmost || !m2_out || !vnz_out || !rnz_out)
        return CSX_EINVAL;
    const int64_t nnz = Ap[n];
    for (int64_t p = 0; p < nnz; p++)
        if (Ai[p] < 0 || Ai[p] >= m) return CSX_EINVAL;
    // ---- column elimination tree: the tree of A'A without forming it (a row links the columns it touches) ----
    {
        std::vector<int32_t> anc((size_t)n, -1), prev((size_t)m, -1);
        for (int32_t k = 0; k < n; k++) {
            parent[k] = -1;
            for (int32_t p = Ap[k]; p < Ap[k + 1]; p++) {
                int32_t i = prev[(size_t)Ai[p]];
                while (i != -1 && i < k) {
                    const int32_t up = anc[(size_t)i];
                    anc[(size_t)i] = k;
                    if (up == -1) parent[i] = k;
                    i = up;
                }
                prev[(size_t)Ai[p]] = k;
            }
        }
    }
    // ---- postorder (children in ascending order, roots in ascending order) ----
    std::vector<int32_t> post;
    post.reserve((size_t)n);
    {
        std::vector<int32_t> first_child((size_t)n, -1), sibling((size_t)n, -1), stack;
        for (int32_t j = n - 1; j >= 0; j--)
            if (parent[j] != -1) {
                sibling[(size_t)j] = first_child[(size_t)parent[j]];
                first_child[(size_t)parent[j]] = j;
            }
        for (int32_t root = 0; root < n; root++) {
            if (parent[root] != -1) continue;
            stack.assign(1, root);
            while (!stack.empty()) {
                const int32_t top = stack.back();
                const int32_t c = first_child[(size_t)top];
                if (c == -1) {
                    post.push_back(top);
                    stack.pop_back();
                } else {
                    first_child[(size_t)top] = sibling[(size_t)c];
                    stack.push_back(c);
                }
            }
        }
    }
    // ---- rows of A (pattern of A'), by a counting sort: row i lists its columns in ascending order ----
    std::vector<int32_t> ATp((size_t)m + 1, 0), ATi((size_t)nnz);
    for (int64_t p = 0; p < nnz; p++) ATp[(size_t)Ai[p] + 1]++;
    for (int32_t i = 0; i < m; i++) ATp[(size_t)i + 1] += ATp[(size_t)i];
    {
        std::vector<int32_t> fill(ATp.begin(), ATp.end() - 1);
        for (int32_t k = 0; k < n; k++)
            for (int32_t p = Ap[k]; p < Ap[k + 1]; p++) ATi[(size_t)fill[(size_t)Ai[p]]++] = k;
    }
    // ---- column counts of chol(A'A): rows grouped by the postorder rank of their leftmost column, then the
    //      skeleton / leaf counting over those rows ----
    {
        std::vector<int32_t> rank((size_t)n, 0), head((size_t)n + 1, -1), nxt((size_t)m, -1);
        for (int32_t k = 0; k < n; k++) rank[(size_t)post[(size_t)k]] = k;
        for (int32_t i = 0; i < m; i++) {
            int32_t k = n;
            for (int32_t p = ATp[(size_t)i]; p < ATp[(size_t)i + 1]; p++) k = std::min(k, rank[(size_t)ATi[(size_t)p]]);
            nxt[(size_t)i] = head[(size_t)k];
            head[(size_t)k] = i;
        }
        std::vector<int32_t> first((size_t)n, -1), maxfirst((size_t)n, -1), prevleaf((size_t)n, -1), anc((size_t)n);
        for (int32_t k = 0; k < n; k++) {
            int32_t j = post[(size_t)k];
            cp[j] = first[(size_t)j] == -1 ? 1 : 0;                  // cp doubles as delta
            while (j != -1 && first[(size_t)j] == -1) {
                first[(size_t)j] = k;
                j = parent[j];
            }
        }
        for (int32_t j = 0; j < n; j++) anc[(size_t)j] = j;
        for (int32_t k = 0; k < n; k++) {
            const int32_t j = post[(size_t)k];
            if (parent[j] != -1) cp[parent[j]]--;
            for (int32_t J = head[(size_t)k]; J != -1; J = nxt[(size_t)J]) {
                for (int32_t p = ATp[(size_t)J]; p < ATp[(size_t)J + 1]; p++) {
                    const int32_t i = ATi[(size_t)p];
                    if (i <= j || first[(size_t)j] <= maxfirst[(size_t)i]) continue;
                    maxfirst[(size_t)i] = first[(size_t)j];
                    const int32_t jprev = prevleaf[(size_t)i];
                    prevleaf[(size_t)i] = j;
                    cp[j]++;
                    if (jprev != -1) {
                        int32_t q = jprev;
                        while (q != anc[(size_t)q]) q = anc[(size_t)q];
                        for (int32_t s = jprev; s != q;) {
                            const int32_t sp = anc[(size_t)s];
                            anc[(size_t)s] = q;
                            s = sp;
                        }
                        cp[q]--;
                    }
                }
            }
            if (parent[j] != -1) anc[(size_t)j] = parent[j];
        }
        for (int32_t j = 0; j < n; j++)
            if (parent[j] != -1) cp[parent[j]] += cp[j];
    }
    int64_t rnz = 0;
    for (int32_t j = 0; j < n; j++) rnz += cp[j];
    // ---- cs_vcount: leftmost column of every row, rows handed to the columns along the tree, pinv, m2, nnz(V) ----
    for (int32_t i = 0; i < m + n; i++) pinv[i] = -1;
    for (int32_t i = 0; i < m; i++) leftmost[i] = -1;
    for (int32_t k = n - 1; k >= 0; k--)
        for (int32_t p = Ap[k]; p < Ap[k + 1]; p++) leftmost[Ai[p]] = k;
    std::vector<int32_t> head((size_t)n, -1), tail((size_t)n, -1), count((size_t)n, 0), nxt((size_t)m, -1);
    for (int32_t i = m - 1; i >= 0; i--) {
        const int32_t k = leftmost[i];
        if (k == -1) continue;
        if (count[(size_t)k]++ == 0) tail[(size_t)k] = i;
        nxt[(size_t)i] = head[(size_t)k];
        head[(size_t)k] = i;
    }
    int64_t vnz = 0;
    int32_t m2 = m;
    for (int32_t k = 0; k < n; k++) {
        int32_t i = head[(size_t)k];
        vnz++;
        if (i < 0) i = m2++;                                       // a fictitious row for a column without one
        pinv[i] = k;
        if (--count[(size_t)k] <= 0) continue;
        vnz += count[(size_t)k];
        const int32_t pa = parent[k];
        if (pa != -1) {
            if (count[(size_t)pa] == 0) tail[(size_t)pa] = tail[(size_t)k];
            nxt[(size_t)tail[(size_t)k]] = head[(size_t)pa];
            head[(size_t)pa] = nxt[(size_t)i];
            count[(size_t)pa] += count[(size_t)k];
        }
    }
    for (int32_t i = 0, k = n; i < m; i++)
        if (pinv[i] < 0) pinv[i] = k++;
    *m2_out = m2;
    *vnz_out = vnz;
    *rnz_out = rnz;
    return CSX_OK;
}

// ---- refactor: cs_lu's numeric steps with the pivots and the patterns of L and U kept ----------------
// Column k (in the factorisation's column order) in pivot-row space: x = 0 on the rows of U(:,k) and L(:,k), x[pinv[i]] =
// A(i,k) in storage order (assignment, as cs_spsolve); for every entry J of U(:,k) but the last, in storage order: U.x = x[J],
// x[L.i[t]] -= L.x[t] x[J] over L(:,J) after its unit diagonal; the pivot x[k] goes last into U(:,k) and L(:,k) = x / pivot
// after the unit diagonal.  The stored order is the topological order cs_lu solved in, so L and U come out byte-equal to
// cs_lu's whenever it would choose the same pivots.  x: n zeros on entry, left zero.  *ok = 0 at the first pivot that is 0 or
// not finite (the columns before it are written).  *ratio = min over the columns of |pivot| / max |x_i| over L(:,k)'s rows
// (pivot included) -- 1.0 when every kept pivot is a largest candidate.
namespace csx {
int lu_refactor_columns(int32_t n, const int32_t *cols, int32_t ncols, const int32_t *Ap, const int32_t *Ai,
                        const double *Ax, const int32_t *pinv, const int32_t *Lp, const int32_t *Li, double *Lx,
                        const int32_t *Up, const int32_t *Ui, double *Ux, double *x, int *ok, double *ratio) {
#pragma clang fp contract(off)
    *ok = 1;
    double rmin = 1.0;
    for (int32_t c = 0; c < ncols; c++) {
        const int32_t k = cols ? cols[c] : c;
        const int32_t ue = Up[k + 1] - 1;
        if (ue < Up[k] || Ui[ue] != k || Lp[k + 1] <= Lp[k] || Li[Lp[k]] != k) return CSX_EINVAL;
        for (int32_t t = Up[k]; t <= ue; t++) x[Ui[t]] = 0.0;
        for (int32_t t = Lp[k]; t < Lp[k + 1]; t++) x[Li[t]] = 0.0;
        for (int32_t t = Ap[k]; t < Ap[k + 1]; t++) x[pinv[Ai[t]]] = Ax[t];
        for (int32_t t = Up[k]; t < ue; t++) {
            const int32_t J = Ui[t];
            if (J >= k) return CSX_EINVAL;
            const double xj = x[J];
            Ux[t] = xj;
            for (int32_t s = Lp[J] + 1; s < Lp[J + 1]; s++) {
                const double prod = Lx[s] * xj;
                x[Li[s]] = x[Li[s]] - prod;
            }
        }
        const double piv = x[k];
        Ux[ue] = piv;
        double big = std::fabs(piv);
        for (int32_t s = Lp[k] + 1; s < Lp[k + 1]; s++) big = std::fmax(big, std::fabs(x[Li[s]]));
        const bool bad = piv == 0.0 || !std::isfinite(piv);
        if (!bad) rmin = std::fmin(rmin, std::fabs(piv) / big);
        Lx[Lp[k]] = 1.0;
        for (int32_t s = Lp[k] + 1; s < Lp[k + 1]; s++) Lx[s] = x[Li[s]] / piv;
        for (int32_t t = Up[k]; t <= ue; t++) x[Ui[t]] = 0.0;
        for (int32_t t = Lp[k]; t < Lp[k + 1]; t++) x[Li[t]] = 0.0;
        if (bad) {
            *ok = 0;
            break;
        }
    }
    *ratio = rmin;
    return CSX_OK;
}
}  // namespace csx

extern "C" int csx_lu_refactor_host(int32_t n, const int32_t *Ap, const int32_t *Ai, const double *Ax, const int32_t *pinv,
                                    const int32_t *Lp, const int32_t *Li, double *Lx, const int32_t *Up, const int32_t *Ui,
                                    double *Ux, int *ok, double *ratio) {
    if (n < 0 || !Ap || !Ai || !Ax || !pinv || !Lp || !Li || !Lx || !Up || !Ui || !Ux || !ok || !ratio) return CSX_EINVAL;
    // every index inside [0, n), the patterns' pointers from 0 and non-decreasing, A(:,k)'s rows in L(:,k) or U(:,k)
    std::vector<int32_t> mark((size_t)n, -1);
    if (Ap[0] != 0 || Lp[0] != 0 || Up[0] != 0) return CSX_EINVAL;
    for (int32_t i = 0; i < n; i++)
        if (pinv[i] < 0 || pinv[i] >= n || mark[pinv[i]] >= 0) return CSX_EINVAL;
        else mark[pinv[i]] = n;
    for (int32_t k = 0; k < n; k++) {
        if (Ap[k + 1] < Ap[k] || Lp[k + 1] < Lp[k] || Up[k + 1] < Up[k]) return CSX_EINVAL;
        for (int32_t t = Lp[k]; t < Lp[k + 1]; t++)
            if (Li[t] < k || Li[t] >= n) return CSX_EINVAL;
            else mark[Li[t]] = k;
        for (int32_t t = Up[k]; t < Up[k + 1]; t++)
            if (Ui[t] < 0 || Ui[t] > k) return CSX_EINVAL;
            else mark[Ui[t]] = k;
        for (int32_t t = Ap[k]; t < Ap[k + 1]; t++)
            if (Ai[t] < 0 || Ai[t] >= n || mark[pinv[Ai[t]]] != k) return CSX_EINVAL;
    }
    std::vector<double> x((size_t)n, 0.0);
    return csx::lu_refactor_columns(n, nullptr, n, Ap, Ai, Ax, pinv, Lp, Li, Lx, Up, Ui, Ux, x.data(), ok, ratio);
}

// ---- assembly plan (include/csx.h has the definition) ------------------------------------------------
// The reference's two loops on the indices alone.  cs_compress: a stable counting sort of the triplets by column.  cs_dupl:
// down every column, a row seen before in this column (where[r] >= the column's first slot) lands in the slot of its first
// occurrence, any other row opens the next slot.  What the loops did to the values is kept as lists: slot s is the fold of
// the triplets src[sp[s] .. sp[s + 1]), ascending (the order the counting sort keeps and cs_dupl adds in).
extern "C" int csx_assemble_plan_host(int32_t m, int32_t n, int64_t nz, const int32_t *Ti, const int32_t *Tj, int32_t *Cp,
                                      int32_t *Ci, int32_t *sp, int32_t *src, int32_t *nnz_out) {
    if (m < 0 || n < 0 || nz < 0 || nz > INT32_MAX || !Cp || !sp || !nnz_out || (nz > 0 && (!Ti || !Tj || !Ci || !src)))
        return CSX_EINVAL;
    for (int64_t k = 0; k < nz; k++)
        if (Ti[k] < 0 || Ti[k] >= m || Tj[k] < 0 || Tj[k] >= n) return CSX_EINVAL;   // the reference would raise IndexError
    const int32_t cnt = (int32_t)nz;
    // the counting sort: src[q] = the triplet at position q of cs_compress's result (src is scratch until the last loop)
    std::vector<int32_t> next((size_t)n + 1, 0);
    for (int32_t k = 0; k < cnt; k++) next[(size_t)Tj[k] + 1]++;
    for (int32_t j = 0; j < n; j++) next[(size_t)j + 1] += next[j];
    std::vector<int32_t> colp(next);   // column pointers of the compressed form
    for (int32_t k = 0; k < cnt; k++) src[next[Tj[k]]++] = k;
    // the first-occurrence scan: slot[k] = where triplet k lands, sp[s + 1] = how many land in slot s
    std::vector<int32_t> where((size_t)m, -1), slot((size_t)cnt);
    int32_t nnz = 0;
    sp[0] = 0;
    for (int32_t j = 0; j < n; j++) {
        const int32_t start = nnz;
        for (int32_t q = colp[j]; q < colp[(size_t)j + 1]; q++) {
            const int32_t k = src[q], r = Ti[k];
            if (where[r] >= start) {
                sp[(size_t)where[r] + 1]++;
                slot[k] = where[r];
            } else {
                where[r] = nnz;
                Ci[nnz] = r;
                sp[(size_t)nnz + 1] = 1;
                slot[k] = nnz++;
            }
        }
        Cp[j] = start;
    }
    Cp[n] = nnz;
    for (int32_t s = 0; s < nnz; s++) sp[(size_t)s + 1] += sp[s];
    // grouped by slot, ascending inside a slot: the triplets in their own order, each to the next free place of its slot
    std::vector<int32_t> fill(sp, sp + nnz);
    for (int32_t k = 0; k < cnt; k++) src[fill[slot[k]]++] = k;
    *nnz_out = nnz;
    return CSX_OK;
}

// Cx[s] = ((Tx[t0] + Tx[t1]) + Tx[t2]) + ... over src[sp[s] .. sp[s + 1]): the first term assigned, one addition per further
// term (no multiply: nothing to contract)
extern "C" int csx_assemble_host(int32_t nnz, const int32_t *sp, const int32_t *src, const double *Tx, double *Cx) {
    if (nnz < 0 || !sp || (nnz > 0 && (!src || !Tx || !Cx))) return CSX_EINVAL;
    for (int32_t s = 0; s < nnz; s++) {
        if (sp[s + 1] <= sp[s]) return CSX_EINVAL;
        double acc = Tx[src[sp[s]]];
        for (int32_t t = sp[s] + 1; t < sp[s + 1]; t++) acc = acc + Tx[src[t]];
        Cx[s] = acc;
    }
    return CSX_OK;
}

// ---- multiply plan (include/csx.h has the definition) -------------------------------------------------
// cs_multiply's two nested loops on the indices alone.  Column j of C: down B(:,j) in storage order, down A(:, B.i[ib]) in
// storage order; a row met for the first time in this column (where[r] < the column's first slot) opens the next slot, any
// other product lands in the slot of its row.  What the loops did to the values is kept as lists: slot s is the fold of the
// products pair[2t], pair[2t + 1] = (ia, ib), t in sp[s] .. sp[s + 1], in the order the loops met them.
namespace {
// pointers from 0 and non-decreasing, every index inside [0, rows)
bool pattern_ok(int32_t rows, int32_t cols, const int32_t *p, const int32_t *i) {
    if (!p || p[0] != 0) return false;
    for (int32_t j = 0; j < cols; j++)
        if (p[j + 1] < p[j]) return false;
    if (p[cols] > 0 && !i) return false;
    for (int32_t t = 0; t < p[cols]; t++)
        if (i[t] < 0 || i[t] >= rows) return false;
    return true;
}

// The walk itself.  Cp / Ci / sp / pair may all be null (csx_multiply_plan_count).  A column's slots are consecutive and so
// are their products, so each column is counted, then placed, with no array of the products' size beside pair.
int multiply_plan_walk(int32_t m, int32_t n, const int32_t *Ap, const int32_t *Ai, const int32_t *Bp, const int32_t *Bi,
                       int32_t *Cp, int32_t *Ci, int32_t *sp, int32_t *pair, int64_t *nnz_out, int64_t *products_out) {
    std::vector<int64_t> where((size_t)m, -1);
    std::vector<int32_t> rows;   // of the column in hand: its slots' rows ...
    std::vector<int64_t> fill;   // ... and their product counts, then the next free place of each slot
    int64_t nnz = 0, products = 0;
    for (int32_t j = 0; j < n; j++) {
        const int64_t start = nnz;
        rows.clear();
        fill.clear();
        for (int32_t ib = Bp[j]; ib < Bp[j + 1]; ib++) {
            const int32_t c = Bi[ib];
            for (int32_t ia = Ap[c]; ia < Ap[c + 1]; ia++) {
                const int32_t r = Ai[ia];
                if (where[r] < start) {
                    where[r] = nnz++;
                    rows.push_back(r);
                    fill.push_back(1);
                } else {
                    fill[(size_t)(where[r] - start)]++;
                }
            }
        }
        if (Cp) {
            if (nnz > INT32_MAX || (!rows.empty() && (!Ci || !pair))) return CSX_EINVAL;   // (Ci, pair may be null while empty)
            Cp[j] = (int32_t)start;
            for (size_t q = 0; q < rows.size(); q++) {
                const int64_t len = fill[q];
                Ci[start + (int64_t)q] = rows[q];
                if (products + len > INT32_MAX) {
                    csx::set_error("multiply plan: more than 2^31 - 1 products do not fit its int32 pointers");
                    return CSX_EINVAL;
                }
                sp[start + (int64_t)q] = (int32_t)products;
                fill[q] = products;
                products += len;
            }
            for (int32_t ib = Bp[j]; ib < Bp[j + 1]; ib++) {
                const int32_t c = Bi[ib];
                for (int32_t ia = Ap[c]; ia < Ap[c + 1]; ia++) {
                    const int64_t t = fill[(size_t)(where[Ai[ia]] - start)]++;
                    pair[2 * t] = ia;
                    pair[2 * t + 1] = ib;
                }
            }
        } else {
            for (int64_t len : fill) products += len;
        }
    }
    if (Cp) {
        Cp[n] = (int32_t)nnz;
        sp[nnz] = (int32_t)products;
    }
    *nnz_out = nnz;
    *products_out = products;
    return CSX_OK;
}
}  // namespace

extern "C" int csx_multiply_plan_count(int32_t m, int32_t k, int32_t n, const int32_t *Ap, const int32_t *Ai, const int32_t *Bp,
                                       const int32_t *Bi, int64_t *nnz, int64_t *products) {
    if (m < 0 || k < 0 || n < 0 || !nnz || !products) return CSX_EINVAL;
    if (!pattern_ok(m, k, Ap, Ai) || !pattern_ok(k, n, Bp, Bi)) return CSX_EINVAL;   // the reference would raise IndexError
    return multiply_plan_walk(m, n, Ap, Ai, Bp, Bi, nullptr, nullptr, nullptr, nullptr, nnz, products);
}

extern "C" int csx_multiply_plan_host(int32_t m, int32_t k, int32_t n, const int32_t *Ap, const int32_t *Ai, const int32_t *Bp,
                                      const int32_t *Bi, int32_t *Cp, int32_t *Ci, int32_t *sp, int32_t *pair) {
    if (m < 0 || k < 0 || n < 0 || !Cp || !sp) return CSX_EINVAL;
    if (!pattern_ok(m, k, Ap, Ai) || !pattern_ok(k, n, Bp, Bi)) return CSX_EINVAL;
    int64_t nnz = 0, products = 0;
    return multiply_plan_walk(m, n, Ap, Ai, Bp, Bi, Cp, Ci, sp, pair, &nnz, &products);
}

// Cx[s] = ((b0 a0) + b1 a1) + ... over the slot's products: every product rounded on its own, the first assigned, one
// addition per further product -- never a fused multiply-add
extern "C" int csx_multiply_fold_host(int32_t nnz, const int32_t *sp, const int32_t *pair, const double *Ax, const double *Bx,
                                      double *Cx) {
#pragma clang fp contract(off)
    if (nnz < 0 || !sp || (nnz > 0 && (!pair || !Ax || !Bx || !Cx))) return CSX_EINVAL;
    for (int32_t s = 0; s < nnz; s++) {
        if (sp[s + 1] <= sp[s]) return CSX_EINVAL;
        int64_t t = sp[s];
        double acc = Bx[pair[2 * t + 1]] * Ax[pair[2 * t]];
        for (t++; t < sp[s + 1]; t++) {
            const double term = Bx[pair[2 * t + 1]] * Ax[pair[2 * t]];
            acc = acc + term;
        }
        Cx[s] = acc;
    }
    return CSX_OK;
}

// ---- add plan (include/csx.h has the definition) ------------------------------------------------------
// cs_add's loop on the indices alone, for k operands: column j of C is cs_scatter of A_0(:,j), then A_1(:,j), ... in stored
// order; a row met for the first time in this column (where[r] < the column's first slot) opens the next slot, any other entry
// lands in the slot of its row.  What the loops did to the values is kept as lists: slot s is the fold of the entries
// src[sp[s] .. sp[s + 1]) -- positions in the concatenation of the operands' value arrays -- in the order the loops met them.
// A column's slots are consecutive and so are their terms, so each column is counted, then placed.
extern "C" int csx_add_plan_host(int32_t m, int32_t n, int32_t k, const int32_t *const *Ap, const int32_t *const *Ai, int32_t *Cp,
                                 int32_t *Ci, int32_t *sp, int32_t *src, int32_t *nnz_out) {
    if (m < 0 || n < 0 || k < 2 || k > 8 || !Ap || !Ai || !Cp || !sp || !nnz_out) return CSX_EINVAL;
    int64_t off[9] = {0};
    for (int32_t r = 0; r < k; r++) {
        if (!pattern_ok(m, n, Ap[r], Ai[r])) return CSX_EINVAL;   // the reference would raise IndexError
        off[r + 1] = off[r] + Ap[r][n];
    }
    if (off[k] > INT32_MAX) {
        csx::set_error("add plan: %lld terms do not fit its int32 pointers", (long long)off[k]);
        return CSX_EINVAL;
    }
    if (off[k] > 0 && (!Ci || !src)) return CSX_EINVAL;
    std::vector<int32_t> where((size_t)m, -1);
    std::vector<int32_t> fill;   // of the column in hand: its slots' term counts, then the next free place of each slot
    int32_t nnz = 0, terms = 0;
    for (int32_t j = 0; j < n; j++) {
        const int32_t start = nnz;
        fill.clear();
        for (int32_t r = 0; r < k; r++)
            for (int32_t e = Ap[r][j]; e < Ap[r][j + 1]; e++) {
                const int32_t row = Ai[r][e];
                if (where[row] < start) {
                    where[row] = nnz;
                    Ci[nnz++] = row;
                    fill.push_back(1);
                } else {
                    fill[(size_t)(where[row] - start)]++;
                }
            }
        Cp[j] = start;
        for (size_t q = 0; q < fill.size(); q++) {
            const int32_t len = fill[q];
            sp[(size_t)start + q] = terms;
            fill[q] = terms;
            terms += len;
        }
        for (int32_t r = 0; r < k; r++)
            for (int32_t e = Ap[r][j]; e < Ap[r][j + 1]; e++) src[fill[(size_t)(where[Ai[r][e]] - start)]++] = (int32_t)off[r] + e;
    }
    Cp[n] = nnz;
    sp[nnz] = terms;
    *nnz_out = nnz;
    return CSX_OK;
}

// Cx[s] = ((c x) + c' x') + ... over the slot's terms: term t is coef[r] * X[r][src[t] - off[r]] for the operand r that holds
// position src[t] (off[r] <= src[t] < off[r + 1]), rounded on its own, the first assigned, one addition per further term --
// never a fused multiply-add
extern "C" int csx_add_fold_host(int32_t nnz, int32_t k, const int32_t *sp, const int32_t *src, const int32_t *off,
                                 const double *coef, const double *const *X, double *Cx) {
#pragma clang fp contract(off)
    if (nnz < 0 || k < 2 || k > 8 || !sp || !off || !coef || !X || (nnz > 0 && (!src || !Cx))) return CSX_EINVAL;
    for (int32_t r = 0; r < k; r++)
        if (off[r + 1] < off[r] || (off[r + 1] > off[r] && !X[r])) return CSX_EINVAL;
    for (int32_t s = 0; s < nnz; s++) {
        if (sp[s + 1] <= sp[s]) return CSX_EINVAL;
        double acc = 0.0;
        for (int32_t t = sp[s]; t < sp[s + 1]; t++) {
            const int32_t g = src[t];
            if (g < off[0] || g >= off[k]) return CSX_EINVAL;
            int32_t r = 0;
            while (g >= off[r + 1]) r++;
            const double term = coef[r] * X[r][g - off[r]];
            acc = t == sp[s] ? term : acc + term;
        }
        Cx[s] = acc;
    }
    return CSX_OK;
}

// csx_residual_block's value rule on host arrays (csx_residual.hip): R = B - op(A) X for row-major blocks of nrhs
// columns, omega[c] = max_i |r| / (|op(A)| |X| + |B|), rnorm[c] = max_i |r|.  Row i's terms in ascending (column, storage
// position) order for op(A) = A -- a sweep over the columns in storage order gives every row exactly that order -- and in the
// storage order of column i of A for op(A) = A'.  Product rounded, then the subtraction: never a fused multiply-add.  The maxima
// over the bit patterns of the non-negative doubles (NaN above inf, any order).  R may be B (or NULL).
extern "C" int csx_residual_host(int32_t m, int32_t n, const int32_t *p, const int32_t *i, const double *x, int32_t nrhs, int trans,
                                 const double *X, const double *B, double *R, double *omega, double *rnorm) {
#pragma clang fp contract(off)
    if (m < 0 || n < 0 || nrhs < 1 || !p || p[0] != 0) return CSX_EINVAL;
    const int32_t nnz = p[n];
    if (nnz < 0 || (nnz > 0 && (!i || !x))) return CSX_EINVAL;
    const int32_t rows = trans ? n : m, cols = trans ? m : n;
    if ((rows > 0 && !B) || (rows > 0 && cols > 0 && nnz > 0 && !X)) return CSX_EINVAL;
    for (int32_t j = 0; j < n; j++)
        if (p[j + 1] < p[j]) return CSX_EINVAL;
    for (int32_t q = 0; q < nnz; q++)
        if (i[q] < 0 || i[q] >= m) return CSX_EINVAL;
    const size_t k = (size_t)nrhs;
    std::vector<double> r((size_t)rows * k), d((size_t)rows * k);
    for (size_t t = 0; t < r.size(); t++) {
        r[t] = B[t];
        d[t] = std::fabs(B[t]);
    }
    for (int32_t j = 0; j < n; j++)
        for (int32_t q = p[j]; q < p[j + 1]; q++) {
            const double a = x[q], aa = std::fabs(a);
            const size_t out = (size_t)(trans ? j : i[q]) * k, in = (size_t)(trans ? i[q] : j) * k;
            for (size_t c = 0; c < k; c++) {
                const double t = a * X[in + c];
                r[out + c] = r[out + c] - t;
                const double u = aa * std::fabs(X[in + c]);
                d[out + c] = d[out + c] + u;
            }
        }
    std::vector<uint64_t> wmax(k, 0), amax(k, 0);
    for (size_t t = 0; t < r.size(); t++) {
        const double ar = std::fabs(r[t]);
        const double ratio = (ar == 0.0 && d[t] == 0.0) ? 0.0 : ar / d[t];
        const double av = std::fabs(ratio);
        uint64_t wb, ab;
        std::memcpy(&wb, &av, 8);
        std::memcpy(&ab, &ar, 8);
        wmax[t % k] = std::max(wmax[t % k], wb);
        amax[t % k] = std::max(amax[t % k], ab);
    }
    if (omega) std::memcpy(omega, wmax.data(), k * 8);
    if (rnorm) std::memcpy(rnorm, amax.data(), k * 8);
    if (R) std::memcpy(R, r.data(), r.size() * 8);
    return CSX_OK;
}

// csx_residual_sym_block's value rule on host arrays (csx_residual_sym.hip): R = B - S X with S the stored
// entries of A with row <= column, mirrored.  Row i's terms: first the entries of stored column i with A.i[q] <= i, in storage
// order; then the entries of row i with column > i in ascending (column, storage position) order.  One sweep over the columns
// in storage order gives every row exactly that: column j's kept entries go to row j first (rows below j have not been swept
// to yet, rows above took theirs before), then its strictly upper entries go to their own rows, which have had their phase 1
// and the columns before j.  Strictly lower entries are skipped, never added as zeros.  Otherwise as csx_residual_host.
extern "C" int csx_residual_sym_host(int32_t n, const int32_t *p, const int32_t *i, const double *x, int32_t nrhs, const double *X,
                                     const double *B, double *R, double *omega, double *rnorm) {
#pragma clang fp contract(off)
    if (n < 0 || nrhs < 1 || !p || p[0] != 0) return CSX_EINVAL;
    const int32_t nnz = p[n];
    if (nnz < 0 || (nnz > 0 && (!i || !x))) return CSX_EINVAL;
    if ((n > 0 && !B) || (n > 0 && nnz > 0 && !X)) return CSX_EINVAL;
    for (int32_t j = 0; j < n; j++)
        if (p[j + 1] < p[j]) return CSX_EINVAL;
    for (int32_t q = 0; q < nnz; q++)
        if (i[q] < 0 || i[q] >= n) return CSX_EINVAL;
    const size_t k = (size_t)nrhs;
    std::vector<double> r((size_t)n * k), d((size_t)n * k);
    for (size_t t = 0; t < r.size(); t++) {
        r[t] = B[t];
        d[t] = std::fabs(B[t]);
    }
    for (int32_t j = 0; j < n; j++)
        for (int phase = 0; phase < 2; phase++)
            for (int32_t q = p[j]; q < p[j + 1]; q++) {
                if (phase == 0 ? i[q] > j : i[q] >= j) continue;
                const double a = x[q], aa = std::fabs(a);
                const size_t out = (size_t)(phase == 0 ? j : i[q]) * k, in = (size_t)(phase == 0 ? i[q] : j) * k;
                for (size_t c = 0; c < k; c++) {
                    const double t = a * X[in + c];
                    r[out + c] = r[out + c] - t;
                    const double u = aa * std::fabs(X[in + c]);
                    d[out + c] = d[out + c] + u;
                }
            }
    std::vector<uint64_t> wmax(k, 0), amax(k, 0);
    for (size_t t = 0; t < r.size(); t++) {
        const double ar = std::fabs(r[t]);
        const double ratio = (ar == 0.0 && d[t] == 0.0) ? 0.0 : ar / d[t];
        const double av = std::fabs(ratio);
        uint64_t wb, ab;
        std::memcpy(&wb, &av, 8);
        std::memcpy(&ab, &ar, 8);
        wmax[t % k] = std::max(wmax[t % k], wb);
        amax[t % k] = std::max(amax[t % k], ab);
    }
    if (omega) std::memcpy(omega, wmax.data(), k * 8);
    if (rnorm) std::memcpy(rnorm, amax.data(), k * 8);
    if (R) std::memcpy(R, r.data(), r.size() * 8);
    return CSX_OK;
}

// csx_ldl_factor's value rule on host arrays (csx_ldl.hip): L D L' = C, C = upper(P A P') as cs_chol reads it
// (stored entries with row <= column, of duplicates the last, lower entries ignored), on the given pattern of L (rows
// ascending, the diagonal first), 1x1 pivots in the given order.  Columns ascending (descendants in the elimination tree come
// first); column j takes the updates of the columns k < j with L(j,k) in the pattern in ascending k -- the row view, built here
// by one sweep over the columns -- each from the slot of L(j,k) to the end of column k: w = L(j,k) d[k] rounded, then every
// product rounded and every subtraction rounded.  info[4] = positive pivots, negative pivots, perturbed pivots, the smallest
// column whose pivot is 0 or not finite (-1: none; L.x and d are then not a factorisation).
// The first ncols columns of that rule on the work array Lx (Lp[n] doubles: C scattered into every slot of the pattern, then
// the columns j < ncols factored; the columns beyond hold C still).  rp / rpos: the row view, for csx_schur_host.
static int ldl_host_columns(int32_t n, const int32_t *Ap, const int32_t *Ai, const double *Ax, const int32_t *pinv, const int32_t *Lp,
                            const int32_t *Li, int32_t ncols, double tau, double *Lx, double *d, int64_t *info,
                            std::vector<int32_t> &rp, std::vector<int32_t> &rpos) {
#pragma clang fp contract(off)
    if (n < 0 || !Ap || !Lp || !info || Ap[0] != 0 || Lp[0] != 0 || !(tau >= 0.0)) return CSX_EINVAL;
    const int32_t anz = Ap[n], lnz = Lp[n];
    if (anz < 0 || lnz < n || (anz > 0 && (!Ai || !Ax)) || (n > 0 && (!Li || !Lx || (ncols > 0 && !d)))) return CSX_EINVAL;
    for (int32_t j = 0; j < n; j++) {
        if (Ap[j + 1] < Ap[j] || Lp[j + 1] <= Lp[j] || Li[Lp[j]] != j) return CSX_EINVAL;
        for (int32_t q = Lp[j] + 1; q < Lp[j + 1]; q++)
            if (Li[q] <= Li[q - 1] || Li[q] >= n) return CSX_EINVAL;
        if (pinv && (pinv[j] < 0 || pinv[j] >= n)) return CSX_EINVAL;
    }
    // the entry map (k_chol_winner's): slot of L <- the last stored entry of A that lands there
    std::vector<int32_t> win((size_t)lnz, -1);
    for (int32_t j = 0; j < n; j++) {
        const int32_t j2 = pinv ? pinv[j] : j;
        for (int32_t q = Ap[j]; q < Ap[j + 1]; q++) {
            const int32_t r0 = Ai[q];
            if (r0 < 0 || r0 >= n) return CSX_EINVAL;
            if (r0 > j) continue;
            const int32_t i2 = pinv ? pinv[r0] : r0;
            const int32_t c = std::min(i2, j2), r = std::max(i2, j2);
            const int32_t *b = Li + Lp[c], *e = Li + Lp[c + 1];
            const int32_t *at = std::lower_bound(b, e, r);
            if (at == e || *at != r) return CSX_EINVAL;   // the pattern does not contain this entry
            win[(size_t)(at - Li)] = q;
        }
    }
    for (int32_t q = 0; q < lnz; q++) Lx[q] = win[(size_t)q] >= 0 ? Ax[win[(size_t)q]] : 0.0;
    // the row view: for row j the slots of L(j,k), k ascending
    rp.assign((size_t)n + 1, 0);
    rpos.resize((size_t)lnz);
    for (int32_t q = 0; q < lnz; q++) rp[(size_t)Li[q] + 1]++;
    for (int32_t j = 0; j < n; j++) rp[(size_t)j + 1] += rp[(size_t)j];
    {
        std::vector<int32_t> next(rp.begin(), rp.end() - 1);
        for (int32_t k = 0; k < n; k++)
            for (int32_t q = Lp[k]; q < Lp[k + 1]; q++) rpos[(size_t)next[(size_t)Li[q]]++] = q;
    }
    std::vector<int32_t> slot((size_t)n, -1);
    int64_t pos = 0, neg = 0, perturbed = 0, broke = -1;
    for (int32_t j = 0; j < ncols; j++) {
        const int32_t base = Lp[j], end = Lp[j + 1];
        for (int32_t q = base; q < end; q++) slot[(size_t)Li[q]] = q;
        for (int32_t t = rp[(size_t)j]; t < rp[(size_t)j + 1] - 1; t++) {   // (the row ends with the diagonal)
            const int32_t at = rpos[(size_t)t];
            const int32_t k = (int32_t)(std::upper_bound(Lp, Lp + n + 1, at) - Lp) - 1;
            const double w = Lx[at] * d[k];
            for (int32_t q = at; q < Lp[k + 1]; q++) {
                const int32_t s = slot[(size_t)Li[q]];
                if (s < base) return CSX_EINVAL;          // not the pattern of a Cholesky factor
                const double v = Lx[q] * w;
                Lx[s] = Lx[s] - v;
            }
        }
        double dj = Lx[base];
        if (tau > 0.0 && std::fabs(dj) < tau) {
            dj = std::copysign(tau, dj);
            perturbed++;
        }
        if ((dj == 0.0 || !std::isfinite(dj)) && broke < 0) broke = j;
        pos += dj > 0.0;
        neg += dj < 0.0;
        d[j] = dj;
        Lx[base] = 1.0;
        for (int32_t q = base + 1; q < end; q++) Lx[q] = Lx[q] / dj;
    }
    info[0] = pos;
    info[1] = neg;
    info[2] = perturbed;
    info[3] = broke;
    return CSX_OK;
}

extern "C" int csx_ldl_host(int32_t n, const int32_t *Ap, const int32_t *Ai, const double *Ax, const int32_t *pinv, const int32_t *Lp,
                            const int32_t *Li, double tau, double *Lx, double *d, int64_t *info) {
    std::vector<int32_t> rp, rpos;
    return ldl_host_columns(n, Ap, Ai, Ax, pinv, Lp, Li, n, tau, Lx, d, info, rp, rpos);
}

// csx_schur_factor's value rule on host arrays (csx_schur.hip; the definition is the comment of csx_schur_factor in
// include/csx.h): the columns j < n1 by the rule above on the FULL pattern Lfp / Lfi, then every column j >= n1 takes the
// updates of the row view of row j with k < n1 in ascending k into sums indexed by the row itself -- no pivot, no division --
// and lands in both triangles of S.  Lpx: the values of Lp (the first Lfp[n1] of the factored work array, then ns times 1.0).
extern "C" int csx_schur_host(int32_t n, const int32_t *Ap, const int32_t *Ai, const double *Ax, const int32_t *pinv, const int32_t *Lfp,
                              const int32_t *Lfi, int32_t n1, double tau, double *Lpx, double *d, double *S, int64_t *info) {
#pragma clang fp contract(off)
    if (n < 0 || n1 < 0 || n1 > n || !Lfp || Lfp[0] != 0 || Lfp[n] < n) return CSX_EINVAL;
    const int64_t ns = (int64_t)n - n1;
    if (ns * ns >= ((int64_t)1 << 31) || (ns > 0 && (!S || !Lpx)) || (n1 > 0 && !Lpx)) return CSX_EINVAL;
    std::vector<double> W((size_t)std::max(Lfp[n], 1));
    std::vector<int32_t> rp, rpos;
    const int st = ldl_host_columns(n, Ap, Ai, Ax, pinv, Lfp, Lfi, n1, tau, W.data(), d, info, rp, rpos);
    if (st != CSX_OK) return st;
    const int32_t head = Lfp[n1];
    for (int32_t q = 0; q < head; q++) Lpx[q] = W[(size_t)q];
    for (int64_t t = 0; t < ns; t++) Lpx[head + t] = 1.0;
    std::vector<double> acc((size_t)n);
    for (int32_t j = n1; j < n; j++) {
        for (int32_t r = j; r < n; r++) acc[(size_t)r] = 0.0;
        for (int32_t q = Lfp[j]; q < Lfp[j + 1]; q++) acc[(size_t)Lfi[q]] = W[(size_t)q];
        for (int32_t t = rp[(size_t)j]; t < rp[(size_t)j + 1] - 1; t++) {
            const int32_t at = rpos[(size_t)t];
            const int32_t k = (int32_t)(std::upper_bound(Lfp, Lfp + n + 1, at) - Lfp) - 1;
            if (k >= n1) break;                           // (k ascending: the trailing columns take no update from each other)
            const double w = W[(size_t)at] * d[k];
            for (int32_t q = at; q < Lfp[k + 1]; q++) {
                const double v = W[(size_t)q] * w;
                acc[(size_t)Lfi[q]] = acc[(size_t)Lfi[q]] - v;
            }
        }
        for (int32_t r = j; r < n; r++) {
            S[(int64_t)(r - n1) * ns + (j - n1)] = acc[(size_t)r];
            S[(int64_t)(j - n1) * ns + (r - n1)] = acc[(size_t)r];
        }
    }
    return CSX_OK;
}

// csx_slu_factor's value rule on host arrays (csx_slu.hip): L U = C = P A(prow, :) P' on the given pattern (rows
// ascending, the diagonal first), no pivot search.  Entry (i, j) of A is C(i2, j2), i2 = pinv[prinv[i]], j2 = pinv[j]; of
// duplicates the last counts.  Lx: unit lower L; Utx: column k = row k of U, the pivot first.  Columns ascending; column j takes
// the updates of the columns k < j with (j,k) in the pattern in ascending k (the row view), each from the slot of row j to the
// end of column k: every product rounded, then every subtraction rounded.  info[4] = positive pivots, negative pivots, perturbed
// pivots, the smallest column whose pivot is 0 or not finite (-1: none).
extern "C" int csx_slu_host(int32_t n, const int32_t *Ap, const int32_t *Ai, const double *Ax, const int32_t *prow, const int32_t *pinv,
                            const int32_t *Lp, const int32_t *Li, double tau, double *Lx, double *Utx, int64_t *info) {
#pragma clang fp contract(off)
    if (n < 0 || !Ap || !Lp || !info || Ap[0] != 0 || Lp[0] != 0 || !(tau >= 0.0)) return CSX_EINVAL;
    const int32_t anz = Ap[n], lnz = Lp[n];
    if (anz < 0 || lnz < n || (anz > 0 && (!Ai || !Ax)) || (n > 0 && (!Li || !Lx || !Utx))) return CSX_EINVAL;
    std::vector<int32_t> prinv((size_t)n, -1), seen((size_t)n, 0);
    for (int32_t j = 0; j < n; j++) {
        if (Ap[j + 1] < Ap[j] || Lp[j + 1] <= Lp[j] || Li[Lp[j]] != j) return CSX_EINVAL;
        for (int32_t q = Lp[j] + 1; q < Lp[j + 1]; q++)
            if (Li[q] <= Li[q - 1] || Li[q] >= n) return CSX_EINVAL;
        if (pinv && (pinv[j] < 0 || pinv[j] >= n || seen[(size_t)pinv[j]]++)) return CSX_EINVAL;
        const int32_t r = prow ? prow[j] : j;
        if (r < 0 || r >= n || prinv[(size_t)r] >= 0) return CSX_EINVAL;
        prinv[(size_t)r] = j;
    }
    // the two entry maps (k_slu_entry_map's): slot <- the last stored entry of A that lands there
    std::vector<int32_t> winL((size_t)lnz, -1), winU((size_t)lnz, -1);
    for (int32_t j = 0; j < n; j++) {
        const int32_t j2 = pinv ? pinv[j] : j;
        for (int32_t q = Ap[j]; q < Ap[j + 1]; q++) {
            if (Ai[q] < 0 || Ai[q] >= n) return CSX_EINVAL;
            const int32_t i1 = prinv[(size_t)Ai[q]];
            const int32_t i2 = pinv ? pinv[i1] : i1;
            const int32_t c = std::min(i2, j2), r = std::max(i2, j2);
            const int32_t *b = Li + Lp[c], *e = Li + Lp[c + 1];
            const int32_t *at = std::lower_bound(b, e, r);
            if (at == e || *at != r) return CSX_EINVAL;   // the pattern does not contain this entry
            if (i2 >= j2) winL[(size_t)(at - Li)] = q;
            if (i2 <= j2) winU[(size_t)(at - Li)] = q;
        }
    }
    for (int32_t q = 0; q < lnz; q++) {
        Lx[q] = winL[(size_t)q] >= 0 ? Ax[winL[(size_t)q]] : 0.0;
        Utx[q] = winU[(size_t)q] >= 0 ? Ax[winU[(size_t)q]] : 0.0;
    }
    // the row view: for row j the slots of (j,k), k ascending
    std::vector<int32_t> rp((size_t)n + 1, 0), rpos((size_t)lnz);
    for (int32_t q = 0; q < lnz; q++) rp[(size_t)Li[q] + 1]++;
    for (int32_t j = 0; j < n; j++) rp[(size_t)j + 1] += rp[(size_t)j];
    {
        std::vector<int32_t> next(rp.begin(), rp.end() - 1);
        for (int32_t k = 0; k < n; k++)
            for (int32_t q = Lp[k]; q < Lp[k + 1]; q++) rpos[(size_t)next[(size_t)Li[q]]++] = q;
    }
    std::vector<int32_t> slot((size_t)n, -1);
    int64_t pos = 0, neg = 0, perturbed = 0, broke = -1;
    for (int32_t j = 0; j < n; j++) {
        const int32_t base = Lp[j], end = Lp[j + 1];
        for (int32_t q = base; q < end; q++) slot[(size_t)Li[q]] = q;
        for (int32_t t = rp[(size_t)j]; t < rp[(size_t)j + 1] - 1; t++) {   // (the row ends with the diagonal)
            const int32_t at = rpos[(size_t)t];
            const int32_t k = (int32_t)(std::upper_bound(Lp, Lp + n + 1, at) - Lp) - 1;
            const double l = Lx[at], u = Utx[at];
            for (int32_t q = at; q < Lp[k + 1]; q++) {
                const int32_t s = slot[(size_t)Li[q]];
                if (s < base) return CSX_EINVAL;          // not the pattern of a Cholesky factor
                const double a = Lx[q] * u, b = Utx[q] * l;
                Lx[s] = Lx[s] - a;
                Utx[s] = Utx[s] - b;
            }
        }
        double dj = Utx[base];
        if (tau > 0.0 && std::fabs(dj) < tau) {
            dj = std::copysign(tau, dj);
            perturbed++;
        }
        if ((dj == 0.0 || !std::isfinite(dj)) && broke < 0) broke = j;
        pos += dj > 0.0;
        neg += dj < 0.0;
        Utx[base] = dj;
        Lx[base] = 1.0;
        for (int32_t q = base + 1; q < end; q++) Lx[q] = Lx[q] / dj;
    }
    info[0] = pos;
    info[1] = neg;
    info[2] = perturbed;
    info[3] = broke;
    return CSX_OK;
}

// ---- Householder QR on a pattern known before the values (csx_hqr.hip) ----------------------------------------
// The loop of csx_qr_host with the values left out: V.p, V.i (the diagonal first, then the rows in the order that loop finds
// them) and R.p, R.i (the order the reflections are applied in, the diagonal last) -- csx_qr_host's own on the same analysis.
// Unlike that loop it trusts nothing: CSX_EINVAL for an analysis that is not this matrix's (an index out of range, a walk that
// leaves the tree below k, a row without a slot, a column whose rows never reached its parent), so that what passes has the
// two properties the device schedule stands on: every c in R(:,k) is a descendant of k, and every row of V(:,c) is a slot of
// R(:,k) or V(:,k).
namespace csx {
int hqr_symbolic(int32_t m, int32_t n, int32_t m2, const int32_t *Ap, const int32_t *Ai, const int32_t *q, const int32_t *parent,
                 const int32_t *pinv, const int32_t *leftmost, std::vector<int32_t> &Vp, std::vector<int32_t> &Vi,
                 std::vector<int32_t> &Rp, std::vector<int32_t> &Ri) {
    if (m < 0 || n < 0 || m < n || m2 < m || !Ap || Ap[0] != 0 || (n > 0 && !parent) || (m > 0 && (!pinv || !leftmost)))
        return CSX_EINVAL;
    for (int32_t k = 0; k < n; k++)
        if (Ap[k + 1] < Ap[k] || (parent[k] != -1 && (parent[k] <= k || parent[k] >= n))) return CSX_EINVAL;
    if (Ap[n] > 0 && !Ai) return CSX_EINVAL;
    {
        std::vector<char> seen((size_t)m2, 0), seenq((size_t)n, 0);
        for (int32_t i = 0; i < m; i++)
            if (pinv[i] < 0 || pinv[i] >= m2 || seen[(size_t)pinv[i]]++) return CSX_EINVAL;
        for (int32_t k = 0; q && k < n; k++)
            if (q[k] < 0 || q[k] >= n || seenq[(size_t)q[k]]++) return CSX_EINVAL;
    }
    std::vector<int32_t> stamp((size_t)m2, -1);      // stamp[r] == k: row / column r already collected for column k
    std::vector<int32_t> order((size_t)n > 0 ? (size_t)n : 1), path((size_t)n > 0 ? (size_t)n : 1);
    std::vector<char> passed((size_t)n, 0);          // V(:,c)'s rows have reached V(:,parent[c])
    constexpr size_t LIMIT = 0x7ffffff0;
    Vp.assign((size_t)n + 1, 0);
    Rp.assign((size_t)n + 1, 0);
    Vi.clear();
    Ri.clear();
    for (int32_t k = 0; k < n; k++) {
        if (Vi.size() > LIMIT || Ri.size() > LIMIT) return CSX_EINVAL;
        Rp[(size_t)k] = (int32_t)Ri.size();
        Vp[(size_t)k] = (int32_t)Vi.size();
        stamp[(size_t)k] = k;                        // the diagonal position leads V(:,k)
        Vi.push_back(k);
        int32_t front = n;                           // order[front..n) = reflections to apply, children before parents
        const int32_t col = q ? q[k] : k;
        for (int32_t p = Ap[col]; p < Ap[col + 1]; p++) {
            if (Ai[p] < 0 || Ai[p] >= m) return CSX_EINVAL;
            int32_t len = 0;
            for (int32_t c = leftmost[Ai[p]];; c = parent[c]) {
                if (c < 0 || c > k) return CSX_EINVAL;      // the walk must end in k
                if (stamp[(size_t)c] == k) break;
                path[(size_t)len++] = c;
                stamp[(size_t)c] = k;
            }
            while (len > 0) order[(size_t)--front] = path[(size_t)--len];
            const int32_t r = pinv[Ai[p]];
            if (r < k && stamp[(size_t)r] != k) return CSX_EINVAL;   // a row above the diagonal that is no entry of R(:,k)
            if (r > k && stamp[(size_t)r] < k) {     // a row below the diagonal not yet in V(:,k)'s pattern
                Vi.push_back(r);
                stamp[(size_t)r] = k;
            }
        }
        for (int32_t t = front; t < n; t++) {
            const int32_t c = order[(size_t)t];
            Ri.push_back(c);
            if (parent[c] == k) {                    // V(:,c)'s rows below c pass on to V(:,k)
                passed[(size_t)c] = 1;
                for (int32_t p = Vp[(size_t)c] + 1; p < Vp[(size_t)c + 1]; p++) {
                    const int32_t r = Vi[(size_t)p];
                    if (r < k) return CSX_EINVAL;
                    if (stamp[(size_t)r] < k) {
                        stamp[(size_t)r] = k;
                        Vi.push_back(r);
                    }
                }
            } else if (!passed[(size_t)c]) {
                return CSX_EINVAL;
            }
        }
        Ri.push_back(k);
    }
    Rp[(size_t)n] = (int32_t)Ri.size();
    Vp[(size_t)n] = (int32_t)Vi.size();
    return CSX_OK;
}
}  // namespace csx

extern "C" int csx_hqr_symbolic_host(int32_t m, int32_t n, int32_t m2, const int32_t *Ap, const int32_t *Ai, const int32_t *q,
                                     const int32_t *parent, const int32_t *pinv, const int32_t *leftmost, int32_t vcap,
                                     int32_t rcap, int32_t *Vp, int32_t *Vi, int32_t *Rp, int32_t *Ri) {
    if (!Vp || !Rp || (n > 0 && (!Vi || !Ri))) return CSX_EINVAL;
    std::vector<int32_t> vp, vi, rp, ri;
    CSX_TRY(csx::hqr_symbolic(m, n, m2, Ap, Ai, q, parent, pinv, leftmost, vp, vi, rp, ri));
    if ((int64_t)vi.size() > vcap || (int64_t)ri.size() > rcap) return CSX_EINVAL;
    std::memcpy(Vp, vp.data(), vp.size() * sizeof(int32_t));
    std::memcpy(Rp, rp.data(), rp.size() * sizeof(int32_t));
    if (!vi.empty()) std::memcpy(Vi, vi.data(), vi.size() * sizeof(int32_t));
    if (!ri.empty()) std::memcpy(Ri, ri.data(), ri.size() * sizeof(int32_t));
    return CSX_OK;
}

// cs_house on (head, tail2), statement for statement as csx_qr_host: *v0 the new head of the vector, *b beta, returns s
static inline double hqr_house(double head, double tail2, double *v0, double *b) {
#pragma clang fp contract(off)
    double s;
    if (tail2 == 0.0) {
        s = std::fabs(head);
        *b = head <= 0.0 ? 2.0 : 0.0;
        *v0 = 1.0;
    } else {
        s = std::sqrt(head * head + tail2);
        *v0 = head <= 0.0 ? head - s : -tail2 / (head + s);
        *b = -1.0 / (s * *v0);
    }
    return s;
}

// part[0] after the fixed tree over 64 partial sums (what a wave's butterfly leaves in every lane)
static inline double hqr_tree(double *part) {
#pragma clang fp contract(off)
    for (int s = 32; s >= 1; s >>= 1)
        for (int l = 0; l < s; l++) part[l] = part[l] + part[l + s];
    return part[0];
}

// csx_hqr_factor's value rule on host arrays (csx_hqr.hip; the statement is the comment of csx_hqr_factor in
// include/csx.h): csx_qr_host's arguments and csx_qr_host's patterns; a reflection's dot product and the squared tail of a
// column are summed in 64 strided partial sums and a fixed tree, every product rounded before it is added or subtracted.
extern "C" int csx_hqr_host(int32_t m, int32_t n, int32_t m2, const int32_t *Ap, const int32_t *Ai, const double *Ax,
                            const int32_t *q, const int32_t *parent, const int32_t *pinv, const int32_t *leftmost,
                            int32_t vcap, int32_t rcap, int32_t *Vp, int32_t *Vi, double *Vx, int32_t *Rp, int32_t *Ri,
                            double *Rx, double *beta) {
#pragma clang fp contract(off)
    CSX_TRY(csx_hqr_symbolic_host(m, n, m2, Ap, Ai, q, parent, pinv, leftmost, vcap, rcap, Vp, Vi, Rp, Ri));
    if ((Ap[n] > 0 && !Ax) || (n > 0 && (!Vx || !Rx || !beta))) return CSX_EINVAL;
    std::vector<double> work((size_t)m2, 0.0);
    double part[64];
    for (int32_t k = 0; k < n; k++) {
        const int32_t col = q ? q[k] : k;
        for (int32_t p = Ap[col]; p < Ap[col + 1]; p++) work[(size_t)pinv[Ai[p]]] = Ax[p];
        for (int32_t t = Rp[k]; t < Rp[k + 1] - 1; t++) {
            const int32_t c = Ri[t];
            for (int l = 0; l < 64; l++) part[l] = 0.0;
            for (int32_t p = Vp[c]; p < Vp[c + 1]; p++) {
                const int l = (p - Vp[c]) & 63;
                part[l] = part[l] + Vx[p] * work[(size_t)Vi[p]];
            }
            const double tau = hqr_tree(part) * beta[c];
            for (int32_t p = Vp[c]; p < Vp[c + 1]; p++) work[(size_t)Vi[p]] = work[(size_t)Vi[p]] - Vx[p] * tau;
            Rx[t] = work[(size_t)c];
            work[(size_t)c] = 0.0;
        }
        const int32_t vstart = Vp[k];
        for (int32_t p = vstart; p < Vp[k + 1]; p++) {
            Vx[p] = work[(size_t)Vi[p]];
            work[(size_t)Vi[p]] = 0.0;
        }
        for (int l = 0; l < 64; l++) part[l] = 0.0;
        for (int32_t p = vstart + 1; p < Vp[k + 1]; p++) {
            const int l = (p - vstart - 1) & 63;
            part[l] = part[l] + Vx[p] * Vx[p];
        }
        const double tail2 = hqr_tree(part);
        Rx[Rp[k + 1] - 1] = hqr_house(Vx[vstart], tail2, &Vx[vstart], &beta[k]);
    }
    return CSX_OK;
}

// ---- the Gram-Schmidt rule of restarted GMRES (csx_gmres.hip) on host arrays ----
#include "csx_gs.h"

extern "C" int csx_gmres_limits(int32_t *out) {   // (no device needed)
    if (!out) return CSX_EINVAL;
    out[0] = GS_CHUNK;
    out[1] = GS_FAN;
    out[2] = GS_GROUP;
    out[3] = GS_TILE;
    return CSX_OK;
}

extern "C" int csx_gs_work_len(int64_t rows, int32_t nrhs, int32_t nblocks, int64_t *len) {   // (no device needed)
    if (!len || rows < 0 || rows > ((int64_t)1 << 40) || nrhs < 1 || nblocks < 1) return CSX_EINVAL;
    *len = gs_work_len(rows, nrhs, nblocks);
    return CSX_OK;
}

namespace {
// the inner levels of the ordered sum over the leaf sums in `node`
double gs_tree(std::vector<double> &node) {
    size_t count = node.size();
    while (count > 1) {
        const size_t next = (count + GS_FAN - 1) / GS_FAN;
        for (size_t j = 0; j < next; j++) {
            double s = 0.0;
            for (size_t i = j * GS_FAN; i < std::min(count, (j + 1) * GS_FAN); i++) s = s + node[i];
            node[j] = s;
        }
        count = next;
    }
    return node[0];
}
}  // namespace

// op 0 project: out[i nrhs + c] = ordered sum of V_i[:, c] (+-W[:, c]), i < nv
// op 1 update:  W <- (+-W) - coef[0, c] V_0 - ... in ascending i; out[c] = ordered sum of the squares of the new W[:, c]
// op 2 scale:   V_nv[r, c] = W[r, c] / coef[c]   (nv is the slot)
// op 3 combine: out[r nrhs + c] = coef[0, c] V_0[r, c] + ... over i < len[c]: the first product, then rounded additions
extern "C" int csx_gs_host(int op, int64_t rows, int32_t nrhs, int32_t nv, double *V, double *W, const int32_t *mask, int negate,
                           const double *coef, const int32_t *len, double *out) {
#pragma clang fp contract(off)
    if (op < 0 || op > 3 || rows < 0 || nrhs < 1 || !mask || !V || (op != 3 && !W)) return CSX_EINVAL;
    if ((op == 2 ? nv < 0 : nv < 1) || (op != 0 && !coef) || (op != 2 && !out) || (op == 3 && !len)) return CSX_EINVAL;
    const int64_t block = rows * nrhs;
    const size_t nch = (size_t)gs_chunks(rows);
    std::vector<double> node(nch);
    for (int32_t c = 0; c < nrhs; c++) {
        if (!mask[c]) continue;
        if (op == 0) {
            for (int32_t i = 0; i < nv; i++) {
                const double *Vi = V + i * block;
                for (size_t l = 0; l < nch; l++) {
                    double s = 0.0;
                    for (int64_t r = (int64_t)l * GS_CHUNK; r < std::min(rows, (int64_t)(l + 1) * GS_CHUNK); r++) {
                        const double w = negate ? -W[r * nrhs + c] : W[r * nrhs + c];
                        const double p = Vi[r * nrhs + c] * w;
                        s = s + p;
                    }
                    node[l] = s;
                }
                out[(int64_t)i * nrhs + c] = gs_tree(node);
            }
        } else if (op == 1) {
            for (size_t l = 0; l < nch; l++) {
                double s = 0.0;
                for (int64_t r = (int64_t)l * GS_CHUNK; r < std::min(rows, (int64_t)(l + 1) * GS_CHUNK); r++) {
                    double w = negate ? -W[r * nrhs + c] : W[r * nrhs + c];
                    for (int32_t i = 0; i < nv; i++) {
                        const double p = coef[(int64_t)i * nrhs + c] * V[i * block + r * nrhs + c];
                        w = w - p;
                    }
                    W[r * nrhs + c] = w;
                    const double q = w * w;
                    s = s + q;
                }
                node[l] = s;
            }
            out[c] = gs_tree(node);
        } else if (op == 2) {
            for (int64_t r = 0; r < rows; r++) V[nv * block + r * nrhs + c] = W[r * nrhs + c] / coef[c];
        } else {
            if (len[c] < 0 || len[c] > nv) return CSX_EINVAL;
            for (int64_t r = 0; r < rows; r++) {
                double u = 0.0;
                for (int32_t i = 0; i < len[c]; i++) {
                    const double p = coef[(int64_t)i * nrhs + c] * V[i * block + r * nrhs + c];
                    u = i == 0 ? p : u + p;
                }
                out[r * nrhs + c] = u;
            }
        }
    }
    return CSX_OK;
}

// ---- the block rule of eigsh() in which columns mix (csx_bgs.hip) on host arrays ----
extern "C" int csx_bgs_limits(int32_t *out) {   // (no device needed)
    if (!out) return CSX_EINVAL;
    out[0] = GS_CHUNK;
    out[1] = GS_FAN;
    out[2] = BGS_MAXW;
    out[3] = BGS_GROUP;
    out[4] = BGS_TILE;
    return CSX_OK;
}

extern "C" int csx_bgs_work_len(int64_t rows, int32_t b, int32_t q, int32_t nblocks, int64_t *len) {   // (no device needed)
    if (!len || rows < 0 || rows > ((int64_t)1 << 40) || b < 1 || b > BGS_MAXW || q < 1 || q > BGS_MAXW || nblocks < 0)
        return CSX_EINVAL;
    *len = bgs_work_len(rows, b, q, nblocks);
    return CSX_OK;
}

// op 0 gram:    out[(i b + a) q + c] = ordered sum over r of V_i[r, a] (+-W[r, c]), i < nv
// op 1 update:  W[r, c] <- W[r, c] - coef[0, 0, c] V_0[r, 0] - coef[0, 1, c] V_0[r, 1] - ... in ascending (i, a)
// op 2 combine: out[r q + c] = coef[0, 0, c] V_0[r, 0] + ...: the first product, then rounded additions; +0.0 for nv == 0
extern "C" int csx_bgs_host(int op, int64_t rows, int32_t b, int32_t q, int32_t nv, const double *V, double *W, int negate,
                            const double *coef, double *out) {
#pragma clang fp contract(off)
    if (op < 0 || op > 2 || rows < 0 || nv < 0 || b < 1 || b > BGS_MAXW || q < 1 || q > BGS_MAXW) return CSX_EINVAL;
    const bool none = rows == 0 || nv == 0;   // an array that holds nothing may be null
    if ((!V && !none) || (op != 2 && !W && rows > 0) || (op != 0 && !coef && nv > 0)) return CSX_EINVAL;
    if (!out && ((op == 0 && nv > 0) || (op == 2 && rows > 0))) return CSX_EINVAL;
    const int64_t block = rows * b;
    if (op == 0) {
        const size_t nch = (size_t)gs_chunks(rows);
        std::vector<double> node(nch);
        for (int32_t i = 0; i < nv; i++)
            for (int32_t a = 0; a < b; a++)
                for (int32_t c = 0; c < q; c++) {
                    const double *Vi = V + i * block;
                    for (size_t l = 0; l < nch; l++) {
                        double s = 0.0;
                        for (int64_t r = (int64_t)l * GS_CHUNK; r < std::min(rows, (int64_t)(l + 1) * GS_CHUNK); r++) {
                            const double w = negate ? -W[r * q + c] : W[r * q + c];
                            const double p = Vi[r * b + a] * w;
                            s = s + p;
                        }
                        node[l] = s;
                    }
                    out[((int64_t)i * b + a) * q + c] = gs_tree(node);
                }
        return CSX_OK;
    }
    for (int64_t r = 0; r < rows; r++)
        for (int32_t c = 0; c < q; c++) {
            double x = op == 1 ? W[r * q + c] : 0.0;
            for (int32_t i = 0; i < nv; i++)
                for (int32_t a = 0; a < b; a++) {
                    const double p = coef[((int64_t)i * b + a) * q + c] * V[i * block + r * b + a];
                    if (op == 1) x = x - p;
                    else x = (i == 0 && a == 0) ? p : x + p;
                }
            (op == 1 ? W : out)[r * q + c] = x;
        }
    return CSX_OK;
}
