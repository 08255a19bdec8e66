// csx_gaxpy_block: Y += A X for an n-by-nrhs block X (row-major, the layout of every batched solve), i.e.
// cs_gaxpy (csparse.py:1199-1213) applied to every column of X at once.
//
// Block kernel (both modes): the row-block shape (csx_rowblock.h) on A's cached row gather (A->rows: the
// entries of row r in ascending (column, position) order = the order in which the reference adds them into y[r]).  A
// lane starts from Y[r, c] and adds val[q] * X[idx[q], c] over the row in that order, the product rounded before the
// sum (no FMA): every column of Y is bit-identical to csx_gaxpy EXACT on that column, and a run is deterministic.  The
// order costs nothing here (each lane owns its own sum); only the multiply and the add are two instructions where an FMA
// could be one, in a kernel bound by the gathers.
//   * A group reads the row's (idx, val) pairs once for all of its columns and gathers whole pieces of X rows: G V 8
//     bytes per entry (1 KiB per wave instruction at nrhs >= 128).
//   * A workgroup owns ROWBLOCK_TILE consecutive rows, so the rows of one dense block of a block-structured matrix
//     (G-spd) gather the same X rows on one CU.  Measured, that is not yet enough: with ~256 tiles live per XCD the X
//     rows do not stay in its L2, and G-spd at k = 128 fetches 4.5x its algorithmic bytes.
//
// Column route (AUTO only, matrices with a tiled plan, narrow blocks): X and Y are transposed into nrhs
// contiguous vectors, csx_gaxpy's own plan runs once per column, and the columns of Y are transposed back:
// every column bit-identical to csx_gaxpy AUTO on it.  DESIGN.md 10 has the measurements behind the rule.
//
// Algorithmic bytes per call: 12 nnz + 4 (m + 1) + 8 n nrhs + 16 m nrhs.
#include "csx_rowblock.h"

namespace csx {

#pragma clang fp contract(off)
// Rows outer, column passes inner: a group reads its row pointers once.  Lanes whose columns lie past nrhs do nothing.
template <int G, int V, int U>
__global__ __launch_bounds__(256) void k_gaxpy_block(int32_t rows, int32_t nrhs, const int32_t *__restrict__ ptr,
                                                     const int32_t *__restrict__ idx, const double *__restrict__ val,
                                                     const double *__restrict__ X, double *__restrict__ Y) {
    typedef typename Cols<V>::T T;
    constexpr int GROUPS = 256 / G;
    const int sub = threadIdx.x & (G - 1);
    const int gid = G == 64 ? __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) : (int)(threadIdx.x / G);
    const int64_t r0 = (int64_t)blockIdx.x * ROWBLOCK_TILE;
    const int64_t r1 = r0 + ROWBLOCK_TILE < rows ? r0 + ROWBLOCK_TILE : rows;
    for (int64_t r = r0 + gid; r < r1; r += GROUPS) {
        const int32_t b = ptr[r], e = ptr[r + 1];
        for (int32_t c0 = 0; c0 < nrhs; c0 += G * V) {
            const int32_t c = c0 + sub * V;
            if (c >= nrhs) continue;
            T acc = Cols<V>::load(Y + r * nrhs + c);
            for (int32_t q = b; q < e; q += U) {
                int32_t j[U];
                double v[U];
                T xv[U];
#pragma unroll
                for (int u = 0; u < U; u++) {
                    const bool in = q + u < e;
                    j[u] = in ? idx[q + u] : 0;
                    v[u] = in ? val[q + u] : 0.0;
                }
#pragma unroll
                for (int u = 0; u < U; u++) xv[u] = Cols<V>::load(X + (int64_t)j[u] * nrhs + c);
#pragma unroll
                for (int u = 0; u < U; u++)
                    if (q + u < e) {   // skipped, not added as 0: -0.0 + 0.0 would change the sign of a zero sum
                        const T t = v[u] * xv[u];
                        acc = acc + t;
                    }
            }
            Cols<V>::store(Y + r * nrhs + c, acc);
        }
    }
}
#pragma clang fp contract(fast)

// out (cols x rows, row-major) = in (rows x cols, row-major)': 32 x 32 tiles through LDS, tile (bi, bj) in
// workgroup bj * row_tiles + bi (either dimension may be the large one).
__global__ __launch_bounds__(256) void k_block_transpose(int64_t rows, int64_t cols, int64_t row_tiles,
                                                         const double *__restrict__ in, double *__restrict__ out) {
    __shared__ double tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int64_t i0 = ((int64_t)blockIdx.x % row_tiles) * 32;
    const int64_t c0 = ((int64_t)blockIdx.x / row_tiles) * 32;
#pragma unroll
    for (int k = 0; k < 32; k += 8) {
        const int64_t i = i0 + ty + k;
        if (i < rows && c0 + tx < cols) tile[ty + k][tx] = in[i * cols + c0 + tx];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 32; k += 8) {
        const int64_t c = c0 + ty + k;
        if (c < cols && i0 + tx < rows) out[(int64_t)c * rows + i0 + tx] = tile[tx][ty + k];
    }
}

static int block_transpose(int64_t rows, int64_t cols, const double *in, double *out) {
    if (rows == 0 || cols == 0) return CSX_OK;
    const int64_t gx = (rows + 31) / 32, gy = (cols + 31) / 32;
    if (gx * gy > 0x7fffffff) return CSX_EINVAL;
    hipLaunchKernelGGL(k_block_transpose, dim3((unsigned)(gx * gy)), dim3(256), 0, ctx().stream, rows, cols, gx, in, out);
    CSX_LAUNCH_CHECK();
    return CSX_OK;
}

static int run_block(const Gather *g, int32_t nrhs, const double *X, double *Y) {
    if (g->rows == 0) return CSX_OK;
    const unsigned blocks = (unsigned)(((int64_t)g->rows + ROWBLOCK_TILE - 1) / ROWBLOCK_TILE);
    rowblock_launch(nrhs, aligned16(X, Y), [&](auto sh) {
        hipLaunchKernelGGL((k_gaxpy_block<sh.G, sh.V, sh.U>), dim3(blocks), dim3(256), 0, ctx().stream, g->rows, nrhs,
                           g->ptr.get(), g->idx.get(), g->val.get(), X, Y);
    });
    CSX_LAUNCH_CHECK();
    return CSX_OK;
}

// nrhs passes of the matrix's own single-vector plan on transposed copies of X and Y.
static int run_columns(Csc *A, int32_t nrhs, const double *X, double *Y) {
    DevBuf<double> xc, yc;
    CSX_TRY(xc.alloc((size_t)A->n * nrhs));
    CSX_TRY(yc.alloc((size_t)A->m * nrhs));
    CSX_TRY(block_transpose(A->n, nrhs, X, xc));
    CSX_TRY(block_transpose(A->m, nrhs, Y, yc));
    for (int32_t c = 0; c < nrhs; c++)
        CSX_TRY(gaxpy_device(A, xc + (int64_t)c * A->n, yc + (int64_t)c * A->m, CSX_GAXPY_AUTO));
    return block_transpose(nrhs, A->m, yc, Y);
}

// AUTO takes the column route for blocks of at most this many columns on a matrix with a tiled plan.
constexpr int32_t COLUMN_ROUTE_MAX_NRHS = 4;

}  // namespace csx

using namespace csx;

extern "C" int csx_gaxpy_block(csx_handle_t hA, csx_handle_t hX, csx_handle_t hY, int32_t nrhs, int mode) {
    CSX_TRY(require_ready());
    Csc *A = csc(hA);
    Vec *X = vec(hX), *Y = vec(hY);
    if (!A || !X || !Y || !A->x || nrhs < 1) return CSX_EINVAL;
    if (mode != CSX_GAXPY_EXACT && mode != CSX_GAXPY_AUTO) return CSX_EINVAL;
    const int64_t xlen = (int64_t)A->n * nrhs, ylen = (int64_t)A->m * nrhs;
    if (X->len < xlen || Y->len < ylen || hX == hY) return CSX_EINVAL;
    if (ranges_overlap(X->d, xlen, Y->d, ylen)) return CSX_EINVAL;   // wrapped views of one buffer
    if (A->m == 0 || A->n == 0 || A->nnz == 0) return CSX_OK;
    const double *xd = (const double *)X->d;
    double *yd = (double *)Y->d;
    if (nrhs == 1) return gaxpy_device(A, xd, yd, mode);
    if (mode == CSX_GAXPY_AUTO) {
        // the decision csx_gaxpy AUTO makes for this matrix, made the same way (so a csx_gaxpy after this call
        // runs the plan it would have run without it)
        if (!A->tiled && !A->rows) CSX_TRY(gaxpy_prepare_device(A, CSX_GAXPY_AUTO));
        int route = ctx().opt.gaxpy_block_route;
        if (route == 0) route = A->tiled && nrhs <= COLUMN_ROUTE_MAX_NRHS ? 2 : 1;
        if (route == 2) return run_columns(A, nrhs, xd, yd);
    }
    CSX_TRY(build_row_gather(A));
    return run_block(A->rows.get(), nrhs, xd, yd);
}
