// The host forms of csx_pattern_outer and csx_assemble_pullback (include/csx.h has the rules).  Plain C++ with no
// device code and no other part of the library, so that they can be built and checked alone on a CPU.
#include "../../include/csx.h"
#include "csx_pattern_outer.h"

using namespace csx;

#pragma clang fp contract(off)
extern "C" int csx_pattern_outer_host(int32_t m, int32_t n, const int32_t *p, const int32_t *i, int32_t nrhs, int mode,
                                      double alpha, const double *U, const double *V, double *out) {
    if (m < 0 || n < 0 || nrhs < 1 || (mode != 0 && mode != 1) || (mode == 1 && m != n) || !p || p[0] != 0) return CSX_EINVAL;
    for (int32_t j = 0; j < n; j++)
        if (p[j + 1] < p[j]) return CSX_EINVAL;
    const int32_t nnz = p[n];
    if (nnz > 0 && (!i || !U || !V || !out)) return CSX_EINVAL;
    for (int32_t q = 0; q < nnz; q++)
        if (i[q] < 0 || i[q] >= m) return CSX_EINVAL;
    const int W = po_width(nrhs);
    for (int32_t j = 0; j < n; j++)
        for (int32_t q = p[j]; q < p[j + 1]; q++) {
            const int32_t r = i[q];
            if (mode == 1 && r > j) {
                out[q] = 0.0;
                continue;
            }
            const bool two = mode == 1 && r < j;
            const double *u = U + (int64_t)r * nrhs, *v = V + (int64_t)j * nrhs;
            const double *u2 = U + (int64_t)j * nrhs, *v2 = V + (int64_t)r * nrhs;   // sym: the mirrored place
            double s[PO_LANES];
            for (int l = 0; l < W; l++) {
                double acc = 0.0;
                for (int32_t c = l; c < nrhs; c += W) {
                    const double t = u[c] * v[c];
                    acc = c == l ? t : acc + t;
                    if (two) {
                        const double t2 = u2[c] * v2[c];
                        acc = acc + t2;
                    }
                }
                s[l] = acc;
            }
            for (int d = W / 2; d >= 1; d >>= 1)
                for (int l = 0; l < d; l++) s[l] = s[l] + s[l + d];
            out[q] = alpha * s[0];
        }
    return CSX_OK;
}
#pragma clang fp contract(fast)

extern "C" int csx_pattern_outer_limits(int64_t *out) {
    if (!out) return CSX_EINVAL;
    out[0] = PO_LANES;
    out[1] = PO_CHUNK;
    out[2] = PO_WAVE_CHUNK;
    out[3] = PO_FLIGHT;
    out[4] = PO_KEPT;
    return CSX_OK;
}

extern "C" int csx_assemble_pullback_host(int32_t nnz, int64_t nz, const int32_t *sp, const int32_t *src, const double *g,
                                          double *out) {
    if (nnz < 0 || nz < 0 || nz > INT32_MAX || !sp || sp[0] != 0) return CSX_EINVAL;
    for (int32_t s = 0; s < nnz; s++)
        if (sp[s + 1] < sp[s]) return CSX_EINVAL;
    if (sp[nnz] != nz || (nz > 0 && (!src || !g || !out))) return CSX_EINVAL;
    for (int64_t u = 0; u < nz; u++)
        if (src[u] < 0 || src[u] >= nz) return CSX_EINVAL;
    for (int32_t s = 0; s < nnz; s++)
        for (int32_t u = sp[s]; u < sp[s + 1]; u++) out[src[u]] = g[s];
    return CSX_OK;
}
