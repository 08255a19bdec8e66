// The constants of the ordered sum and of the Gram-Schmidt kernels (csx_gmres.hip), shared with their host rule
// (csx_host.cpp: csx_gs_host, csx_gmres_limits, csx_gs_work_len).  DESIGN.md §28.
#pragma once
#include <cstdint>

namespace csx {

constexpr int GS_CHUNK = 256;   // rows of a leaf of the ordered sum, added in ascending row order
constexpr int GS_FAN = 16;      // children of an inner node, added in ascending order
constexpr int GS_GROUP = 8;     // basis vectors whose sums one pass of csx_gs_project carries in registers
constexpr int GS_TILE = 8;      // rows of W that csx_gs_update / csx_gs_combine hold in registers per coefficient load

// doubles of the work vector the csx_gs_* calls take, for blocks of rows x nrhs and at most nblocks basis blocks in a call:
// nrhs (the mask and the lengths, as int32), 2 nblocks nrhs (coefficients in, sums out), and the partial sums of one register
// group over the leaves and over the first inner level (the further levels go back and forth between the two)
inline int64_t gs_chunks(int64_t rows) { return rows > 0 ? (rows + GS_CHUNK - 1) / GS_CHUNK : 1; }
inline int64_t gs_work_len(int64_t rows, int32_t nrhs, int32_t nblocks) {
    const int64_t nch = gs_chunks(rows), n1 = (nch + GS_FAN - 1) / GS_FAN;
    return (int64_t)nrhs * (1 + 2 * (int64_t)nblocks + GS_GROUP * (nch + n1));
}

}  // namespace csx
