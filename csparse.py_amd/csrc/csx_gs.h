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

// ---- the block kernels in which columns mix (csx_bgs.hip, csx_bgs_host) ----
constexpr int BGS_MAXW = 32;     // widest block (b of the basis, q of W / U) a call takes
constexpr int BGS_GROUP = 4;     // basis blocks whose b x q sums one pass of csx_bgs_gram carries: W crosses memory once per group
constexpr int BGS_TILE = 1024;   // doubles of one block's row tile in LDS: BGS_TILE / max(b, q) rows (GS_CHUNK at the most)

// doubles of the work vector the csx_bgs_* calls take for rows x b basis blocks (nblocks of them at most in a call) and a
// rows x q block: b q nblocks coefficients in and as many sums out, and the leaf sums of one group of BGS_GROUP basis blocks with
// their first inner level: BGS_GROUP b q / GS_CHUNK <= min(b, q) / 2 doubles per row, under half a rows x max(b, q) block
inline int64_t bgs_work_len(int64_t rows, int32_t b, int32_t q, int32_t nblocks) {
    const int64_t nch = gs_chunks(rows), n1 = (nch + GS_FAN - 1) / GS_FAN;
    return (int64_t)b * q * (2 * (int64_t)nblocks + BGS_GROUP * (nch + n1));
}

}  // namespace csx
