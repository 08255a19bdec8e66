// Constants of csx_pattern_outer (include/csx.h has the rule), shared by the kernel and the host rule.
#pragma once
#include <cstdint>

namespace csx {

constexpr int PO_LANES = 16;         // most partial sums of an entry: 16 lanes x 8 bytes = one 128-byte line of a block row
constexpr int PO_CHUNK = 1024;       // entries of a workgroup (4 waves)
constexpr int PO_WAVE_CHUNK = 256;   // consecutive entries of the chunk that one wave takes
constexpr int PO_FLIGHT = 4;         // entries whose row gathers a lane group issues before it consumes the first
constexpr int PO_KEPT = 8;           // passes of a column's own rows a lane keeps in registers: nrhs <= PO_KEPT * PO_LANES

// W of the rule: min(PO_LANES, smallest power of two >= nrhs)
inline int po_width(int32_t nrhs) {
    int w = 1;
    while (w < nrhs && w < PO_LANES) w <<= 1;
    return w;
}

}  // namespace csx
