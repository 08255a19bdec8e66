// ranges_overlap and residual_blocks_ok (csx_internal.h) on host memory, for a run under a sanitizer:
//     hipcc --offload-arch=gfx950 --offload-host-only -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all
//           -Icsparse.py_amd/csrc tools/check_block_args.cpp -o check_block_args && ./check_block_args
// (host code only, no device needed: the sanitizers never touch a GPU.)
// Both are address arithmetic: nothing is dereferenced, so the views below are made of one host array.
#include <cstdio>

#include "csx_internal.h"

namespace csx {
void dfree(void *) {}   // (~Vec; the views own nothing)
}
using namespace csx;

static int failed = 0;
#define EXPECT(cond)                                                    \
    do {                                                                \
        if (!(cond)) {                                                  \
            std::printf("line %d: %s does not hold\n", __LINE__, #cond); \
            failed++;                                                   \
        }                                                               \
    } while (0)

static void view(Vec &v, double *d, int64_t len) {
    v.d = d;
    v.len = len;
    v.owns = false;
}

int main() {
    static double buf[64];
    // empty ranges and length 0: nothing is shared, wherever they point (null included)
    EXPECT(!ranges_overlap(buf, 0, buf, 0) && !ranges_overlap(buf, 0, buf, 8) && !ranges_overlap(buf + 4, 8, buf + 6, 0));
    EXPECT(!ranges_overlap(nullptr, 0, buf, 8) && !ranges_overlap(nullptr, 0, nullptr, 0));
    // adjacent, one double shared, nested, identical; both argument orders
    EXPECT(!ranges_overlap(buf, 8, buf + 8, 8) && !ranges_overlap(buf + 8, 8, buf, 8));
    EXPECT(ranges_overlap(buf, 9, buf + 8, 8) && ranges_overlap(buf + 8, 8, buf, 9));
    EXPECT(ranges_overlap(buf, 32, buf + 8, 8) && ranges_overlap(buf + 8, 8, buf, 32));
    EXPECT(ranges_overlap(buf + 8, 1, buf + 8, 1) && ranges_overlap(buf, 64, buf, 64));
    EXPECT(!ranges_overlap(buf + 63, 1, buf + 62, 1) && !ranges_overlap(buf, 1, buf + 63, 1));

    Vec X, B, R, B2, S;
    view(X, buf, 16);
    view(B, buf + 16, 8);
    view(R, buf + 24, 8);
    EXPECT(residual_blocks_ok(&X, 16, &B, &R, 8) && residual_blocks_ok(&X, 16, &B, nullptr, 8));
    EXPECT(residual_blocks_ok(&X, 16, &B, &B, 8));                                      // in place: the same vector
    view(B2, buf + 16, 8);
    EXPECT(residual_blocks_ok(&X, 16, &B, &B2, 8));                                     // ... the same address under another handle
    EXPECT(!residual_blocks_ok(&X, 17, &B, &R, 8) && !residual_blocks_ok(&X, 16, &B, &R, 9));   // too short
    EXPECT(!residual_blocks_ok(&X, 16, &B, nullptr, 9));
    EXPECT(!residual_blocks_ok(&X, 8, &X, &R, 8) && !residual_blocks_ok(&X, 8, &B, &X, 8));     // X as B, X as R
    EXPECT(!residual_blocks_ok(&X, 0, &X, nullptr, 0));                                 // ... at length 0 too
    view(S, buf + 15, 8);
    EXPECT(!residual_blocks_ok(&X, 16, &S, &R, 8) && !residual_blocks_ok(&X, 16, &B, &S, 8));   // one double into X
    view(S, buf + 20, 8);
    EXPECT(!residual_blocks_ok(&X, 16, &B, &S, 8));                                     // R over half of B
    EXPECT(residual_blocks_ok(&X, 16, &B, &S, 4));                                      // ... and beside the half in use
    view(S, buf + 4, 8);
    EXPECT(!residual_blocks_ok(&X, 16, &S, nullptr, 8) && residual_blocks_ok(&X, 4, &S, nullptr, 8));   // nested in X; X ends before it
    EXPECT(residual_blocks_ok(&X, 0, &S, &S, 8) && residual_blocks_ok(&X, 16, &S, &S, 0));   // an empty side shares nothing
    std::printf(failed ? "FAILED: %d\n" : "ok\n", failed);
    return failed != 0;
}
