// What the row-block kernels share -- k_gaxpy_block, k_residual_block, k_residual_sym: one group of G lanes
// per row of a (ptr, idx, val) gather and one lane per right-hand side of a row-major block of nrhs columns.
//   * G is a power of two, 4 .. 64; G == 64: the row is wave-uniform and its (idx, val) pairs are scalar loads.
//   * V columns per lane: V = 2 moves 16 bytes per load and needs nrhs even and every block 16-byte aligned.
//   * U entries of a row are requested before the first is used: the chain ptr -> idx/val -> X row is latency-bound.
//   * A workgroup of 256 lanes owns ROWBLOCK_TILE consecutive rows; nrhs > G V takes several passes over a row.
// Value rule of all three: a term's product is rounded before it is added (no FMA), the terms of a row come in the written
// order, and an entry that is not a term is skipped, never added as a zero (-0.0 + 0.0 would change the sign of a zero
// sum).  The entry loops themselves are still written out per kernel: DESIGN.md 40 has what one shared loop measured.
#pragma once
#include "csx_internal.h"

namespace csx {

typedef double f64x2 __attribute__((ext_vector_type(2)));

constexpr int ROWBLOCK_TILE = 64;   // rows per workgroup: one G-spd dense block

// V columns of one row of a block, as a lane holds them
template <int V>
struct Cols;
template <>
struct Cols<1> {
    typedef double T;
    static __device__ __forceinline__ T load(const double *p) { return *p; }
    static __device__ __forceinline__ void store(double *p, T v) { *p = v; }
    static __device__ __forceinline__ T abs(T v) { return fabs(v); }
    static __device__ __forceinline__ double at(T v, int) { return v; }
};
template <>
struct Cols<2> {
    typedef f64x2 T;
    static __device__ __forceinline__ T load(const double *p) { return *reinterpret_cast<const f64x2 *>(p); }
    static __device__ __forceinline__ void store(double *p, T v) { *reinterpret_cast<f64x2 *>(p) = v; }
    static __device__ __forceinline__ T abs(T v) {
        T a;
        a.x = fabs(v.x);
        a.y = fabs(v.y);
        return a;
    }
    static __device__ __forceinline__ double at(T v, int k) { return k ? v.y : v.x; }
};

// The launch table of the three kernels: launch(RowBlockShape<G, V>()) for the instance a block of nrhs columns takes;
// aligned: every block the lanes load or store starts on 16 bytes.
template <int G_, int V_>
struct RowBlockShape {
    static constexpr int G = G_, V = V_, U = 8;
};
inline bool aligned16(const void *a, const void *b, const void *c = nullptr) {
    return ((uintptr_t)a % 16) == 0 && ((uintptr_t)b % 16) == 0 && ((uintptr_t)c % 16) == 0;
}
template <class LAUNCH>
void rowblock_launch(int32_t nrhs, bool aligned, LAUNCH launch) {
    const bool pairs = nrhs % 2 == 0 && aligned;
    if (nrhs > 64) {
        if (pairs) launch(RowBlockShape<64, 2>());
        else launch(RowBlockShape<64, 1>());
    } else if (nrhs > 32) launch(RowBlockShape<64, 1>());
    else if (nrhs > 16) launch(RowBlockShape<32, 1>());
    else if (nrhs > 8) launch(RowBlockShape<16, 1>());
    else if (nrhs > 4) launch(RowBlockShape<8, 1>());
    else launch(RowBlockShape<4, 1>());
}

}  // namespace csx
