// bp_quant.hpp — the broad phase's compact candidate row: an AABB quantised to 6 x 16 bits on a frame around the step's grid, plus the collider's world index.
//   bpQuantFrame     the frame of a grid: origin - one cell .. origin + (dims + 1) cells per axis, mapped to [0, 65535]
//   bpQuantRow       THE quantiser: minima rounded down, maxima rounded up, both clamped; a row with a NaN in it covers the whole range
//   bpQuantOverlap   the test on two rows
// CONSERVATIVE: every pair the exact closed-interval test (aabbOverlap) accepts passes bpQuantOverlap, for any two boxes (well-formed or not) and any frame:
//   amax >= bmin  =>  q_up(amax) >= t(amax) >= t(bmin) >= q_down(bmin),   t(x) = (x - f0) * scale in fp32 per axis, scale >= 0
// t is monotone wherever it is a number (a rounded subtraction of a constant and a rounded product with a non-negative constant are), floor / ceil and the clamp keep the
// order, and wherever t is NOT a number — a NaN bound, which the exact test accepts against everything (all of its comparisons are false), an infinite bound on an
// infinite frame, 0 x inf — the row gets [0, 65535] on every axis and passes against every row.  Both sides of every comparison come from this one function on one frame:
// the pair kernel reads its own collider's row from the array like any candidate's and never quantises a box itself.
// Plain C++ (a host compiler builds it for tests/test_bp_quant.py); included by kernels_broad.hpp.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MI_BPQ_HD __host__ __device__ __forceinline__
#else
#define MI_BPQ_HD inline
#endif

namespace mi {

struct BpQuantFrame { float f0[3]; float scale[3]; };

MI_BPQ_HD BpQuantFrame bpQuantFrame(const float origin[3], const uint32_t dims[3], float cell) {
    BpQuantFrame f;
    for (int a = 0; a < 3; ++a) {
        f.f0[a] = origin[a] - cell;
        const float s = 65535.f / (((float)dims[a] + 2.f) * cell);
        f.scale[a] = s >= 0.f ? s : 0.f;   // (a negative or NaN cell: every number maps to 0 and every pair passes)
    }
    return f;
}

// Row layout, chosen for the test: w0 = min.x | min.y << 16, w1 = min.z | max.z << 16, w2 = max.x | max.y << 16, w3 = the collider's world index.
MI_BPQ_HD void bpQuantRow(const BpQuantFrame& f, const float mn[3], const float mx[3], uint32_t index, uint32_t row[4]) {
    uint32_t lo[3], hi[3];
    bool nan = false;
    for (int a = 0; a < 3; ++a) {
        const float tl = (mn[a] - f.f0[a]) * f.scale[a], th = (mx[a] - f.f0[a]) * f.scale[a];
        nan = nan || tl != tl || th != th;   // (tested explicitly: fminf / fmaxf would return the other operand)
        const float ql = floorf(tl), qh = ceilf(th);
        lo[a] = (uint32_t)(ql > 0.f ? (ql < 65535.f ? ql : 65535.f) : 0.f);
        hi[a] = (uint32_t)(qh > 0.f ? (qh < 65535.f ? qh : 65535.f) : 0.f);
    }
    if (nan) { lo[0] = lo[1] = lo[2] = 0u; hi[0] = hi[1] = hi[2] = 65535u; }
    row[0] = lo[0] | (lo[1] << 16); row[1] = lo[2] | (hi[2] << 16); row[2] = hi[0] | (hi[1] << 16); row[3] = index;
}

// two 16-bit lanes of a - b, each saturating at 0 (gfx950: one packed instruction)
MI_BPQ_HD uint32_t bpPkSubSat(uint32_t a, uint32_t b) {
#if defined(__clang__)
    typedef unsigned short bpq_us2 __attribute__((ext_vector_type(2)));
    const bpq_us2 r = __builtin_elementwise_sub_sat(__builtin_bit_cast(bpq_us2, a), __builtin_bit_cast(bpq_us2, b));
    return __builtin_bit_cast(uint32_t, r);
#else
    const uint32_t al = a & 0xFFFFu, bl = b & 0xFFFFu, ah = a >> 16, bh = b >> 16;
    return (al > bl ? al - bl : 0u) | ((ah > bh ? ah - bh : 0u) << 16);
#endif
}
// A min above a max on any axis leaves a non-zero half: bmin - amax (x, y), amin - bmax (x, y), and for z {bmin, amin} - {amax, bmax}.
MI_BPQ_HD bool bpQuantOverlap(const uint32_t a[4], const uint32_t b[4]) {
    const uint32_t zmin = (b[1] & 0xFFFFu) | (a[1] << 16);          // b.min.z | a.min.z << 16
    const uint32_t zmax = (a[1] >> 16) | (b[1] & 0xFFFF0000u);      // a.max.z | b.max.z << 16
    return (bpPkSubSat(b[0], a[2]) | bpPkSubSat(a[0], b[2]) | bpPkSubSat(zmin, zmax)) == 0u;
}

}  // namespace mi
