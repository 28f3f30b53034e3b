// kernels_distance.hpp — batched distance scene queries (mi_world_distance*, include/mi_physics.h): the collider nearest to a sphere, capsule,
// cylinder, box or hull, with the distance, the two closest points and the direction between them.  Part of the ONE translation unit of the
// physics library (world.hip includes it after kernels_sweep.hpp, whose simplex machinery, box trimming and wave minimum it uses, and through it
// kernels_overlap.hpp's volume rows and admission test and kernels_query.hpp's grid).  Host side: world_query.inc.
//
// Read-only with respect to the step: everything here reads query-owned rows and writes the caller's records.
//   distancePair             the pair test: GJK on the Minkowski difference volume - collider of the CORES (spheres and capsules are a point /
//                            segment plus a radius margin, as in the casts): the closest vector v from the collider to the volume, the
//                            witness on the collider; the witness on the volume is that one + v
//   k_q_distance             one wave per volume: the large list first (it seeds the best distance), then the grid in expanding shells of
//                            cells about the volume's own cell range, until everything outside the walked box is provably farther than the best
//                            distance or max_distance; a volume over many cells, or a world without a grid, strides over all colliders
//   k_q_distance_exhaustive  the yardstick: every collider for every volume, rows computed for the call, nothing skipped
// Both kernels decide through dsCandidate (admission: ovAdmit) and write through dsFinalise: the same winner key (distance bits << 32 |
// collider) gives the same bytes.  THE INVARIANT behind that: the distance a candidate reports (dsResolve) is never below the gap of the two
// world AABBs, and that gap is never below the bound of a shell that left the candidate out (dsShellBound, padded); skipping compares
// strictly, so candidates at equal distance still meet and the lowest index wins on every route.
// No atomics, no dependence between workgroups; every loop is bounded by a constant, the collider count or the grid.
#pragma once
#include "kernels_sweep.hpp"

namespace mi {

constexpr uint32_t kDistanceMaxIter = 64;      // iterations of the pair test; a pair that reaches it reports its current (upper-bound) distance with kDistanceUnconverged
constexpr uint32_t kDistanceOverlap = 1u, kDistanceUnconverged = 2u;   // MI_DISTANCE_*
constexpr uint32_t kDistanceRecordRows = 4;    // mi_distance_hit: four rows of 16 bytes

// ---- the pair test
struct DistanceResult { float distance; V3 pointCollider, pointVolume, normal; uint32_t flags; };

// An upper bound of the distance between a volume (its AABB [mn, mx]) and a box collider: from the AABB's centre to its clamp onto the box, plus
// the AABB's half-diagonal (some point of the volume lies that close to the centre).  The closest point of the box then lies inside the
// volume's AABB grown by that much: what swClipBox keeps of the box.
__device__ inline Shape dsClipBox(const Shape& b, V3 mn, V3 mx) {
    if (b.type != T_AABB && b.type != T_OBB) return b;
    const V3 centre = mn * 0.5f + mx * 0.5f, half = mx * 0.5f - mn * 0.5f;
    const V3 c = b.type == T_AABB ? centre : rotate(conj(b.rot), centre - b.a);
    const V3 lo = b.type == T_AABB ? b.a : V3() - b.b, hi = b.b;
    const V3 clamped = vmin(qvmax(c, lo), hi);
    const float reach = len(c - clamped) + len(half);
    return swClipBox(b, mn - V3(reach), mx + V3(reach));
}

// THE pair test.  A = the volume, `collider` = B; both stand still.  GJK on C = A - B (the cores' difference; R = the sum of the margins): v is
// the point of the current simplex closest to the origin, a vector from B's core to A's, so |v| - R is an UPPER bound of the distance at every
// iteration; the support point w of C against v gives the LOWER bound dot(v, w) / |v| - R.  The search ends converged once the two are within
// a tolerance relative to the coordinates (kSweepTolRel, no absolute threshold), and STALLED when an iteration brings a support point the
// simplex holds or does not shorten v: converged if the bounds are within kSweepStallTol tolerances, each grown by the lower bound's own rounding (v
// carries the coordinates' rounding, so its DIRECTION is only good to tolerance / |v|, which moves the support plane at a support point L = |w - v|
// beside v by L x tolerance / |v|: a cap a hair above a face), kDistanceUnconverged beyond them or out of iterations (the current distance: too
// far, never too near).  The shapes count as touching (kDistanceOverlap, distance 0; points and normal
// are the caller's) unless some support plane separated them by more than the margins, the sweep's rule for an initial overlap, or when the
// origin lies inside the simplex.  pointCollider / pointVolume: on the surfaces, the witnesses moved by the margins along normal = v / |v|.
// The result depends on (A, B) alone; one body (distancePair below, not inlined) serves the candidate test and the record writer of both kernels.
// kTriangle: the collider is a terrain triangle (swTerrainShape; no margin, nothing to clip), its support swTriangleSupport — an instance of its own, as
// sweepPairBody has one, so that the world's pair test is compiled without the triangle case (kSwTriangle, kernels_sweep.hpp).
template <bool kTriangle> __device__ __forceinline__ Shape dsColliderShape(const Shape& collider, V3 volumeMin, V3 volumeMax) {
    if constexpr (kTriangle) return collider; else return dsClipBox(collider, volumeMin, volumeMax);
}
template <bool kTriangle> __device__ __forceinline__ DistanceResult distancePairBody(const Shape& A, V3 volumeMin, V3 volumeMax, const Shape& collider, const HullSet& hs) {
    DistanceResult r; r.distance = 0.f; r.flags = kDistanceOverlap;
    const Shape B = dsColliderShape<kTriangle>(collider, volumeMin, volumeMax);
    const float mA = swMargin(A), mB = swMargin(B), R = mA + mB;   // (a triangle's type has no margin)
    V3 witness = swColliderSupport<kTriangle>(B, hs, V3());   // on B's core; the one on A's is witness + v, or witnessA where A's simplex points lie closer together
    SwSimplex s; s.n = 0u;
    {
        const V3 pa = swSupport(A, hs, V3());
        swPush(s, witness - pa, witness);
    }
    V3 v = V3() - s.y0, witnessA = witness + v;
    bool anchorA = false;
    float scale = qmax(1.f, qmax(swMaxAbs(witness), swMaxAbs(witness + v)));
    bool separated = false, done = false;
    float lv = len(v);
    for (uint32_t it = 0; it < kDistanceMaxIter; ++it) {
        if (!(lv > 0.f)) return r;   // the cores meet
        const V3 pb = swColliderSupport<kTriangle>(B, hs, v), pa = swSupport(A, hs, V3() - v), p = pb - pa;
        scale = qmax(scale, qmax(swMaxAbs(pa), swMaxAbs(pb)));
        const float tol = kSweepTolRel * qmax(scale, R);
        const float lower = -dot(v, p) / lv - R, slack = (lv - R) - lower;
        if (lower > 0.f) separated = true;
        if (slack <= tol) { done = true; break; }
        const bool dup = (p.x == s.y0.x && p.y == s.y0.y && p.z == s.y0.z) || (s.n > 1u && p.x == s.y1.x && p.y == s.y1.y && p.z == s.y1.z) ||
                         (s.n > 2u && p.x == s.y2.x && p.y == s.y2.y && p.z == s.y2.z) || (s.n > 3u && p.x == s.y3.x && p.y == s.y3.y && p.z == s.y3.z);
        // what a stall may leave between the bounds: kSweepStallTol tolerances, each grown by the rounding of v's direction (above); or any gap that a
        // tilt of v explains which float32 cannot see in |v|: the support point lies L beside v, a tilt of slack / L lowers its plane by `slack` (first
        // order) and lengthens v by |v| tilt^2 / 2 (second order): converged when that is within the tolerance
        const float beside = len(p + v), tilt = beside > 0.f ? slack / beside : 0.f;
        const bool stallOk = slack <= kSweepStallTol * tol * (1.f + beside / lv) || 0.5f * lv * tilt * tilt <= tol;
        if (dup) { done = stallOk; break; }
        swPush(s, p, pb);   // (at most three points were kept: a proper tetrahedron ended the search, a flat one kept a face)
        SwWeights w; V3 nv;
        if (!swClosest(s.n, V3() - s.y0, V3() - s.y1, V3() - s.y2, V3() - s.y3, w, nv)) return r;   // the origin inside the simplex: the cores overlap
        const float nl = len(nv);
        if (!(nl < lv)) { done = stallOk; break; }   // (no shorter: v, its witness and its bounds stand)
        witness = s.b0 * w.w0;
        if (s.n > 1u) witness = witness + s.b1 * w.w1;
        if (s.n > 2u) witness = witness + s.b2 * w.w2;
        if (s.n > 3u) witness = witness + s.b3 * w.w3;
        // the same weights on A's support points a_i = b_i - y_i, and which of the two sets lies closer together: the weights of a thin simplex are
        // good to a rounding of its vertices' spread, so the witness of the tighter set is the one to trust (a 1e-2 volume over a 50-unit cylinder)
        witnessA = (s.b0 - s.y0) * w.w0;
        float spreadA = 0.f, spreadB = 0.f;
        if (s.n > 1u) { witnessA = witnessA + (s.b1 - s.y1) * w.w1; spreadB = qmax(spreadB, sqlen(s.b1 - s.b0)); spreadA = qmax(spreadA, sqlen((s.b1 - s.y1) - (s.b0 - s.y0))); }
        if (s.n > 2u) { witnessA = witnessA + (s.b2 - s.y2) * w.w2; spreadB = qmax(spreadB, sqlen(s.b2 - s.b0)); spreadA = qmax(spreadA, sqlen((s.b2 - s.y2) - (s.b0 - s.y0))); }
        if (s.n > 3u) { witnessA = witnessA + (s.b3 - s.y3) * w.w3; spreadB = qmax(spreadB, sqlen(s.b3 - s.b0)); spreadA = qmax(spreadA, sqlen((s.b3 - s.y3) - (s.b0 - s.y0))); }
        anchorA = spreadA < spreadB;
        // keep the vertices that carry the closest point
        SwSimplex k; k.n = 0u;
        if (w.w0 > 0.f) swPush(k, s.y0, s.b0);
        if (s.n > 1u && w.w1 > 0.f) swPush(k, s.y1, s.b1);
        if (s.n > 2u && w.w2 > 0.f) swPush(k, s.y2, s.b2);
        if (s.n > 3u && w.w3 > 0.f) swPush(k, s.y3, s.b3);
        if (k.n == 0u) swPush(k, s.y0, s.b0);
        s = k;
        v = nv; lv = nl;
    }
    if (!separated || !(lv - R > 0.f)) return r;
    r.flags = done ? 0u : kDistanceUnconverged;
    r.distance = lv - R;
    r.normal = v * (1.f / lv);
    if (anchorA) witness = witnessA - v;
    r.pointCollider = witness + r.normal * mB;
    r.pointVolume = (witness + v) - r.normal * mA;
    return r;
}
__device__ __noinline__ DistanceResult distancePair(const Shape& A, V3 volumeMin, V3 volumeMax, const Shape& collider, const HullSet& hs) {
    return distancePairBody<false>(A, volumeMin, volumeMax, collider, hs);
}
// ... against a terrain triangle (swTerrainShape): one body (not inlined) for the candidate test and the record writer of both terrain kernels
// (kernels_terrain_distance.hpp)
__device__ __noinline__ DistanceResult distanceTrianglePair(const Shape& A, const Shape& triangle, const HullSet& hs) {
    return distancePairBody<true>(A, V3(), V3(), triangle, hs);
}

// ---- kernels
// what a query is: the volume (rows of k_ov_prepare) and the largest distance it reports
struct DistanceQuery { OverlapVolume q; float maxD; bool valid; };

__device__ __forceinline__ DistanceQuery dsLoadQuery(const float4* __restrict__ vShape, const float4* __restrict__ vMin, const float4* __restrict__ vMax, const uint32_t* __restrict__ vRange,
                                                    const float* __restrict__ maxDistances, uint32_t v, uint32_t include) {
    DistanceQuery d;
    d.q = ovLoadVolume(vShape, vMin, vMax, vRange, v, include);
    d.maxD = maxDistances ? maxDistances[v] : __uint_as_float(0x7F800000u);
    d.valid = d.q.valid && d.maxD >= 0.f;   // (a NaN fails the test)
    return d;
}
// The gap of the volume's world AABB and the box [a, b]: a lower bound of the distance of what the two boxes hold; 0 when they touch.
__device__ __forceinline__ V3 dsBoxGapVector(const OverlapVolume& q, V3 a, V3 b) {
    return V3(qmax(qmax(a.x - q.mx.x, q.mn.x - b.x), 0.f), qmax(qmax(a.y - q.mx.y, q.mn.y - b.y), 0.f), qmax(qmax(a.z - q.mx.z, q.mn.z - b.z), 0.f));
}
// THE distance a pair reports: the pair test's, raised to the boxes' gap (both are the true distance up to rounding; the gap is what candidates and
// shells are skipped by).  A pair the search calls touching while the boxes are apart (by roundings: the search's tolerance) is NOT an overlap:
// it reports the gap, so nothing that was skipped by a smaller bound could have beaten it.
__device__ __forceinline__ float dsResolve(const DistanceResult& r, float boxGap, uint32_t& flags) {
    flags = r.flags;
    if ((r.flags & kDistanceOverlap) && boxGap > 0.f) flags = 0u;
    return (flags & kDistanceOverlap) ? 0.f : qmax(r.distance, boxGap);
}
// THE candidate test: collider k against the query -> key = distance bits << 32 | k, or ~0.  ovAdmit (object type, entity range, a finite AABB),
// the boxes' gap (kSkip: a candidate whose gap lies strictly above `limit` = min(best distance so far, max_distance) cannot win), the pair test.
template <bool kSkip> __device__ inline unsigned long long dsCandidate(const OverlapScene& s, const DistanceQuery& d, uint32_t k, float limit) {
    float4 a, b; uint32_t tag;
    if (!ovAdmit(s, d.q, k, a, b, tag)) return ~0ull;
    const float boxGap = len(dsBoxGapVector(d.q, xyz(a), xyz(b)));
    if (kSkip && boxGap > limit) return ~0ull;
    const DistanceResult r = distancePair(d.q.s, d.q.mn, d.q.mx, loadShape(s.shape, k, tag & 0xFFu), s.hs);
    uint32_t flags;
    const float dist = dsResolve(r, boxGap, flags);
    if (!(dist <= d.maxD) || !qFinite(dist)) return ~0ull;   // (coordinates whose distance overflows: a miss)
    return ((unsigned long long)__float_as_uint(dist + 0.f) << 32) | k;
}
// THE record writer (one lane): the winner's pair test once more (it depends on the pair alone: the same bits); a miss is all zeros behind row 0
// but for the query's index; touching shapes report the volume's pose position twice and no direction.
__device__ inline void dsFinalise(const OverlapScene& s, const DistanceQuery& d, unsigned long long key, float4 pose, uint32_t v, uint4* __restrict__ out) {
    uint4 row0 = make_uint4(kRayMiss, kRayMiss, 0x7F800000u /* +inf */, 0u);
    V3 pc, pv, n; uint32_t flags = 0u;
    if (key != ~0ull) {
        const uint32_t col = (uint32_t)key;
        const float4 a = s.mn[col], b = s.mx[col];
        const uint32_t tag = __float_as_uint(a.w);
        row0 = make_uint4(s.cEntity[col], col, (uint32_t)(key >> 32), (tag >> 8) & 0xFFu);
        const V3 gap = dsBoxGapVector(d.q, xyz(a), xyz(b));
        const float boxGap = len(gap);
        const DistanceResult r = distancePair(d.q.s, d.q.mn, d.q.mx, loadShape(s.shape, col, tag & 0xFFu), s.hs);
        dsResolve(r, boxGap, flags);
        if (flags & kDistanceOverlap) { pc = pv = V3(pose.x, pose.y, pose.z); }
        else if (r.flags & kDistanceOverlap) {
            // (touching by the search, apart by the boxes: the boxes' gap, between the volume's box and its clamp towards the collider's)
            const V3 sign(xyz(a).x > d.q.mx.x ? -1.f : 1.f, xyz(a).y > d.q.mx.y ? -1.f : 1.f, xyz(a).z > d.q.mx.z ? -1.f : 1.f);
            n = V3(gap.x * sign.x, gap.y * sign.y, gap.z * sign.z) * (1.f / boxGap);
            pv = vmin(qvmax(d.q.mn * 0.5f + d.q.mx * 0.5f, xyz(a)), xyz(b)); pv = vmin(qvmax(pv, d.q.mn), d.q.mx);
            pc = pv - n * boxGap;
        } else { pc = r.pointCollider; pv = r.pointVolume; n = r.normal; }
    }
    uint4* rec = out + kDistanceRecordRows * (size_t)v;
    rec[0] = row0;
    rec[1] = make_uint4(__float_as_uint(pc.x), __float_as_uint(pc.y), __float_as_uint(pc.z), flags);
    rec[2] = make_uint4(__float_as_uint(pv.x), __float_as_uint(pv.y), __float_as_uint(pv.z), v);
    rec[3] = make_uint4(__float_as_uint(n.x), __float_as_uint(n.y), __float_as_uint(n.z), 0u);
}
// the wave's best key so far as the limit of the candidates to come: its distance (never above max_distance), or max_distance while nothing is found
__device__ __forceinline__ float dsLimit(unsigned long long key, float maxD) {
    const unsigned long long m = swWaveMin(key);
    return m != ~0ull ? __uint_as_float((uint32_t)(m >> 32)) : maxD;
}

// A lower bound of the distance from the volume's AABB to every collider the grid holds OUTSIDE the cell box [lo - r, hi + r] (rings 0 .. r), from
// the box's world coordinates: the smallest over the six sides of the side's plane to the AABB's far face, less a relative padding (kSwPad's kind,
// and the insertion margin on top: a collider wholly beyond cell c on an axis has its AABB beyond the cell's plane by the margin it was
// inserted with, up to a rounding of the cell arithmetic).  A side at the grid's border has nothing beyond it: cells are clamped to the grid.
// +inf: the box covers the grid.
__device__ __forceinline__ float dsShellBound(const QueryGrid& g, const OverlapVolume& q, const uint32_t lo[3], const uint32_t hi[3], uint32_t r) {
    const float mn[3] = {q.mn.x, q.mn.y, q.mn.z}, mx[3] = {q.mx.x, q.mx.y, q.mx.z}, o[3] = {g.minX, g.minY, g.minZ};
    const uint32_t dim[3] = {g.dimX, g.dimY, g.dimZ};
    float bound = __uint_as_float(0x7F800000u);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        if (hi[i] + r + 1u < dim[i]) {
            const float plane = o[i] + (float)(hi[i] + r + 1u) * g.cell;
            bound = fminr(bound, qmax(plane - mx[i] - kSwPad * (fabsf(plane) + fabsf(mx[i]) + fabsf(o[i]) + 1.f), 0.f));
        }
        if (lo[i] > r) {
            const float plane = o[i] + (float)(lo[i] - r) * g.cell;
            bound = fminr(bound, qmax(mn[i] - plane - kSwPad * (fabsf(plane) + fabsf(mn[i]) + fabsf(o[i]) + 1.f), 0.f));
        }
    }
    return bound;
}

// ---- accelerated: one wave per volume.  Ring r = the cells at Chebyshev cell distance r from the volume's clamped cell range [lo, hi].  A
// collider (cells [klo, khi], qCellRange, which inserted it) is found in ring max_i max(0, klo_i - hi_i, lo_i - khi_i) and only there, from the entry
// in cell max(klo_i, lo_i - r) per axis, which lies on that ring's shell: each collider once.  The cells of one x row are neighbours in `entries`,
// so the lanes stride over the span of a row: the whole row inside the box where y or z lies on the shell's boundary (and in ring 0), its two
// end cells elsewhere.
__device__ __forceinline__ unsigned long long dsSpan(const OverlapScene& s, const DistanceQuery& d, const QueryGrid& g, const uint32_t lo[3], const uint32_t hi[3], uint32_t r,
                                                     uint32_t row, uint32_t x0, uint32_t x1, uint32_t y, uint32_t z, const uint32_t* __restrict__ start,
                                                     const uint32_t* __restrict__ entries, uint32_t lane, unsigned long long best, float& limit) {
    const uint32_t e0 = start[row + x0], e1 = start[row + x1 + 1u];
    for (uint32_t eb = e0; eb < e1; eb += 64u) {
        const uint32_t e = eb + lane;
        if (e < e1) {
            const uint32_t k = entries[e];
            uint32_t klo[3], khi[3];
            if (qCellRange(g, s.mn[k], s.mx[k], klo, khi)) {
                uint32_t ring = 0u, cell[3];
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    if (klo[i] > hi[i]) ring = max(ring, klo[i] - hi[i]);
                    if (lo[i] > khi[i]) ring = max(ring, lo[i] - khi[i]);
                    cell[i] = max(klo[i], lo[i] > r ? lo[i] - r : 0u);
                }
                if (ring == r && cell[1] == y && cell[2] == z) {
                    const uint32_t c = row + cell[0];
                    if (start[c] <= e && e < start[c + 1u]) best = min(best, dsCandidate<true>(s, d, k, limit));
                }
            }
        }
        limit = dsLimit(best, d.maxD);
    }
    return best;
}
__global__ __launch_bounds__(64 * kOvWaves) void k_q_distance(uint32_t count, uint32_t include, OverlapScene s, const float4* __restrict__ vShape, const float4* __restrict__ vMin,
                                                             const float4* __restrict__ vMax, const uint32_t* __restrict__ vRange, const float4* __restrict__ vPos,
                                                             const float* __restrict__ maxDistances, const QueryGrid* __restrict__ grid, const uint32_t* __restrict__ start,
                                                             const uint32_t* __restrict__ entries, const uint32_t* __restrict__ large, uint4* __restrict__ out) {
    const uint32_t lane = threadIdx.x & 63u, v = blockIdx.x * kOvWaves + (threadIdx.x >> 6);
    if (v >= count) return;
    const DistanceQuery d = dsLoadQuery(vShape, vMin, vMax, vRange, maxDistances, v, include);
    unsigned long long best = ~0ull;
    if (d.valid) {
        const QueryGrid g = *grid;
        uint32_t lo[3], hi[3];
        float limit = d.maxD;
        if (ovCellRange(g, d.q, lo, hi)) {
            const uint32_t nl = g.numLarge;
            for (uint32_t i0 = 0; i0 < nl; i0 += 64u) {
                const uint32_t i = i0 + lane;
                if (i < nl) best = min(best, dsCandidate<true>(s, d, large[i], limit));
                limit = dsLimit(best, d.maxD);
            }
            const uint32_t rings = max(g.dimX, max(g.dimY, g.dimZ));
            for (uint32_t r = 0; r < rings; ++r) {
                const uint32_t z0 = lo[2] > r ? lo[2] - r : 0u, z1 = min(hi[2] + r, g.dimZ - 1u), y0 = lo[1] > r ? lo[1] - r : 0u, y1 = min(hi[1] + r, g.dimY - 1u);
                const uint32_t x0 = lo[0] > r ? lo[0] - r : 0u, x1 = min(hi[0] + r, g.dimX - 1u);
                const bool lowX = lo[0] >= r, highX = hi[0] + r < g.dimX;   // the shell's two x faces lie inside the grid
                for (uint32_t z = z0; z <= z1; ++z)
                    for (uint32_t y = y0; y <= y1; ++y) {
                        const uint32_t row = (z * g.dimY + y) * g.dimX;
                        const bool whole = r == 0u || z + r == lo[2] || z == hi[2] + r || y + r == lo[1] || y == hi[1] + r;
                        if (whole) best = dsSpan(s, d, g, lo, hi, r, row, x0, x1, y, z, start, entries, lane, best, limit);
                        else {
                            if (lowX) best = dsSpan(s, d, g, lo, hi, r, row, x0, x0, y, z, start, entries, lane, best, limit);
                            if (highX) best = dsSpan(s, d, g, lo, hi, r, row, x1, x1, y, z, start, entries, lane, best, limit);
                        }
                    }
                if (dsShellBound(g, d.q, lo, hi, r) > limit) break;   // (+inf once the box covers the grid; a limit of +inf with nothing found ends there too)
                if (x0 == 0u && y0 == 0u && z0 == 0u && x1 == g.dimX - 1u && y1 == g.dimY - 1u && z1 == g.dimZ - 1u) break;
            }
        } else {
            for (uint32_t k0 = 0; k0 < s.nc; k0 += 64u) {
                const uint32_t k = k0 + lane;
                if (k < s.nc) best = min(best, dsCandidate<true>(s, d, k, limit));
                limit = dsLimit(best, d.maxD);
            }
        }
    }
    best = swWaveMin(best);
    if (lane == 0u) dsFinalise(s, d, best, vPos[v], v, out);
}

// ---- exhaustive: one wave per volume over every collider, no grid, no skipping; the rows in `s` are computed for the call, not taken from the cache
__global__ __launch_bounds__(64 * kOvWaves) void k_q_distance_exhaustive(uint32_t count, uint32_t include, OverlapScene s, const float4* __restrict__ vShape, const float4* __restrict__ vMin,
                                                                        const float4* __restrict__ vMax, const uint32_t* __restrict__ vRange, const float4* __restrict__ vPos,
                                                                        const float* __restrict__ maxDistances, uint4* __restrict__ out) {
    const uint32_t lane = threadIdx.x & 63u, v = blockIdx.x * kOvWaves + (threadIdx.x >> 6);
    if (v >= count) return;
    const DistanceQuery d = dsLoadQuery(vShape, vMin, vMax, vRange, maxDistances, v, include);
    unsigned long long best = ~0ull;
    if (d.valid)
        for (uint32_t k = lane; k < s.nc; k += 64u) best = min(best, dsCandidate<false>(s, d, k, 0.f));
    best = swWaveMin(best);
    if (lane == 0u) dsFinalise(s, d, best, vPos[v], v, out);
}

}  // namespace mi
