// kernels_sweep.hpp — batched shape-cast (sweep) scene queries (mi_world_sweep*, include/mi_physics.h): the first collider a sphere, capsule,
// cylinder, box or hull touches when it is moved along a displacement, with the time, the point and the normal.  Part of the ONE translation
// unit of the physics library (world.hip includes it after kernels_overlap.hpp, whose volume rows and grid it uses).  Host side: world_query.inc.
//
// Read-only with respect to the step: everything here reads query-owned rows and writes the caller's records.
//   sweepPair             the pair test: a convex cast in the relative frame (van den Bergen's GJK ray cast against the Minkowski difference
//                         collider - volume), spheres and capsules as a point / segment core plus a radius margin; sweepTrianglePair: the same
//                         body against a terrain triangle (three vertices, no margin)
//   k_q_sweep             one wave per cast: the lanes stride over the entries of the grid cells the SWEPT AABB overlaps, then over the large
//                         list; a cast over many cells strides over all colliders instead; a candidate whose conservative entry time lies
//                         behind the wave's best time so far is skipped
//   k_q_sweep_exhaustive  the yardstick: every collider for every cast, rows computed for the call, nothing skipped
//   k_q_sweep_terrain     the heightmap's collision triangles (MI_QUERY_TERRAIN), launched behind k_q_sweep: one wave per cast walks the aligned
//                         8 x 8-cell blocks under the swept AABB, block row by block row in the direction of travel, culled by the min/max mips
//   k_q_sweep_terrain_exhaustive  behind k_q_sweep_exhaustive: every triangle of every chunk that has heights, no mips, nothing skipped
// Both kernels decide through swCandidate (admission: kernels_overlap.hpp's ovAdmit, shared with the overlap predicate) and write through swFinalise:
// the same winner key (t bits << 32 | collider) gives the same bytes.  The terrain kernels likewise: swTerrainCandidate (key = t bits << 32 | triangle),
// swTerrainFinalise, which merges with the colliders' record.  Colliders and terrain share the candidate tail (swCandidateKey: slab test, skip, pair
// test, key) and the record tail (swWriteRecord: point and normal of an initial overlap, the three rows).
// No atomics, no dependence between workgroups; every loop is bounded by a constant, the collider count or the grid.
#pragma once
#include "kernels_overlap.hpp"

namespace mi {

constexpr uint32_t kSweepMaxIter = 32;        // iterations of the pair test; a pair that reaches it reports its (lower-bound) t with kSweepUnconverged
constexpr uint32_t kSweepInitialOverlap = 1u, kSweepUnconverged = 2u;   // MI_SWEEP_*
constexpr float kSweepTolRel = 2e-6f;         // touching = closer than this times the largest coordinate seen (a few float32 ulps of the support points)
constexpr float kSweepStallTol = 16.f;        // a search that has STALLED (see sweepPair) counts as touching within this many tolerances (stalls of rounding alone measured up to 4)
constexpr uint32_t kSweepRecordRows = 3;      // mi_sweep_hit: three rows of 16 bytes
constexpr int kSwTriangle = T_HULL + 1;       // a terrain triangle as the pair test's collider: vertices a, b and rot's x, y, z; this file's alone, never stored in a world row
constexpr float kSwPad = 1e-5f;               // relative padding of the candidates' slab test
constexpr float kSwCullPad = 2e-5f;           // ... of a box that stands for several candidates: at least the padding of every box inside it (|a| + |b| of an inner interval is at most twice the outer one's)

// ---- the pair test
struct SweepResult { bool hit; float t; V3 normal, point; uint32_t flags; };

// Support point of a shape's CORE along dir (any length, zero included: some point of the core, never NaN).  Spheres and capsules are their
// centre / segment (the radius is the margin); cylinders, boxes and hulls are the whole shape.
__device__ inline V3 swSupport(const Shape& s, const HullSet& hs, V3 dir) {
    switch (s.type) {
        case T_SPHERE: return s.a;
        case T_CAPSULE: return dot(dir, s.a - s.b) > 0.f ? s.a : s.b;
        case T_CYLINDER: {
            const V3 ax = s.b - s.a, far = dot(dir, ax) < 0.f ? s.a : s.b;
            const float aa = sqlen(ax);
            V3 perp = aa > 0.f ? dir - ax * (dot(dir, ax) / aa) : dir;
            // once more: under a dir nearly along the axis (a cap flat on something) the short remainder keeps rounding error ALONG the axis of the order
            // of 1e-7 |dir|, which the scaling to the radius blows up: the "rim" point then lies off the cap's plane by radius x 1e-7 |dir| / |perp|
            // (measured: a cylinder of radius 6 reported its touch 5.6e-3 past the true one).  The second pass leaves 1e-7 |perp|.
            if (aa > 0.f) perp = perp - ax * (dot(perp, ax) / aa);
            const float pl = sqlen(perp);
            return pl > 1e-12f * sqlen(dir) ? far + perp * (s.radius / sqrtf(pl)) : far;   // (dir along the axis, or too short to square: the cap's centre)
        }
        case T_AABB: return V3(dir.x < 0.f ? s.a.x : s.b.x, dir.y < 0.f ? s.a.y : s.b.y, dir.z < 0.f ? s.a.z : s.b.z);
        case T_OBB: {
            const V3 l = rotate(conj(s.rot), dir);
            return s.a + rotate(s.rot, V3(l.x < 0.f ? -s.b.x : s.b.x, l.y < 0.f ? -s.b.y : s.b.y, l.z < 0.f ? -s.b.z : s.b.z));
        }
        default: {
            const V3 l = rotate(conj(s.rot), dir);
            const uint32_t first = hs.ranges[2 * s.hull], count = hs.ranges[2 * s.hull + 1];
            V3 best; float maxD = -FLT_MAX;
            for (uint32_t i = 0; i < count; ++i) {
                const float4 q = hs.verts[first + i]; const V3 v(q.x, q.y, q.z);
                const float d = dot(l, v);
                if (d > maxD) { maxD = d; best = v; }
            }
            return s.a + rotate(s.rot, best);
        }
    }
}
// ... and of a terrain triangle (type kSwTriangle: vertices a, b and rot's x, y, z; no margin).  Not a case of the switch above: the pair test of the world's
// shapes is compiled without it (as a seventh case it cost the sixteen-cell casts of tools/bench_sweep.py 0.7 %, measured), the terrain has an instance of its own.
__device__ __forceinline__ V3 swTriangleSupport(const Shape& s, V3 dir) {
    const V3 c(s.rot.x, s.rot.y, s.rot.z);
    const float da = dot(dir, s.a), db = dot(dir, s.b), dc = dot(dir, c);
    return da >= db ? (da >= dc ? s.a : c) : (db >= dc ? s.b : c);
}
template <bool kTriangle> __device__ __forceinline__ V3 swColliderSupport(const Shape& s, const HullSet& hs, V3 dir) {
    if (kTriangle) return swTriangleSupport(s, dir);
    return swSupport(s, hs, dir);
}
__device__ __forceinline__ float swMargin(const Shape& s) { return s.type <= T_CAPSULE ? s.radius : 0.f; }
__device__ __forceinline__ float swMaxAbs(V3 a) { return qmax(fabsf(a.x), qmax(fabsf(a.y), fabsf(a.z))); }

// The simplex: up to four points of the Minkowski difference (collider - volume) with their witnesses on the collider, in named slots (no runtime
// indexing: it stays in registers).
struct SwSimplex { V3 y0, y1, y2, y3, b0, b1, b2, b3; uint32_t n; };
struct SwWeights { float w0, w1, w2, w3; };

// closest point of the triangle (a, b, c) to the origin as barycentric weights (Ericson, Real-Time Collision Detection 5.1.5; every quotient guarded) and
// the point itself; in the interior the point is the origin's projection along the triangle's normal, not the weighted sum: its DIRECTION is then exact
// however far apart the vertices lie (the weighted sum of large vertices cancels down to a short vector with the vertices' rounding error)
__device__ inline void swTriangleWeights(V3 a, V3 b, V3 c, float& u, float& v, float& w, bool& interior) {
    interior = false;
    const V3 ab = b - a, ac = c - a;
    const float d1 = -dot(ab, a), d2 = -dot(ac, a);
    if (d1 <= 0.f && d2 <= 0.f) { u = 1.f; v = 0.f; w = 0.f; return; }
    const float d3 = -dot(ab, b), d4 = -dot(ac, b);
    if (d3 >= 0.f && d4 <= d3) { u = 0.f; v = 1.f; w = 0.f; return; }
    const float vc = d1 * d4 - d3 * d2;
    if (vc <= 0.f && d1 >= 0.f && d3 <= 0.f) { const float den = d1 - d3; v = den > 0.f ? d1 / den : 0.f; u = 1.f - v; w = 0.f; return; }
    const float d5 = -dot(ab, c), d6 = -dot(ac, c);
    if (d6 >= 0.f && d5 <= d6) { u = 0.f; v = 0.f; w = 1.f; return; }
    const float vb = d5 * d2 - d1 * d6;
    if (vb <= 0.f && d2 >= 0.f && d6 <= 0.f) { const float den = d2 - d6; w = den > 0.f ? d2 / den : 0.f; u = 1.f - w; v = 0.f; return; }
    const float va = d3 * d6 - d5 * d4;
    if (va <= 0.f && (d4 - d3) >= 0.f && (d5 - d6) >= 0.f) { const float den = (d4 - d3) + (d5 - d6); w = den > 0.f ? (d4 - d3) / den : 0.f; u = 0.f; v = 1.f - w; return; }
    const float sum = va + vb + vc;
    if (!(sum > 0.f)) { u = 1.f; v = 0.f; w = 0.f; return; }   // (a triangle without area whose edges all declined: keep a vertex, the caller's next support point replaces it)
    v = vb / sum; w = vc / sum; u = 1.f - v - w; interior = true;
}
__device__ inline V3 swTriangle(V3 a, V3 b, V3 c, float& u, float& v, float& w) {
    bool interior;
    swTriangleWeights(a, b, c, u, v, w, interior);
    if (interior) {
        const V3 n = cross(b - a, c - a); const float nn = sqlen(n);
        if (nn > 0.f) return n * (dot(n, a) / nn);
    }
    return a * u + b * v + c * w;
}
// Closest point of the simplex (points p_i = x - y_i) to the origin: the weights of its vertices (0 = dropped) and the point.  false: the
// origin lies inside a proper tetrahedron (x is inside the Minkowski difference).
__device__ inline bool swClosest(uint32_t n, V3 p0, V3 p1, V3 p2, V3 p3, SwWeights& w, V3& v) {
    w.w0 = 1.f; w.w1 = w.w2 = w.w3 = 0.f;
    if (n == 1u) { v = p0; return true; }
    if (n == 2u) {
        const V3 e = p1 - p0; const float ee = sqlen(e), t = ee > 0.f ? qclamp01(-dot(p0, e) / ee) : 0.f;
        w.w0 = 1.f - t; w.w1 = t; v = p0 * w.w0 + p1 * w.w1; return true;
    }
    if (n == 3u) { v = swTriangle(p0, p1, p2, w.w0, w.w1, w.w2); return true; }
    // The closest point of the tetrahedron's surface: the nearest of its four triangles (right wherever the origin is outside).  The origin counts as
    // INSIDE only when the tetrahedron is proper, no face is a needle, and the origin lies on the inner side of every face by a clear margin; each face
    // sees its opposite vertex at the height of the one determinant `det`, so one sign serves all four.  Anything doubtful is "outside": the nearest
    // triangle then gives a distance within the noise of zero, which ends the search just as well.
    const V3 nrm = cross(p1 - p0, p2 - p0);
    const float det = dot(p3 - p0, nrm);
    bool inside = det * det > 1e-6f * sqlen(nrm) * sqlen(p3 - p0);
    float bestD = FLT_MAX;
    v = V3();
#define MI_SW_FACE(A, B, C, WA, WB, WC, WO)                                                                   \
    {                                                                                                         \
        const V3 e1 = B - A, e2 = C - A, fn = cross(e1, e2);                                                  \
        const float ff = sqlen(fn), sp = -dot(A, fn);   /* the origin's height over the face, times |fn| */  \
        if (!(ff > 1e-6f * sqlen(e1) * sqlen(e2)) || !(sp * det > 0.f) || !(sp * sp > 1e-8f * ff * sqlen(A))) inside = false; \
        float fu, fv, fw;                                                                                     \
        const V3 c = swTriangle(A, B, C, fu, fv, fw); const float dd = sqlen(c);                              \
        if (dd < bestD) { bestD = dd; v = c; w.WA = fu; w.WB = fv; w.WC = fw; w.WO = 0.f; }                   \
    }
    MI_SW_FACE(p0, p1, p2, w0, w1, w2, w3)
    MI_SW_FACE(p0, p2, p3, w0, w2, w3, w1)
    MI_SW_FACE(p0, p3, p1, w0, w3, w1, w2)
    MI_SW_FACE(p1, p3, p2, w1, w3, w2, w0)
#undef MI_SW_FACE
    return !inside;
}
__device__ __forceinline__ void swPush(SwSimplex& s, V3 y, V3 b) {
    if (s.n == 0u) { s.y0 = y; s.b0 = b; } else if (s.n == 1u) { s.y1 = y; s.b1 = b; } else if (s.n == 2u) { s.y2 = y; s.b2 = b; } else { s.y3 = y; s.b3 = b; }
    ++s.n;
}

// A box collider cut down to the neighbourhood of the cast: its part inside the cast's swept AABB (sweptMin, sweptMax: the union of the volume's AABB at
// t = 0 and t = 1), grown by a margin; an OBB is cut in its own frame by the swept AABB's bounds there.  The volume touches the collider only inside its
// swept AABB, so time, point and normal are those of the whole box (a plane that supports a convex shape near the touching point supports all of it), but
// the simplex of a ground box a hundred units wide no longer has vertices a hundred units apart: float32 keeps its closest point.
__device__ inline Shape swClipBox(const Shape& b, V3 sweptMin, V3 sweptMax) {
    if (b.type != T_AABB && b.type != T_OBB) return b;
    const V3 ext = sweptMax - sweptMin;
    const float grow = 0.05f * qmax(ext.x, qmax(ext.y, ext.z)) + 1e-3f;
    Shape r = b;
    if (b.type == T_AABB) {
        const V3 lo = qvmax(b.a, sweptMin - V3(grow)), hi = vmin(b.b, sweptMax + V3(grow));
        if (lo.x <= hi.x && lo.y <= hi.y && lo.z <= hi.z) { r.a = lo; r.b = hi; }   // (apart: the pair test says so on the whole box)
        return r;
    }
    // the swept AABB's centre and half-extents in the box's frame: |R^T| applied to the half-extents
    const V3 c = rotate(conj(b.rot), (sweptMin + sweptMax) * 0.5f - b.a), h = ext * 0.5f + V3(grow);
    const V3 ex = vabs(rotate(conj(b.rot), V3(h.x, 0.f, 0.f))), ey = vabs(rotate(conj(b.rot), V3(0.f, h.y, 0.f))), ez = vabs(rotate(conj(b.rot), V3(0.f, 0.f, h.z)));
    const V3 e = ex + ey + ez;
    const V3 lo = qvmax(-b.b, c - e), hi = vmin(b.b, c + e);
    if (lo.x <= hi.x && lo.y <= hi.y && lo.z <= hi.z) { r.a = b.a + rotate(b.rot, (lo + hi) * 0.5f); r.b = (hi - lo) * 0.5f; }
    return r;
}

// THE pair test.  Volume A keeps its orientation and moves by t * d, t in [0, 1]; collider B stands still.  A(t) touches B when t * d reaches
// C = B - A, so the cast is the ray x = t * d from the origin against C (the cores' difference, grown by both margins R): x advances only by
// clipping against support planes of C (every clip is safe: t never passes the true time of impact), and the simplex of C's points closest to x
// ends the search once x is within R + tolerance of it.  normal: unit, from B towards A; point: on B's surface.
// Never clipped = the shapes touch at t = 0: kSweepInitialOverlap (normal and point are the caller's).  Out of iterations: the current t with
// kSweepUnconverged.  STALLED = an iteration that neither clips nor moves the closest point: its support point is one the simplex holds, or one the
// simplex takes and drops again (the closest vector comes out bit for bit the same; every further iteration would repeat it).  In exact arithmetic
// that happens only at distance <= R, so what is left of the distance is rounding: a cast that never clipped stays an initial overlap (no plane
// separates the shapes; the distance plays no part), any other ends converged within kSweepStallTol tolerances (degenerate touches end here:
// parallel faces and edges, a cap flat on a face) and with kSweepUnconverged beyond them (measured: a box of 1e-2 on the side of a cylinder of
// radius 15 stalls 42 tolerances = 2.5e-3 short of the touch, on a thin triangle of far-apart points of the curved side).
// The result depends on (A, B, d) alone; one body (not inlined) serves the candidate test and the record writer of both kernels.
// kTriangle: the collider is a terrain triangle (sweepTrianglePair below); everything but its support function is the same code.
template <bool kTriangle> __device__ __forceinline__ SweepResult sweepPairBody(const Shape& A, V3 sweptMin, V3 sweptMax, const Shape& collider, const HullSet& hs, V3 d) {
    SweepResult r; r.hit = false; r.t = 0.f; r.flags = 0u;
    const Shape B = swClipBox(collider, sweptMin, sweptMax);
    const float R = swMargin(A) + swMargin(B);
    float lambda = 0.f, scale = 1.f;
    V3 x, n, witness, v = swSupport(A, hs, V3()) - swColliderSupport<kTriangle>(B, hs, V3());   // (from some point of B to some point of A)
    if (sqlen(v) == 0.f) v = V3(1.f, 0.f, 0.f);
    bool clipped = false, done = false;
    SwSimplex s; s.n = 0u;
    float dist2 = FLT_MAX, tol = 0.f;
    for (uint32_t it = 0; it < kSweepMaxIter && !done; ++it) {
        const V3 pb = swColliderSupport<kTriangle>(B, hs, v), pa = swSupport(A, hs, -v), p = pb - pa;
        scale = qmax(scale, qmax(swMaxAbs(pa), swMaxAbs(pb)));
        tol = kSweepTolRel * qmax(scale, R);
        const float lv = len(v), vw = dot(v, x - p) - R * lv;
        const bool clip = vw > 0.f;
        if (clip) {   // the plane through C's support point along v separates x from C: clip the ray against it
            const float vd = dot(v, d);
            if (vd >= 0.f) return r;   // moving along or away from it: a miss
            lambda = lambda - vw / vd;
            if (!(lambda <= 1.f)) return r;   // (t is a lower bound: the touch lies behind the end of the displacement; coordinates that overflowed into a NaN are a miss too)
            x = d * lambda; n = v; clipped = true;
        }
        // a support point the simplex already holds brings nothing new: the search has stalled unless this iteration clipped
        const bool dup = (s.n > 0u && p.x == s.y0.x && p.y == s.y0.y && p.z == s.y0.z) || (s.n > 1u && p.x == s.y1.x && p.y == s.y1.y && p.z == s.y1.z) ||
                         (s.n > 2u && p.x == s.y2.x && p.y == s.y2.y && p.z == s.y2.z) || (s.n > 3u && p.x == s.y3.x && p.y == s.y3.y && p.z == s.y3.z);
        const float stallR = R + kSweepStallTol * tol;
        if (dup && !clip) { done = !clipped || dist2 <= stallR * stallR; break; }
        if (!dup) swPush(s, p, pb);   // (at most three points were kept: a proper tetrahedron ended the search, a flat one kept a face)
        SwWeights w;
        const V3 before = v;
        const bool outside = swClosest(s.n, x - s.y0, x - s.y1, x - s.y2, x - s.y3, w, v);
        if (!outside) { v = V3(); dist2 = 0.f; done = true; break; }
        witness = s.b0 * w.w0;
        if (s.n > 1u) witness = witness + s.b1 * w.w1;
        if (s.n > 2u) witness = witness + s.b2 * w.w2;
        if (s.n > 3u) witness = witness + s.b3 * w.w3;
        // keep the vertices that carry the closest point
        SwSimplex k; k.n = 0u;
        if (w.w0 > 0.f) swPush(k, s.y0, s.b0);
        if (s.n > 1u && w.w1 > 0.f) swPush(k, s.y1, s.b1);
        if (s.n > 2u && w.w2 > 0.f) swPush(k, s.y2, s.b2);
        if (s.n > 3u && w.w3 > 0.f) swPush(k, s.y3, s.b3);
        if (k.n == 0u) swPush(k, s.y0, s.b0);
        s = k;
        dist2 = sqlen(v);
        done = dist2 <= (R + tol) * (R + tol);
        if (!done && !clip && v.x == before.x && v.y == before.y && v.z == before.z) { done = !clipped || dist2 <= stallR * stallR; break; }   // (took the point and dropped it again)
    }
    r.hit = true; r.t = lambda;
    if (!done) r.flags |= kSweepUnconverged;
    if (!clipped) { r.flags |= kSweepInitialOverlap; r.t = 0.f; return r; }
    // round pairs end at distance R from the cores: x - closest is the exact contact normal; flat pairs end at distance 0: the last clip plane's
    const V3 dir = (R > 0.f && dist2 > 0.25f * R * R) ? v : n;
    r.normal = dir * (1.f / len(dir));
    r.point = witness + r.normal * swMargin(B);
    return r;
}
__device__ __noinline__ SweepResult sweepPair(const Shape& A, V3 sweptMin, V3 sweptMax, const Shape& collider, const HullSet& hs, V3 d) {
    return sweepPairBody<false>(A, sweptMin, sweptMax, collider, hs, d);
}
// ... against a terrain triangle (swTerrainShape): one body (not inlined) for the candidate test and the record writer of both terrain kernels
__device__ __noinline__ SweepResult sweepTrianglePair(const Shape& A, V3 sweptMin, V3 sweptMax, const Shape& triangle, const HullSet& hs, V3 d) {
    return sweepPairBody<true>(A, sweptMin, sweptMax, triangle, hs, d);
}

// The overlap query's pair test (declared in kernels_overlap.hpp): the cast by a zero displacement.  No plane can be clipped against, so the search
// ends at the first support plane that separates the shapes by more than the margins (apart) or once the distance is within tolerance of the
// margins, has stalled or has run out of iterations (touching: nothing separated them; measured on the pair matrix of tests/overlap_matrix.py:
// shapes up to 4.7e-5 of their largest coordinate apart end this way, overlapping shapes never end as apart).  The same body as the casts': on
// the pairs that come here a cast's initial-overlap flag and the overlap query agree by construction.
__device__ bool swOverlaps(const Shape& volume, V3 volumeMin, V3 volumeMax, const Shape& collider, const HullSet& hs) {
    return sweepPair(volume, volumeMin, volumeMax, collider, hs, V3()).hit;
}

// ---- kernels
// what a cast is: the volume (rows of k_ov_prepare), its displacement, the swept bounds
struct SweepCast { OverlapVolume q; V3 d, centre, half, sweptMin, sweptMax; bool valid; };

__device__ __forceinline__ SweepCast swLoadCast(const float4* __restrict__ vShape, const float4* __restrict__ vMin, const float4* __restrict__ vMax, const uint32_t* __restrict__ vRange,
                                               const float4* __restrict__ disp, uint32_t v, uint32_t include) {
    SweepCast c;
    c.q = ovLoadVolume(vShape, vMin, vMax, vRange, v, include);
    const float4 d4 = disp[v];
    c.d = V3(d4.x, d4.y, d4.z);
    c.centre = c.q.mn * 0.5f + c.q.mx * 0.5f; c.half = c.q.mx * 0.5f - c.q.mn * 0.5f;   // (halved first: bounds near FLT_MAX must not overflow into an infinite centre)
    const V3 end = c.q.mx + c.d, begin = c.q.mn + c.d;
    c.sweptMin = vmin(c.q.mn, begin); c.sweptMax = qvmax(c.q.mx, end);
    c.valid = c.q.valid && qFinite(c.d.x) && qFinite(c.d.y) && qFinite(c.d.z) && qFinite(end.x) && qFinite(end.y) && qFinite(end.z) && qFinite(begin.x) && qFinite(begin.y) && qFinite(begin.z);
    return c;
}
// the swept AABB (the union of the volume's AABB at t = 0 and at t = 1) as the volume the grid helpers take
__device__ __forceinline__ OverlapVolume swSweptBounds(const SweepCast& c) {
    OverlapVolume q = c.q;
    q.mn = c.sweptMin; q.mx = c.sweptMax;
    return q;
}
// One axis of the slab test: the displacement from the volume's centre o against the interval [ca, cb] grown by the volume's half-extent and a relative padding.
__device__ __forceinline__ bool swSlabAxis(float o, float half, float d, float ca, float cb, float padRel, float& t0, float& t1) {
    const float lo = ca - half - o, hi = cb + half - o;
    const float pad = padRel * (fabsf(o) + fabsf(ca) + fabsf(cb) + 1.f);
    const float l = lo - pad, h = hi + pad;
    if (d == 0.f) return !(l > 0.f || h < 0.f);
    const float ta = l / d, tb = h / d; t0 = qmax(t0, fminr(ta, tb)); t1 = fminr(t1, qmax(ta, tb));
    return true;
}
// The slab test of a cast against the box [a, b]: false = the swept volume's AABB never meets it; t0 = the conservative entry time in [0, 1].
__device__ __forceinline__ bool swSlab(const SweepCast& c, V3 a, V3 b, float padRel, float& t0) {
    float t1 = 1.f; t0 = 0.f;
    if (!swSlabAxis(c.centre.x, c.half.x, c.d.x, a.x, b.x, padRel, t0, t1)) return false;
    if (!swSlabAxis(c.centre.y, c.half.y, c.d.y, a.y, b.y, padRel, t0, t1)) return false;
    if (!swSlabAxis(c.centre.z, c.half.z, c.d.z, a.z, b.z, padRel, t0, t1)) return false;
    return t0 <= t1 && qFinite(t1);
}
// THE candidate tail of colliders and terrain triangles: the candidate's box [mn, mx], its index in the key and `pair()`, its pair test (sweepPair or
// sweepTrianglePair) -> key = t bits << 32 | index, or ~0.  The slab test of the displacement against the box grown by the volume's half-extents (a
// conservative entry time; padded by a few ulps), then the pair test.  The reported t is never below the entry time (both are lower bounds of the
// true time), so with kSkip a candidate whose entry lies strictly behind bestT cannot win and is not evaluated.
template <bool kSkip, class Pair> __device__ __forceinline__ unsigned long long swCandidateKey(const SweepCast& c, V3 mn, V3 mx, uint32_t index, float bestT, Pair pair) {
    float t0;
    if (!swSlab(c, mn, mx, kSwPad, t0)) return ~0ull;
    if (kSkip && t0 > bestT) return ~0ull;
    const SweepResult r = pair();
    if (!r.hit) return ~0ull;
    const float t = (r.flags & kSweepInitialOverlap) ? 0.f : qmax(r.t, t0);
    return ((unsigned long long)__float_as_uint(t + 0.f) << 32) | index;
}
// THE candidate test: collider k against the cast -> key = t bits << 32 | k, or ~0.  ovAdmit (object type, entity range, a finite AABB), then the tail.
template <bool kSkip> __device__ inline unsigned long long swCandidate(const OverlapScene& s, const SweepCast& c, uint32_t k, float bestT) {
    float4 a, b; uint32_t tag;
    if (!ovAdmit(s, c.q, k, a, b, tag)) return ~0ull;
    return swCandidateKey<kSkip>(c, xyz(a), xyz(b), k, bestT, [&] { return sweepPair(c.q.s, c.sweptMin, c.sweptMax, loadShape(s.shape, k, tag & 0xFFu), s.hs, c.d); });
}
__device__ __forceinline__ unsigned long long swWaveMin(unsigned long long key) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)key, off, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(key >> 32), off, 64);
        const unsigned long long other = ((unsigned long long)hi << 32) | lo;
        if (other < key) key = other;
    }
    return key;
}
// THE record tail (one lane) of colliders and terrain: row 0 is the caller's (who was hit, at what t); a cast that starts in touch reports the volume's
// position and the reversed direction of travel, any other the pair test's point and normal; three rows of 16 bytes
__device__ __forceinline__ void swWriteRecord(const SweepCast& c, const SweepResult& r, uint4 row0, float4 pose, uint32_t v, uint4* out) {
    V3 p = r.point, n = r.normal;
    const float dl = len(c.d);
    if (r.flags & kSweepInitialOverlap) { p = V3(pose.x, pose.y, pose.z); n = dl > 0.f ? c.d * (-1.f / dl) : V3(); }
    out[kSweepRecordRows * (size_t)v] = row0;
    out[kSweepRecordRows * (size_t)v + 1] = make_uint4(__float_as_uint(p.x), __float_as_uint(p.y), __float_as_uint(p.z), r.flags);
    out[kSweepRecordRows * (size_t)v + 2] = make_uint4(__float_as_uint(n.x), __float_as_uint(n.y), __float_as_uint(n.z), v);
}
// THE record writer (one lane): the winner's pair test once more (it depends on the pair alone: the same bits), then the tail; a miss is all zeros behind row 0
__device__ inline void swFinalise(const OverlapScene& s, const SweepCast& c, unsigned long long key, float4 pose, uint32_t v, uint4* __restrict__ out) {
    uint4 row0 = make_uint4(kRayMiss, kRayMiss, 0x7F800000u /* +inf */, 0u);
    SweepResult r{};   // (a miss: no flags, point and normal zero)
    if (key != ~0ull) {
        const uint32_t col = (uint32_t)key, tag = __float_as_uint(s.mn[col].w);
        row0 = make_uint4(s.cEntity[col], col, (uint32_t)(key >> 32), (tag >> 8) & 0xFFu);
        r = sweepPair(c.q.s, c.sweptMin, c.sweptMax, loadShape(s.shape, col, tag & 0xFFu), s.hs, c.d);
    }
    swWriteRecord(c, r, row0, pose, v, out);
}
__device__ __forceinline__ float swBestT(unsigned long long key) { return __uint_as_float((uint32_t)(swWaveMin(key) >> 32)); }   // (~0: a NaN pattern, nothing is "behind" it)

// ---- accelerated: one wave per cast over the grid cells of the swept AABB (the dedup rule of ovGridWalk: a collider is taken from the entry in the
// lowest cell of the intersection of its range with the cast's), then the large list; or the stride over all colliders.  The walk is written out here
// and in ovGridWalk: as one enumerator with a visitor, and the rows and the grid passed as two structs, it cost the one-cell casts of
// tools/bench_sweep.py 7 % at unchanged registers and occupancy (profiles/query_device_walk_ab.txt).
__global__ __launch_bounds__(64 * kOvWaves) void k_q_sweep(uint32_t count, uint32_t include, OverlapScene s, const float4* __restrict__ vShape, const float4* __restrict__ vMin,
                                                          const float4* __restrict__ vMax, const uint32_t* __restrict__ vRange, const float4* __restrict__ vPos,
                                                          const float4* __restrict__ disp, const QueryGrid* __restrict__ grid, const uint32_t* __restrict__ start,
                                                          const uint32_t* __restrict__ entries, const uint32_t* __restrict__ large, uint4* __restrict__ out) {
    const uint32_t lane = threadIdx.x & 63u, v = blockIdx.x * kOvWaves + (threadIdx.x >> 6);
    if (v >= count) return;
    const SweepCast c = swLoadCast(vShape, vMin, vMax, vRange, disp, v, include);
    unsigned long long best = ~0ull;
    if (c.valid) {
        const QueryGrid g = *grid;
        const OverlapVolume swept = swSweptBounds(c);
        uint32_t lo[3], hi[3];
        float bestT = __uint_as_float(0x7F800000u);
        if (ovCellRange(g, swept, lo, hi)) {
            for (uint32_t z = lo[2]; z <= hi[2]; ++z)
                for (uint32_t y = lo[1]; y <= hi[1]; ++y) {
                    const uint32_t row = (z * g.dimY + y) * g.dimX;
                    const uint32_t e0 = start[row + lo[0]], e1 = start[row + hi[0] + 1u];
                    for (uint32_t eb = e0; eb < e1; eb += 64u) {
                        const uint32_t e = eb + lane;
                        if (e < e1) {
                            const uint32_t k = entries[e];
                            uint32_t klo[3], khi[3];
                            if (qCellRange(g, s.mn[k], s.mx[k], klo, khi) && max(klo[1], lo[1]) == y && max(klo[2], lo[2]) == z) {
                                const uint32_t cell = row + max(klo[0], lo[0]);
                                if (start[cell] <= e && e < start[cell + 1u]) best = min(best, swCandidate<true>(s, c, k, bestT));
                            }
                        }
                        bestT = swBestT(best);
                    }
                }
            const uint32_t nl = g.numLarge;
            for (uint32_t i0 = 0; i0 < nl; i0 += 64u) {
                const uint32_t i = i0 + lane;
                if (i < nl) best = min(best, swCandidate<true>(s, c, large[i], bestT));
                bestT = swBestT(best);
            }
        } else {
            for (uint32_t k0 = 0; k0 < s.nc; k0 += 64u) {
                const uint32_t k = k0 + lane;
                if (k < s.nc) best = min(best, swCandidate<true>(s, c, k, bestT));
                bestT = swBestT(best);
            }
        }
    }
    best = swWaveMin(best);
    if (lane == 0u) swFinalise(s, c, best, vPos[v], v, out);
}

// ---- exhaustive: one wave per cast over every collider, no grid, no skipping; the rows in `s` are computed for the call, not taken from the cache
__global__ __launch_bounds__(64 * kOvWaves) void k_q_sweep_exhaustive(uint32_t count, uint32_t include, OverlapScene s, const float4* __restrict__ vShape, const float4* __restrict__ vMin,
                                                                     const float4* __restrict__ vMax, const uint32_t* __restrict__ vRange, const float4* __restrict__ vPos,
                                                                     const float4* __restrict__ disp, uint4* __restrict__ out) {
    const uint32_t lane = threadIdx.x & 63u, v = blockIdx.x * kOvWaves + (threadIdx.x >> 6);
    if (v >= count) return;
    const SweepCast c = swLoadCast(vShape, vMin, vMax, vRange, disp, v, include);
    unsigned long long best = ~0ull;
    if (c.valid)
        for (uint32_t k = lane; k < s.nc; k += 64u) best = min(best, swCandidate<false>(s, c, k, 0.f));
    best = swWaveMin(best);
    if (lane == 0u) swFinalise(s, c, best, vPos[v], v, out);
}

// ---- the terrain (MI_QUERY_TERRAIN): the heightmap's collision triangles, (A, B, C) and (C, B, D) of every cell of a chunk that has heights, what the
// ray cast hits (qTerrainCellVertices); two-sided surfaces without volume.  A launch of its own behind the collider kernel, whose record it merges with:
// k_q_sweep stays what it is, a world without terrain pays nothing; a terrain hit does not prune the collider pass this way.
// The rule of qTerrainIncluded (the host launches these kernels only for a world with a heightmap)
__device__ __forceinline__ bool swTerrainIncluded(const SweepCast& c) {
    return c.valid && (c.q.include & kQueryTerrain) && kRayTerrain >= c.q.lo && kRayTerrain < c.q.hi;
}
// a vertex coordinate along x or z in hmVertex's arithmetic (the same bits): vertex v (0..128) of chunk `chunk`
__device__ __forceinline__ float swTerrainCoord(const HeightmapParams& hm, uint32_t chunk, uint32_t v, float mapMin) {
    return (float)v * hm.chunkScale + ((float)chunk * hm.chunkSize + mapMin);
}
__device__ __forceinline__ float swTerrainHeight(const HeightmapParams& hm, uint32_t h) { return (float)h * hm.heightScale + (0.f + hm.minY); }
// triangle `tri` of cell (gx, gz) (of a chunk that has heights) as sweepTrianglePair's collider, loaded as qTerrainCellVertices loads it
__device__ __forceinline__ Shape swTerrainShape(const HeightmapParams& hm, uint32_t gx, uint32_t gz, uint32_t tri) {
    const uint32_t cx = gx >> 7, cz = gz >> 7, qx = gx & 127u, qz = gz & 127u;
    const uint16_t* heights = hm.heights + (size_t)hm.chunkSlot[cz * hm.chunksPerDim + cx] * kHmVerts * kHmVerts;
    const V3 chunkMin = V3((float)cx * hm.chunkSize, 0.f, (float)cz * hm.chunkSize) + V3(hm.minX, hm.minY, hm.minZ);
    const V3 b = hmVertex(hm, heights, chunkMin, qx, qz + 1u), c = hmVertex(hm, heights, chunkMin, qx + 1u, qz);
    const V3 e = tri ? hmVertex(hm, heights, chunkMin, qx + 1u, qz + 1u) : hmVertex(hm, heights, chunkMin, qx, qz);
    Shape s; s.type = kSwTriangle; s.radius = 0.f; s.hull = 0u;
    s.a = tri ? c : e; s.b = b;
    const V3 third = tri ? e : c;
    s.rot = Q4(third.x, third.y, third.z, 0.f);
    return s;
}
// THE terrain candidate test: the candidate tail on the triangle's AABB with sweepTrianglePair -> key = t bits << 32 | (gz * n + gx) * 2 + tri, or ~0
template <bool kSkip> __device__ inline unsigned long long swTerrainCandidate(const HeightmapParams& hm, const HullSet& hs, const SweepCast& c, uint32_t gx, uint32_t gz,
                                                                             uint32_t tri, float bestT) {
    const Shape T = swTerrainShape(hm, gx, gz, tri);
    const V3 third(T.rot.x, T.rot.y, T.rot.z);
    return swCandidateKey<kSkip>(c, vmin(vmin(T.a, T.b), third), qvmax(qvmax(T.a, T.b), third), (gz * (hm.chunksPerDim * kHmSegs) + gx) * 2u + tri, bestT,
                                 [&] { return sweepTrianglePair(c.q.s, c.sweptMin, c.sweptMax, T, hs, c.d); });
}
// THE terrain record writer (one lane): merges with the record the collider kernel wrote for this cast — the terrain replaces it only when that is a miss or
// its t is strictly greater (as float bits: both are non-negative), so a collider wins a tie —, then the winner's pair test once more and the record tail
__device__ inline void swTerrainFinalise(const HeightmapParams& hm, const HullSet& hs, const SweepCast& c, unsigned long long key, float4 pose, uint32_t v, uint4* out) {
    if (key == ~0ull) return;
    const uint32_t tBits = (uint32_t)(key >> 32), index = (uint32_t)key, n = hm.chunksPerDim * kHmSegs;
    const uint4 have = out[kSweepRecordRows * (size_t)v];
    if (have.x != kRayMiss && !(have.z > tBits)) return;
    const uint32_t cell = index >> 1;
    const SweepResult r = sweepTrianglePair(c.q.s, c.sweptMin, c.sweptMax, swTerrainShape(hm, cell % n, cell / n, index & 1u), hs, c.d);
    swWriteRecord(c, r, make_uint4(kRayTerrain, kRayTerrain, tBits, OBJ_STATIC), pose, v, out);
}

// ---- exhaustive: one wave per cast, the lanes over every triangle (32 cells of one row at a time: one chunk), nothing skipped
__global__ __launch_bounds__(64 * kOvWaves) void k_q_sweep_terrain_exhaustive(uint32_t count, uint32_t include, HeightmapParams hm, HullSet hs, const float4* __restrict__ vShape,
                                                                             const float4* __restrict__ vMin, const float4* __restrict__ vMax, const uint32_t* __restrict__ vRange,
                                                                             const float4* __restrict__ vPos, const float4* __restrict__ disp, uint4* out) {
    const uint32_t lane = threadIdx.x & 63u, v = blockIdx.x * kOvWaves + (threadIdx.x >> 6);
    if (v >= count) return;
    const SweepCast c = swLoadCast(vShape, vMin, vMax, vRange, disp, v, include);
    if (!swTerrainIncluded(c)) return;
    const uint32_t n = hm.chunksPerDim * kHmSegs;
    unsigned long long best = ~0ull;
    for (uint32_t gz = 0; gz < n; ++gz)
        for (uint32_t gx0 = 0; gx0 < n; gx0 += 32u) {
            if (hm.chunkSlot[(gz >> 7) * hm.chunksPerDim + (gx0 >> 7)] == 0xFFFFFFFFu) continue;
            best = min(best, swTerrainCandidate<false>(hm, hs, c, gx0 + (lane >> 1), gz, lane & 1u, 0.f));
        }
    best = swWaveMin(best);
    if (lane == 0u) swTerrainFinalise(hm, hs, c, best, vPos[v], v, out);
}

// ---- accelerated: one wave per cast.  bestT starts at the t of the colliders' record.  The cells under the XZ footprint of the swept AABB (padded, clipped to the
// map) are walked in aligned 8 x 8 blocks, block row by block row along the dominant horizontal axis of the displacement in the direction of travel; a lane
// takes a block of the row (its box: the block's extent and the height range of mip level 3), the 64 lanes then the 64 cells of every surviving block (mip level 0).
// Every culling box contains the padded box of every triangle it stands for (the same vertex arithmetic, kSwCullPad), so its entry time is a lower bound
// of theirs: what is dropped lies strictly behind bestT or is never met, and the winner is the exhaustive kernel's.  The walk ends at the first block row
// entered behind bestT along the dominant axis (monotone along the walk).  Every loop is bounded by the map's dimensions.
__global__ __launch_bounds__(64 * kOvWaves) void k_q_sweep_terrain(uint32_t count, uint32_t include, HeightmapParams hm, HullSet hs, const float4* __restrict__ vShape,
                                                                  const float4* __restrict__ vMin, const float4* __restrict__ vMax, const uint32_t* __restrict__ vRange,
                                                                  const float4* __restrict__ vPos, const float4* __restrict__ disp, uint4* out) {
    const uint32_t lane = threadIdx.x & 63u, v = blockIdx.x * kOvWaves + (threadIdx.x >> 6);
    if (v >= count) return;
    const SweepCast c = swLoadCast(vShape, vMin, vMax, vRange, disp, v, include);
    if (!swTerrainIncluded(c)) return;
    const uint4 have = out[kSweepRecordRows * (size_t)v];
    float bestT = have.x == kRayMiss ? __uint_as_float(0x7F800000u) : __uint_as_float(have.z);
    const uint32_t n = hm.chunksPerDim * kHmSegs;
    // the footprint in cells, [lo, hi] per horizontal axis
    uint32_t cellLo[2], cellHi[2];
    const float mapMin[2] = {hm.minX, hm.minZ}, sMin[2] = {c.sweptMin.x, c.sweptMin.z}, sMax[2] = {c.sweptMax.x, c.sweptMax.z};
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        const float mapMax = mapMin[a] + (float)hm.chunksPerDim * hm.chunkSize;
        const float pad = kSwCullPad * (qmax(fabsf(sMin[a]), fabsf(sMax[a])) + 2.f * qmax(fabsf(mapMin[a]), fabsf(mapMax)) + 1.f);
        const float fl = (sMin[a] - pad - mapMin[a]) / hm.chunkScale, fh = (sMax[a] + pad - mapMin[a]) / hm.chunkScale;
        if (!(fh >= 0.f) || !(fl <= (float)n)) return;   // beside the map
        cellLo[a] = (uint32_t)fminr(qmax(floorf(fl), 0.f), (float)(n - 1u));
        cellHi[a] = (uint32_t)fminr(qmax(floorf(fh), 0.f), (float)(n - 1u));
    }
    const bool domX = fabsf(c.d.x) >= fabsf(c.d.z);
    const int u = domX ? 0 : 1, w = 1 - u;   // the dominant axis and the other one (0 = x, 1 = z)
    const float dU = domX ? c.d.x : c.d.z, oU = domX ? c.centre.x : c.centre.z, halfU = domX ? c.half.x : c.half.z;
    const uint32_t uLo = cellLo[u] >> 3, uHi = cellHi[u] >> 3, wLo = cellLo[w] >> 3, wHi = cellHi[w] >> 3;
    const uint32_t* __restrict__ mips = hm.mips;
    unsigned long long best = ~0ull;
    for (uint32_t r = 0; r <= uHi - uLo; ++r) {
        const uint32_t bu = dU < 0.f ? uHi - r : uLo + r;
        if (dU != 0.f) {
            float t0 = 0.f, t1 = 1.f;
            swSlabAxis(oU, halfU, dU, swTerrainCoord(hm, bu >> 4, (bu & 15u) * 8u, mapMin[u]), swTerrainCoord(hm, bu >> 4, (bu & 15u) * 8u + 8u, mapMin[u]), kSwCullPad, t0, t1);
            if (t0 > bestT || t0 > 1.f) break;
        }
        for (uint32_t w0 = wLo; w0 <= wHi; w0 += 64u) {
            const uint32_t bw = w0 + lane;
            bool alive = bw <= wHi;
            if (alive) {
                const uint32_t bx = domX ? bu : bw, bz = domX ? bw : bu;
                const uint32_t slot = hm.chunkSlot[(bz >> 4) * hm.chunksPerDim + (bx >> 4)];
                alive = slot != 0xFFFFFFFFu;
                if (alive) {
                    const uint32_t mm = mips[(size_t)slot * kHmMipEntries + hmMipOffset(3u) + (bz & 15u) * (kHmSegs >> 3) + (bx & 15u)];
                    const V3 mn(swTerrainCoord(hm, bx >> 4, (bx & 15u) * 8u, hm.minX), swTerrainHeight(hm, mm & 0xFFFFu), swTerrainCoord(hm, bz >> 4, (bz & 15u) * 8u, hm.minZ));
                    const V3 mx(swTerrainCoord(hm, bx >> 4, (bx & 15u) * 8u + 8u, hm.minX), swTerrainHeight(hm, mm >> 16), swTerrainCoord(hm, bz >> 4, (bz & 15u) * 8u + 8u, hm.minZ));
                    float t0;
                    alive = swSlab(c, mn, mx, kSwCullPad, t0) && !(t0 > bestT);
                }
            }
            for (unsigned long long m = __ballot(alive); m; m &= m - 1ull) {
                const uint32_t bs = w0 + (uint32_t)__ffsll((long long)m) - 1u;
                const uint32_t bx = domX ? bu : bs, bz = domX ? bs : bu;
                const uint32_t gx = bx * 8u + (lane & 7u), gz = bz * 8u + (lane >> 3);
                if (gx >= cellLo[0] && gx <= cellHi[0] && gz >= cellLo[1] && gz <= cellHi[1]) {
                    const uint32_t slot = hm.chunkSlot[(gz >> 7) * hm.chunksPerDim + (gx >> 7)];
                    const uint32_t mm = mips[(size_t)slot * kHmMipEntries + (gz & 127u) * kHmSegs + (gx & 127u)];
                    const V3 mn(swTerrainCoord(hm, gx >> 7, gx & 127u, hm.minX), swTerrainHeight(hm, mm & 0xFFFFu), swTerrainCoord(hm, gz >> 7, gz & 127u, hm.minZ));
                    const V3 mx(swTerrainCoord(hm, gx >> 7, (gx & 127u) + 1u, hm.minX), swTerrainHeight(hm, mm >> 16), swTerrainCoord(hm, gz >> 7, (gz & 127u) + 1u, hm.minZ));
                    float t0;
                    if (swSlab(c, mn, mx, kSwCullPad, t0) && !(t0 > bestT)) {
                        best = min(best, swTerrainCandidate<true>(hm, hs, c, gx, gz, 0u, bestT));
                        best = min(best, swTerrainCandidate<true>(hm, hs, c, gx, gz, 1u, bestT));
                    }
                }
                const float tb = swBestT(best);
                if (tb < bestT) bestT = tb;
            }
        }
    }
    best = swWaveMin(best);
    if (lane == 0u) swTerrainFinalise(hm, hs, c, best, vPos[v], v, out);
}

}  // namespace mi
