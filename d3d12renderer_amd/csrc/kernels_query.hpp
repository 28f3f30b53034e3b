// kernels_query.hpp — batched ray-cast scene queries (mi_world_raycast*, include/mi_physics.h): closest hit with point and normal.
// Part of the ONE translation unit of the physics library (world.hip includes it after gjk.hpp and heightmap.hpp, whose ray and
// terrain helpers it uses).  Host side: world_query.inc.
//
// Read-only with respect to the step: everything here writes query-owned buffers only (QueryCache in world.hip).
//   k_q_colliders   one lane per collider: world AABB at the current poses (worldCollider's math, into the query's own rows), extent partials
//   k_q_mean, k_q_filter, k_q_params   cell size from the collider extents, bounds, grid dimensions (all on the device: no read-back)
//   k_q_count       one lane per collider: cells its (inflated) AABB overlaps, or the large list
//   k_exclusive_scan  cell starts
//   k_q_scatter     one lane per collider: collider index into every cell it overlaps
//   k_q_raycast     one lane per ray: 3D DDA over the cells, the large list, the terrain (2D DDA, min/max of every cell), finalisation
//   k_q_exhaustive  one workgroup per ray over every collider (the yardstick), the terrain without the min/max test, finalisation
// Both ray kernels end in qFinalise: the same winner key gives the same bytes.
#pragma once
#include "kernels.hpp"
#include "gjk.hpp"
#include "heightmap.hpp"

namespace mi {

constexpr uint32_t kQMaxCellsPerCollider = 32;   // a collider overlapping more cells goes to the large list (every ray tests it)
constexpr uint32_t kQParamThreads = 1024;
constexpr uint32_t kRayMiss = 0xFFFFFFFFu, kRayTerrain = 0xFFFFFFFEu;
constexpr uint32_t kQueryRigid = 1u, kQueryStatic = 2u, kQueryTerrain = 4u, kQueryTriggers = 8u, kQueryForceFields = 16u;

struct QueryGrid {
    float minX, minY, minZ, cell, invCell, margin, largeExtent, pad;
    uint32_t dimX, dimY, dimZ, numCells, numLarge, pad1, pad2, pad3;
};

__device__ __forceinline__ bool qFinite(float v) { return fabsf(v) <= FLT_MAX; }

// The queries' own arithmetic (grids, slabs, the sweep's tolerances) restates no reference code: its max keeps the second argument when
// the two do not compare (a NaN, zeros of opposite sign), whatever dmath.hpp's fmaxr, which follows the reference's template, returns.
__device__ __forceinline__ float qmax(float a, float b) { return a > b ? a : b; }
__device__ __forceinline__ float qclamp01(float v) { return fminr(1.f, qmax(0.f, v)); }
__device__ __forceinline__ V3 qvmax(V3 a, V3 b) { return V3(qmax(a.x, b.x), qmax(a.y, b.y), qmax(a.z, b.z)); }

__device__ __forceinline__ float qExtent(float4 mn, float4 mx) {
    if (!(qFinite(mn.x) && qFinite(mn.y) && qFinite(mn.z) && qFinite(mx.x) && qFinite(mx.y) && qFinite(mx.z))) return -1.f;
    return qmax(mx.x - mn.x, qmax(mx.y - mn.y, mx.z - mn.z));
}

// Grid parameters: cell size = the mean extent of the colliders no larger than 4 x the mean extent of all; bounds = those colliders'
// AABBs, grown by twice the insertion margin; the cell grows until the grid has at most maxCells cells.  Two reductions over all
// colliders, each as per-workgroup partials (k_q_colliders, k_q_filter) summed by one workgroup (k_q_mean, k_q_params) in a fixed order:
// the same grid for the same poses.
struct QPartial { float sum, cnt, mnx, mny, mnz, mxx, mxy, mxz; };
__device__ __forceinline__ QPartial qEmptyPartial() { QPartial p; p.sum = p.cnt = 0.f; p.mnx = p.mny = p.mnz = FLT_MAX; p.mxx = p.mxy = p.mxz = -FLT_MAX; return p; }
__device__ __forceinline__ void qCombine(QPartial& a, const QPartial& b) {
    a.sum += b.sum; a.cnt += b.cnt;
    a.mnx = fminr(a.mnx, b.mnx); a.mny = fminr(a.mny, b.mny); a.mnz = fminr(a.mnz, b.mnz);
    a.mxx = qmax(a.mxx, b.mxx); a.mxy = qmax(a.mxy, b.mxy); a.mxz = qmax(a.mxz, b.mxz);
}
// tree reduction of one partial per thread (blockDim.x a power of two, <= kQParamThreads); the result in sP[0]
__device__ __forceinline__ void qBlockReduce(QPartial* sP, QPartial mine) {
    const uint32_t tid = threadIdx.x;
    sP[tid] = mine;
    __syncthreads();
    for (uint32_t st = blockDim.x / 2; st > 0; st >>= 1) { if (tid < st) qCombine(sP[tid], sP[tid + st]); __syncthreads(); }
}

__global__ __launch_bounds__(256) void k_q_colliders(uint32_t nc, ColliderRows rows /* the world's colliders at the current poses -> the query's rows */, QPartial* __restrict__ partA) {
    __shared__ QPartial sP[256];
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    QPartial p = qEmptyPartial();
    if (k < nc) {
        float4 mn, mx;
        worldCollider<false>(k, rows, mn, mx);
        const float e = qExtent(mn, mx);
        if (e >= 0.f) { p.sum = e; p.cnt = 1.f; }
    }
    qBlockReduce(sP, p);
    if (threadIdx.x == 0) partA[blockIdx.x] = sP[0];
}
// one workgroup: the mean extent of all colliders -> the large-collider threshold
__global__ __launch_bounds__(kQParamThreads) void k_q_mean(uint32_t numPartials, const QPartial* __restrict__ partA, QueryGrid* __restrict__ g) {
    __shared__ QPartial sP[kQParamThreads];
    QPartial p = qEmptyPartial();
    for (uint32_t i = threadIdx.x; i < numPartials; i += kQParamThreads) qCombine(p, partA[i]);
    qBlockReduce(sP, p);
    if (threadIdx.x == 0) { QueryGrid q{}; q.largeExtent = sP[0].cnt > 0.f ? 4.f * (sP[0].sum / sP[0].cnt) : 0.f; *g = q; }
}
// per workgroup: extent sum, count and bounds of the colliders no larger than the threshold
__global__ __launch_bounds__(256) void k_q_filter(uint32_t nc, const float4* __restrict__ qMin, const float4* __restrict__ qMax, const QueryGrid* __restrict__ g, QPartial* __restrict__ partB) {
    __shared__ QPartial sP[256];
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    const float largeExtent = g->largeExtent;
    QPartial p = qEmptyPartial();
    if (k < nc) {
        const float4 a = qMin[k], b = qMax[k];
        const float e = qExtent(a, b);
        if (e >= 0.f && e <= largeExtent) { p.sum = e; p.cnt = 1.f; p.mnx = a.x; p.mny = a.y; p.mnz = a.z; p.mxx = b.x; p.mxy = b.y; p.mxz = b.z; }
    }
    qBlockReduce(sP, p);
    if (threadIdx.x == 0) partB[blockIdx.x] = sP[0];
}
__global__ __launch_bounds__(kQParamThreads) void k_q_params(uint32_t numPartials, uint32_t maxCells, const QPartial* __restrict__ partB, QueryGrid* __restrict__ g) {
    __shared__ QPartial sP[kQParamThreads];
    QPartial p = qEmptyPartial();
    for (uint32_t i = threadIdx.x; i < numPartials; i += kQParamThreads) qCombine(p, partB[i]);
    qBlockReduce(sP, p);
    if (threadIdx.x != 0) return;
    const QPartial r = sP[0];
    QueryGrid q{};
    q.largeExtent = g->largeExtent;
    if (r.cnt > 0.f) {
        float cell = qmax(r.sum / r.cnt, 1e-3f);
        const V3 lo(r.mnx, r.mny, r.mnz), hi(r.mxx, r.mxy, r.mxz);
        const float scale = qmax(qmax(fabsf(lo.x), fabsf(hi.x)), qmax(qmax(fabsf(lo.y), fabsf(hi.y)), qmax(fabsf(lo.z), fabsf(hi.z))));
        for (int it = 0; it < 64; ++it) {
            const float margin = 2e-3f * cell + 4e-6f * scale;
            const V3 ext = hi - lo + V3(4.f * margin);
            const float dx = qmax(1.f, ceilf(ext.x / cell)), dy = qmax(1.f, ceilf(ext.y / cell)), dz = qmax(1.f, ceilf(ext.z / cell));
            const double cells = (double)dx * (double)dy * (double)dz;
            if (cells > (double)maxCells) { cell *= qmax(1.01f, (float)cbrt(cells / (double)maxCells) * 1.01f); continue; }
            q.minX = lo.x - 2.f * margin; q.minY = lo.y - 2.f * margin; q.minZ = lo.z - 2.f * margin;
            q.cell = cell; q.invCell = 1.f / cell; q.margin = margin;
            q.dimX = (uint32_t)dx; q.dimY = (uint32_t)dy; q.dimZ = (uint32_t)dz; q.numCells = q.dimX * q.dimY * q.dimZ;
            break;
        }
    }
    *g = q;
}

// the cells a collider is inserted into (false: it belongs to the large list); the same answer in the count and the scatter pass
__device__ __forceinline__ bool qCellRange(const QueryGrid& g, float4 mn, float4 mx, uint32_t lo[3], uint32_t hi[3]) {
    const float e = qExtent(mn, mx);
    if (!(e >= 0.f) || e > g.largeExtent || g.numCells == 0u) return false;
    const float a[3] = {mn.x, mn.y, mn.z}, b[3] = {mx.x, mx.y, mx.z}, o[3] = {g.minX, g.minY, g.minZ};
    const uint32_t dim[3] = {g.dimX, g.dimY, g.dimZ};
    uint32_t cells = 1u;
    for (int i = 0; i < 3; ++i) {
        const float l = floorf((a[i] - g.margin - o[i]) * g.invCell), h = floorf((b[i] + g.margin - o[i]) * g.invCell);
        lo[i] = (uint32_t)fminr(qmax(l, 0.f), (float)(dim[i] - 1u)); hi[i] = (uint32_t)fminr(qmax(h, 0.f), (float)(dim[i] - 1u));
        cells *= hi[i] - lo[i] + 1u;
        if (cells > kQMaxCellsPerCollider) return false;
    }
    return true;
}

__global__ __launch_bounds__(256) void k_q_count(uint32_t nc, const float4* __restrict__ qMin, const float4* __restrict__ qMax, QueryGrid* __restrict__ g,
                                                 uint32_t* __restrict__ count, uint32_t* __restrict__ large) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nc) return;
    const QueryGrid q = *g;
    uint32_t lo[3], hi[3];
    if (!qCellRange(q, qMin[k], qMax[k], lo, hi)) { large[atomicAdd(&g->numLarge, 1u)] = k; return; }
    for (uint32_t z = lo[2]; z <= hi[2]; ++z)
        for (uint32_t y = lo[1]; y <= hi[1]; ++y)
            for (uint32_t x = lo[0]; x <= hi[0]; ++x) atomicAdd(&count[(z * q.dimY + y) * q.dimX + x], 1u);
}

// `cursor` = the counts, cleared by the scan: the slots of a cell are handed out in any order (the ray kernel's result does not depend on it)
__global__ __launch_bounds__(256) void k_q_scatter(uint32_t nc, const float4* __restrict__ qMin, const float4* __restrict__ qMax, const QueryGrid* __restrict__ g,
                                                   const uint32_t* __restrict__ start, uint32_t* __restrict__ cursor, uint32_t* __restrict__ entries) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nc) return;
    const QueryGrid q = *g;
    uint32_t lo[3], hi[3];
    if (!qCellRange(q, qMin[k], qMax[k], lo, hi)) return;
    for (uint32_t z = lo[2]; z <= hi[2]; ++z)
        for (uint32_t y = lo[1]; y <= hi[1]; ++y)
            for (uint32_t x = lo[0]; x <= hi[0]; ++x) {
                const uint32_t c = (z * q.dimY + y) * q.dimX + x;
                entries[start[c] + atomicAdd(&cursor[c], 1u)] = k;
            }
}

// ---- what a ray sees
struct QueryScene {
    uint32_t nc;
    const uint32_t* cTypeBody; const uint32_t* cObject; const uint32_t* cEntity;
    const float4* cShape; const float4* cStaticPos; const float4* cStaticRot;
    const float4* bPos; const float4* bRot;
    HullFaces hf;
    HeightmapParams hm; uint32_t hasTerrain;
};
struct QueryRay { V3 o, d; float maxT; uint32_t lo, hi, include; bool valid; };

__device__ __forceinline__ QueryRay qLoadRay(const float* __restrict__ rays, const uint32_t* __restrict__ ranges, uint32_t r, uint32_t include) {
    QueryRay q;
    const float4 a = reinterpret_cast<const float4*>(rays)[2 * r], b = reinterpret_cast<const float4*>(rays)[2 * r + 1];
    q.o = V3(a.x, a.y, a.z); q.d = V3(a.w, b.x, b.y); q.maxT = b.z;
    q.lo = ranges ? ranges[2 * r] : 0u; q.hi = ranges ? ranges[2 * r + 1] : 0xFFFFFFFFu; q.include = include;
    q.valid = qFinite(q.o.x) && qFinite(q.o.y) && qFinite(q.o.z) && qFinite(q.d.x) && qFinite(q.d.y) && qFinite(q.d.z) &&
              (q.d.x != 0.f || q.d.y != 0.f || q.d.z != 0.f) && q.maxT >= 0.f;   // (a NaN max_t fails the last test)
    return q;
}
__device__ __forceinline__ uint32_t qObjectType(const QueryScene& s, uint32_t k, uint32_t body) { return body != kNoBody ? (uint32_t)OBJ_RIGID_BODY : (s.cObject[k] & 0xFFu); }
__device__ __forceinline__ uint32_t qFlagOf(uint32_t objType) {
    return objType == OBJ_RIGID_BODY ? kQueryRigid : objType == OBJ_STATIC ? kQueryStatic : objType == OBJ_TRIGGER ? kQueryTriggers : kQueryForceFields;
}
__device__ __forceinline__ void qPose(const QueryScene& s, uint32_t k, uint32_t body, V3& pos, Q4& rot) {
    if (body != kNoBody) { pos = xyz(s.bPos[body]); rot = toQ(s.bRot[body]); }
    else { pos = xyz(s.cStaticPos[k]); rot = toQ(s.cStaticRot[k]); }
}
// rayVsCollider with t in the units of any direction.  Only the slab test of the boxes is homogeneous in d; the reference's other tests are
// written for |d| = 1: raySphere outright, rayCylinder through its absolute epsilons (delta = b^2 - a c scales with |d|^2 r^2, `t <= epsilon`
// is a distance only for a unit ray), rayPlane and rayTriangle through `|dot(d, n)| < 1e-6`.  So spheres, capsules, cylinders and hulls run
// on d / |d| and their t is divided by |d|.  A direction whose length rounds to exactly 1 takes rayVsCollider's arithmetic unchanged (so unit
// rays see the t mi_world_test_interactions sees).
__device__ __forceinline__ V3 qUnitDirection(V3 d, float& l) { l = len(d); return l == 1.f ? d : d * (1.f / l); }
// rayTriangle with the plane's normal normalised whatever its length: the reference's noz() returns the zero vector for a cross product
// shorter than 1e-4, so a triangle with edges under about 1e-2 was invisible to every ray.  The same arithmetic, hence the same t, for
// every triangle rayTriangle sees.
__device__ inline bool qRayTriangle(V3 o, V3 d, V3 a, V3 b, V3 c, float& t) {
    const V3 cr = cross(b - a, c - a);
    const float sl = sqlen(cr);
    if (!(sl > 0.f)) return false;
    const V3 normal = cr * (1.f / sqrtf(sl));
    const float pd = -dot(normal, a), nDotR = dot(d, normal);
    if (fabsf(nDotR) <= 1e-6f) return false;
    t = -(dot(o, normal) + pd) / nDotR;
    return t >= 0.f && pointInTriangle(o + t * d, a, b, c);
}
// the hull loop of rayVsCollider over qRayTriangle: the first triangle with the smallest t, and its (unnormalised) outward normal in the hull's frame
__device__ inline bool qRayHull(float4 s0, float4 s1, const HullFaces& hf, V3 o, V3 d, float& t, V3& n) {
    const Q4 inv = conj(Q4(s0.x, s0.y, s0.z, s0.w)); const V3 pos(s1.x, s1.y, s1.z);
    const uint32_t geom = __float_as_uint(s1.w);
    const V3 lo = rotate(inv, o - pos), ld = rotate(inv, d);
    const uint32_t v0 = hf.ranges[2 * geom], f0 = hf.triRanges[2 * geom], nf = hf.triRanges[2 * geom + 1];
    float minT = FLT_MAX; bool result = false;
    for (uint32_t f = 0; f < nf; ++f) {
        float tt;
        const V3 a = xyz(hf.verts[v0 + hf.tris[3 * (f0 + f)]]), b = xyz(hf.verts[v0 + hf.tris[3 * (f0 + f) + 1]]), c = xyz(hf.verts[v0 + hf.tris[3 * (f0 + f) + 2]]);
        if (qRayTriangle(lo, ld, a, b, c, tt) && tt < minT) { minT = tt; n = cross(b - a, c - a); result = true; }
    }
    t = minT;
    return result;
}
// rayCylinder once more for a ray it missed, its comparisons of lengths (the side hit's height against [0, height], the cap hit's distance from
// the axis against the radius) widened from the absolute 1e-6 to `tol`, a few float32 roundings of the coordinates involved: at coordinates
// of about 1 a ray aimed exactly at the rim otherwise passes between side and cap, and the cap of a cylinder tens of units long is missed
// whenever o.y + t d.y rounds above height + 1e-6.  The thresholds on delta and on t stay.
__device__ inline bool qRayCylinderWidened(V3 o, V3 d, V3 pa, V3 pb, float radius, float tol, float& t) {
    const V3 axis = pb - pa;
    const float height = len(axis);
    const Q4 q = rotateFromTo(axis, V3(0.f, 1.f, 0.f));
    o = rotate(q, o - pa); d = rotate(q, d);
    const float epsilon = 1e-6f;
    float y = -1.f - tol;
    t = 0.f;
    if (o.x * o.x + o.z * o.z > radius * radius) {
        const float a = d.x * d.x + d.z * d.z, b = d.x * o.x + d.z * o.z, c = o.x * o.x + o.z * o.z - radius * radius;
        const float delta = b * b - a * c;
        if (delta < epsilon) return false;
        t = (-b - sqrtf(delta)) / a;
        if (t <= epsilon) return false;
        y = o.y + t * d.y;
    }
    if (y > height + tol || y < -tol) {
        float dist;
        if (d.y < 0.f && rayPlane(o, d, V3(0.f, 1.f, 0.f), -height, dist) && len(o + dist * d - V3(0.f, height, 0.f)) <= radius + tol) t = dist;
        if (d.y > 0.f && rayPlane(o, d, V3(0.f, -1.f, 0.f), 0.f, dist) && len(o + dist * d) <= radius + tol) t = dist;
        y = o.y + t * d.y;
    }
    return y > -tol && y < height + tol;
}
// Round shapes, in two steps the reference does not take.  (1) An origin more than 32 bounding radii in front of the shape is first moved
// along the ray to the shape's bounding sphere: the quadratics subtract r^2 from |o - c|^2, and from 20 units a collider of 1e-2 was hit 5e-3
// early or late, or missed.  (2) A cylinder the reference's test misses is tried once more with widened comparisons (above).  A unit ray that
// starts within 32 radii and that the reference's test hits sees rayVsCollider's arithmetic unchanged, to the byte.
__device__ inline bool qRayVsCollider(uint32_t type, float4 s0, float4 s1, float4 s2, const HullFaces& hf, V3 o, V3 d, float& t) {
    if (type == T_AABB || type == T_OBB) return rayVsCollider(type, s0, s1, s2, hf, o, d, t);
    float l;
    const V3 u = qUnitDirection(d, l);
    if (type == T_HULL) { V3 n; float tt; if (!qRayHull(s0, s1, hf, o, u, tt, n)) return false; t = l == 1.f ? tt : tt / l; return true; }
    V3 centre = xyz(s0); float bound = s0.w;
    if (type != T_SPHERE) { const V3 pb(s0.w, s1.x, s1.y); centre = 0.5f * (centre + pb); bound = 0.5f * len(pb - xyz(s0)) + s1.z; }
    const float ahead = dot(centre - o, u) - bound;
    const bool far = bound > 0.f && ahead > 32.f * bound;
    const V3 start = far ? o + ahead * u : o;
    float tt;
    bool hit = rayVsCollider(type, s0, s1, s2, hf, start, u, tt);
    if (!hit && type == T_CYLINDER) hit = qRayCylinderWidened(start, u, xyz(s0), V3(s0.w, s1.x, s1.y), s1.z, 2e-6f * (1.f + bound + len(start - centre)), tt);
    if (!hit) return false;
    if (far) tt += ahead;
    t = l == 1.f ? tt : tt / l;
    return true;
}
// collider k against the ray in its entity's frame (qRayVsCollider; rayVsCollider, as mi_world_test_interactions, for unit rays): key = t bits << 32 | k, or ~0
__device__ __forceinline__ unsigned long long qTestCollider(const QueryScene& s, const QueryRay& q, uint32_t k) {
    const uint32_t type = s.cTypeBody[2 * k], body = s.cTypeBody[2 * k + 1], ent = s.cEntity[k];
    if (ent < q.lo || ent >= q.hi) return ~0ull;
    if (!(q.include & qFlagOf(qObjectType(s, k, body)))) return ~0ull;
    V3 pos; Q4 rot; qPose(s, k, body, pos, rot);
    const Q4 inv = conj(rot);
    float t;
    if (!qRayVsCollider(type, s.cShape[3 * k], s.cShape[3 * k + 1], s.cShape[3 * k + 2], s.hf, rotate(inv, q.o - pos), rotate(inv, q.d), t)) return ~0ull;
    if (!(t >= 0.f && t <= q.maxT && t < FLT_MAX)) return ~0ull;   // negative / non-finite t (the cylinder test's caps can return one) = no hit
    return ((unsigned long long)__float_as_uint(t + 0.f) << 32) | k;
}

// ---- terrain: the collision triangles of heightmap.hpp, (A, B, C) and (C, B, D) of cell (qx, qz); a point on a shared edge belongs to both
// the four vertices of cell (gx, gz), of a chunk that has heights: a (qx, qz), b (qx, qz + 1), c (qx + 1, qz), e (qx + 1, qz + 1)
__device__ __forceinline__ void qTerrainCellVertices(const HeightmapParams& hm, uint32_t gx, uint32_t gz, V3& a, V3& b, V3& c, V3& e) {
    const uint32_t cx = gx >> 7, cz = gz >> 7, qx = gx & 127u, qz = gz & 127u;
    const uint16_t* heights = hm.heights + (size_t)hm.chunkSlot[cz * hm.chunksPerDim + cx] * kHmVerts * kHmVerts;
    const V3 chunkMin = V3((float)cx * hm.chunkSize, 0.f, (float)cz * hm.chunkSize) + V3(hm.minX, hm.minY, hm.minZ);
    a = hmVertex(hm, heights, chunkMin, qx, qz); b = hmVertex(hm, heights, chunkMin, qx, qz + 1u);
    c = hmVertex(hm, heights, chunkMin, qx + 1u, qz); e = hmVertex(hm, heights, chunkMin, qx + 1u, qz + 1u);
}
// the upward normal (not unit) of triangle `tri` of the cell
__device__ __forceinline__ V3 qTerrainNormal(const HeightmapParams& hm, uint32_t gx, uint32_t gz, uint32_t tri) {
    V3 a, b, c, e; qTerrainCellVertices(hm, gx, gz, a, b, c, e);
    return tri == 0u ? cross(b - a, c - a) : cross(b - c, e - c);
}
// The ray against the two triangles of cell (gx, gz), which its footprint crosses from parameter ta to tb.  Watertight by construction: the decision
// is a change of sign of the ray's height above the surface between SAMPLES, and every sample on the cell's rim is one both neighbours compute
// from the same numbers: the same t (one cell's exit is the next one's entry), the same two vertex heights, the same coordinate along the
// edge relative to the same vertex.  The cell's diagonal, where the footprint crosses it (tDiag), is sampled once for both triangles.  So a
// ray whose samples begin above the surface and end below it finds the sign change in exactly one place, whatever o + t d rounds to at
// coordinates of thousands.  Only where the ray begins (entry 0) there is no rim sample: the plane of the triangle under it is, at the
// ray's point relative to the cell's corner (the plane's height times the cell's area: only signs are compared).
// t is the crossing of the owning triangle's plane, held to that triangle's piece of [ta, tb]: never a neighbour's plane beyond a rounding
// of the rim.  A sample of exactly zero counts for both sides: an origin on the surface is a hit at t = 0.
__device__ __forceinline__ float qRayOverEdge(float oy, float dy, float r0, float dr, float s, float h0, float h1, float t) {
    const float f = qclamp01(fmaf(t, dr, r0) / s);   // along the edge from the vertex of h0; fmaf by name: no contraction to differ between two inlined copies
    return fmaf(-f, h1 - h0, fmaf(t, dy, oy - h0));
}
__device__ __forceinline__ bool qSignChange(float g0, float g1) { return (g0 <= 0.f && g1 >= 0.f) || (g0 >= 0.f && g1 <= 0.f); }
// entry: 0 the ray begins in this cell (at ta), 1 it came in through an x line, 2 through a z line; exitX: it leaves through an x line (at tb)
__device__ inline bool qRayTerrainCell(const HeightmapParams& hm, uint32_t gx, uint32_t gz, V3 o, V3 d, float ta, float tb, int entry, bool exitX, float& t, uint32_t& tri) {
    V3 a, b, c, e; qTerrainCellVertices(hm, gx, gz, a, b, c, e);
    const float s = hm.chunkScale, rx = o.x - a.x, rz = o.z - a.z;   // relative to the cell's corner before anything is multiplied
    // the footprint is on triangle 0's side of the diagonal while rx + rz + t (d.x + d.z) < s
    const float along = d.x + d.z, left = s - rx - rz;
    const uint32_t first = (along > 0.f || (along == 0.f && left >= 0.f)) ? 0u : 1u;
    const float tDiag = along != 0.f ? left / along : FLT_MAX;
    const V3 n0 = cross(b - a, c - a), n1 = cross(b - c, e - c);
    const uint32_t kA = ta < tDiag ? first : 1u - first;
    const bool lowX = d.x > 0.f, lowZ = d.z > 0.f;               // the side it comes in through; it leaves through the other
    const V3 start(fmaf(ta, d.x, rx), fmaf(ta, d.y, o.y - a.y), fmaf(ta, d.z, rz));   // the ray's point at ta from the corner, as the rim samples take it
    const float gA = entry == 0 ? (kA == 0u ? dot(start, n0) : dot(start - (c - a), n1))
                   : entry == 1 ? (lowX ? qRayOverEdge(o.y, d.y, rz, d.z, s, a.y, b.y, ta) : qRayOverEdge(o.y, d.y, rz, d.z, s, c.y, e.y, ta))
                                : (lowZ ? qRayOverEdge(o.y, d.y, rx, d.x, s, a.y, c.y, ta) : qRayOverEdge(o.y, d.y, rx, d.x, s, b.y, e.y, ta));
    const float gB = exitX ? (lowX ? qRayOverEdge(o.y, d.y, rz, d.z, s, c.y, e.y, tb) : qRayOverEdge(o.y, d.y, rz, d.z, s, a.y, b.y, tb))
                           : (lowZ ? qRayOverEdge(o.y, d.y, rx, d.x, s, b.y, e.y, tb) : qRayOverEdge(o.y, d.y, rx, d.x, s, a.y, c.y, tb));
    float lo = ta, hi = tb;
    tri = kA;
    if (tDiag > ta && tDiag < tb) {
        const float gD = qRayOverEdge(o.y, d.y, rx, d.x, s, b.y, c.y, tDiag);
        if (qSignChange(gA, gD)) hi = tDiag;
        else if (qSignChange(gD, gB)) { lo = tDiag; tri = 1u - first; }
        else return false;
    } else if (!qSignChange(gA, gB)) return false;
    const V3 p0 = tri == 0u ? a : c, n = tri == 0u ? n0 : n1;
    const float dn = dot(d, n);
    t = dn != 0.f ? dot(p0 - o, n) / dn : lo;
    if (!(t >= lo)) t = lo;
    if (t > hi) t = hi;
    return true;
}
// 2D DDA over the terrain cells from t = 0 on; ends at the first cell that holds a crossing: the ray's first, and behind tMax a miss, so which
// crossing is found does not depend on tMax.  useBounds: an 8 x 8-cell block whose height range (the mips' level 3) the ray's y range over
// the block misses by more than a tolerance is crossed without testing its cells, and so is a cell whose own range (level 0) it misses; only
// such cells are not tested, so the hit is the one the walk without them finds.  Out: t and its triangle.
__device__ inline bool qTerrainWalk(const HeightmapParams& hm, V3 o, V3 d, float tMax, bool useBounds, float& bestT, uint32_t& bestCell, uint32_t& bestTri) {
    const uint32_t n = hm.chunksPerDim * kHmSegs;
    const float s = hm.chunkScale, x0 = hm.minX, z0 = hm.minZ, x1 = x0 + (float)hm.chunksPerDim * hm.chunkSize, z1 = z0 + (float)hm.chunksPerDim * hm.chunkSize;
    float tIn = 0.f, tOut = FLT_MAX;
    if (d.x == 0.f) { if (o.x < x0 || o.x > x1) return false; }
    else { const float a = (x0 - o.x) / d.x, b = (x1 - o.x) / d.x; tIn = qmax(tIn, fminr(a, b)); tOut = fminr(tOut, qmax(a, b)); }
    if (d.z == 0.f) { if (o.z < z0 || o.z > z1) return false; }
    else { const float a = (z0 - o.z) / d.z, b = (z1 - o.z) / d.z; tIn = qmax(tIn, fminr(a, b)); tOut = fminr(tOut, qmax(a, b)); }
    const float tDom = tOut;
    tOut = fminr(tOut, tMax);
    if (!(tIn <= tOut)) return false;
    const float px = o.x + tIn * d.x, pz = o.z + tIn * d.z;
    int gx = (int)fminr(qmax(floorf((px - x0) / s), 0.f), (float)(n - 1u)), gz = (int)fminr(qmax(floorf((pz - z0) / s), 0.f), (float)(n - 1u));
    const int sx = d.x > 0.f ? 1 : -1, sz = d.z > 0.f ? 1 : -1;
    const float eps = 1e-3f / hm.invAmplitudeScale + 1e-5f * fabsf(o.y);
    bool blockMiss = false;
    float tCell = tIn;
    int entry = 0;
    int blockX = -1, blockZ = -1;
    for (uint32_t it = 0; it < 2u * n + 2u; ++it) {
        const float tx = d.x == 0.f ? FLT_MAX : (x0 + (float)(gx + (sx > 0 ? 1 : 0)) * s - o.x) / d.x;
        const float tz = d.z == 0.f ? FLT_MAX : (z0 + (float)(gz + (sz > 0 ? 1 : 0)) * s - o.z) / d.z;
        const float tExit = fminr(tx, tz);
        const uint32_t slot = hm.chunkSlot[(uint32_t)(gz >> 7) * hm.chunksPerDim + (uint32_t)(gx >> 7)];
        bool test = slot != 0xFFFFFFFFu;
        if (test && useBounds && ((gx >> 3) != blockX || (gz >> 3) != blockZ)) {   // entering a block (a line enters a rectangle once), at tCell
            blockX = gx >> 3; blockZ = gz >> 3;
            const uint32_t mm = hm.mips[(size_t)slot * kHmMipEntries + hmMipOffset(3u) + (uint32_t)((gz & 127) >> 3) * (kHmSegs >> 3) + (uint32_t)((gx & 127) >> 3)];
            const float hmin = (float)(mm & 0xFFFFu) * hm.heightScale + hm.minY, hmax = (float)(mm >> 16) * hm.heightScale + hm.minY;
            const float bx0 = x0 + (float)(blockX * 8) * s, bz0 = z0 + (float)(blockZ * 8) * s;
            const float bxOut = d.x == 0.f ? FLT_MAX : ((d.x > 0.f ? bx0 + 8.f * s : bx0) - o.x) / d.x;
            const float bzOut = d.z == 0.f ? FLT_MAX : ((d.z > 0.f ? bz0 + 8.f * s : bz0) - o.z) / d.z;
            const float tb = fminr(fminr(bxOut, bzOut), tDom);
            const float ya = o.y + tCell * d.y, yb = o.y + tb * d.y;
            blockMiss = fminr(ya, yb) > hmax + eps || qmax(ya, yb) < hmin - eps;
        }
        if (test && useBounds && blockMiss) test = false;
        if (test && useBounds) {
            const uint32_t mm = hm.mips[(size_t)slot * kHmMipEntries + (uint32_t)(gz & 127) * kHmSegs + (uint32_t)(gx & 127)];
            const float hmin = (float)(mm & 0xFFFFu) * hm.heightScale + hm.minY, hmax = (float)(mm >> 16) * hm.heightScale + hm.minY;
            const float ta = tCell, tb = fminr(tExit, tDom);
            const float ya = o.y + ta * d.y, yb = o.y + tb * d.y;
            if (fminr(ya, yb) > hmax + eps || qmax(ya, yb) < hmin - eps) test = false;
        }
        float t; uint32_t tri;
        if (test && qRayTerrainCell(hm, (uint32_t)gx, (uint32_t)gz, o, d, tCell, tExit, entry, tx < tz, t, tri)) {
            if (!(t <= tMax && t < FLT_MAX)) return false;
            bestT = t + 0.f; bestCell = (uint32_t)gz * n + (uint32_t)gx; bestTri = tri;
            return true;
        }
        if (tExit > tOut) break;
        if (tx < tz) { gx += sx; entry = 1; if (gx < 0 || gx >= (int)n) break; }
        else { gz += sz; entry = 2; if (gz < 0 || gz >= (int)n) break; }
        tCell = tExit;
    }
    return false;
}

// ---- the one finalisation both ray kernels use: the hit record of the winner (key = t bits << 32 | collider, kRayTerrain for the terrain)
__device__ __forceinline__ V3 qBoxNormal(V3 o, V3 d, V3 mn, V3 mx) {   // the entering slab's face, in rayAABB's arithmetic
    const V3 inv(1.f / d.x, 1.f / d.y, 1.f / d.z);
    const float xn = fminr((mn.x - o.x) * inv.x, (mx.x - o.x) * inv.x), yn = fminr((mn.y - o.y) * inv.y, (mx.y - o.y) * inv.y), zn = fminr((mn.z - o.z) * inv.z, (mx.z - o.z) * inv.z);
    int axis = 0; float cur = xn;
    if (!(cur > yn)) { axis = 1; cur = yn; }
    if (!(cur > zn)) { axis = 2; }
    V3 n; n.set(axis, d.get(axis) > 0.f ? -1.f : 1.f);
    return n;
}
__device__ inline V3 qLocalNormal(uint32_t type, float4 s0, float4 s1, float4 s2, const HullFaces& hf, V3 o, V3 d, float t) {
    const V3 h = o + t * d;
    switch (type) {
        case T_SPHERE: return h - xyz(s0);
        case T_CAPSULE: {
            const V3 pa = xyz(s0), pb(s0.w, s1.x, s1.y), ab = pb - pa;
            const float aa = dot(ab, ab), u = aa > 0.f ? qclamp01(dot(h - pa, ab) / aa) : 0.f;
            return h - (pa + u * ab);
        }
        case T_CYLINDER: {
            const V3 pa = xyz(s0), pb(s0.w, s1.x, s1.y); const float r = s1.z;
            const V3 u = noz(pb - pa); const float height = len(pb - pa);
            const float y = dot(h - pa, u); const V3 rv = (h - pa) - y * u;
            const float dSide = fabsf(len(rv) - r), dBottom = fabsf(y), dTop = fabsf(y - height);
            if (dBottom <= dSide && dBottom <= dTop) return -u;
            if (dTop <= dSide) return u;
            return rv;
        }
        case T_AABB: return qBoxNormal(o, d, xyz(s0), V3(s0.w, s1.x, s1.y));
        case T_OBB: {
            const Q4 q(s0.x, s0.y, s0.z, s0.w), inv = conj(q); const V3 c(s1.x, s1.y, s1.z), r(s1.w, s2.x, s2.y);
            return rotate(q, qBoxNormal(rotate(inv, o - c), rotate(inv, d), V3() - r, V3() + r));
        }
        default: {   // the hit triangle, found as qRayVsCollider found it: the same unit direction, so the same triangle wins
            float l, tt; V3 n;
            qRayHull(s0, s1, hf, o, qUnitDirection(d, l), tt, n);
            const float sl = sqlen(n);
            if (sl > 0.f && sl < 1e-8f) n = n * (1.f / sqrtf(sl));   // (qFinalise's noz() would take the normal of a small triangle for zero)
            return rotate(Q4(s0.x, s0.y, s0.z, s0.w), n);
        }
    }
}
__device__ inline void qFinalise(const QueryScene& s, const QueryRay& q, unsigned long long key, uint32_t terrainCell, uint32_t terrainTri, uint32_t* __restrict__ out) {
    uint32_t ent = kRayMiss, col = kRayMiss, obj = 0u;
    float t = __uint_as_float(0x7F800000u);   // +inf
    V3 p, n;
    if (key != ~0ull) {
        col = (uint32_t)key; t = __uint_as_float((uint32_t)(key >> 32));
        p = q.o + t * q.d;
        if (col == kRayTerrain) {
            ent = kRayTerrain; obj = OBJ_STATIC;
            const uint32_t nn = s.hm.chunksPerDim * kHmSegs;
            n = qTerrainNormal(s.hm, terrainCell % nn, terrainCell / nn, terrainTri);
        } else {
            const uint32_t type = s.cTypeBody[2 * col], body = s.cTypeBody[2 * col + 1];
            ent = s.cEntity[col]; obj = qObjectType(s, col, body);
            V3 pos; Q4 rot; qPose(s, col, body, pos, rot);
            const Q4 inv = conj(rot);
            n = rotate(rot, qLocalNormal(type, s.cShape[3 * col], s.cShape[3 * col + 1], s.cShape[3 * col + 2], s.hf, rotate(inv, q.o - pos), rotate(inv, q.d), t));
        }
        n = noz(n);
        if (t == 0.f || (n.x == 0.f && n.y == 0.f && n.z == 0.f)) n = -normalize(q.d);
    }
    out[0] = ent; out[1] = col; out[2] = __float_as_uint(t);
    out[3] = __float_as_uint(p.x); out[4] = __float_as_uint(p.y); out[5] = __float_as_uint(p.z);
    out[6] = __float_as_uint(n.x); out[7] = __float_as_uint(n.y); out[8] = __float_as_uint(n.z);
    out[9] = obj;
}
__device__ __forceinline__ bool qTerrainIncluded(const QueryScene& s, const QueryRay& q) {
    return s.hasTerrain && (q.include & kQueryTerrain) && kRayTerrain >= q.lo && kRayTerrain < q.hi;
}

// ---- accelerated: one lane per ray
__global__ __launch_bounds__(256) void k_q_raycast(uint32_t count, const float* __restrict__ rays /* origin3, direction3, max_t, - */, const uint32_t* __restrict__ ranges,
                                                  uint32_t include, QueryScene s, const QueryGrid* __restrict__ grid, const uint32_t* __restrict__ start,
                                                  const uint32_t* __restrict__ entries, const uint32_t* __restrict__ large, uint32_t* __restrict__ out /* [count][10] */) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= count) return;
    const QueryRay q = qLoadRay(rays, ranges, r, include);
    unsigned long long best = ~0ull;
    uint32_t tCell = 0u, tTri = 0u;
    if (q.valid) {
        const QueryGrid g = *grid;
        if (g.numCells) {   // clip to the grid box, then Amanatides-Woo
            const float mn[3] = {g.minX, g.minY, g.minZ}, o[3] = {q.o.x, q.o.y, q.o.z}, d[3] = {q.d.x, q.d.y, q.d.z};
            const uint32_t dim[3] = {g.dimX, g.dimY, g.dimZ};
            float tIn = 0.f, tOut = q.maxT; bool inside = true;
            for (int a = 0; a < 3; ++a) {
                const float lo = mn[a], hi = mn[a] + (float)dim[a] * g.cell;
                if (d[a] == 0.f) { if (o[a] < lo || o[a] > hi) inside = false; }
                else { const float t0 = (lo - o[a]) / d[a], t1 = (hi - o[a]) / d[a]; tIn = qmax(tIn, fminr(t0, t1)); tOut = fminr(tOut, qmax(t0, t1)); }
            }
            if (inside && tIn <= tOut) {
                int c[3], st[3];
                for (int a = 0; a < 3; ++a) {
                    c[a] = (int)fminr(qmax(floorf((o[a] + tIn * d[a] - mn[a]) * g.invCell), 0.f), (float)(dim[a] - 1u));
                    st[a] = d[a] > 0.f ? 1 : -1;
                }
                for (uint32_t it = 0; it < g.dimX + g.dimY + g.dimZ + 3u; ++it) {
                    const uint32_t cell = ((uint32_t)c[2] * g.dimY + (uint32_t)c[1]) * g.dimX + (uint32_t)c[0];
                    const uint32_t e0 = start[cell], e1 = start[cell + 1];
                    for (uint32_t e = e0; e < e1; ++e) { const unsigned long long k = qTestCollider(s, q, entries[e]); if (k < best) best = k; }
                    float tn[3];
                    for (int a = 0; a < 3; ++a) tn[a] = d[a] == 0.f ? FLT_MAX : (mn[a] + (float)(c[a] + (st[a] > 0 ? 1 : 0)) * g.cell - o[a]) / d[a];
                    const int ax = tn[0] < tn[1] ? (tn[0] < tn[2] ? 0 : 2) : (tn[1] < tn[2] ? 1 : 2);
                    const float tExit = tn[ax];
                    // every collider whose hit lies before the exit of this cell was in a cell visited so far (a hit point lies in the collider's AABB)
                    if (best != ~0ull && __uint_as_float((uint32_t)(best >> 32)) <= tExit) break;
                    if (tExit > tOut) break;
                    c[ax] += st[ax];
                    if (c[ax] < 0 || c[ax] >= (int)dim[ax]) break;
                }
            }
        }
        const uint32_t nl = g.numLarge;
        for (uint32_t i = 0; i < nl; ++i) { const unsigned long long k = qTestCollider(s, q, large[i]); if (k < best) best = k; }
        if (qTerrainIncluded(s, q)) {
            const float limit = best == ~0ull ? q.maxT : fminr(q.maxT, __uint_as_float((uint32_t)(best >> 32)));
            float tt; uint32_t cell, tri;
            if (qTerrainWalk(s.hm, q.o, q.d, limit, true, tt, cell, tri)) {
                const unsigned long long k = ((unsigned long long)__float_as_uint(tt) << 32) | kRayTerrain;
                if (k < best) { best = k; tCell = cell; tTri = tri; }
            }
        }
    }
    qFinalise(s, q, best, tCell, tTri, out + 10 * (size_t)r);
}

// ---- exhaustive: one workgroup per ray over every collider (k_ray_interactions' scan, every object type), the terrain without the bounds test
__global__ __launch_bounds__(256) void k_q_exhaustive(const float* __restrict__ rays, const uint32_t* __restrict__ ranges, uint32_t include, QueryScene s, uint32_t* __restrict__ out) {
    __shared__ unsigned long long best[256];
    const uint32_t r = blockIdx.x;
    const QueryRay q = qLoadRay(rays, ranges, r, include);
    unsigned long long mine = ~0ull;
    if (q.valid)
        for (uint32_t k = threadIdx.x; k < s.nc; k += blockDim.x) { const unsigned long long key = qTestCollider(s, q, k); if (key < mine) mine = key; }
    best[threadIdx.x] = mine;
    __syncthreads();
    for (uint32_t st = 128; st > 0; st >>= 1) { if (threadIdx.x < st && best[threadIdx.x + st] < best[threadIdx.x]) best[threadIdx.x] = best[threadIdx.x + st]; __syncthreads(); }
    if (threadIdx.x != 0) return;
    unsigned long long b = best[0];
    uint32_t tCell = 0u, tTri = 0u;
    if (q.valid && qTerrainIncluded(s, q)) {
        float tt; uint32_t cell, tri;
        if (qTerrainWalk(s.hm, q.o, q.d, q.maxT, false, tt, cell, tri)) {
            const unsigned long long k = ((unsigned long long)__float_as_uint(tt) << 32) | kRayTerrain;
            if (k < b) { b = k; tCell = cell; tTri = tri; }
        }
    }
    qFinalise(s, q, b, tCell, tTri, out + 10 * (size_t)r);
}

}  // namespace mi
