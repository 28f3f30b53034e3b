// kernels_overlap.hpp — batched volume-overlap scene queries (mi_world_overlap*, include/mi_physics.h): which colliders touch a sphere,
// capsule, cylinder, box or hull.  Part of the ONE translation unit of the physics library (world.hip includes it after kernels_query.hpp,
// whose grid it walks).  Host side: world_query.inc.
//
// Read-only with respect to the step: everything here writes query-owned buffers (QueryCache in world.hip) or the caller's result.
//   k_ov_unpack             one lane per volume: validation; the volume as the rows of a static collider with its pose; entity range
//   k_ov_prepare            one lane per volume: world shape rows and AABB through worldCollider
//   k_q_overlap             one wave per volume, pass 0 = count, pass 1 = write: the lanes stride over the entries of the grid cells the
//                           volume's AABB overlaps, then over the large list; a volume over many cells, or with a long result, strides
//                           over all colliders instead
//   k_exclusive_scan        counts -> offsets (the CSR row starts), between the passes
//   k_q_overlap_exhaustive  the yardstick: every collider for every volume, the same two passes
// Every route decides through ovTest (admission: ovAdmit, which the shape casts of kernels_sweep.hpp share) and writes through ovWrite, and every segment leaves in ascending collider index: the same bytes.
#pragma once
#include "kernels_query.hpp"

namespace mi {

constexpr uint32_t kOvWaves = 4;            // volumes per 256-thread workgroup
constexpr uint32_t kOvMaxCells = 512;       // a volume over more cells strides over all colliders instead (ordered by construction)
constexpr uint32_t kOvSortMax = 1024;       // longest segment a wave sorts in LDS; a longer one is written by the stride over all colliders
constexpr uint32_t kOvInvalid = 0xFFu;      // world type of a volume that reports nothing
constexpr uint32_t kOvPassCount = 1u, kOvPassWrite = 2u;   // what one overlapEnqueue runs (world_query.inc)
constexpr uint32_t kOvVolumeWords = 24;     // mi_query_volume: type, hull_geometry, shape[12], position[3], pad, rotation[4], pad[2]

// what a volume sees: the world rows of the colliders at the current poses (k_q_colliders) and who they belong to
struct OverlapScene {
    uint32_t nc;
    const uint32_t* cEntity;
    const float4* shape; const float4* mn; const float4* mx;   // mn.w = world type | object type << 8 (worldCollider)
    HullSet hs;
};
struct OverlapVolume { Shape s; V3 mn, mx; uint32_t lo, hi, include; bool valid; };

// the volumes as static colliders of entities at their poses (the rows worldCollider reads); an invalid one gets the type kOvInvalid
__global__ __launch_bounds__(256) void k_ov_unpack(uint32_t count, const uint32_t* __restrict__ volumes, const uint32_t* __restrict__ ranges, uint32_t numHulls,
                                                   uint32_t* __restrict__ vcTypeBody, uint32_t* __restrict__ vcObject, float4* __restrict__ vcShape,
                                                   float4* __restrict__ vcPos, float4* __restrict__ vcRot, uint32_t* __restrict__ vRange) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= count) return;
    uint32_t w[kOvVolumeWords];
    const uint4* src = reinterpret_cast<const uint4*>(volumes) + (size_t)v * (kOvVolumeWords / 4);
#pragma unroll
    for (uint32_t i = 0; i < kOvVolumeWords / 4; ++i) { const uint4 q = src[i]; w[4 * i] = q.x; w[4 * i + 1] = q.y; w[4 * i + 2] = q.z; w[4 * i + 3] = q.w; }
    const uint32_t type = w[0], geom = w[1];
    float s[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) s[i] = __uint_as_float(w[2 + i]);
    // the words the type reads: sphere 4, capsule / cylinder 7, aabb 6, obb 10, hull 7
    const uint32_t used = type == T_SPHERE ? 4u : type == T_AABB ? 6u : type == T_OBB ? 10u : 7u;
    bool valid = type <= (uint32_t)T_HULL;
#pragma unroll
    for (uint32_t i = 0; i < 12; ++i) if (i < used && !qFinite(s[i])) valid = false;
#pragma unroll
    for (uint32_t i = 14; i < 22; ++i) if (i != 17u && !qFinite(__uint_as_float(w[i]))) valid = false;
    switch (type) {
        case T_SPHERE: if (!(s[3] >= 0.f)) valid = false; break;
        case T_CAPSULE: case T_CYLINDER: if (!(s[6] >= 0.f)) valid = false; break;
        case T_AABB: if (!(s[3] >= s[0] && s[4] >= s[1] && s[5] >= s[2])) valid = false; break;
        case T_OBB: if (!(s[7] >= 0.f && s[8] >= 0.f && s[9] >= 0.f)) valid = false; break;
        case T_HULL: if (geom >= numHulls) valid = false; break;
        default: break;
    }
    if (type == T_HULL) s[7] = __uint_as_float(geom);   // as upload() packs a hull collider
    vcTypeBody[2 * v] = valid ? type : kOvInvalid; vcTypeBody[2 * v + 1] = kNoBody;
    vcObject[v] = OBJ_STATIC;
    vcShape[3 * (size_t)v] = make_float4(s[0], s[1], s[2], s[3]); vcShape[3 * (size_t)v + 1] = make_float4(s[4], s[5], s[6], s[7]);
    vcShape[3 * (size_t)v + 2] = make_float4(s[8], s[9], s[10], s[11]);
    vcPos[v] = make_float4(__uint_as_float(w[14]), __uint_as_float(w[15]), __uint_as_float(w[16]), 0.f);
    vcRot[v] = make_float4(__uint_as_float(w[18]), __uint_as_float(w[19]), __uint_as_float(w[20]), __uint_as_float(w[21]));
    vRange[2 * v] = ranges ? ranges[2 * v] : 0u; vRange[2 * v + 1] = ranges ? ranges[2 * v + 1] : 0xFFFFFFFFu;
}
// one lane per volume: world shape rows and AABB by worldCollider itself
__global__ __launch_bounds__(256) void k_ov_prepare(uint32_t count, ColliderRows rows /* the volumes as static colliders (k_ov_unpack) -> the volumes' world rows */) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= count) return;
    float4* __restrict__ vShape = rows.wShape; float4* __restrict__ vMin = rows.aabbMin; float4* __restrict__ vMax = rows.aabbMax;
    if (rows.cTypeBody[2 * v] != kOvInvalid) {
        float4 mn, mx;
        worldCollider<false>(v, rows, mn, mx);
        if (qExtent(mn, mx) >= 0.f) return;   // (a pose or size that overflows leaves a non-finite box: reports nothing)
    }
    vShape[3 * (size_t)v] = make_float4(0, 0, 0, 0); vShape[3 * (size_t)v + 1] = make_float4(0, 0, 0, 0); vShape[3 * (size_t)v + 2] = make_float4(0, 0, 0, 1);
    vMin[v] = make_float4(0, 0, 0, __uint_as_float(kOvInvalid)); vMax[v] = make_float4(0, 0, 0, 0);
}

__device__ __forceinline__ OverlapVolume ovLoadVolume(const float4* __restrict__ vShape, const float4* __restrict__ vMin, const float4* __restrict__ vMax,
                                                      const uint32_t* __restrict__ vRange, uint32_t v, uint32_t include) {
    OverlapVolume q;
    const float4 a = vMin[v], b = vMax[v];
    const uint32_t type = __float_as_uint(a.w) & 0xFFu;
    q.valid = type != kOvInvalid;
    q.s = loadShape(vShape, v, q.valid ? type : (uint32_t)T_SPHERE);
    q.mn = xyz(a); q.mx = xyz(b);
    q.lo = vRange[2 * v]; q.hi = vRange[2 * v + 1]; q.include = include;
    return q;
}
// The shape cast's pair test at a zero displacement (kernels_sweep.hpp, which includes this file: defined there): do the volume and the
// collider touch?  Its float32 distance search with a tolerance relative to the coordinates (kSweepTolRel), no absolute threshold.
__device__ bool swOverlaps(const Shape& volume, V3 volumeMin, V3 volumeMax, const Shape& collider, const HullSet& hs);

// THE QUERY'S pair test (the step's triggers keep overlapCheck, gjk.hpp: the reference's bits).  The reference's closed forms where they
// decide geometrically right, with their bits: spheres and capsules among themselves, a sphere against a box, boxes against boxes (SAT).
// Everything else goes to swOverlaps: the reference's sphere / capsule vs cylinder compares a squared distance with a radius beyond the caps,
// and its GJK (every pair with a cylinder or a hull, a capsule against a box) gives up at absolute thresholds (|dir|^2 < 1e-4, +-1e-5 in the
// simplex update), so shapes of a few centimetres never overlap anything.  A capsule of zero length (a sphere; valid) goes there too: the
// reference's closest point on its segment divides by the segment's length.
__device__ __forceinline__ bool ovPointCapsule(const Shape& s) { return s.type == T_CAPSULE && s.a.x == s.b.x && s.a.y == s.b.y && s.a.z == s.b.z; }
__device__ inline bool ovQueryCheck(const OverlapVolume& q, const Shape& c, const HullSet& hs) {
    const int lo = min((int)c.type, q.s.type), hi = max((int)c.type, q.s.type);
    const bool closedForm = ((hi <= T_CAPSULE) || (lo == T_SPHERE && (hi == T_AABB || hi == T_OBB)) || (lo >= T_AABB && hi <= T_OBB)) && !ovPointCapsule(q.s) && !ovPointCapsule(c);
    if (!closedForm) return swOverlaps(q.s, q.mn, q.mx, c, hs);
    return (int)c.type < q.s.type ? overlapCheck(c, q.s, hs) : overlapCheck(q.s, c, hs);
}
// THE admission test of overlaps and casts: object type, entity range, a finite world AABB.  Loads the collider's box rows once (tag = a.w).
__device__ __forceinline__ bool ovAdmit(const OverlapScene& s, const OverlapVolume& q, uint32_t k, float4& a, float4& b, uint32_t& tag) {
    a = s.mn[k]; b = s.mx[k]; tag = __float_as_uint(a.w);
    if (!(q.include & qFlagOf((tag >> 8) & 0xFFu))) return false;
    const uint32_t ent = s.cEntity[k];
    if (ent < q.lo || ent >= q.hi) return false;
    return qExtent(a, b) >= 0.f;
}
// THE predicate: is collider k reported for this volume?  ovAdmit, closed world AABBs, then ovQueryCheck.  kBoxesOnly: everything but the
// pair test — the candidates of the contact query (kernels_contacts_query.hpp), whose narrow phase decides instead.
template <bool kBoxesOnly> __device__ inline bool ovTest(const OverlapScene& s, const OverlapVolume& q, uint32_t k) {
    float4 a, b; uint32_t tag;
    if (!ovAdmit(s, q, k, a, b, tag)) return false;
    const V3 qmn = q.mn, qmx = q.mx;   // (loaded at once: read one by one under the short-circuit, each comparison waits for its own load, 5 to 10 % of a batch)
    if ((qmx.x < a.x) | (qmn.x > b.x) | (qmx.y < a.y) | (qmn.y > b.y) | (qmx.z < a.z) | (qmn.z > b.z)) return false;
    if (kBoxesOnly) return true;
    return ovQueryCheck(q, loadShape(s.shape, k, tag & 0xFFu), s.hs);
}
// THE record writer: slot = position in the whole result; nothing is written at or past capacity
__device__ __forceinline__ void ovWrite(const OverlapScene& s, uint4* __restrict__ hits, uint32_t capacity, uint32_t slot, uint32_t k, uint32_t v) {
    if (slot >= capacity) return;
    hits[slot] = make_uint4(s.cEntity[k], k, (__float_as_uint(s.mn[k].w) >> 8) & 0xFFu, v);
}

// one wave over all colliders in index order: the count, and with `write` the records from `base` on (ascending by construction)
template <bool kBoxesOnly> __device__ inline uint32_t ovLinear(const OverlapScene& s, const OverlapVolume& q, uint32_t v, uint32_t lane, bool write, uint4* __restrict__ hits, uint32_t capacity, uint32_t base) {
    uint32_t n = 0;
    for (uint32_t k0 = 0; k0 < s.nc; k0 += 64u) {
        const uint32_t k = k0 + lane;
        const bool hit = k < s.nc && ovTest<kBoxesOnly>(s, q, k);
        const unsigned long long m = __ballot(hit);
        if (write && hit) ovWrite(s, hits, capacity, base + n + (uint32_t)__popcll(m & ((1ull << lane) - 1ull)), k, v);
        n += (uint32_t)__popcll(m);
    }
    return n;
}

// the cells a volume's AABB overlaps, clamped to the grid (no margin: a collider was inserted with one, and floor((x - o) * inv) is
// monotonic in x, so overlapping closed AABBs always share a cell of both clamped ranges); false: stride over all colliders
__device__ __forceinline__ bool ovCellRange(const QueryGrid& g, const OverlapVolume& q, uint32_t lo[3], uint32_t hi[3]) {
    if (g.numCells == 0u) return false;
    const float a[3] = {q.mn.x, q.mn.y, q.mn.z}, b[3] = {q.mx.x, q.mx.y, q.mx.z}, o[3] = {g.minX, g.minY, g.minZ};
    const uint32_t dim[3] = {g.dimX, g.dimY, g.dimZ};
    uint32_t cells = 1u;
    for (int i = 0; i < 3; ++i) {
        const float l = floorf((a[i] - o[i]) * g.invCell), h = floorf((b[i] - o[i]) * g.invCell);
        lo[i] = (uint32_t)fminr(qmax(l, 0.f), (float)(dim[i] - 1u)); hi[i] = (uint32_t)fminr(qmax(h, 0.f), (float)(dim[i] - 1u));
        cells *= hi[i] - lo[i] + 1u;
        if (cells > kOvMaxCells) return false;
    }
    return true;
}

__device__ __forceinline__ void ovKeep(uint32_t* keys, uint32_t slot, bool hit, uint32_t k) { if (keys && hit && slot < kOvSortMax) keys[slot] = k; }   // (never past the wave's LDS row)

// The grid walk of one wave.  The cells of one x row are neighbours in `entries` (cell index = x fastest, starts = a prefix sum), so the
// lanes stride over the row's whole span.  A collider sits in every cell of its range; it is reported from ONE entry: the one in the lowest
// cell, per axis, of the intersection of its range (qCellRange, which inserted it) with the volume's.  keys != null: the matches are
// compacted into keys[0 .. n) (LDS, any order); the caller guarantees n <= kOvSortMax.
template <bool kBoxesOnly> __device__ inline uint32_t ovGridWalk(const OverlapScene& s, const OverlapVolume& q, const QueryGrid& g, const uint32_t lo[3], const uint32_t hi[3],
                                      const uint32_t* __restrict__ start, const uint32_t* __restrict__ entries, const uint32_t* __restrict__ large, uint32_t lane,
                                      uint32_t* keys) {
    uint32_t n = 0;
    for (uint32_t z = lo[2]; z <= hi[2]; ++z)
        for (uint32_t y = lo[1]; y <= hi[1]; ++y) {
            const uint32_t row = (z * g.dimY + y) * g.dimX;
            const uint32_t e0 = start[row + lo[0]], e1 = start[row + hi[0] + 1u];
            for (uint32_t eb = e0; eb < e1; eb += 64u) {
                const uint32_t e = eb + lane;
                bool hit = false; uint32_t k = 0u;
                if (e < e1) {
                    k = entries[e];
                    uint32_t klo[3], khi[3];
                    if (qCellRange(g, s.mn[k], s.mx[k], klo, khi) && max(klo[1], lo[1]) == y && max(klo[2], lo[2]) == z) {
                        const uint32_t c = row + max(klo[0], lo[0]);
                        hit = start[c] <= e && e < start[c + 1u] && ovTest<kBoxesOnly>(s, q, k);
                    }
                }
                const unsigned long long m = __ballot(hit);
                ovKeep(keys, n + (uint32_t)__popcll(m & ((1ull << lane) - 1ull)), hit, k);
                n += (uint32_t)__popcll(m);
            }
        }
    const uint32_t nl = g.numLarge;
    for (uint32_t i0 = 0; i0 < nl; i0 += 64u) {
        const uint32_t i = i0 + lane;
        const uint32_t k = i < nl ? large[i] : 0u;
        const bool hit = i < nl && ovTest<kBoxesOnly>(s, q, k);
        const unsigned long long m = __ballot(hit);
        ovKeep(keys, n + (uint32_t)__popcll(m & ((1ull << lane) - 1ull)), hit, k);
        n += (uint32_t)__popcll(m);
    }
    return n;
}

// pass 0: counts[v] (and counts[count] = 0 for the scan).  pass 1: offsets = the scanned counts; the segment of volume v is written in
// ascending collider index: a grid-walk segment is sorted in LDS by its wave, the others come from the stride over all colliders.
template <bool kBoxesOnly> __global__ __launch_bounds__(64 * kOvWaves) void k_q_overlap(uint32_t pass, uint32_t count, uint32_t include, OverlapScene s, const float4* __restrict__ vShape,
                                                             const float4* __restrict__ vMin, const float4* __restrict__ vMax, const uint32_t* __restrict__ vRange,
                                                             const QueryGrid* __restrict__ grid, const uint32_t* __restrict__ start, const uint32_t* __restrict__ entries,
                                                             const uint32_t* __restrict__ large, uint32_t* __restrict__ counts, const uint32_t* __restrict__ offsets,
                                                             uint4* __restrict__ hits, uint32_t capacity, uint32_t* __restrict__ total) {
    __shared__ uint32_t sKeys[kOvWaves][kOvSortMax];
    __shared__ uint32_t sN[kOvWaves];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, v = blockIdx.x * kOvWaves + wave;
    if (blockIdx.x == 0 && threadIdx.x == 0) { if (pass == 0u) counts[count] = 0u; else if (total) total[0] = offsets[count]; }
    uint32_t nSort = 0, base = 0;
    if (v < count) {
        const OverlapVolume q = ovLoadVolume(vShape, vMin, vMax, vRange, v, include);
        const QueryGrid g = *grid;
        uint32_t lo[3], hi[3];
        const bool walk = q.valid && ovCellRange(g, q, lo, hi);
        if (pass == 0u) {
            const uint32_t n = !q.valid ? 0u : walk ? ovGridWalk<kBoxesOnly>(s, q, g, lo, hi, start, entries, large, lane, nullptr) : ovLinear<kBoxesOnly>(s, q, v, lane, false, nullptr, 0u, 0u);
            if (lane == 0u) counts[v] = n;
        } else {
            base = offsets[v];
            const uint32_t n = offsets[v + 1u] - base;
            if (n != 0u && base < capacity) {
                if (walk && n <= kOvSortMax) nSort = min(ovGridWalk<kBoxesOnly>(s, q, g, lo, hi, start, entries, large, lane, sKeys[wave]), n);   // (= n: the count pass walked the same entries)
                else ovLinear<kBoxesOnly>(s, q, v, lane, true, hits, capacity, base);
            }
        }
    }
    if (pass == 0u) return;   // (uniform over the workgroup)
    // bitonic sort of every wave's keys, all waves in step: the padded length is the workgroup's longest
    if (lane == 0u) sN[wave] = nSort;
    __syncthreads();
    uint32_t longest = 0;
#pragma unroll
    for (uint32_t i = 0; i < kOvWaves; ++i) longest = max(longest, sN[i]);
    if (longest == 0u) return;
    uint32_t padded = 64u;
    while (padded < longest) padded <<= 1;
    uint32_t* keys = sKeys[wave];
    for (uint32_t i = nSort + lane; i < padded; i += 64u) keys[i] = 0xFFFFFFFFu;
    __syncthreads();
    for (uint32_t size = 2u; size <= padded; size <<= 1)
        for (uint32_t stride = size >> 1; stride > 0u; stride >>= 1) {
            for (uint32_t t = lane; t < (padded >> 1); t += 64u) {
                const uint32_t i = 2u * t - (t & (stride - 1u)), j = i + stride;
                const uint32_t a = keys[i], b = keys[j];
                const bool up = (i & size) == 0u;
                if ((a > b) == up) { keys[i] = b; keys[j] = a; }
            }
            __syncthreads();
        }
    for (uint32_t i = lane; i < nSort; i += 64u) ovWrite(s, hits, capacity, base + i, keys[i], v);
}

// ---- exhaustive: one wave per volume over every collider, no grid; the rows in `s` are computed for the call, not taken from the cache
template <bool kBoxesOnly> __global__ __launch_bounds__(64 * kOvWaves) void k_q_overlap_exhaustive(uint32_t pass, uint32_t count, uint32_t include, OverlapScene s, const float4* __restrict__ vShape,
                                                                        const float4* __restrict__ vMin, const float4* __restrict__ vMax, const uint32_t* __restrict__ vRange,
                                                                        uint32_t* __restrict__ counts, const uint32_t* __restrict__ offsets, uint4* __restrict__ hits,
                                                                        uint32_t capacity, uint32_t* __restrict__ total) {
    const uint32_t lane = threadIdx.x & 63u, v = blockIdx.x * kOvWaves + (threadIdx.x >> 6);
    if (blockIdx.x == 0 && threadIdx.x == 0) { if (pass == 0u) counts[count] = 0u; else if (total) total[0] = offsets[count]; }
    if (v >= count) return;
    const OverlapVolume q = ovLoadVolume(vShape, vMin, vMax, vRange, v, include);
    if (pass == 0u) {
        const uint32_t n = q.valid ? ovLinear<kBoxesOnly>(s, q, v, lane, false, nullptr, 0u, 0u) : 0u;
        if (lane == 0u) counts[v] = n;
    } else if (q.valid && offsets[v] < capacity) ovLinear<kBoxesOnly>(s, q, v, lane, true, hits, capacity, offsets[v]);
}

}  // namespace mi
