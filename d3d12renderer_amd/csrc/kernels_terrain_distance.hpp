// kernels_terrain_distance.hpp — batched terrain distance queries (mi_world_terrain_distance*, include/mi_physics.h): the heightmap's collision triangle
// nearest to a sphere, capsule, cylinder, box or hull, with the distance, the two closest points and the direction between them: ground clearance.
// Part of the ONE translation unit of the physics library (world.hip includes it after kernels_distance.hpp, whose pair test, record and box gap it
// uses, and through it kernels_sweep.hpp's terrain triangles: swTerrainShape, swTerrainCoord, swTerrainHeight).  Host side: world_query.inc.
//
// Read-only with respect to the step: everything here reads query-owned rows and the heightmap buffers and writes the caller's records.
//   distanceTrianglePair             (kernels_distance.hpp) the pair test: distancePair's body with the triangle's support
//   k_q_terrain_distance             one wave per volume: the 8 x 8 blocks of cells under the volume's footprint (ring 0: it seeds the best distance),
//                                    then Chebyshev rings of blocks outward, culled by the chunk's, the block's and the cell's height range (mip
//                                    levels 7, 3 and 0), until everything outside the walked rings is provably farther than the limit
//   k_q_terrain_distance_exhaustive  the yardstick: every triangle of every chunk that has heights, no mips, nothing skipped
// Both kernels decide through tdCandidate and write through tdFinalise (which applies the merge rule): the same winner key (distance bits << 32 |
// (gz * n + gx) * 2 + tri) gives the same bytes.  THE INVARIANT behind that is kernels_distance.hpp's: the distance a candidate reports (dsResolve
// against the triangle's AABB) is never below the gap of the volume's AABB and the triangle's; a culling box (cell, block, chunk) contains the boxes
// of its triangles by the same vertex arithmetic, so its gap is never above theirs (every operation of the gap is monotone), and the bound of a ring
// is padded; skipping compares strictly, so triangles at equal distance still meet and the lowest index wins on every route.
// No atomics, no LDS, no dependence between waves; every loop is bounded by the map's dimensions.
#pragma once
#include "kernels_distance.hpp"

namespace mi {

__device__ __forceinline__ uint32_t tdIndex(const HeightmapParams& hm, uint32_t gx, uint32_t gz, uint32_t tri) { return (gz * (hm.chunksPerDim * kHmSegs) + gx) * 2u + tri; }
__device__ __forceinline__ void tdTriangleBox(const Shape& T, V3& mn, V3& mx) {
    const V3 third(T.rot.x, T.rot.y, T.rot.z);
    mn = vmin(vmin(T.a, T.b), third); mx = qvmax(qvmax(T.a, T.b), third);
}
// the gap of the volume's AABB and the box of the aligned square of `cells` cells at cell (gx, gz) of one chunk, with the height range `mm` (min | max << 16)
__device__ __forceinline__ float tdBoxGap(const HeightmapParams& hm, const OverlapVolume& q, uint32_t gx, uint32_t gz, uint32_t cells, uint32_t mm) {
    const V3 mn(swTerrainCoord(hm, gx >> 7, gx & 127u, hm.minX), swTerrainHeight(hm, mm & 0xFFFFu), swTerrainCoord(hm, gz >> 7, gz & 127u, hm.minZ));
    const V3 mx(swTerrainCoord(hm, gx >> 7, (gx & 127u) + cells, hm.minX), swTerrainHeight(hm, mm >> 16), swTerrainCoord(hm, gz >> 7, (gz & 127u) + cells, hm.minZ));
    return len(dsBoxGapVector(q, mn, mx));
}
// THE terrain candidate test: triangle `tri` of cell (gx, gz) (of a chunk that has heights) against the query -> key = distance bits << 32 | index, or ~0.
// kSkip: a triangle whose box gap lies strictly above `limit` cannot win.
template <bool kSkip> __device__ inline unsigned long long tdCandidate(const HeightmapParams& hm, const HullSet& hs, const DistanceQuery& d, uint32_t gx, uint32_t gz,
                                                                      uint32_t tri, float limit) {
    const Shape T = swTerrainShape(hm, gx, gz, tri);
    V3 a, b; tdTriangleBox(T, a, b);
    const float boxGap = len(dsBoxGapVector(d.q, a, b));
    if (kSkip && boxGap > limit) return ~0ull;
    const DistanceResult r = distanceTrianglePair(d.q.s, T, hs);
    uint32_t flags;
    const float dist = dsResolve(r, boxGap, flags);
    if (!(dist <= d.maxD) || !qFinite(dist)) return ~0ull;
    return ((unsigned long long)__float_as_uint(dist + 0.f) << 32) | tdIndex(hm, gx, gz, tri);
}
// THE terrain record writer (one lane).  merge: `out` holds the record of a mi_world_distance call for this volume, which the terrain replaces only when that
// is a miss or its distance is strictly greater (as float bits: both are non-negative), so a collider wins a tie; a terrain miss and an invalid volume leave it
// untouched.  Then the winner's pair test once more (it depends on the pair alone: the same bits) and dsFinalise's record.
__device__ inline void tdFinalise(const HeightmapParams& hm, const HullSet& hs, const DistanceQuery& d, unsigned long long key, float4 pose, uint32_t v, uint32_t merge, uint4* out) {
    uint4* rec = out + kDistanceRecordRows * (size_t)v;
    if (merge) {
        if (key == ~0ull) return;
        const uint4 have = rec[0];
        if (have.x != kRayMiss && !(have.z > (uint32_t)(key >> 32))) return;
    }
    uint4 row0 = make_uint4(kRayMiss, kRayMiss, 0x7F800000u /* +inf */, 0u);
    V3 pc, pv, n; uint32_t flags = 0u;
    if (key != ~0ull) {
        const uint32_t index = (uint32_t)key, cell = index >> 1, cells = hm.chunksPerDim * kHmSegs;
        row0 = make_uint4(kRayTerrain, kRayTerrain, (uint32_t)(key >> 32), OBJ_STATIC);
        const Shape T = swTerrainShape(hm, cell % cells, cell / cells, index & 1u);
        V3 a, b; tdTriangleBox(T, a, b);
        const V3 gap = dsBoxGapVector(d.q, a, b);
        const float boxGap = len(gap);
        const DistanceResult r = distanceTrianglePair(d.q.s, T, hs);
        dsResolve(r, boxGap, flags);
        if (flags & kDistanceOverlap) { pc = pv = V3(pose.x, pose.y, pose.z); }
        else if (r.flags & kDistanceOverlap) {
            // (touching by the search, apart by the boxes: the boxes' gap, between the volume's box and its clamp towards the triangle's, as dsFinalise)
            const V3 sign(a.x > d.q.mx.x ? -1.f : 1.f, a.y > d.q.mx.y ? -1.f : 1.f, a.z > d.q.mx.z ? -1.f : 1.f);
            n = V3(gap.x * sign.x, gap.y * sign.y, gap.z * sign.z) * (1.f / boxGap);
            pv = vmin(qvmax(d.q.mn * 0.5f + d.q.mx * 0.5f, a), b); pv = vmin(qvmax(pv, d.q.mn), d.q.mx);
            pc = pv - n * boxGap;
        } else { pc = r.pointCollider; pv = r.pointVolume; n = r.normal; }
    }
    rec[0] = row0;
    rec[1] = make_uint4(__float_as_uint(pc.x), __float_as_uint(pc.y), __float_as_uint(pc.z), flags);
    rec[2] = make_uint4(__float_as_uint(pv.x), __float_as_uint(pv.y), __float_as_uint(pv.z), v);
    rec[3] = make_uint4(__float_as_uint(n.x), __float_as_uint(n.y), __float_as_uint(n.z), 0u);
}

// ---- a world without a heightmap: every record a miss
__global__ __launch_bounds__(256) void k_q_terrain_distance_none(uint32_t count, uint4* __restrict__ out) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= count) return;
    uint4* rec = out + kDistanceRecordRows * (size_t)v;
    rec[0] = make_uint4(kRayMiss, kRayMiss, 0x7F800000u /* +inf */, 0u);
    rec[1] = make_uint4(0u, 0u, 0u, 0u); rec[2] = make_uint4(0u, 0u, 0u, v); rec[3] = make_uint4(0u, 0u, 0u, 0u);
}

// ---- exhaustive: one wave per volume, the lanes over every triangle (32 cells of one row at a time: one chunk), nothing skipped
__global__ __launch_bounds__(64 * kOvWaves) void k_q_terrain_distance_exhaustive(uint32_t count, uint32_t merge, HeightmapParams hm, HullSet hs, const float4* __restrict__ vShape,
                                                                                const float4* __restrict__ vMin, const float4* __restrict__ vMax, const uint32_t* __restrict__ vRange,
                                                                                const float4* __restrict__ vPos, const float* __restrict__ maxDistances, uint4* out) {
    const uint32_t lane = threadIdx.x & 63u, v = blockIdx.x * kOvWaves + (threadIdx.x >> 6);
    if (v >= count) return;
    const DistanceQuery d = dsLoadQuery(vShape, vMin, vMax, vRange, maxDistances, v, 0u);
    const uint32_t n = hm.chunksPerDim * kHmSegs;
    unsigned long long best = ~0ull;
    if (d.valid)
        for (uint32_t gz = 0; gz < n; ++gz)
            for (uint32_t gx0 = 0; gx0 < n; gx0 += 32u) {
                if (hm.chunkSlot[(gz >> 7) * hm.chunksPerDim + (gx0 >> 7)] == 0xFFFFFFFFu) continue;
                best = min(best, tdCandidate<false>(hm, hs, d, gx0 + (lane >> 1), gz, lane & 1u, 0.f));
            }
    best = swWaveMin(best);
    if (lane == 0u) tdFinalise(hm, hs, d, best, vPos[v], v, merge, out);
}

// A lower bound of the horizontal distance from the volume's AABB to every cell OUTSIDE the block box [x0, x1] x [z0, z1] (signed, unclamped; nb blocks a
// side): the smallest over the four sides of the side's coordinate to the AABB's far face, less a relative padding (dsShellBound's; it also covers the ulp by
// which vertex 128 of a chunk may lie past vertex 0 of the next).  A side at the map's border has nothing beyond it.  +inf: the box covers the map.
__device__ __forceinline__ float tdRingBound(const HeightmapParams& hm, const OverlapVolume& q, int x0, int x1, int z0, int z1, int nb) {
    const float mn[2] = {q.mn.x, q.mn.z}, mx[2] = {q.mx.x, q.mx.z}, o[2] = {hm.minX, hm.minZ};
    const int lo[2] = {x0, z0}, hi[2] = {x1, z1};
    float bound = __uint_as_float(0x7F800000u);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        if (hi[i] + 1 < nb) {
            const uint32_t b = (uint32_t)(hi[i] + 1);
            const float plane = swTerrainCoord(hm, b >> 4, (b & 15u) * 8u, o[i]);
            bound = fminr(bound, qmax(plane - mx[i] - kSwPad * (fabsf(plane) + fabsf(mx[i]) + fabsf(o[i]) + 1.f), 0.f));
        }
        if (lo[i] > 0) {
            const uint32_t b = (uint32_t)(lo[i] - 1);
            const float plane = swTerrainCoord(hm, b >> 4, (b & 15u) * 8u + 8u, o[i]);
            bound = fminr(bound, qmax(mn[i] - plane - kSwPad * (fabsf(plane) + fabsf(mn[i]) + fabsf(o[i]) + 1.f), 0.f));
        }
    }
    return bound;
}

// ---- accelerated: one wave per volume.  [bLo, bHi]: the blocks under the volume's footprint, clamped to the map (a volume beside the map stands over the rim).
// Ring r = the blocks at Chebyshev distance r from that rectangle: ring 0 its rows, ring r > 0 the two rows and two columns of its border, clipped to the map.
// A lane takes a block of a row or column: dropped when its chunk is a hole or the chunk's box (mip level 7) or the block's (level 3) lies beyond the limit =
// min(best so far, max_distance, the merged record's distance); the 64 lanes then take the 64 cells of every surviving block (level 0), both triangles of a cell
// within the limit go to the pair test.  Ends at the first ring beyond which everything is horizontally farther than the limit, or that covers the map.
__global__ __launch_bounds__(64 * kOvWaves) void k_q_terrain_distance(uint32_t count, uint32_t merge, HeightmapParams hm, HullSet hs, const float4* __restrict__ vShape,
                                                                     const float4* __restrict__ vMin, const float4* __restrict__ vMax, const uint32_t* __restrict__ vRange,
                                                                     const float4* __restrict__ vPos, const float* __restrict__ maxDistances, uint4* out) {
    const uint32_t lane = threadIdx.x & 63u, v = blockIdx.x * kOvWaves + (threadIdx.x >> 6);
    if (v >= count) return;
    const DistanceQuery d = dsLoadQuery(vShape, vMin, vMax, vRange, maxDistances, v, 0u);
    unsigned long long best = ~0ull;
    if (d.valid) {
        float limit = d.maxD;
        if (merge) {
            const uint4 have = out[kDistanceRecordRows * (size_t)v];
            if (have.x != kRayMiss) limit = fminr(limit, __uint_as_float(have.z));
        }
        const uint32_t n = hm.chunksPerDim * kHmSegs;
        const int nb = (int)(n >> 3);
        int bLo[2], bHi[2];
        const float mapMin[2] = {hm.minX, hm.minZ}, qMin[2] = {d.q.mn.x, d.q.mn.z}, qMax[2] = {d.q.mx.x, d.q.mx.z};
#pragma unroll
        for (int a = 0; a < 2; ++a) {   // (any rectangle of blocks is a valid ring 0: it only seeds the limit)
            const float fl = (qMin[a] - mapMin[a]) / hm.chunkScale, fh = (qMax[a] - mapMin[a]) / hm.chunkScale;
            const uint32_t lo = (uint32_t)fminr(qmax(floorf(fl), 0.f), (float)(n - 1u)), hi = (uint32_t)fminr(qmax(floorf(fh), 0.f), (float)(n - 1u));
            bLo[a] = (int)(min(lo, hi) >> 3); bHi[a] = (int)(max(lo, hi) >> 3);
        }
        const uint32_t* __restrict__ mips = hm.mips;
        for (int r = 0; r < nb; ++r) {
            const int x0 = bLo[0] - r, x1 = bHi[0] + r, z0 = bLo[1] - r, z1 = bHi[1] + r;
            const int cx0 = max(x0, 0), cx1 = min(x1, nb - 1), cz0 = max(z0, 0), cz1 = min(z1, nb - 1);
            const int spans = r == 0 ? cz1 - cz0 + 1 : 4;
            for (int sp = 0; sp < spans; ++sp) {
                // span sp: the blocks (fixed, w) or (w, fixed), w in [wLo, wHi]
                bool row = true; int fixed = cz0 + sp, wLo = cx0, wHi = cx1;
                if (r != 0) {
                    row = sp < 2;
                    fixed = sp == 0 ? z0 : sp == 1 ? z1 : sp == 2 ? x0 : x1;
                    if (fixed < 0 || fixed >= nb) continue;
                    if (!row) { wLo = max(z0 + 1, 0); wHi = min(z1 - 1, nb - 1); }
                }
                for (int w0 = wLo; w0 <= wHi; w0 += 64) {
                    const int bw = w0 + (int)lane;
                    bool alive = bw <= wHi;
                    if (alive) {
                        const uint32_t bx = (uint32_t)(row ? bw : fixed), bz = (uint32_t)(row ? fixed : bw);
                        const uint32_t slot = hm.chunkSlot[(bz >> 4) * hm.chunksPerDim + (bx >> 4)];
                        alive = slot != 0xFFFFFFFFu;
                        if (alive) {
                            const uint32_t* __restrict__ chunkMips = mips + (size_t)slot * kHmMipEntries;
                            alive = !(tdBoxGap(hm, d.q, (bx >> 4) << 7, (bz >> 4) << 7, kHmSegs, chunkMips[hmMipOffset(7u)]) > limit) &&
                                    !(tdBoxGap(hm, d.q, bx << 3, bz << 3, 8u, chunkMips[hmMipOffset(3u) + (bz & 15u) * (kHmSegs >> 3) + (bx & 15u)]) > limit);
                        }
                    }
                    for (unsigned long long m = __ballot(alive); m; m &= m - 1ull) {
                        const uint32_t bs = (uint32_t)w0 + (uint32_t)__ffsll((long long)m) - 1u;
                        const uint32_t bx = row ? bs : (uint32_t)fixed, bz = row ? (uint32_t)fixed : bs;
                        const uint32_t gx = bx * 8u + (lane & 7u), gz = bz * 8u + (lane >> 3);
                        const uint32_t slot = hm.chunkSlot[(gz >> 7) * hm.chunksPerDim + (gx >> 7)];
                        const uint32_t mm = mips[(size_t)slot * kHmMipEntries + (gz & 127u) * kHmSegs + (gx & 127u)];
                        if (!(tdBoxGap(hm, d.q, gx, gz, 1u, mm) > limit)) {
                            best = min(best, tdCandidate<true>(hm, hs, d, gx, gz, 0u, limit));
                            best = min(best, tdCandidate<true>(hm, hs, d, gx, gz, 1u, limit));
                        }
                        limit = fminr(limit, dsLimit(best, limit));
                    }
                }
            }
            if (tdRingBound(hm, d.q, x0, x1, z0, z1, nb) > limit) break;   // (+inf once the box covers the map)
            if (x0 <= 0 && z0 <= 0 && x1 >= nb - 1 && z1 >= nb - 1) break;
        }
    }
    best = swWaveMin(best);
    if (lane == 0u) tdFinalise(hm, hs, d, best, vPos[v], v, merge, out);
}

}  // namespace mi
