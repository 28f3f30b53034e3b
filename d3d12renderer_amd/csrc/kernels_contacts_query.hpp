// kernels_contacts_query.hpp — batched contact-manifold scene queries (mi_world_volume_contacts*, include/mi_physics.h): where a sphere,
// capsule, cylinder, box or hull touches the world, along which normal and how deep.  Part of the ONE translation unit of the physics
// library (world.hip includes it after kernels_overlap.hpp, whose volume rows, predicate and ordering it uses).  Host side: world_query.inc.
//
// Read-only with respect to the step: everything here writes query-owned buffers (QueryCache in world.hip) or the caller's result.
//   candidates      the overlap query's passes with ovTest<true> (object type, entity range, closed AABBs; no overlapCheck) into a
//                   library-owned buffer of (entity, collider, object type, volume): ascending collider index per volume
//   k_vc_narrow     one lane per candidate: the step's narrow phase of the pair into a fixed 96-byte slot.  Primitive pairs through
//                   intersectPair, box pairs through obbSat + obbContactsLds (clip polygons in LDS); a GJK-backed pair only enters a queue
//   k_vc_gjk        one wave per queued candidate: gjkPhaseWave + epaPhaseWave, the functions the step's k_narrow_gjk_wave runs (polytope
//                   in LDS; the lane-per-pair form with ~12 KB of scratch per lane stays out of both kernels)
//   k_exclusive_scan   over "slot has a contact"
//   k_vc_write      slots with a contact -> the caller's records, candidate offsets -> record offsets, the two totals
// No collision arithmetic lives here: A = the smaller world type (the volume for equal types), and (A, B) go to the step's functions.
// `bound` = the candidates the staging holds (the host passes what it reserved): every count read from device memory is clamped to it.
#pragma once
#include "kernels_overlap.hpp"

namespace mi {

constexpr uint32_t kVcSlotRows = 6;          // mi_volume_contact: 96 bytes = 6 rows of 16
constexpr uint32_t kVcGjkMaxBlocks = 16384;  // k_vc_gjk strides over its queue

struct VcPair { Shape a, b; uint32_t ta, tb, volumeIsB; bool ok; };
// candidate i -> (A, B) as the narrow phase takes them
__device__ __forceinline__ VcPair vcLoadPair(const uint4 c, uint32_t count, const OverlapScene& s, const float4* __restrict__ vShape, const float4* __restrict__ vMin) {
    VcPair r; r.ok = false; r.ta = r.tb = 0u; r.volumeIsB = 0u;
    const uint32_t k = c.y, v = c.w;
    if (k >= s.nc || v >= count) return r;   // (never: the candidate pass wrote them)
    const uint32_t tk = __float_as_uint(s.mn[k].w) & 0xFFu, tv = __float_as_uint(vMin[v].w) & 0xFFu;
    if (tk > (uint32_t)T_HULL || tv > (uint32_t)T_HULL) return r;
    const Shape sk = loadShape(s.shape, k, tk), sv = loadShape(vShape, v, tv);
    r.volumeIsB = tk < tv ? 1u : 0u;
    if (r.volumeIsB) { r.a = sk; r.b = sv; r.ta = tk; r.tb = tv; } else { r.a = sv; r.b = sk; r.ta = tv; r.tb = tk; }
    r.ok = true;
    return r;
}
// (static indices: the manifold stays in registers)
__device__ __forceinline__ void vcWriteSlot(uint4* __restrict__ slots, uint32_t* __restrict__ flags, uint32_t i, const uint4 c, uint32_t volumeIsB, bool hit, const Manifold& m) {
    const uint32_t cnt = hit ? min(m.count, 4u) : 0u;
    flags[i] = cnt ? 1u : 0u;
    if (!cnt) return;
    uint4* o = slots + (size_t)i * kVcSlotRows;
    o[0] = c;
    o[1] = make_uint4(__float_as_uint(m.n.x), __float_as_uint(m.n.y), __float_as_uint(m.n.z), cnt | (volumeIsB << 8));
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k)
        o[2 + k] = k < cnt ? make_uint4(__float_as_uint(m.p[k].x), __float_as_uint(m.p[k].y), __float_as_uint(m.p[k].z), __float_as_uint(m.d[k])) : make_uint4(0u, 0u, 0u, 0u);
}

// lanes [0, n): the pair of candidate i; lanes [n, bound]: flags = 0 (the scan reads bound + 1 words).  n = min(candidates found, bound).
__global__ __launch_bounds__(256) void k_vc_narrow(uint32_t bound, uint32_t count, const uint32_t* __restrict__ candOffsets, const uint4* __restrict__ cand, OverlapScene s,
                                                   const float4* __restrict__ vShape, const float4* __restrict__ vMin, uint4* __restrict__ slots, uint32_t* __restrict__ flags,
                                                   uint32_t* __restrict__ gjkQueue, uint32_t* __restrict__ gjkCount) {
    __shared__ float4 polyMem[kLdsPolyVerts * kLdsPolyStride];   // 32 KiB: one clip polygon per lane, as in k_narrow_clip
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t n = min(candOffsets[count], bound);
    bool queued = false;
    if (i >= n) { if (i <= bound) flags[i] = 0u; }
    else {
        const uint4 c = cand[i];
        const VcPair pr = vcLoadPair(c, count, s, vShape, vMin);
        Manifold m; m.count = 0;
        if (!pr.ok) flags[i] = 0u;
        else if (gjkMode(pr.ta, pr.tb) >= 0) { queued = true; flags[i] = 0u; }   // (k_vc_gjk sets it)
        else if (pr.tb == T_OBB && (pr.ta == T_OBB || pr.ta == T_AABB)) {
            Q4 arot, brot; V3 acen, arad, bcen, brad;
            boxPairOfShapes(pr.a, pr.b, pr.ta, arot, acen, arad, brot, bcen, brad);
            ObbSat res;
            bool hit = false;
            if (obbSat(arot, acen, arad, brot, bcen, brad, res)) {
                LdsPoly poly{polyMem + threadIdx.x, 0u};
                hit = obbContactsLds(arot, acen, arad, brot, bcen, brad, res, poly, m);
            }
            vcWriteSlot(slots, flags, i, c, pr.volumeIsB, hit, m);
        } else {
            const bool hit = intersectPair(pr.a, pr.b, s.hs, m);
            vcWriteSlot(slots, flags, i, c, pr.volumeIsB, hit, m);
        }
    }
    const uint32_t slot = waveAppendSlot(queued, gjkCount);   // (i < n <= bound: the queue of `bound` words holds every candidate)
    if (queued && slot < bound) gjkQueue[slot] = i;
}

// one wave per queued candidate (any order: the slot is the candidate's)
__global__ __launch_bounds__(64) void k_vc_gjk(uint32_t bound, uint32_t count, const uint32_t* __restrict__ candOffsets, const uint4* __restrict__ cand, OverlapScene s,
                                               const float4* __restrict__ vShape, const float4* __restrict__ vMin, uint4* __restrict__ slots, uint32_t* __restrict__ flags,
                                               const uint32_t* __restrict__ gjkQueue, const uint32_t* __restrict__ gjkCount) {
    __shared__ __attribute__((aligned(16))) unsigned char ldsRaw[sizeof(EpaLds)];
    EpaLds& lds = *reinterpret_cast<EpaLds*>(ldsRaw);
    const uint32_t lane = threadIdx.x;
    const uint32_t n = min(candOffsets[count], bound), queued = min(gjkCount[0], n);
    for (uint32_t entry = blockIdx.x; entry < queued; entry += gridDim.x) {
        const uint32_t i = gjkQueue[entry];
        if (i >= n) continue;   // (uniform; never: k_vc_narrow queued lanes below n)
        const uint4 c = cand[i];
        const VcPair pr = vcLoadPair(c, count, s, vShape, vMin);
        const int mode = pr.ok ? gjkMode(pr.ta, pr.tb) : -1;
        if (mode < 0) continue;   // (uniform)
        Simplex sx; Manifold m; m.count = 0;
        const int r = gjkPhaseWave(pr.a, pr.b, s.hs, mode, sx, m, lane);
        if (r == 2) epaPhaseWave(pr.a, pr.b, s.hs, mode, sx, lds, m, lane);
        if (lane == 0) vcWriteSlot(slots, flags, i, c, pr.volumeIsB, r != 0, m);
        __syncthreads();   // the polytope in LDS is reused by the next entry
    }
}

// scan = exclusive scan of flags over [0, bound]: scan[i] = the record of candidate i, scan[n] = the records
__global__ __launch_bounds__(256) void k_vc_write(uint32_t bound, uint32_t count, uint32_t capacity, const uint32_t* __restrict__ candOffsets, const uint32_t* __restrict__ flags,
                                                  const uint32_t* __restrict__ scan, const uint4* __restrict__ slots, uint4* __restrict__ out, uint32_t* __restrict__ outOffsets,
                                                  uint32_t* __restrict__ totals2) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t found = candOffsets[count], n = min(found, bound);
    if (i == 0u && totals2) { totals2[0] = scan[n]; totals2[1] = found; }
    if (i <= count) outOffsets[i] = scan[min(candOffsets[i], n)];
    if (i < n && flags[i]) {
        const uint32_t r = scan[i];
        if (r < capacity) {
#pragma unroll
            for (uint32_t k = 0; k < kVcSlotRows; ++k) out[(size_t)r * kVcSlotRows + k] = slots[(size_t)i * kVcSlotRows + k];
        }
    }
}

}  // namespace mi
