// kernels_terrain_query.hpp — batched terrain contact queries of query volumes (mi_world_terrain_contacts*, include/mi_physics.h): the
// contacts a rigid body of the volume's shape at the volume's pose would get from the heightmap terrain in one step, in the reference's
// emission order.  Part of the ONE translation unit of the physics library (world.hip includes it after kernels_contacts_query.hpp).
// Host side: world_query.inc.
//
// There is no terrain code here: the query IS the step's terrain pipeline (heightmap.hpp: k_hm_lowest, k_hm_contacts<WRITE, LARGE>,
// k_hm_write_stashed), instantiated with the policy below in place of the step's HmOut.  Its colliders are the volume rows of
// k_ov_unpack / k_ov_prepare (kernels_overlap.hpp), its per-collider counts are plain 32-bit words scanned straight into the caller's
// offsets, and its WRITE passes put contact j of volume v into the caller's record offsets[v] + j — nothing at or past `capacity`.
// Read-only with respect to the step: everything writes query-owned buffers (QueryCache in world.hip) or the caller's result.
#pragma once
#include "heightmap.hpp"
#include "kernels_overlap.hpp"

namespace mi {

constexpr uint32_t kTqRecordRows = 2;   // mi_terrain_contact: (point, depth), (normal, volume)

struct HmQueryOut {
    uint32_t capacity; float4* records;   // [capacity][kTqRecordRows]
    typedef uint32_t Packed;              // the contacts of a volume; their exclusive scan = the CSR offsets
    static __device__ __forceinline__ bool active(const float4& mn, const float4&, uint32_t& type) {   // the volume row is valid (k_ov_unpack / k_ov_prepare)
        type = __float_as_uint(mn.w) & 0xFFu;
        return type != kOvInvalid;
    }
    static __device__ __forceinline__ Packed pack(uint32_t found) { return found; }
    __device__ __forceinline__ bool ready() const { return true; }
    __device__ __forceinline__ uint32_t first(const Packed* __restrict__ offsets, uint32_t v) const { return offsets[v]; }
    __device__ __forceinline__ uint32_t total(const Packed* __restrict__ offsets, uint32_t count) const { return min(offsets[count], capacity); }   // (the contacts that have a record)
    __device__ __forceinline__ void put(uint32_t first, uint32_t v, uint32_t j, uint32_t, const TriContact& t) const {
        const uint32_t p = first + j;
        if (p >= capacity) return;
        records[kTqRecordRows * (size_t)p] = f4(t.point, t.depth);
        records[kTqRecordRows * (size_t)p + 1] = f4(t.normal, __uint_as_float(v));
    }
};

// behind the scan: the full total for the caller (device variant)
__global__ void k_tq_total(uint32_t count, const uint32_t* __restrict__ offsets, uint32_t* __restrict__ total) { total[0] = offsets[count]; }

}  // namespace mi
