// Part of world.hip (one translation unit; #included there, after world_state.inc): batched ray-cast scene queries (include/mi_physics.h,
// mi_world_raycast*; kernels in kernels_query.hpp).
//
// The query structure (world AABBs, uniform grid, large list) is built lazily on the world's stream and cached per pose epoch: every
// internal step, upload (any topology or heightmap edit), body-state write, checkpoint load and shard import bumps mi_world::poseEpoch,
// and the first query of a new epoch rebuilds.  A build enqueues nine launches and no host synchronisation; it writes the query's own
// buffers only, so a query never changes what a later step computes.

int mi_world::queryBuild() {
    QueryCache& qc = query;
    const uint32_t nc = (uint32_t)colliders.size(), nb = (uint32_t)bodies.size();
    if (qc.builtEpoch == poseEpoch && qc.nc == nc) return MI_OK;
    const uint32_t maxCells = std::min<uint32_t>(std::max<uint32_t>(4u * nc, 4096u), 1u << 22);
    HIP_TRY(qc.shape.ensure(3 * (size_t)std::max(nc, 1u))); HIP_TRY(qc.mn.ensure(std::max(nc, 1u))); HIP_TRY(qc.mx.ensure(std::max(nc, 1u)));
    HIP_TRY(qc.grid.ensure(1)); HIP_TRY(qc.large.ensure(std::max(nc, 1u))); HIP_TRY(qc.partials.ensure(2 * (size_t)divUp(std::max(nc, 1u), 256)));
    HIP_TRY(qc.entries.ensure((size_t)std::max(nc, 1u) * kQMaxCellsPerCollider));
    HIP_TRY(qc.count.ensure((size_t)maxCells + 1)); HIP_TRY(qc.start.ensure((size_t)maxCells + 1));
    Launcher& L = qc.L;
    L.begin(false, false);
    HIP_TRY(L.memsetAsync(qc.count.p, 0, ((size_t)maxCells + 1) * sizeof(uint32_t), stream));
    if (nc) {
        const uint32_t blocks = divUp(nc, 256);
        L.launch(k_q_colliders, dim3(blocks), dim3(256), 0, stream, nc, nb, cTypeBody.p, cObject.p, cShape.p, cStaticPos.p, cStaticRot.p, bPos.p, bRot.p, hullAabb.p,
                 qc.shape.p, qc.mn.p, qc.mx.p, qc.partials.p);
        L.launch(k_q_mean, dim3(1), dim3(kQParamThreads), 0, stream, blocks, (const QPartial*)qc.partials.p, qc.grid.p);
        L.launch(k_q_filter, dim3(blocks), dim3(256), 0, stream, nc, (const float4*)qc.mn.p, (const float4*)qc.mx.p, (const QueryGrid*)qc.grid.p, qc.partials.p + blocks);
        L.launch(k_q_params, dim3(1), dim3(kQParamThreads), 0, stream, blocks, maxCells, (const QPartial*)(qc.partials.p + blocks), qc.grid.p);
        L.launch(k_q_count, dim3(divUp(nc, 256)), dim3(256), 0, stream, nc, (const float4*)qc.mn.p, (const float4*)qc.mx.p, qc.grid.p, qc.count.p, qc.large.p);
        HIP_TRY(qc.scan.run(L, qc.count.p, qc.start.p, maxCells + 1, stream, true));
        L.launch(k_q_scatter, dim3(divUp(nc, 256)), dim3(256), 0, stream, nc, (const float4*)qc.mn.p, (const float4*)qc.mx.p, (const QueryGrid*)qc.grid.p,
                 (const uint32_t*)qc.start.p, qc.count.p, qc.entries.p);
    } else {
        HIP_TRY(L.memsetAsync(qc.grid.p, 0, sizeof(QueryGrid), stream));
        HIP_TRY(L.memsetAsync(qc.start.p, 0, ((size_t)maxCells + 1) * sizeof(uint32_t), stream));
    }
    if (L.firstError != hipSuccess) return fail(MI_ERR_DEVICE, std::string("query structure: ") + hipGetErrorString(L.firstError));
    qc.builtEpoch = poseEpoch; qc.nc = nc;
    return MI_OK;
}

static QueryScene queryScene(mi_world* w) {
    QueryScene s{};
    s.nc = (uint32_t)w->colliders.size();
    s.cTypeBody = w->cTypeBody.p; s.cObject = w->cObject.p; s.cEntity = w->cEntity.p;
    s.cShape = w->cShape.p; s.cStaticPos = w->cStaticPos.p; s.cStaticRot = w->cStaticRot.p;
    s.bPos = w->bPos.p; s.bRot = w->bRot.p;
    s.hf = HullFaces{w->hullVerts.p, w->hullRanges.p, w->hullTris.p, w->hullTriRanges.p};
    s.hasTerrain = 0u;
    if (w->heightmap) { s.hm = w->hmParams; s.hasTerrain = 1u; }
    return s;
}
// what every variant checks first; afterwards the device holds the current scene (pending host edits uploaded)
static int queryPrepare(mi_world* w) {
    if (w->shard.enabled) return fail(MI_ERR_UNSUPPORTED, "ray queries on a sharded world: a rank holds only its tile");
    return ensureUploaded(w);
}
// accelerated (exhaustive = false) or exhaustive ray kernel over rays already on the device
static int queryEnqueue(mi_world* w, uint32_t count, const float* raysDev, uint32_t include, const uint32_t* rangesDev, void* outDev, bool exhaustive) {
    const QueryScene s = queryScene(w);
    uint32_t* out = static_cast<uint32_t*>(outDev);
    if (exhaustive) {
        k_q_exhaustive<<<count, 256, 0, w->stream>>>(raysDev, rangesDev, include, s, out);
    } else {
        int rc = w->queryBuild(); if (rc != MI_OK) return rc;
        mi_world::QueryCache& qc = w->query;
        k_q_raycast<<<divUp(count, 256), 256, 0, w->stream>>>(count, raysDev, rangesDev, include, s, qc.grid.p, qc.start.p, qc.entries.p, qc.large.p, out);
    }
    HIP_TRY(hipGetLastError());
    return MI_OK;
}
static int queryHost(mi_world* w, uint32_t count, const float* origins, const float* directions, const float* maxT, uint32_t include, const uint32_t* ranges,
                     mi_ray_hit* out, bool exhaustive) {
    if (!w || (count && (!origins || !directions || !out))) return fail(MI_ERR_INVALID_ARGUMENT, "null argument");
    int rc = queryPrepare(w); if (rc != MI_OK) return rc;
    if (!count) return MI_OK;
    std::vector<float> rays(8 * (size_t)count, 0.f);
    for (uint32_t r = 0; r < count; ++r) {
        for (int k = 0; k < 3; ++k) { rays[8 * (size_t)r + k] = origins[3 * (size_t)r + k]; rays[8 * (size_t)r + 3 + k] = directions[3 * (size_t)r + k]; }
        rays[8 * (size_t)r + 6] = maxT ? maxT[r] : std::numeric_limits<float>::infinity();
    }
    mi_world::QueryCache& qc = w->query;
    HIP_TRY(qc.rays.ensure(rays.size())); HIP_TRY(qc.hits.ensure(10 * (size_t)count));
    HIP_TRY(hipMemcpyAsync(qc.rays.p, rays.data(), rays.size() * sizeof(float), hipMemcpyHostToDevice, w->stream));
    if (ranges) {
        HIP_TRY(qc.ranges.ensure(2 * (size_t)count));
        HIP_TRY(hipMemcpyAsync(qc.ranges.p, ranges, 2 * (size_t)count * sizeof(uint32_t), hipMemcpyHostToDevice, w->stream));
    }
    rc = queryEnqueue(w, count, qc.rays.p, include, ranges ? qc.ranges.p : nullptr, qc.hits.p, exhaustive); if (rc != MI_OK) return rc;
    HIP_TRY(hipMemcpyAsync(out, qc.hits.p, (size_t)count * sizeof(mi_ray_hit), hipMemcpyDeviceToHost, w->stream));
    HIP_TRY(hipStreamSynchronize(w->stream));   // (the rays / ranges were pageable host memory as well)
    return MI_OK;
}

extern "C" {

MI_API int mi_world_raycast(mi_world* w, uint32_t count, const float* origins3, const float* directions3, const float* maxT, uint32_t include,
                            const uint32_t* ranges2, mi_ray_hit* out) {
    return queryHost(w, count, origins3, directions3, maxT, include, ranges2, out, false);
}
MI_API int mi_debug_raycast_exhaustive(mi_world* w, uint32_t count, const float* origins3, const float* directions3, const float* maxT, uint32_t include,
                                       const uint32_t* ranges2, mi_ray_hit* out) {
    return queryHost(w, count, origins3, directions3, maxT, include, ranges2, out, true);
}
MI_API int mi_world_raycast_device_async(mi_world* w, uint32_t count, const float* rays8Dev, uint32_t include, const uint32_t* ranges2Dev, mi_ray_hit* outDev) {
    if (!w || (count && (!rays8Dev || !outDev))) return fail(MI_ERR_INVALID_ARGUMENT, "null argument");
    int rc = queryPrepare(w); if (rc != MI_OK) return rc;
    if (!count) return MI_OK;
    return queryEnqueue(w, count, rays8Dev, include, ranges2Dev, outDev, false);
}

}  // extern "C"
