// Part of world.hip (one translation unit; #included there, after world_state.inc): batched scene queries (include/mi_physics.h): ray casts
// (mi_world_raycast*; kernels in kernels_query.hpp), volume overlaps (mi_world_overlap*; kernels in kernels_overlap.hpp) and the contact manifolds of
// query volumes (mi_world_volume_contacts*; kernels in kernels_contacts_query.hpp).
//
// The query structure (world AABBs, uniform grid, large list) is built lazily on the world's stream and cached per pose epoch: every
// internal step, upload (any topology or heightmap edit), body-state write, checkpoint load and shard import bumps mi_world::poseEpoch,
// and the first query of a new epoch rebuilds.  A build enqueues nine launches and no host synchronisation; it writes the query's own
// buffers only, so a query never changes what a later step computes.

int mi_world::queryBuild() {
    QueryCache& qc = query;
    const uint32_t nc = (uint32_t)colliders.size();
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
        L.launch(k_q_colliders, dim3(blocks), dim3(256), 0, stream, nc, colliderRows(bPos.p, bRot.p, qc.shape.p, qc.mn.p, qc.mx.p), qc.partials.p);
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
    if (w->shard.enabled) return fail(MI_ERR_UNSUPPORTED, "scene queries on a sharded world: a rank holds only its tile");
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


// ---- volume overlaps.  Volume rows (two launches), count pass, device scan, write pass: five launches behind the (shared) grid build, no read-back between them.
// passes: kOvPassCount = volume rows, count pass and scan; kOvPassWrite = the write pass over what a count pass of the same arguments left (nothing else
// enqueued in between).  boxesOnly: ovTest without overlapCheck — the candidates of the contact query.
int mi_world::overlapEnqueue(uint32_t count, const uint32_t* volumesDev, uint32_t include, const uint32_t* rangesDev, uint32_t* offsetsDev, uint4* hitsDev,
                             uint32_t capacity, uint32_t* totalDev, bool exhaustive, uint32_t passes, bool boxesOnly) {
    QueryCache& qc = query;
    const uint32_t nc = (uint32_t)colliders.size();
    const bool first = (passes & kOvPassCount) != 0u;
    if (!exhaustive && first) { int rc = queryBuild(); if (rc != MI_OK) return rc; }
    HIP_TRY(qc.vShape.ensure(3 * (size_t)count)); HIP_TRY(qc.vMn.ensure(count)); HIP_TRY(qc.vMx.ensure(count));
    HIP_TRY(qc.vRange.ensure(2 * (size_t)count)); HIP_TRY(qc.vCount.ensure((size_t)count + 1));
    HIP_TRY(qc.vcTypeBody.ensure(2 * (size_t)count)); HIP_TRY(qc.vcObject.ensure(count)); HIP_TRY(qc.vcShape.ensure(3 * (size_t)count)); HIP_TRY(qc.vcPos.ensure(count)); HIP_TRY(qc.vcRot.ensure(count));
    OverlapScene s{};
    s.nc = nc; s.cEntity = cEntity.p; s.hs = HullSet{hullVerts.p, hullRanges.p};
    Launcher& L = qc.L;
    L.begin(false, false);
    if (exhaustive) {   // its own world rows at the current poses: the yardstick does not trust the cache
        HIP_TRY(qc.xShape.ensure(3 * (size_t)std::max(nc, 1u))); HIP_TRY(qc.xMn.ensure(std::max(nc, 1u))); HIP_TRY(qc.xMx.ensure(std::max(nc, 1u)));
        HIP_TRY(qc.xPartials.ensure(divUp(std::max(nc, 1u), 256)));
        if (nc && first) L.launch(k_q_colliders, dim3(divUp(nc, 256)), dim3(256), 0, stream, nc, colliderRows(bPos.p, bRot.p, qc.xShape.p, qc.xMn.p, qc.xMx.p), qc.xPartials.p);
        s.shape = qc.xShape.p; s.mn = qc.xMn.p; s.mx = qc.xMx.p;
    } else { s.shape = qc.shape.p; s.mn = qc.mn.p; s.mx = qc.mx.p; }
    const dim3 grid(divUp(count, kOvWaves)), block(64 * kOvWaves);
    if (first) {
        L.launch(k_ov_unpack, dim3(divUp(count, 256)), dim3(256), 0, stream, count, volumesDev, rangesDev, (uint32_t)hulls.size(), qc.vcTypeBody.p, qc.vcObject.p, qc.vcShape.p,
                 qc.vcPos.p, qc.vcRot.p, qc.vRange.p);
        ColliderRows volumes = colliderRows(nullptr, nullptr /* (no bodies) */, qc.vShape.p, qc.vMn.p, qc.vMx.p);   // the volumes as static colliders; the world's hulls
        volumes.cTypeBody = qc.vcTypeBody.p; volumes.cObject = qc.vcObject.p; volumes.cShape = qc.vcShape.p; volumes.cStaticPos = qc.vcPos.p; volumes.cStaticRot = qc.vcRot.p; volumes.nb = 0u;
        L.launch(k_ov_prepare, dim3(divUp(count, 256)), dim3(256), 0, stream, count, volumes);
    }
    for (uint32_t pass = 0; pass < 2u; ++pass) {
        if (!(passes & (pass ? kOvPassWrite : kOvPassCount))) continue;
        if (exhaustive)
            L.launch(boxesOnly ? k_q_overlap_exhaustive<true> : k_q_overlap_exhaustive<false>, grid, block, 0, stream, pass, count, include, s, (const float4*)qc.vShape.p,
                     (const float4*)qc.vMn.p, (const float4*)qc.vMx.p, (const uint32_t*)qc.vRange.p, qc.vCount.p, (const uint32_t*)offsetsDev, hitsDev, capacity, totalDev);
        else
            L.launch(boxesOnly ? k_q_overlap<true> : k_q_overlap<false>, grid, block, 0, stream, pass, count, include, s, (const float4*)qc.vShape.p, (const float4*)qc.vMn.p,
                     (const float4*)qc.vMx.p, (const uint32_t*)qc.vRange.p, (const QueryGrid*)qc.grid.p, (const uint32_t*)qc.start.p, (const uint32_t*)qc.entries.p,
                     (const uint32_t*)qc.large.p, qc.vCount.p, (const uint32_t*)offsetsDev, hitsDev, capacity, totalDev);
        if (pass == 0u) HIP_TRY(qc.scan2.run(L, qc.vCount.p, offsetsDev, count + 1u, stream, false));
    }
    if (L.firstError != hipSuccess) return fail(MI_ERR_DEVICE, std::string("overlap query: ") + hipGetErrorString(L.firstError));
    return MI_OK;
}
static int overlapHost(mi_world* w, uint32_t count, const mi_query_volume* volumes, uint32_t include, const uint32_t* ranges, uint32_t* outOffsets, mi_overlap_hit* outHits,
                       uint32_t capacity, uint32_t* outTotal, bool exhaustive) {
    if (!w || (count && (!volumes || !outOffsets || !outTotal || (capacity && !outHits)))) return fail(MI_ERR_INVALID_ARGUMENT, "null argument");
    int rc = queryPrepare(w); if (rc != MI_OK) return rc;
    if (outTotal) *outTotal = 0u;
    if (outOffsets) outOffsets[0] = 0u;
    if (!count) return MI_OK;
    mi_world::QueryCache& qc = w->query;
    HIP_TRY(qc.volumes.ensure(kOvVolumeWords * (size_t)count)); HIP_TRY(qc.vOffsets.ensure((size_t)count + 1)); HIP_TRY(qc.vHits.ensure(std::max(capacity, 1u)));
    HIP_TRY(hipMemcpyAsync(qc.volumes.p, volumes, (size_t)count * sizeof(mi_query_volume), hipMemcpyHostToDevice, w->stream));
    if (ranges) {
        HIP_TRY(qc.ranges.ensure(2 * (size_t)count));
        HIP_TRY(hipMemcpyAsync(qc.ranges.p, ranges, 2 * (size_t)count * sizeof(uint32_t), hipMemcpyHostToDevice, w->stream));
    }
    rc = w->overlapEnqueue(count, qc.volumes.p, include, ranges ? qc.ranges.p : nullptr, qc.vOffsets.p, qc.vHits.p, capacity, nullptr, exhaustive, capacity == 0u ? kOvPassCount : kOvPassCount | kOvPassWrite, false);
    if (rc != MI_OK) return rc;
    HIP_TRY(hipMemcpyAsync(outOffsets, qc.vOffsets.p, ((size_t)count + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, w->stream));
    HIP_TRY(hipStreamSynchronize(w->stream));
    const uint32_t total = outOffsets[count];
    *outTotal = total;
    const uint32_t n = std::min(total, capacity);
    if (n) {
        HIP_TRY(hipMemcpyAsync(outHits, qc.vHits.p, (size_t)n * sizeof(mi_overlap_hit), hipMemcpyDeviceToHost, w->stream));
        HIP_TRY(hipStreamSynchronize(w->stream));
    }
    if (total > capacity && (capacity || outHits)) return fail(MI_ERR_CAPACITY, "capacity < overlap records (out_total holds the number)");
    return MI_OK;
}

// ---- contact manifolds of query volumes.  Candidates by the overlap passes in boxes-only mode, then narrow phase, GJK queue, scan and write: no read-back
// between them.  `bound` = the candidates evaluated, at most what contactsReserve() sized the staging for.
int mi_world::contactsReserve(uint32_t maxCandidates) {
    QueryCache& qc = query;
    if (maxCandidates <= qc.candCap) return MI_OK;
    const size_t n = maxCandidates;
    HIP_TRY(qc.cCand.ensure(n)); HIP_TRY(qc.cSlots.ensure(n * kVcSlotRows)); HIP_TRY(qc.cFlags.ensure(n + 1)); HIP_TRY(qc.cScan.ensure(n + 1));
    HIP_TRY(qc.cQueue.ensure(n)); HIP_TRY(qc.cQueueN.ensure(1));
    qc.candCap = maxCandidates;
    return MI_OK;
}
int mi_world::contactsEnqueue(uint32_t count, uint32_t bound, uint32_t capacity, uint4* contactsDev, uint32_t* offsetsDev, uint32_t* totals2Dev, bool exhaustive) {
    QueryCache& qc = query;
    if (bound > qc.candCap) return fail(MI_ERR_INVALID_ARGUMENT, "contact query: more candidates than reserved");
    HIP_TRY(qc.cFlags.ensure(1)); HIP_TRY(qc.cScan.ensure(1)); HIP_TRY(qc.cQueueN.ensure(1));   // (bound 0: the scan still reads one word)
    OverlapScene s{};
    s.nc = (uint32_t)colliders.size(); s.cEntity = cEntity.p; s.hs = HullSet{hullVerts.p, hullRanges.p};
    if (exhaustive) { s.shape = qc.xShape.p; s.mn = qc.xMn.p; s.mx = qc.xMx.p; } else { s.shape = qc.shape.p; s.mn = qc.mn.p; s.mx = qc.mx.p; }
    Launcher& L = qc.L;
    L.begin(false, false);
    HIP_TRY(L.memsetAsync(qc.cQueueN.p, 0, sizeof(uint32_t), stream));
    qc.cTimed = timingLevel != 0u;   // (opt-in, as the step's stage times: events between launches leave the device idle for a few microseconds)
    if (qc.cTimed) for (hipEvent_t& e : qc.cEv) if (!e) HIP_TRY(hipEventCreate(&e));
    if (qc.cTimed) HIP_TRY(hipEventRecord(qc.cEv[0], stream));
    L.launch(k_vc_narrow, dim3(divUp(bound + 1u, 256)), dim3(256), 0, stream, bound, count, (const uint32_t*)qc.cOffsets.p, (const uint4*)qc.cCand.p, s, (const float4*)qc.vShape.p,
             (const float4*)qc.vMn.p, qc.cSlots.p, qc.cFlags.p, qc.cQueue.p, qc.cQueueN.p);
    if (qc.cTimed) HIP_TRY(hipEventRecord(qc.cEv[1], stream));
    if (bound)
        L.launch(k_vc_gjk, dim3(std::min(bound, kVcGjkMaxBlocks)), dim3(64), 0, stream, bound, count, (const uint32_t*)qc.cOffsets.p, (const uint4*)qc.cCand.p, s, (const float4*)qc.vShape.p,
                 (const float4*)qc.vMn.p, qc.cSlots.p, qc.cFlags.p, (const uint32_t*)qc.cQueue.p, (const uint32_t*)qc.cQueueN.p);
    if (qc.cTimed) HIP_TRY(hipEventRecord(qc.cEv[2], stream));
    HIP_TRY(qc.scan3.run(L, qc.cFlags.p, qc.cScan.p, bound + 1u, stream, false));
    L.launch(k_vc_write, dim3(divUp(std::max(bound, count + 1u), 256)), dim3(256), 0, stream, bound, count, capacity, (const uint32_t*)qc.cOffsets.p, (const uint32_t*)qc.cFlags.p,
             (const uint32_t*)qc.cScan.p, (const uint4*)qc.cSlots.p, contactsDev, offsetsDev, totals2Dev);
    if (qc.cTimed) HIP_TRY(hipEventRecord(qc.cEv[3], stream));
    if (L.firstError != hipSuccess) return fail(MI_ERR_DEVICE, std::string("contact query: ") + hipGetErrorString(L.firstError));
    return MI_OK;
}
static int contactsHost(mi_world* w, uint32_t count, const mi_query_volume* volumes, uint32_t include, const uint32_t* ranges, uint32_t* outOffsets, mi_volume_contact* outContacts,
                        uint32_t capacity, uint32_t* outTotal, bool exhaustive) {
    if (!w || (count && (!volumes || !outOffsets || !outTotal || (capacity && !outContacts)))) return fail(MI_ERR_INVALID_ARGUMENT, "null argument");
    int rc = queryPrepare(w); if (rc != MI_OK) return rc;
    if (outTotal) *outTotal = 0u;
    if (outOffsets) outOffsets[0] = 0u;
    if (!count) return MI_OK;
    mi_world::QueryCache& qc = w->query;
    HIP_TRY(qc.volumes.ensure(kOvVolumeWords * (size_t)count)); HIP_TRY(qc.cOffsets.ensure((size_t)count + 1)); HIP_TRY(qc.cOutOffsets.ensure((size_t)count + 1));
    HIP_TRY(qc.cOut.ensure((size_t)std::max(capacity, 1u) * kVcSlotRows)); HIP_TRY(qc.cTotals.ensure(2));
    HIP_TRY(hipMemcpyAsync(qc.volumes.p, volumes, (size_t)count * sizeof(mi_query_volume), hipMemcpyHostToDevice, w->stream));
    if (ranges) {
        HIP_TRY(qc.ranges.ensure(2 * (size_t)count));
        HIP_TRY(hipMemcpyAsync(qc.ranges.p, ranges, 2 * (size_t)count * sizeof(uint32_t), hipMemcpyHostToDevice, w->stream));
    }
    const uint32_t* rangesDev = ranges ? qc.ranges.p : nullptr;
    // the candidate total is read back once (this call synchronises anyway) and sizes the staging; the write pass follows on the same rows
    rc = w->overlapEnqueue(count, qc.volumes.p, include, rangesDev, qc.cOffsets.p, nullptr, 0u, nullptr, exhaustive, kOvPassCount, true); if (rc != MI_OK) return rc;
    uint32_t candidates = 0;
    HIP_TRY(hipMemcpyAsync(&candidates, qc.cOffsets.p + count, sizeof(uint32_t), hipMemcpyDeviceToHost, w->stream));
    HIP_TRY(hipStreamSynchronize(w->stream));
    rc = w->contactsReserve(candidates); if (rc != MI_OK) return rc;
    if (candidates) { rc = w->overlapEnqueue(count, qc.volumes.p, include, rangesDev, qc.cOffsets.p, qc.cCand.p, candidates, nullptr, exhaustive, kOvPassWrite, true); if (rc != MI_OK) return rc; }
    rc = w->contactsEnqueue(count, candidates, capacity, qc.cOut.p, qc.cOutOffsets.p, qc.cTotals.p, exhaustive); if (rc != MI_OK) return rc;
    HIP_TRY(hipMemcpyAsync(outOffsets, qc.cOutOffsets.p, ((size_t)count + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, w->stream));
    HIP_TRY(hipStreamSynchronize(w->stream));
    const uint32_t total = outOffsets[count];
    *outTotal = total;
    const uint32_t n = std::min(total, capacity);
    if (n) {
        HIP_TRY(hipMemcpyAsync(outContacts, qc.cOut.p, (size_t)n * sizeof(mi_volume_contact), hipMemcpyDeviceToHost, w->stream));
        HIP_TRY(hipStreamSynchronize(w->stream));
    }
    if (total > capacity && (capacity || outContacts)) return fail(MI_ERR_CAPACITY, "capacity < contact records (out_total holds the number)");
    return MI_OK;
}

extern "C" {

MI_API int mi_world_volume_contacts(mi_world* w, uint32_t count, const mi_query_volume* volumes, uint32_t include, const uint32_t* ranges2, uint32_t* outOffsets,
                                    mi_volume_contact* outContacts, uint32_t capacity, uint32_t* outTotal) {
    return contactsHost(w, count, volumes, include, ranges2, outOffsets, outContacts, capacity, outTotal, false);
}
MI_API int mi_debug_volume_contacts_exhaustive(mi_world* w, uint32_t count, const mi_query_volume* volumes, uint32_t include, const uint32_t* ranges2, uint32_t* outOffsets,
                                               mi_volume_contact* outContacts, uint32_t capacity, uint32_t* outTotal) {
    return contactsHost(w, count, volumes, include, ranges2, outOffsets, outContacts, capacity, outTotal, true);
}
MI_API int mi_debug_volume_contacts_times(mi_world* w, float* outMs3) {
    if (!w || !outMs3) return fail(MI_ERR_INVALID_ARGUMENT, "null argument");
    outMs3[0] = outMs3[1] = outMs3[2] = 0.f;
    mi_world::QueryCache& qc = w->query;
    if (!qc.cTimed) return MI_OK;
    HIP_TRY(hipEventSynchronize(qc.cEv[3]));
    HIP_TRY(hipEventElapsedTime(&outMs3[0], qc.cEv[0], qc.cEv[1])); HIP_TRY(hipEventElapsedTime(&outMs3[1], qc.cEv[1], qc.cEv[2])); HIP_TRY(hipEventElapsedTime(&outMs3[2], qc.cEv[0], qc.cEv[3]));
    return MI_OK;
}
MI_API int mi_world_volume_contacts_reserve(mi_world* w, uint32_t maxCandidates) {
    if (!w) return fail(MI_ERR_INVALID_ARGUMENT, "null argument");
    if (w->shard.enabled) return fail(MI_ERR_UNSUPPORTED, "scene queries on a sharded world: a rank holds only its tile");
    HIP_TRY(hipStreamSynchronize(w->stream));   // (growing frees the old staging: nothing enqueued may still read it)
    return w->contactsReserve(maxCandidates);
}
MI_API int mi_world_volume_contacts_device_async(mi_world* w, uint32_t count, const mi_query_volume* volumesDev, uint32_t include, const uint32_t* ranges2Dev, uint32_t* offsetsDev,
                                                 mi_volume_contact* contactsDev, uint32_t capacity, uint32_t* totals2Dev) {
    if (!w || (count && (!volumesDev || !offsetsDev || !totals2Dev || (capacity && !contactsDev)))) return fail(MI_ERR_INVALID_ARGUMENT, "null argument");
    int rc = queryPrepare(w); if (rc != MI_OK) return rc;
    if (!count) return MI_OK;
    mi_world::QueryCache& qc = w->query;
    if (!qc.candCap) return fail(MI_ERR_CAPACITY, "no candidate staging: call mi_world_volume_contacts_reserve first");
    HIP_TRY(qc.cOffsets.ensure((size_t)count + 1));
    rc = w->overlapEnqueue(count, reinterpret_cast<const uint32_t*>(volumesDev), include, ranges2Dev, qc.cOffsets.p, qc.cCand.p, qc.candCap, nullptr, false, kOvPassCount | kOvPassWrite, true);
    if (rc != MI_OK) return rc;
    return w->contactsEnqueue(count, qc.candCap, capacity, reinterpret_cast<uint4*>(contactsDev), offsetsDev, totals2Dev, false);
}

}  // extern "C"

extern "C" {

MI_API int mi_world_overlap(mi_world* w, uint32_t count, const mi_query_volume* volumes, uint32_t include, const uint32_t* ranges2, uint32_t* outOffsets,
                            mi_overlap_hit* outHits, uint32_t capacity, uint32_t* outTotal) {
    return overlapHost(w, count, volumes, include, ranges2, outOffsets, outHits, capacity, outTotal, false);
}
MI_API int mi_debug_overlap_exhaustive(mi_world* w, uint32_t count, const mi_query_volume* volumes, uint32_t include, const uint32_t* ranges2, uint32_t* outOffsets,
                                       mi_overlap_hit* outHits, uint32_t capacity, uint32_t* outTotal) {
    return overlapHost(w, count, volumes, include, ranges2, outOffsets, outHits, capacity, outTotal, true);
}
MI_API int mi_world_overlap_device_async(mi_world* w, uint32_t count, const mi_query_volume* volumesDev, uint32_t include, const uint32_t* ranges2Dev, uint32_t* offsetsDev,
                                         mi_overlap_hit* hitsDev, uint32_t capacity, uint32_t* totalDev) {
    if (!w || (count && (!volumesDev || !offsetsDev || !totalDev || (capacity && !hitsDev)))) return fail(MI_ERR_INVALID_ARGUMENT, "null argument");
    int rc = queryPrepare(w); if (rc != MI_OK) return rc;
    if (!count) return MI_OK;
    return w->overlapEnqueue(count, reinterpret_cast<const uint32_t*>(volumesDev), include, ranges2Dev, offsetsDev, reinterpret_cast<uint4*>(hitsDev), capacity, totalDev, false, kOvPassCount | kOvPassWrite, false);
}

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
