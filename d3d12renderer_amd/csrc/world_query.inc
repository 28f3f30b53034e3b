// Part of world.hip (one translation unit; #included there, after world_state.inc): batched scene queries (include/mi_physics.h): ray casts
// (mi_world_raycast*; kernels in kernels_query.hpp), volume overlaps (mi_world_overlap*; kernels in kernels_overlap.hpp), shape casts (mi_world_sweep*;
// kernels in kernels_sweep.hpp), distance queries (mi_world_distance*; kernels in kernels_distance.hpp) and the contact manifolds of
// query volumes (mi_world_volume_contacts*; kernels in kernels_contacts_query.hpp) and their terrain contacts (mi_world_terrain_contacts*; the step's terrain
// kernels of heightmap.hpp under the policy of kernels_terrain_query.hpp).
//
// The query structure (world AABBs, uniform grid, large list) is built lazily on the world's stream and cached per pose epoch: every
// internal step, upload (any topology or heightmap edit), body-state write, checkpoint load and shard import bumps mi_world::poseEpoch,
// and the first query of a new epoch rebuilds.  A build enqueues nine launches and no host synchronisation; it writes the query's own
// buffers only, so a query never changes what a later step computes.

int mi_world::queryBuild() {
    QueryCache::Built& g = query.built;
    const uint32_t nc = (uint32_t)colliders.size();
    if (g.epoch == poseEpoch && g.nc == nc) return MI_OK;
    const uint32_t maxCells = std::min<uint32_t>(std::max<uint32_t>(4u * nc, 4096u), 1u << 22);
    HIP_TRY(g.shape.ensure(3 * (size_t)std::max(nc, 1u))); HIP_TRY(g.mn.ensure(std::max(nc, 1u))); HIP_TRY(g.mx.ensure(std::max(nc, 1u)));
    HIP_TRY(g.grid.ensure(1)); HIP_TRY(g.large.ensure(std::max(nc, 1u))); HIP_TRY(g.partials.ensure(2 * (size_t)divUp(std::max(nc, 1u), 256)));
    HIP_TRY(g.entries.ensure((size_t)std::max(nc, 1u) * kQMaxCellsPerCollider));
    HIP_TRY(g.count.ensure((size_t)maxCells + 1)); HIP_TRY(g.start.ensure((size_t)maxCells + 1));
    Launcher& L = query.L;
    L.begin(false, false);
    HIP_TRY(L.memsetAsync(g.count.p, 0, ((size_t)maxCells + 1) * sizeof(uint32_t), stream));
    if (nc) {
        const uint32_t blocks = divUp(nc, 256);
        L.launch(k_q_colliders, dim3(blocks), dim3(256), 0, stream, nc, colliderRows(bPos.p, bRot.p, g.shape.p, g.mn.p, g.mx.p), g.partials.p);
        L.launch(k_q_mean, dim3(1), dim3(kQParamThreads), 0, stream, blocks, (const QPartial*)g.partials.p, g.grid.p);
        L.launch(k_q_filter, dim3(blocks), dim3(256), 0, stream, nc, (const float4*)g.mn.p, (const float4*)g.mx.p, (const QueryGrid*)g.grid.p, g.partials.p + blocks);
        L.launch(k_q_params, dim3(1), dim3(kQParamThreads), 0, stream, blocks, maxCells, (const QPartial*)(g.partials.p + blocks), g.grid.p);
        L.launch(k_q_count, dim3(divUp(nc, 256)), dim3(256), 0, stream, nc, (const float4*)g.mn.p, (const float4*)g.mx.p, g.grid.p, g.count.p, g.large.p);
        HIP_TRY(g.scan.run(L, g.count.p, g.start.p, maxCells + 1, stream, true));
        L.launch(k_q_scatter, dim3(divUp(nc, 256)), dim3(256), 0, stream, nc, (const float4*)g.mn.p, (const float4*)g.mx.p, (const QueryGrid*)g.grid.p,
                 (const uint32_t*)g.start.p, g.count.p, g.entries.p);
    } else {
        HIP_TRY(L.memsetAsync(g.grid.p, 0, sizeof(QueryGrid), stream));
        HIP_TRY(L.memsetAsync(g.start.p, 0, ((size_t)maxCells + 1) * sizeof(uint32_t), stream));
    }
    if (L.firstError != hipSuccess) return fail(MI_ERR_DEVICE, std::string("query structure: ") + hipGetErrorString(L.firstError));
    g.epoch = poseEpoch; g.nc = nc;
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
// a rank of a sharded world holds only its tile: every query entry point refuses
static int refuseSharded(const mi_world* w) {
    return w->shard.enabled ? fail(MI_ERR_UNSUPPORTED, "scene queries on a sharded world: a rank holds only its tile") : MI_OK;
}
// what every variant checks first; afterwards the device holds the current scene (pending host edits uploaded)
static int queryPrepare(mi_world* w) {
    int rc = refuseSharded(w); if (rc != MI_OK) return rc;
    return ensureUploaded(w);
}
// blocking variants: the optional entity ranges (one [lo, hi) pair per ray / volume) onto the device; *dev = null without ranges
static int stageRanges(mi_world* w, uint32_t count, const uint32_t* ranges, const uint32_t** dev) {
    DBuf<uint32_t>& buf = w->query.host.ranges;
    *dev = nullptr;
    if (!ranges) return MI_OK;
    HIP_TRY(buf.ensure(2 * (size_t)count));
    HIP_TRY(hipMemcpyAsync(buf.p, ranges, 2 * (size_t)count * sizeof(uint32_t), hipMemcpyHostToDevice, w->stream));
    *dev = buf.p;
    return MI_OK;
}
// blocking variants: the query volumes onto the device
static int stageVolumes(mi_world* w, uint32_t count, const mi_query_volume* volumes, const uint32_t** dev) {
    DBuf<uint32_t>& buf = w->query.host.volumes;
    HIP_TRY(buf.ensure(kOvVolumeWords * (size_t)count));
    HIP_TRY(hipMemcpyAsync(buf.p, volumes, (size_t)count * sizeof(mi_query_volume), hipMemcpyHostToDevice, w->stream));
    *dev = buf.p;
    return MI_OK;
}

// ---- ray casts.  Accelerated (exhaustive = false) or exhaustive ray kernel over rays already on the device.
static int raycastEnqueue(mi_world* w, uint32_t count, const float* raysDev, uint32_t include, const uint32_t* rangesDev, void* outDev, bool exhaustive) {
    const QueryScene s = queryScene(w);
    uint32_t* out = static_cast<uint32_t*>(outDev);
    if (exhaustive) {
        k_q_exhaustive<<<count, 256, 0, w->stream>>>(raysDev, rangesDev, include, s, out);
    } else {
        int rc = w->queryBuild(); if (rc != MI_OK) return rc;
        const mi_world::QueryCache::Built& g = w->query.built;
        k_q_raycast<<<divUp(count, 256), 256, 0, w->stream>>>(count, raysDev, rangesDev, include, s, g.grid.p, g.start.p, g.entries.p, g.large.p, out);
    }
    HIP_TRY(hipGetLastError());
    return MI_OK;
}
static int raycastHost(mi_world* w, uint32_t count, const float* origins, const float* directions, const float* maxT, uint32_t include, const uint32_t* ranges,
                       mi_ray_hit* out, bool exhaustive) {
    if (!w || (count && (!origins || !directions || !out))) return fail(MI_ERR_INVALID_ARGUMENT, "null argument");
    int rc = queryPrepare(w); if (rc != MI_OK) return rc;
    if (!count) return MI_OK;
    std::vector<float> rays(8 * (size_t)count, 0.f);
    for (uint32_t r = 0; r < count; ++r) {
        for (int k = 0; k < 3; ++k) { rays[8 * (size_t)r + k] = origins[3 * (size_t)r + k]; rays[8 * (size_t)r + 3 + k] = directions[3 * (size_t)r + k]; }
        rays[8 * (size_t)r + 6] = maxT ? maxT[r] : std::numeric_limits<float>::infinity();
    }
    mi_world::QueryCache::Blocking& h = w->query.host;
    HIP_TRY(h.rays.ensure(rays.size())); HIP_TRY(h.hits.ensure(10 * (size_t)count));
    HIP_TRY(hipMemcpyAsync(h.rays.p, rays.data(), rays.size() * sizeof(float), hipMemcpyHostToDevice, w->stream));
    const uint32_t* rangesDev;
    rc = stageRanges(w, count, ranges, &rangesDev); if (rc != MI_OK) return rc;
    rc = raycastEnqueue(w, count, h.rays.p, include, rangesDev, h.hits.p, exhaustive); if (rc != MI_OK) return rc;
    HIP_TRY(hipMemcpyAsync(out, h.hits.p, (size_t)count * sizeof(mi_ray_hit), hipMemcpyDeviceToHost, w->stream));
    HIP_TRY(hipStreamSynchronize(w->stream));   // (the rays / ranges were pageable host memory as well)
    return MI_OK;
}

// ---- volume overlaps.  Volume rows (two launches), count pass, device scan, write pass: five launches behind the (shared) grid build, no read-back between them.
// The world rows a volume kernel tests against: the exhaustive yardstick's own (at the current poses, computed by the call) or the cached ones of the grid build.
OverlapScene mi_world::overlapScene(bool exhaustive) const {
    OverlapScene s{};
    s.nc = (uint32_t)colliders.size(); s.cEntity = cEntity.p; s.hs = HullSet{hullVerts.p, hullRanges.p};
    if (exhaustive) { s.shape = query.exh.shape.p; s.mn = query.exh.mn.p; s.mx = query.exh.mx.p; }
    else { s.shape = query.built.shape.p; s.mn = query.built.mn.p; s.mx = query.built.mx.p; }
    return s;
}
// The exhaustive yardstick's own world rows at the current poses (one launch on the begun launcher): it does not trust the cache.  launch = false: the rows
// an earlier pass of the same call computed stand.
int mi_world::exhaustiveRowsEnqueue(bool launch) {
    QueryCache::Exhaustive& x = query.exh;
    const uint32_t nc = (uint32_t)colliders.size();
    HIP_TRY(x.shape.ensure(3 * (size_t)std::max(nc, 1u))); HIP_TRY(x.mn.ensure(std::max(nc, 1u))); HIP_TRY(x.mx.ensure(std::max(nc, 1u)));
    HIP_TRY(x.partials.ensure(divUp(std::max(nc, 1u), 256)));
    if (nc && launch) query.L.launch(k_q_colliders, dim3(divUp(nc, 256)), dim3(256), 0, stream, nc, colliderRows(bPos.p, bRot.p, x.shape.p, x.mn.p, x.mx.p), x.partials.p);
    return MI_OK;
}
// The volumes of a call as collider rows (two launches on the begun launcher): what every volume family tests with.
int mi_world::volumeRowsEnqueue(uint32_t count, const uint32_t* volumesDev, const uint32_t* rangesDev) {
    QueryCache::VolumeRows& v = query.vol;
    HIP_TRY(v.shape.ensure(3 * (size_t)count)); HIP_TRY(v.mn.ensure(count)); HIP_TRY(v.mx.ensure(count)); HIP_TRY(v.range.ensure(2 * (size_t)count));
    HIP_TRY(v.cTypeBody.ensure(2 * (size_t)count)); HIP_TRY(v.cObject.ensure(count)); HIP_TRY(v.cShape.ensure(3 * (size_t)count)); HIP_TRY(v.cPos.ensure(count)); HIP_TRY(v.cRot.ensure(count));
    Launcher& L = query.L;
    L.launch(k_ov_unpack, dim3(divUp(count, 256)), dim3(256), 0, stream, count, volumesDev, rangesDev, (uint32_t)hulls.size(), v.cTypeBody.p, v.cObject.p, v.cShape.p,
             v.cPos.p, v.cRot.p, v.range.p);
    ColliderRows volumes = colliderRows(nullptr, nullptr /* (no bodies) */, v.shape.p, v.mn.p, v.mx.p);   // the volumes as static colliders; the world's hulls
    volumes.cTypeBody = v.cTypeBody.p; volumes.cObject = v.cObject.p; volumes.cShape = v.cShape.p; volumes.cStaticPos = v.cPos.p; volumes.cStaticRot = v.cRot.p; volumes.nb = 0u;
    L.launch(k_ov_prepare, dim3(divUp(count, 256)), dim3(256), 0, stream, count, volumes);
    return MI_OK;
}
// passes: kOvPassCount = volume rows, count pass and scan; kOvPassWrite = the write pass over what a count pass of the same arguments left (nothing else
// enqueued in between).  boxesOnly: ovTest without overlapCheck — the candidates of the contact query.
int mi_world::overlapEnqueue(uint32_t count, const uint32_t* volumesDev, uint32_t include, const uint32_t* rangesDev, uint32_t* offsetsDev, uint4* hitsDev,
                             uint32_t capacity, uint32_t* totalDev, bool exhaustive, uint32_t passes, bool boxesOnly) {
    QueryCache::VolumeRows& v = query.vol; const QueryCache::Built& g = query.built;
    const bool first = (passes & kOvPassCount) != 0u;
    if (!exhaustive && first) { int rc = queryBuild(); if (rc != MI_OK) return rc; }
    HIP_TRY(v.count.ensure((size_t)count + 1));
    Launcher& L = query.L;
    L.begin(false, false);
    if (exhaustive) { int rc = exhaustiveRowsEnqueue(first); if (rc != MI_OK) return rc; }
    const OverlapScene s = overlapScene(exhaustive);
    const dim3 grid(divUp(count, kOvWaves)), block(64 * kOvWaves);
    if (first) { int rc = volumeRowsEnqueue(count, volumesDev, rangesDev); if (rc != MI_OK) return rc; }
    for (uint32_t pass = 0; pass < 2u; ++pass) {
        if (!(passes & (pass ? kOvPassWrite : kOvPassCount))) continue;
        if (exhaustive)
            L.launch(boxesOnly ? k_q_overlap_exhaustive<true> : k_q_overlap_exhaustive<false>, grid, block, 0, stream, pass, count, include, s, (const float4*)v.shape.p,
                     (const float4*)v.mn.p, (const float4*)v.mx.p, (const uint32_t*)v.range.p, v.count.p, (const uint32_t*)offsetsDev, hitsDev, capacity, totalDev);
        else
            L.launch(boxesOnly ? k_q_overlap<true> : k_q_overlap<false>, grid, block, 0, stream, pass, count, include, s, (const float4*)v.shape.p, (const float4*)v.mn.p,
                     (const float4*)v.mx.p, (const uint32_t*)v.range.p, (const QueryGrid*)g.grid.p, (const uint32_t*)g.start.p, (const uint32_t*)g.entries.p,
                     (const uint32_t*)g.large.p, v.count.p, (const uint32_t*)offsetsDev, hitsDev, capacity, totalDev);
        if (pass == 0u) HIP_TRY(v.scan.run(L, v.count.p, offsetsDev, count + 1u, stream, false));
    }
    if (L.firstError != hipSuccess) return fail(MI_ERR_DEVICE, std::string("overlap query: ") + hipGetErrorString(L.firstError));
    return MI_OK;
}

// ---- shape casts.  Volume rows (two launches), then one launch: a wave per cast writes its record.  The exhaustive yardstick computes its own world rows first,
// as the overlap yardstick does.  displacementsDev: one row of 16 bytes per cast (w ignored).
int mi_world::sweepEnqueue(uint32_t count, const uint32_t* volumesDev, const float4* displacementsDev, uint32_t include, const uint32_t* rangesDev, uint4* outDev, bool exhaustive) {
    QueryCache::VolumeRows& v = query.vol; const QueryCache::Built& g = query.built;
    if (!exhaustive) { int rc = queryBuild(); if (rc != MI_OK) return rc; }
    Launcher& L = query.L;
    L.begin(false, false);
    if (exhaustive) { int rc = exhaustiveRowsEnqueue(true); if (rc != MI_OK) return rc; }
    const OverlapScene s = overlapScene(exhaustive);
    int rc = volumeRowsEnqueue(count, volumesDev, rangesDev); if (rc != MI_OK) return rc;
    const dim3 grid(divUp(count, kOvWaves)), block(64 * kOvWaves);
    if (exhaustive)
        L.launch(k_q_sweep_exhaustive, grid, block, 0, stream, count, include, s, (const float4*)v.shape.p, (const float4*)v.mn.p, (const float4*)v.mx.p, (const uint32_t*)v.range.p,
                 (const float4*)v.cPos.p, displacementsDev, outDev);
    else
        L.launch(k_q_sweep, grid, block, 0, stream, count, include, s, (const float4*)v.shape.p, (const float4*)v.mn.p, (const float4*)v.mx.p, (const uint32_t*)v.range.p,
                 (const float4*)v.cPos.p, displacementsDev, (const QueryGrid*)g.grid.p, (const uint32_t*)g.start.p, (const uint32_t*)g.entries.p, (const uint32_t*)g.large.p, outDev);
    // the terrain: the matching kernel behind the collider kernel, merging into its records; it reads the heightmap buffers themselves (no cache of its own)
    if (heightmap && (include & kQueryTerrain)) {
        if (hmParams.chunksPerDim > 256u) return fail(MI_ERR_UNSUPPORTED, "sweep query: a heightmap of more than 256 chunks per dimension (the triangle index has 32 bits)");
        L.launch(exhaustive ? k_q_sweep_terrain_exhaustive : k_q_sweep_terrain, grid, block, 0, stream, count, include, hmParams, s.hs, (const float4*)v.shape.p, (const float4*)v.mn.p,
                 (const float4*)v.mx.p, (const uint32_t*)v.range.p, (const float4*)v.cPos.p, displacementsDev, outDev);
    }
    if (L.firstError != hipSuccess) return fail(MI_ERR_DEVICE, std::string("sweep query: ") + hipGetErrorString(L.firstError));
    return MI_OK;
}
static_assert(sizeof(mi_sweep_hit) == kSweepRecordRows * sizeof(uint4), "a sweep record is three rows of 16 bytes");
// the blocking variants: volumes, ranges and displacement rows through the blocking staging, the records read back once
static int sweepHost(mi_world* w, uint32_t count, const mi_query_volume* volumes, const float* displacements3, uint32_t include, const uint32_t* ranges, mi_sweep_hit* out, bool exhaustive) {
    if (!w || (count && (!volumes || !displacements3 || !out))) return fail(MI_ERR_INVALID_ARGUMENT, "null argument");
    int rc = queryPrepare(w); if (rc != MI_OK) return rc;
    if (!count) return MI_OK;
    std::vector<float> rows(4 * (size_t)count, 0.f);
    for (uint32_t i = 0; i < count; ++i) for (int k = 0; k < 3; ++k) rows[4 * (size_t)i + k] = displacements3[3 * (size_t)i + k];
    mi_world::QueryCache::Blocking& h = w->query.host;
    HIP_TRY(h.rays.ensure(rows.size())); HIP_TRY(h.records.ensure((size_t)count * kSweepRecordRows));
    HIP_TRY(hipMemcpyAsync(h.rays.p, rows.data(), rows.size() * sizeof(float), hipMemcpyHostToDevice, w->stream));
    const uint32_t *volumesDev, *rangesDev;
    rc = stageVolumes(w, count, volumes, &volumesDev); if (rc != MI_OK) return rc;
    rc = stageRanges(w, count, ranges, &rangesDev); if (rc != MI_OK) return rc;
    rc = w->sweepEnqueue(count, volumesDev, reinterpret_cast<const float4*>(h.rays.p), include, rangesDev, h.records.p, exhaustive); if (rc != MI_OK) return rc;
    HIP_TRY(hipMemcpyAsync(out, h.records.p, (size_t)count * sizeof(mi_sweep_hit), hipMemcpyDeviceToHost, w->stream));
    HIP_TRY(hipStreamSynchronize(w->stream));   // (the inputs were pageable host memory as well)
    return MI_OK;
}

// ---- distance queries.  Volume rows (two launches), then one launch: a wave per volume writes its record; the exhaustive yardstick computes its own world rows
// first.  maxDistancesDev: one float per volume, or null (+inf).  The terrain is not reported: the terrain bit changes nothing.
int mi_world::distanceEnqueue(uint32_t count, const uint32_t* volumesDev, const float* maxDistancesDev, uint32_t include, const uint32_t* rangesDev, uint4* outDev, bool exhaustive) {
    QueryCache::VolumeRows& v = query.vol; const QueryCache::Built& g = query.built;
    if (!exhaustive) { int rc = queryBuild(); if (rc != MI_OK) return rc; }
    Launcher& L = query.L;
    L.begin(false, false);
    if (exhaustive) { int rc = exhaustiveRowsEnqueue(true); if (rc != MI_OK) return rc; }
    const OverlapScene s = overlapScene(exhaustive);
    int rc = volumeRowsEnqueue(count, volumesDev, rangesDev); if (rc != MI_OK) return rc;
    const dim3 grid(divUp(count, kOvWaves)), block(64 * kOvWaves);
    if (exhaustive)
        L.launch(k_q_distance_exhaustive, grid, block, 0, stream, count, include, s, (const float4*)v.shape.p, (const float4*)v.mn.p, (const float4*)v.mx.p, (const uint32_t*)v.range.p,
                 (const float4*)v.cPos.p, maxDistancesDev, outDev);
    else
        L.launch(k_q_distance, grid, block, 0, stream, count, include, s, (const float4*)v.shape.p, (const float4*)v.mn.p, (const float4*)v.mx.p, (const uint32_t*)v.range.p,
                 (const float4*)v.cPos.p, maxDistancesDev, (const QueryGrid*)g.grid.p, (const uint32_t*)g.start.p, (const uint32_t*)g.entries.p, (const uint32_t*)g.large.p, outDev);
    if (L.firstError != hipSuccess) return fail(MI_ERR_DEVICE, std::string("distance query: ") + hipGetErrorString(L.firstError));
    return MI_OK;
}
static_assert(sizeof(mi_distance_hit) == kDistanceRecordRows * sizeof(uint4) && sizeof(mi_distance_hit) == 64, "a distance record is four rows of 16 bytes");
// the blocking variants: volumes, ranges and the largest distances through the blocking staging, the records read back once
static int distanceHost(mi_world* w, uint32_t count, const mi_query_volume* volumes, const float* maxDistances, uint32_t include, const uint32_t* ranges, mi_distance_hit* out, bool exhaustive) {
    if (!w || (count && (!volumes || !out))) return fail(MI_ERR_INVALID_ARGUMENT, "null argument");
    int rc = queryPrepare(w); if (rc != MI_OK) return rc;
    if (!count) return MI_OK;
    mi_world::QueryCache::Blocking& h = w->query.host;
    HIP_TRY(h.rays.ensure(count)); HIP_TRY(h.records.ensure((size_t)count * kDistanceRecordRows));
    if (maxDistances) HIP_TRY(hipMemcpyAsync(h.rays.p, maxDistances, (size_t)count * sizeof(float), hipMemcpyHostToDevice, w->stream));
    const uint32_t *volumesDev, *rangesDev;
    rc = stageVolumes(w, count, volumes, &volumesDev); if (rc != MI_OK) return rc;
    rc = stageRanges(w, count, ranges, &rangesDev); if (rc != MI_OK) return rc;
    rc = w->distanceEnqueue(count, volumesDev, maxDistances ? h.rays.p : nullptr, include, rangesDev, h.records.p, exhaustive); if (rc != MI_OK) return rc;
    HIP_TRY(hipMemcpyAsync(out, h.records.p, (size_t)count * sizeof(mi_distance_hit), hipMemcpyDeviceToHost, w->stream));
    HIP_TRY(hipStreamSynchronize(w->stream));   // (the inputs were pageable host memory as well)
    return MI_OK;
}

// ---- terrain distance queries (kernels_terrain_distance.hpp).  Volume rows (two launches), then one launch: a wave per volume writes its record, or merges it
// into the record a distanceEnqueue left in outDev (merge != 0).  The kernels read the heightmap buffers themselves (no cache of their own), as the terrain casts
// do.  A world without a heightmap: misses (k_q_terrain_distance_none), or nothing when merging.
int mi_world::terrainDistanceEnqueue(uint32_t count, const uint32_t* volumesDev, const float* maxDistancesDev, uint32_t merge, uint4* outDev, bool exhaustive) {
    QueryCache::VolumeRows& v = query.vol;
    if (heightmap && hmParams.chunksPerDim > 256u) return fail(MI_ERR_UNSUPPORTED, "terrain distance query: a heightmap of more than 256 chunks per dimension (the triangle index has 32 bits)");
    if (!heightmap && merge) return MI_OK;
    Launcher& L = query.L;
    L.begin(false, false);
    if (!heightmap) {
        L.launch(k_q_terrain_distance_none, dim3(divUp(count, 256)), dim3(256), 0, stream, count, outDev);
    } else {
        int rc = volumeRowsEnqueue(count, volumesDev, nullptr); if (rc != MI_OK) return rc;
        const HullSet hs{hullVerts.p, hullRanges.p};
        const dim3 grid(divUp(count, kOvWaves)), block(64 * kOvWaves);
        L.launch(exhaustive ? k_q_terrain_distance_exhaustive : k_q_terrain_distance, grid, block, 0, stream, count, merge, hmParams, hs, (const float4*)v.shape.p, (const float4*)v.mn.p,
                 (const float4*)v.mx.p, (const uint32_t*)v.range.p, (const float4*)v.cPos.p, maxDistancesDev, outDev);
    }
    if (L.firstError != hipSuccess) return fail(MI_ERR_DEVICE, std::string("terrain distance query: ") + hipGetErrorString(L.firstError));
    return MI_OK;
}
// the blocking variants: volumes and the largest distances through the blocking staging; with merge the caller's records go up first; the records read back once
static int terrainDistanceHost(mi_world* w, uint32_t count, const mi_query_volume* volumes, const float* maxDistances, uint32_t merge, mi_distance_hit* out, bool exhaustive) {
    if (!w || (count && (!volumes || !out))) return fail(MI_ERR_INVALID_ARGUMENT, "null argument");
    int rc = queryPrepare(w); if (rc != MI_OK) return rc;
    if (!count) return MI_OK;
    mi_world::QueryCache::Blocking& h = w->query.host;
    HIP_TRY(h.rays.ensure(count)); HIP_TRY(h.records.ensure((size_t)count * kDistanceRecordRows));
    if (maxDistances) HIP_TRY(hipMemcpyAsync(h.rays.p, maxDistances, (size_t)count * sizeof(float), hipMemcpyHostToDevice, w->stream));
    if (merge) HIP_TRY(hipMemcpyAsync(h.records.p, out, (size_t)count * sizeof(mi_distance_hit), hipMemcpyHostToDevice, w->stream));
    const uint32_t* volumesDev;
    rc = stageVolumes(w, count, volumes, &volumesDev); if (rc != MI_OK) return rc;
    rc = w->terrainDistanceEnqueue(count, volumesDev, maxDistances ? h.rays.p : nullptr, merge, h.records.p, exhaustive); if (rc != MI_OK) return rc;
    HIP_TRY(hipMemcpyAsync(out, h.records.p, (size_t)count * sizeof(mi_distance_hit), hipMemcpyDeviceToHost, w->stream));
    HIP_TRY(hipStreamSynchronize(w->stream));   // (the inputs were pageable host memory as well)
    return MI_OK;
}

// ---- contact manifolds of query volumes.  Candidates by the overlap passes in boxes-only mode, then narrow phase, GJK queue, scan and write: no read-back
// between them.  `bound` = the candidates evaluated, at most what contactsReserve() sized the staging for.
int mi_world::contactsReserve(uint32_t maxCandidates) {
    QueryCache::Candidates& c = query.cand;
    if (maxCandidates <= c.cap) return MI_OK;
    const size_t n = maxCandidates;
    HIP_TRY(c.pairs.ensure(n)); HIP_TRY(c.slots.ensure(n * kVcSlotRows)); HIP_TRY(c.flags.ensure(n + 1)); HIP_TRY(c.scanned.ensure(n + 1));
    HIP_TRY(c.queue.ensure(n)); HIP_TRY(c.queueN.ensure(1));
    c.cap = maxCandidates;
    return MI_OK;
}
int mi_world::contactsEnqueue(uint32_t count, uint32_t bound, uint32_t capacity, uint4* contactsDev, uint32_t* offsetsDev, uint32_t* totals2Dev, bool exhaustive) {
    QueryCache::Candidates& c = query.cand; const QueryCache::VolumeRows& v = query.vol;
    if (bound > c.cap) return fail(MI_ERR_INVALID_ARGUMENT, "contact query: more candidates than reserved");
    HIP_TRY(c.flags.ensure(1)); HIP_TRY(c.scanned.ensure(1)); HIP_TRY(c.queueN.ensure(1));   // (bound 0: the scan still reads one word)
    const OverlapScene s = overlapScene(exhaustive);
    Launcher& L = query.L;
    L.begin(false, false);
    HIP_TRY(L.memsetAsync(c.queueN.p, 0, sizeof(uint32_t), stream));
    c.timed = timingLevel != 0u;   // (opt-in, as the step's stage times: events between launches leave the device idle for a few microseconds)
    if (c.timed) for (hipEvent_t& e : c.ev) if (!e) HIP_TRY(hipEventCreate(&e));
    if (c.timed) HIP_TRY(hipEventRecord(c.ev[0], stream));
    L.launch(k_vc_narrow, dim3(divUp(bound + 1u, 256)), dim3(256), 0, stream, bound, count, (const uint32_t*)v.candOffsets.p, (const uint4*)c.pairs.p, s, (const float4*)v.shape.p,
             (const float4*)v.mn.p, c.slots.p, c.flags.p, c.queue.p, c.queueN.p);
    if (c.timed) HIP_TRY(hipEventRecord(c.ev[1], stream));
    if (bound)
        L.launch(k_vc_gjk, dim3(std::min(bound, kVcGjkMaxBlocks)), dim3(64), 0, stream, bound, count, (const uint32_t*)v.candOffsets.p, (const uint4*)c.pairs.p, s, (const float4*)v.shape.p,
                 (const float4*)v.mn.p, c.slots.p, c.flags.p, (const uint32_t*)c.queue.p, (const uint32_t*)c.queueN.p);
    if (c.timed) HIP_TRY(hipEventRecord(c.ev[2], stream));
    HIP_TRY(c.scan.run(L, c.flags.p, c.scanned.p, bound + 1u, stream, false));
    L.launch(k_vc_write, dim3(divUp(std::max(bound, count + 1u), 256)), dim3(256), 0, stream, bound, count, capacity, (const uint32_t*)v.candOffsets.p, (const uint32_t*)c.flags.p,
             (const uint32_t*)c.scanned.p, (const uint4*)c.slots.p, contactsDev, offsetsDev, totals2Dev);
    if (c.timed) HIP_TRY(hipEventRecord(c.ev[3], stream));
    if (L.firstError != hipSuccess) return fail(MI_ERR_DEVICE, std::string("contact query: ") + hipGetErrorString(L.firstError));
    return MI_OK;
}

// ---- terrain contacts of query volumes.  The step's terrain pipeline (heightmap.hpp) with the volume rows as its colliders and HmQueryOut as its policy: volume
// rows (two launches), lowest-point pass, count pass and its large-window instance, the scan of the counts into the caller's offsets, the total, then the three write
// passes straight into the caller's records — no read-back between them.  capacity 0: no write passes.  A world without a heightmap: all-zero offsets.
int mi_world::terrainEnqueue(uint32_t count, const uint32_t* volumesDev, uint32_t* offsetsDev, float4* recordsDev, uint32_t capacity, uint32_t* totalDev) {
    QueryCache::Terrain& t = query.terrain; const QueryCache::VolumeRows& v = query.vol;
    Launcher& L = query.L;
    L.begin(false, false);
    if (!heightmap) {
        HIP_TRY(L.memsetAsync(offsetsDev, 0, ((size_t)count + 1) * sizeof(uint32_t), stream));
        if (totalDev) HIP_TRY(L.memsetAsync(totalDev, 0, sizeof(uint32_t), stream));
        return MI_OK;
    }
    HIP_TRY(t.counts.ensure((size_t)count + 1)); HIP_TRY(t.slow.ensure(count)); HIP_TRY(t.stash.ensure((size_t)count * kHmStash));
    int rc = volumeRowsEnqueue(count, volumesDev, nullptr); if (rc != MI_OK) return rc;
    const HullSet hs{hullVerts.p, hullRanges.p};
    const HmQueryOut out{capacity, recordsDev};
    const dim3 B(256), perWave(divUp(count, 4)), scanning(std::min(divUp(count, 256), kHmScanBlocks));
    const float4 *shape = v.shape.p, *mn = v.mn.p, *mx = v.mx.p;
    L.launch(k_hm_lowest<HmQueryOut>, dim3(divUp(count, 256)), B, 0, stream, count, hmParams, shape, mn, mx, t.slow.p, hs);
    L.launch(k_hm_contacts<false, false, HmQueryOut>, perWave, B, 0, stream, count, hmParams, shape, mn, mx, t.counts.p, t.slow.p, nullptr, out, hs, t.stash.p);
    L.launch(k_hm_contacts<false, true, HmQueryOut>, scanning, B, 0, stream, count, hmParams, shape, mn, mx, t.counts.p, t.slow.p, nullptr, out, hs, t.stash.p);
    HIP_TRY(L.memsetAsync(t.counts.p + count, 0, sizeof(uint32_t), stream));   // (the scan's last input: offsets[count] = the total)
    HIP_TRY(t.scan.run(L, t.counts.p, offsetsDev, count + 1u, stream, false));
    if (totalDev) L.launch(k_tq_total, dim3(1), dim3(1), 0, stream, count, (const uint32_t*)offsetsDev, totalDev);
    if (capacity) {
        const uint32_t* offsets = offsetsDev;
        L.launch(k_hm_contacts<true, false, HmQueryOut>, scanning, B, 0, stream, count, hmParams, shape, mn, mx, t.counts.p, t.slow.p, offsets, out, hs, t.stash.p);
        L.launch(k_hm_contacts<true, true, HmQueryOut>, scanning, B, 0, stream, count, hmParams, shape, mn, mx, t.counts.p, t.slow.p, offsets, out, hs, t.stash.p);
        const uint32_t lanes = (uint32_t)std::min<uint64_t>(capacity, (uint64_t)kHmMaxContacts * count);   // one lane per contact that has a record
        L.launch(k_hm_write_stashed<HmQueryOut>, dim3(divUp(lanes, 256)), B, 0, stream, count, hmParams, shape, mn, mx, (const uint32_t*)t.counts.p, (const uint8_t*)t.slow.p, offsets, out, hs,
                 (const uint32_t*)t.stash.p);
    }
    if (L.firstError != hipSuccess) return fail(MI_ERR_DEVICE, std::string("terrain contact query: ") + hipGetErrorString(L.firstError));
    return MI_OK;
}

// ---- the blocking volume queries (mi_world_overlap, mi_world_volume_contacts, mi_world_terrain_contacts and the exhaustive yardsticks): one protocol.  Argument check, prepare,
// zeroed outputs, volumes and ranges staged, the family's own work, then offsets, total and min(total, capacity) records read back.  What a family brings:
// the bytes of its record, the noun of the capacity error, and the step that enqueues its work on the staged inputs and leaves count + 1 offsets and up to
// `capacity` records in the blocking staging it is handed.
struct VolumeFamily {
    size_t recordBytes; const char* noun;
    int (*enqueue)(mi_world* w, uint32_t count, const uint32_t* volumesDev, uint32_t include, const uint32_t* rangesDev, uint32_t* offsetsDev, uint4* recordsDev, uint32_t capacity, bool exhaustive);
};
static int overlapStep(mi_world* w, uint32_t count, const uint32_t* volumesDev, uint32_t include, const uint32_t* rangesDev, uint32_t* offsetsDev, uint4* recordsDev, uint32_t capacity, bool exhaustive) {
    return w->overlapEnqueue(count, volumesDev, include, rangesDev, offsetsDev, recordsDev, capacity, nullptr, exhaustive, capacity == 0u ? kOvPassCount : kOvPassCount | kOvPassWrite, false);
}
static int contactsStep(mi_world* w, uint32_t count, const uint32_t* volumesDev, uint32_t include, const uint32_t* rangesDev, uint32_t* offsetsDev, uint4* recordsDev, uint32_t capacity, bool exhaustive) {
    mi_world::QueryCache& qc = w->query;
    HIP_TRY(qc.vol.candOffsets.ensure((size_t)count + 1)); HIP_TRY(qc.host.totals.ensure(2));
    // the candidate total is read back once (this call synchronises anyway) and sizes the staging; the write pass follows on the same rows
    int rc = w->overlapEnqueue(count, volumesDev, include, rangesDev, qc.vol.candOffsets.p, nullptr, 0u, nullptr, exhaustive, kOvPassCount, true); if (rc != MI_OK) return rc;
    uint32_t candidates = 0;
    HIP_TRY(hipMemcpyAsync(&candidates, qc.vol.candOffsets.p + count, sizeof(uint32_t), hipMemcpyDeviceToHost, w->stream));
    HIP_TRY(hipStreamSynchronize(w->stream));
    rc = w->contactsReserve(candidates); if (rc != MI_OK) return rc;
    if (candidates) { rc = w->overlapEnqueue(count, volumesDev, include, rangesDev, qc.vol.candOffsets.p, qc.cand.pairs.p, candidates, nullptr, exhaustive, kOvPassWrite, true); if (rc != MI_OK) return rc; }
    return w->contactsEnqueue(count, candidates, capacity, recordsDev, offsetsDev, qc.host.totals.p, exhaustive);
}
static int terrainStep(mi_world* w, uint32_t count, const uint32_t* volumesDev, uint32_t, const uint32_t*, uint32_t* offsetsDev, uint4* recordsDev, uint32_t capacity, bool) {
    return w->terrainEnqueue(count, volumesDev, offsetsDev, reinterpret_cast<float4*>(recordsDev), capacity, nullptr);
}
static const VolumeFamily kOverlapFamily{sizeof(mi_overlap_hit), "overlap", overlapStep};
static const VolumeFamily kContactFamily{sizeof(mi_volume_contact), "contact", contactsStep};
static const VolumeFamily kTerrainFamily{sizeof(mi_terrain_contact), "terrain contact", terrainStep};
static_assert(sizeof(mi_overlap_hit) == sizeof(uint4) && sizeof(mi_volume_contact) == kVcSlotRows * sizeof(uint4) && sizeof(mi_terrain_contact) == kTqRecordRows * sizeof(uint4), "the blocking staging holds records as rows of 16 bytes");

static int volumeQueryHost(mi_world* w, const VolumeFamily& family, uint32_t count, const mi_query_volume* volumes, uint32_t include, const uint32_t* ranges, uint32_t* outOffsets,
                           void* outRecords, uint32_t capacity, uint32_t* outTotal, bool exhaustive) {
    if (!w || (count && (!volumes || !outOffsets || !outTotal || (capacity && !outRecords)))) return fail(MI_ERR_INVALID_ARGUMENT, "null argument");
    int rc = queryPrepare(w); if (rc != MI_OK) return rc;
    if (outTotal) *outTotal = 0u;
    if (outOffsets) outOffsets[0] = 0u;
    if (!count) return MI_OK;
    mi_world::QueryCache::Blocking& h = w->query.host;
    HIP_TRY(h.offsets.ensure((size_t)count + 1)); HIP_TRY(h.records.ensure((size_t)std::max(capacity, 1u) * (family.recordBytes / sizeof(uint4))));
    const uint32_t *volumesDev, *rangesDev;
    rc = stageVolumes(w, count, volumes, &volumesDev); if (rc != MI_OK) return rc;
    rc = stageRanges(w, count, ranges, &rangesDev); if (rc != MI_OK) return rc;
    rc = family.enqueue(w, count, volumesDev, include, rangesDev, h.offsets.p, h.records.p, capacity, exhaustive); if (rc != MI_OK) return rc;
    HIP_TRY(hipMemcpyAsync(outOffsets, h.offsets.p, ((size_t)count + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, w->stream));
    HIP_TRY(hipStreamSynchronize(w->stream));
    const uint32_t total = outOffsets[count];
    *outTotal = total;
    const uint32_t n = std::min(total, capacity);
    if (n) {
        HIP_TRY(hipMemcpyAsync(outRecords, h.records.p, (size_t)n * family.recordBytes, hipMemcpyDeviceToHost, w->stream));
        HIP_TRY(hipStreamSynchronize(w->stream));
    }
    if (total > capacity && (capacity || outRecords)) return fail(MI_ERR_CAPACITY, std::string("capacity < ") + family.noun + " records (out_total holds the number)");
    return MI_OK;
}

extern "C" {

MI_API int mi_world_raycast(mi_world* w, uint32_t count, const float* origins3, const float* directions3, const float* maxT, uint32_t include,
                            const uint32_t* ranges2, mi_ray_hit* out) {
    return raycastHost(w, count, origins3, directions3, maxT, include, ranges2, out, false);
}
MI_API int mi_debug_raycast_exhaustive(mi_world* w, uint32_t count, const float* origins3, const float* directions3, const float* maxT, uint32_t include,
                                       const uint32_t* ranges2, mi_ray_hit* out) {
    return raycastHost(w, count, origins3, directions3, maxT, include, ranges2, out, true);
}
MI_API int mi_world_raycast_device_async(mi_world* w, uint32_t count, const float* rays8Dev, uint32_t include, const uint32_t* ranges2Dev, mi_ray_hit* outDev) {
    if (!w || (count && (!rays8Dev || !outDev))) return fail(MI_ERR_INVALID_ARGUMENT, "null argument");
    int rc = queryPrepare(w); if (rc != MI_OK) return rc;
    if (!count) return MI_OK;
    return raycastEnqueue(w, count, rays8Dev, include, ranges2Dev, outDev, false);
}

MI_API int mi_world_overlap(mi_world* w, uint32_t count, const mi_query_volume* volumes, uint32_t include, const uint32_t* ranges2, uint32_t* outOffsets,
                            mi_overlap_hit* outHits, uint32_t capacity, uint32_t* outTotal) {
    return volumeQueryHost(w, kOverlapFamily, count, volumes, include, ranges2, outOffsets, outHits, capacity, outTotal, false);
}
MI_API int mi_debug_overlap_exhaustive(mi_world* w, uint32_t count, const mi_query_volume* volumes, uint32_t include, const uint32_t* ranges2, uint32_t* outOffsets,
                                       mi_overlap_hit* outHits, uint32_t capacity, uint32_t* outTotal) {
    return volumeQueryHost(w, kOverlapFamily, count, volumes, include, ranges2, outOffsets, outHits, capacity, outTotal, true);
}
MI_API int mi_world_overlap_device_async(mi_world* w, uint32_t count, const mi_query_volume* volumesDev, uint32_t include, const uint32_t* ranges2Dev, uint32_t* offsetsDev,
                                         mi_overlap_hit* hitsDev, uint32_t capacity, uint32_t* totalDev) {
    if (!w || (count && (!volumesDev || !offsetsDev || !totalDev || (capacity && !hitsDev)))) return fail(MI_ERR_INVALID_ARGUMENT, "null argument");
    int rc = queryPrepare(w); if (rc != MI_OK) return rc;
    if (!count) return MI_OK;
    return w->overlapEnqueue(count, reinterpret_cast<const uint32_t*>(volumesDev), include, ranges2Dev, offsetsDev, reinterpret_cast<uint4*>(hitsDev), capacity, totalDev, false, kOvPassCount | kOvPassWrite, false);
}

MI_API int mi_world_sweep(mi_world* w, uint32_t count, const mi_query_volume* volumes, const float* displacements3, uint32_t include, const uint32_t* ranges2, mi_sweep_hit* out) {
    return sweepHost(w, count, volumes, displacements3, include, ranges2, out, false);
}
MI_API int mi_debug_sweep_exhaustive(mi_world* w, uint32_t count, const mi_query_volume* volumes, const float* displacements3, uint32_t include, const uint32_t* ranges2, mi_sweep_hit* out) {
    return sweepHost(w, count, volumes, displacements3, include, ranges2, out, true);
}
MI_API int mi_world_sweep_device_async(mi_world* w, uint32_t count, const mi_query_volume* volumesDev, const float* displacements4Dev, uint32_t include, const uint32_t* ranges2Dev,
                                       mi_sweep_hit* outDev) {
    if (!w || (count && (!volumesDev || !displacements4Dev || !outDev))) return fail(MI_ERR_INVALID_ARGUMENT, "null argument");
    int rc = queryPrepare(w); if (rc != MI_OK) return rc;
    if (!count) return MI_OK;
    return w->sweepEnqueue(count, reinterpret_cast<const uint32_t*>(volumesDev), reinterpret_cast<const float4*>(displacements4Dev), include, ranges2Dev, reinterpret_cast<uint4*>(outDev), false);
}

MI_API int mi_world_distance(mi_world* w, uint32_t count, const mi_query_volume* volumes, const float* maxDistances, uint32_t include, const uint32_t* ranges2, mi_distance_hit* out) {
    return distanceHost(w, count, volumes, maxDistances, include, ranges2, out, false);
}
MI_API int mi_debug_distance_exhaustive(mi_world* w, uint32_t count, const mi_query_volume* volumes, const float* maxDistances, uint32_t include, const uint32_t* ranges2, mi_distance_hit* out) {
    return distanceHost(w, count, volumes, maxDistances, include, ranges2, out, true);
}
MI_API int mi_world_distance_device_async(mi_world* w, uint32_t count, const mi_query_volume* volumesDev, const float* maxDistancesDev, uint32_t include, const uint32_t* ranges2Dev,
                                          mi_distance_hit* outDev) {
    if (!w || (count && (!volumesDev || !outDev))) return fail(MI_ERR_INVALID_ARGUMENT, "null argument");
    int rc = queryPrepare(w); if (rc != MI_OK) return rc;
    if (!count) return MI_OK;
    return w->distanceEnqueue(count, reinterpret_cast<const uint32_t*>(volumesDev), maxDistancesDev, include, ranges2Dev, reinterpret_cast<uint4*>(outDev), false);
}

MI_API int mi_world_terrain_distance(mi_world* w, uint32_t count, const mi_query_volume* volumes, const float* maxDistances, uint32_t merge, mi_distance_hit* out) {
    return terrainDistanceHost(w, count, volumes, maxDistances, merge, out, false);
}
MI_API int mi_debug_terrain_distance_exhaustive(mi_world* w, uint32_t count, const mi_query_volume* volumes, const float* maxDistances, uint32_t merge, mi_distance_hit* out) {
    return terrainDistanceHost(w, count, volumes, maxDistances, merge, out, true);
}
MI_API int mi_world_terrain_distance_device_async(mi_world* w, uint32_t count, const mi_query_volume* volumesDev, const float* maxDistancesDev, uint32_t merge, mi_distance_hit* outDev) {
    if (!w || (count && (!volumesDev || !outDev))) return fail(MI_ERR_INVALID_ARGUMENT, "null argument");
    int rc = queryPrepare(w); if (rc != MI_OK) return rc;
    if (!count) return MI_OK;
    return w->terrainDistanceEnqueue(count, reinterpret_cast<const uint32_t*>(volumesDev), maxDistancesDev, merge, reinterpret_cast<uint4*>(outDev), false);
}

MI_API int mi_world_volume_contacts(mi_world* w, uint32_t count, const mi_query_volume* volumes, uint32_t include, const uint32_t* ranges2, uint32_t* outOffsets,
                                    mi_volume_contact* outContacts, uint32_t capacity, uint32_t* outTotal) {
    return volumeQueryHost(w, kContactFamily, count, volumes, include, ranges2, outOffsets, outContacts, capacity, outTotal, false);
}
MI_API int mi_debug_volume_contacts_exhaustive(mi_world* w, uint32_t count, const mi_query_volume* volumes, uint32_t include, const uint32_t* ranges2, uint32_t* outOffsets,
                                               mi_volume_contact* outContacts, uint32_t capacity, uint32_t* outTotal) {
    return volumeQueryHost(w, kContactFamily, count, volumes, include, ranges2, outOffsets, outContacts, capacity, outTotal, true);
}
MI_API int mi_debug_volume_contacts_times(mi_world* w, float* outMs3) {
    if (!w || !outMs3) return fail(MI_ERR_INVALID_ARGUMENT, "null argument");
    outMs3[0] = outMs3[1] = outMs3[2] = 0.f;
    const mi_world::QueryCache::Candidates& c = w->query.cand;
    if (!c.timed) return MI_OK;
    HIP_TRY(hipEventSynchronize(c.ev[3]));
    HIP_TRY(hipEventElapsedTime(&outMs3[0], c.ev[0], c.ev[1])); HIP_TRY(hipEventElapsedTime(&outMs3[1], c.ev[1], c.ev[2])); HIP_TRY(hipEventElapsedTime(&outMs3[2], c.ev[0], c.ev[3]));
    return MI_OK;
}
MI_API int mi_world_volume_contacts_reserve(mi_world* w, uint32_t maxCandidates) {
    if (!w) return fail(MI_ERR_INVALID_ARGUMENT, "null argument");
    int rc = refuseSharded(w); if (rc != MI_OK) return rc;
    HIP_TRY(hipStreamSynchronize(w->stream));   // (growing frees the old staging: nothing enqueued may still read it)
    return w->contactsReserve(maxCandidates);
}
MI_API int mi_world_volume_contacts_device_async(mi_world* w, uint32_t count, const mi_query_volume* volumesDev, uint32_t include, const uint32_t* ranges2Dev, uint32_t* offsetsDev,
                                                 mi_volume_contact* contactsDev, uint32_t capacity, uint32_t* totals2Dev) {
    if (!w || (count && (!volumesDev || !offsetsDev || !totals2Dev || (capacity && !contactsDev)))) return fail(MI_ERR_INVALID_ARGUMENT, "null argument");
    int rc = queryPrepare(w); if (rc != MI_OK) return rc;
    if (!count) return MI_OK;
    mi_world::QueryCache& qc = w->query;
    if (!qc.cand.cap) return fail(MI_ERR_CAPACITY, "no candidate staging: call mi_world_volume_contacts_reserve first");
    HIP_TRY(qc.vol.candOffsets.ensure((size_t)count + 1));
    rc = w->overlapEnqueue(count, reinterpret_cast<const uint32_t*>(volumesDev), include, ranges2Dev, qc.vol.candOffsets.p, qc.cand.pairs.p, qc.cand.cap, nullptr, false, kOvPassCount | kOvPassWrite, true);
    if (rc != MI_OK) return rc;
    return w->contactsEnqueue(count, qc.cand.cap, capacity, reinterpret_cast<uint4*>(contactsDev), offsetsDev, totals2Dev, false);
}


MI_API int mi_world_terrain_contacts(mi_world* w, uint32_t count, const mi_query_volume* volumes, uint32_t* outOffsets, mi_terrain_contact* outContacts, uint32_t capacity,
                                     uint32_t* outTotal) {
    return volumeQueryHost(w, kTerrainFamily, count, volumes, 0u, nullptr, outOffsets, outContacts, capacity, outTotal, false);
}
MI_API int mi_world_terrain_contacts_device_async(mi_world* w, uint32_t count, const mi_query_volume* volumesDev, uint32_t* offsetsDev, mi_terrain_contact* contactsDev,
                                                  uint32_t capacity, uint32_t* totalDev) {
    if (!w || (count && (!volumesDev || !offsetsDev || !totalDev || (capacity && !contactsDev)))) return fail(MI_ERR_INVALID_ARGUMENT, "null argument");
    int rc = queryPrepare(w); if (rc != MI_OK) return rc;
    if (!count) return MI_OK;
    return w->terrainEnqueue(count, reinterpret_cast<const uint32_t*>(volumesDev), offsetsDev, reinterpret_cast<float4*>(contactsDev), capacity, totalDev);
}

}  // extern "C"
