// Part of world.hip (one translation unit; #included there, in this order): sharded world: include/mi_shard.h (tiles, ghosts, RCCL transport, exact seam, load balance).

// ================================================================================================ sharded world (include/mi_shard.h)
extern "C++" {
namespace {
// tile -> rank: tiles in ascending Morton code of (tx, tz); rank r simulates the r-th of them
uint32_t mortonCode(uint32_t x, uint32_t z) { uint32_t c = 0; for (uint32_t b = 0; b < 16; ++b) c |= ((x >> b) & 1u) << (2 * b) | ((z >> b) & 1u) << (2 * b + 1); return c; }
std::vector<uint32_t> tilesInRankOrder(uint32_t tx, uint32_t tz) {
    std::vector<uint32_t> t((size_t)tx * tz);
    for (uint32_t i = 0; i < t.size(); ++i) t[i] = i;
    std::sort(t.begin(), t.end(), [&](uint32_t a, uint32_t b) { uint32_t ca = mortonCode(a % tx, a / tx), cb = mortonCode(b % tx, b / tx); return ca != cb ? ca < cb : a < b; });
    return t;
}
struct Id128 { char bytes[128]; };   // ncclUniqueId
// RCCL, resolved at run time (the library has no link-time dependency on it; a process that already loaded librccl.so.1 — torch — shares it)
struct Rccl {
    void* lib = nullptr;
    int (*GetUniqueId)(void*) = nullptr;
    int (*CommInitRank)(void**, int, Id128, int) = nullptr;
    int (*CommDestroy)(void*) = nullptr;
    int (*Send)(const void*, size_t, int, int, void*, hipStream_t) = nullptr;
    int (*Recv)(void*, size_t, int, int, void*, hipStream_t) = nullptr;
    int (*GroupStart)() = nullptr; int (*GroupEnd)() = nullptr;
    int (*AllReduce)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
};
Rccl* rccl() {
    static Rccl r; static bool tried = false;
    if (tried) return r.lib ? &r : nullptr;
    tried = true;
    for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
        r.lib = dlopen(name, RTLD_NOW | RTLD_NOLOAD); if (r.lib) break;
    }
    if (!r.lib) for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) { r.lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL); if (r.lib) break; }
    if (!r.lib) return nullptr;
    auto sym = [&](const char* n) { return dlsym(r.lib, n); };
    r.GetUniqueId = (decltype(r.GetUniqueId))sym("ncclGetUniqueId"); r.CommInitRank = (decltype(r.CommInitRank))sym("ncclCommInitRank");
    r.CommDestroy = (decltype(r.CommDestroy))sym("ncclCommDestroy"); r.Send = (decltype(r.Send))sym("ncclSend"); r.Recv = (decltype(r.Recv))sym("ncclRecv");
    r.GroupStart = (decltype(r.GroupStart))sym("ncclGroupStart"); r.GroupEnd = (decltype(r.GroupEnd))sym("ncclGroupEnd"); r.GetErrorString = (decltype(r.GetErrorString))sym("ncclGetErrorString");
    r.AllReduce = (decltype(r.AllReduce))sym("ncclAllReduce");
    if (!r.GetUniqueId || !r.CommInitRank || !r.Send || !r.Recv || !r.GroupStart || !r.GroupEnd) { r.lib = nullptr; return nullptr; }
    return &r;
}
constexpr int kNcclFloat32 = 7;   // ncclFloat32 (rccl.h)
constexpr int kNcclUint64 = 5, kNcclSum = 0;
}
}

// Pack the records every neighbour is owed (device), then — library transport — one RCCL group of sends / receives on the world's stream and
// the unpack kernels behind it; nothing is read back in between.  With the caller's transport the messages wait in sendBuf for mi_world_shard_export.
// An articulated island is owned / ghosted / ignored as ONE (its root = lowest body index decides): union-find over the joints' body pairs.
int mi_world::shardBuildRoots() {
    const uint32_t nb = (uint32_t)bodies.size();
    std::vector<uint32_t> parent(nb);
    for (uint32_t i = 0; i < nb; ++i) parent[i] = i;
    auto find = [&](uint32_t x) { while (parent[x] != x) { parent[x] = parent[parent[x]]; x = parent[x]; } return x; };
    joints.each([&](uint32_t, const auto& t) { for (const uint2& b : t.bodies) { uint32_t x = find(b.x), y = find(b.y); if (x != y) parent[std::max(x, y)] = std::min(x, y); } });
    for (uint32_t i = 0; i < nb; ++i) parent[i] = find(i);
    HIP_TRY(shard.root.ensure(std::max(nb, 1u))); HIP_TRY(shard.active.ensure(std::max(nb, 1u)));
    if (nb) HIP_TRY(hipMemcpy(shard.root.p, parent.data(), (size_t)nb * sizeof(uint32_t), hipMemcpyHostToDevice));
    shard.rootJoints = joints.count(); shard.rootBodies = nb;
    return MI_OK;
}
void mi_world::shardReleaseComm() { if (shard.comm) { if (Rccl* r = rccl()) if (r->CommDestroy) (void)r->CommDestroy(shard.comm); shard.comm = nullptr; } }
// A neighbour message that did not fit is an error, never a silent loss: the packed record counts of the last exchange are checked as soon as
// they are on the host — right after the exchange with the caller's transport (it synchronises anyway), and with the library transport at the
// next exchange or whenever the caller looks at the world in between (counts, owned entities, exchange statistics, checkpoint, detach).
int mi_world::shardCheckOverflow(bool sync) {
    ShardState& sh = shard;
    if (!sh.sentPending) return MI_OK;
    if (sync) HIP_TRY(hipStreamSynchronize(stream));
    sh.sentPending = false;
    if (sh.exchangeTimed) { sh.exchangeMsSum += (double)elapsedMs(sh.exEv[0], sh.exEv[1]); ++sh.exchangesTimed; sh.exchangeTimed = false; }
    for (uint32_t k = 0; k < sh.sp.numPeers; ++k) { sh.sentLast[k] = sh.sentHost[k]; sh.sentSum[k] += sh.sentHost[k]; }
    if (sh.rccl && sh.recvHost) {   // what the neighbours sent in that exchange (the headers of their messages)
        for (uint32_t k = 0; k < sh.sp.numPeers; ++k) {
            // (the first two exchanges after enable / attach travel at full size whatever the policy, so this arrives before any message whose length depends on it)
            if (sh.recvHost[k] == 0xFFFFFFFEu) return fail(MI_ERR_INVALID_ARGUMENT, "the ranks disagree about MI_SHARD_ADAPTIVE (read per world at mi_world_create): set it identically on all ranks");
            if (sh.recvHost[k] == 0xFFFFFFFFu) return fail(MI_ERR_CAPACITY, "a neighbour message outgrew the size both ranks had derived from the previous exchange (more than 1.5 x + 512 records in one step): set MI_SHARD_ADAPTIVE=0 on all ranks for fixed-size messages");
            sh.recvLast[k] = sh.recvHost[k];
        }
        sh.recvValid = true;
    }
    for (uint32_t k = 0; k < sh.sp.numPeers; ++k) if (sh.sentHost[k] > sh.capacity) return fail(MI_ERR_CAPACITY, "shard message overflow: raise mi_shard_desc::max_records (equal on all ranks)");
    if (sh.rccl) for (uint32_t k = 0; k < sh.sp.numPeers; ++k)   // ... and the sender of a message that outgrew its derived size knows it as well as the receiver does
        if (sh.sizedLast[k] && sh.sentHost[k] > sh.sizedLast[k]) return fail(MI_ERR_CAPACITY, "a neighbour message outgrew the size both ranks had derived from the previous exchange (more than 1.5 x + 512 records in one step): set MI_SHARD_ADAPTIVE=0 on all ranks for fixed-size messages");
    return MI_OK;
}
int mi_world::shardExchange() {
    const uint32_t nb = (uint32_t)bodies.size(), nc = (uint32_t)colliders.size();
    if (!nb) return MI_OK;
    ShardState& sh = shard;
    { int rc = shardCheckOverflow(false); if (rc != MI_OK) return rc; }   // (the previous exchange's counts have long arrived: the end-of-step read-back came after them)
    hipStream_t st = stream;
    StepScalars* sc = scalarsPtr();
    ShardBufs sendBufs{}, recvBufs{};
    for (uint32_t k = 0; k < sh.sp.numPeers; ++k) { sendBufs.p[k] = sh.sendBuf[k].p; recvBufs.p[k] = sh.recvBuf[k].p; }
    if (!sh.exEv[0]) { HIP_TRY(hipEventCreate(&sh.exEv[0])); HIP_TRY(hipEventCreate(&sh.exEv[1])); }
    HIP_TRY(hipEventRecord(sh.exEv[0], st));
    // after a valid step the buffer sets are swapped: bPos = the new state, bPosN = the state the step started from; the record counts were cleared by k_reset_scalars
    const bool blockSkip = knobs.shardBlockSkip && sh.blockStamp.p && !sh.blocksAll && sh.prevValid && sh.flagsOfAStep;   // (the stamps describe the step that just ended)
    k_shard_pack<<<blockSkip ? std::min(divUp(nb, 256), kShardGrid) : divUp(nb, 256), 256, 0, st>>>(nb, sh.sp, sh.bordersPending ? sh.spNext : sh.sp, sh.bordersPending ? 1u : 0u, sh.known.p, sh.active.p, bPos.p, bRot.p, bLinVel.p, bAngVel.p, bPosN.p, bRotN.p, bCogInvMass.p, sendBufs, sh.capacity, sc, sh.root.p, blockSkip ? sh.blockStamp.p : nullptr, (uint32_t)totalSteps);
    k_shard_pack_headers<<<1, 64, 0, st>>>(sh.sp.numPeers, sc, sendBufs, nc, sh.rccl ? nullptr : sh.axisDev.p, sh.adaptive ? 1u : 0u, sh.sentHost);   // caller's transport: until the caller hands in the centre statistics
                                                                                                                    // summed over all ranks (mi_world_shard_set_axis_sums), the next step's sweep axis is the one of this rank's own sums
    sh.sentPending = true; sh.exchangeTimed = true;
    if (sh.bordersPending) { sh.sp = sh.spNext; sh.bordersX = sh.nextX; sh.bordersZ = sh.nextZ; sh.bordersPending = false; sh.fullExchanges = 2; sh.sweepFullSteps = 2; sh.blocksAll = true; }   // the next step classifies with the new borders (this exchange hands bodies over: full-size messages, on every rank)
    if (!sh.rccl) {
        // (the axis of this rank's own sums is also what k_pair_finish computed: hs.axisNext, already in sapAxis)
        HIP_TRY(hipEventRecord(sh.exEv[1], st));
        HIP_TRY(hipStreamSynchronize(st));     // the messages are complete when this returns
        sh.axisHostCurrent = true;
        return shardCheckOverflow(false);
    }
    Rccl* r = rccl();
    ShardCaps caps{}; uint32_t maxRecs = 0;
    const bool sized = sh.adaptive && sh.fullExchanges == 0u && sh.recvValid;
    for (uint32_t k = 0; k < 8u; ++k) {
        const uint32_t m = std::max(sh.sentLast[k], sh.recvLast[k]);
        caps.c[k] = sized && k < sh.sp.numPeers ? std::min(sh.capacity, m + m / 2u + 512u) : sh.capacity;
        if (k < sh.sp.numPeers) { sh.sizedLast[k] = caps.c[k]; maxRecs = std::max(maxRecs, caps.c[k]); sh.bytesSentSum += (uint64_t)(caps.c[k] + 1u) * kShardRecordFloats * sizeof(float); }
    }
    if (sh.fullExchanges) --sh.fullExchanges;
    int e = r->GroupStart(); if (e) return fail(MI_ERR_DEVICE, "ncclGroupStart failed");
    for (uint32_t k = 0; k < sh.sp.numPeers && !e; ++k) {
        const size_t n = (size_t)(caps.c[k] + 1u) * kShardRecordFloats;   // header + the records both ends expect at most
        e = r->Send(sh.sendBuf[k].p, n, kNcclFloat32, (int)sh.peerRanks[k], sh.comm, st);
        if (!e) e = r->Recv(sh.recvBuf[k].p, n, kNcclFloat32, (int)sh.peerRanks[k], sh.comm, st);
    }
    const int e2 = r->GroupEnd();
    if (e || e2) return fail(MI_ERR_DEVICE, r->GetErrorString ? r->GetErrorString(e ? e : e2) : "RCCL send / receive failed");
    if (sh.sp.numPeers) {
        k_shard_unpack<<<dim3(divUp(std::max(maxRecs, 1u), 256), sh.sp.numPeers), 256, 0, st>>>(nb, recvBufs, sh.capacity, bPos.p, bRot.p, bLinVel.p, bAngVel.p, sh.known.p, caps, &sc->shardRecv[0], sh.adaptive ? 1u : 0u, sh.blockStamp.p, (uint32_t)totalSteps + 1u);
        if (!sh.recvHost) { HIP_TRY(hipHostMalloc((void**)&sh.recvHost, 8 * sizeof(uint32_t))); std::memset(sh.recvHost, 0, 8 * sizeof(uint32_t)); }
        HIP_TRY(hipMemcpyAsync(sh.recvHost, &sc->shardRecv[0], 8 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));   // (read at the next exchange, like the sent counts)
    }
    // global sweep axis: the centre statistics of the colliders every rank owns, summed over all ranks (72 bytes), stay on the device
    if (r->AllReduce) {
        const int e3 = r->AllReduce(sc->axisSums, sh.axisGlobal.p, kAxisSums, kNcclUint64, kNcclSum, sh.comm, st);
        if (e3) return fail(MI_ERR_DEVICE, r->GetErrorString ? r->GetErrorString(e3) : "ncclAllReduce failed");
        k_shard_axis<<<1, 64, 0, st>>>(sh.axisGlobal.p, nc, sh.axisDev.p);
    } else k_shard_axis<<<1, 64, 0, st>>>(sc->axisSums, nc, sh.axisDev.p);
    sh.axisHostCurrent = false;
    HIP_TRY(hipEventRecord(sh.exEv[1], st));
    hostStale = true;
    return MI_OK;
}
// Exact seam: the hand-over after sweep `sweep` (include/mi_shard.h).  The velocities of the bodies this rank owns and a neighbour holds as ghosts are gathered
// into one fixed-size message per neighbour; library transport: sent / received / scattered on the world's stream; caller's transport: the stream is
// drained and the caller's function moves mi_world_shard_export_sweep -> mi_world_shard_import_sweep.
int mi_world::shardSweepExchange(uint32_t sweep) {
    ShardState& sh = shard;
    hipStream_t st = stream;
    const uint32_t nb = (uint32_t)bodies.size();
    ShardBufs send{}, recv{}; SweepLists lists{};
    for (uint32_t k = 0; k < sh.sp.numPeers; ++k) {
        HIP_TRY(sh.sweepSend[k].ensure(sh.sweepFloats())); HIP_TRY(sh.sweepRecv[k].ensure(sh.sweepFloats()));
        send.p[k] = sh.sweepSend[k].p; recv.p[k] = sh.sweepRecv[k].p; lists.p[k] = sh.sweepList[k].p;
    }
    if (sh.sp.numPeers) k_seam_sweep_pack<<<dim3(divUp(sh.capacity, 256), sh.sp.numPeers), 256, 0, st>>>(lists, sh.sweepCount.p, sh.capacity, gVel.p, send);
    ++sh.sweepExchanges;
    if (sh.sweepsDone++ == 0u && sh.sp.numPeers) {   // once per step: did the lists fit?  (the step is synchronous in this mode anyway)
        uint32_t* counts = sh.sweepCounts;
        HIP_TRY(hipMemcpyAsync(counts, sh.sweepCount.p, 8 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        for (uint32_t k = 0; k < sh.sp.numPeers; ++k) if (counts[k] > sh.capacity) return fail(MI_ERR_CAPACITY, "exact seam: more shared bodies than a neighbour message holds (mi_shard_desc::max_records)");
        if (sh.sweepCut) { sh.sweepCut = false; return fail(MI_ERR_CAPACITY, "exact seam: a sweep message outgrew the size both ranks had derived from the previous step (more than 1.5 x + 64 shared bodies in one step): set MI_SHARD_ADAPTIVE=0 on all ranks"); }
        if (sh.rccl) {   // this step's message sizes: both ends know both list lengths of the PREVIOUS step (their own, and the header of the last message they received)
            const bool sized = sh.adaptive && sh.sweepFullSteps == 0u && sh.sweepRecvValid;
            if (sh.sweepRecvValid) { for (uint32_t k = 0; k < sh.sp.numPeers; ++k) HIP_TRY(hipMemcpyAsync(&sh.sweepPeerHdr[k], sh.sweepRecv[k].p, sizeof(uint32_t), hipMemcpyDeviceToHost, st)); HIP_TRY(hipStreamSynchronize(st)); }
            // ... and the RECEIVER of a message that was cut short fails here as well, at the same point of the same step as its sender (which set sweepCut when it packed more than the
            // derived size): the header carries the sender's true count, sweepSized[k] still holds the size that message travelled at.  Both ranks return before either posts a send / receive,
            // so nobody waits in the stream for a partner that has already given up.
            if (sh.sweepRecvValid) for (uint32_t k = 0; k < sh.sp.numPeers; ++k)
                if (sh.sweepPeerHdr[k] > sh.sweepSized[k]) { sh.sweepCut = false; return fail(MI_ERR_CAPACITY, "exact seam: a neighbour's sweep message outgrew the size both ranks had derived from the previous step (more than 1.5 x + 64 shared bodies in one step): set MI_SHARD_ADAPTIVE=0 on all ranks"); }
            for (uint32_t k = 0; k < sh.sp.numPeers; ++k) {
                const uint32_t m = std::max(sh.sweepPrevOwn[k], sh.sweepPeerHdr[k]);
                sh.sweepSized[k] = sized ? std::min(sh.capacity, m + m / 2u + 64u) : sh.capacity;
                if (counts[k] > sh.sweepSized[k] || (sized && sh.sweepPeerHdr[k] > sh.capacity)) sh.sweepCut = true;   // (sent cut short all the same — the neighbour is already waiting for exactly that many floats —, reported at the next step)
                sh.sweepPrevOwn[k] = counts[k];
            }
            if (sh.sweepFullSteps) --sh.sweepFullSteps;
        }
    }
    if (sh.rccl) {
        Rccl* r = rccl();
        int e = r->GroupStart(); if (e) return fail(MI_ERR_DEVICE, "ncclGroupStart failed");
        ShardCaps caps{};
        for (uint32_t k = 0; k < 8u; ++k) caps.c[k] = k < sh.sp.numPeers ? sh.sweepSized[k] : sh.capacity;
        for (uint32_t k = 0; k < sh.sp.numPeers && !e; ++k) {
            const size_t n = (size_t)(sh.sweepSized[k] + 1u) * kSweepRecordFloats;   // header + the records both ends expect at most
            e = r->Send(sh.sweepSend[k].p, n, kNcclFloat32, (int)sh.peerRanks[k], sh.comm, st);
            if (!e) e = r->Recv(sh.sweepRecv[k].p, n, kNcclFloat32, (int)sh.peerRanks[k], sh.comm, st);
        }
        const int e2 = r->GroupEnd();
        if (e || e2) return fail(MI_ERR_DEVICE, r->GetErrorString ? r->GetErrorString(e ? e : e2) : "RCCL send / receive failed");
        if (sh.sp.numPeers) k_seam_sweep_unpack<<<dim3(divUp(sh.capacity, 256), sh.sp.numPeers), 256, 0, st>>>(nb, recv, sh.capacity, sh.active.p, gVel.p, caps);
        sh.sweepRecvValid = true;
        return MI_OK;
    }
    HIP_TRY(hipStreamSynchronize(st));   // the messages are complete
    if (!sh.sweepFn) return fail(MI_ERR_INVALID_ARGUMENT, "exact seam: neither the library transport is attached nor a sweep exchange callback set — the seam would silently run as block Jacobi");
    { const int rc = sh.sweepFn(sh.sweepUser, this, sweep); if (rc != MI_OK) return fail(MI_ERR_DEVICE, "exact seam: the caller's sweep exchange failed"); }
    return MI_OK;
}
MI_API int mi_world_set_seam_tiling(mi_world* w, const mi_shard_desc* d) {
    if (!w) return fail(MI_ERR_INVALID_ARGUMENT, "null");
    HIP_TRY(hipSetDevice(w->device));
    w->tabValid = false; w->haveEstimates = false;   // the colour ranges mean something else from here on
    if (!d) { w->seamTiling.on = false; return MI_OK; }
    if (w->shard.enabled) return fail(MI_ERR_UNSUPPORTED, "a sharded world takes its tiling from mi_world_shard_enable (mi_world_shard_set_exact_seam)");
    if (!d->tiles_x || !d->tiles_z || !(d->tile_size_x > 0.f) || !(d->tile_size_z > 0.f) || !(d->ghost_margin > 0.f) || 2.f * d->ghost_margin > d->tile_size_x || 2.f * d->ghost_margin > d->tile_size_z)
        return fail(MI_ERR_INVALID_ARGUMENT, "tiles must be at least two ghost margins wide");
    mi_world::SeamTiling& t = w->seamTiling;
    t.bx.clear(); t.bz.clear(); t.margin = d->ghost_margin;
    for (uint32_t i = 1; i < d->tiles_x; ++i) t.bx.push_back((float)((double)d->origin_x + (double)i * (double)d->tile_size_x));
    for (uint32_t i = 1; i < d->tiles_z; ++i) t.bz.push_back((float)((double)d->origin_z + (double)i * (double)d->tile_size_z));
    HIP_TRY(t.dBx.ensure(std::max<size_t>(t.bx.size(), 1))); HIP_TRY(t.dBz.ensure(std::max<size_t>(t.bz.size(), 1)));
    if (!t.bx.empty()) HIP_TRY(hipMemcpy(t.dBx.p, t.bx.data(), t.bx.size() * sizeof(float), hipMemcpyHostToDevice));
    if (!t.bz.empty()) HIP_TRY(hipMemcpy(t.dBz.p, t.bz.data(), t.bz.size() * sizeof(float), hipMemcpyHostToDevice));
    t.on = true;
    if (!w->topologyDirty) { int rc = w->shardBuildRoots(); if (rc != MI_OK) return rc; }   // (an upload builds them otherwise)
    return MI_OK;
}
MI_API int mi_world_shard_set_exact_seam(mi_world* w, uint32_t enable, mi_shard_sweep_fn fn, void* user) {
    if (!w || !w->shard.enabled) return fail(MI_ERR_INVALID_ARGUMENT, "not a sharded world");
    mi_world::ShardState& sh = w->shard;
    if (enable && sh.desc.tiles_x > 1u && sh.desc.tiles_z > 1u) return fail(MI_ERR_UNSUPPORTED, "exact seam: x- or z-slabs only (at a corner a shared body is seen by four tiles)");
    if (enable && (2.f * sh.desc.ghost_margin > sh.desc.tile_size_x || 2.f * sh.desc.ghost_margin > sh.desc.tile_size_z)) return fail(MI_ERR_INVALID_ARGUMENT, "exact seam: tiles must be at least two ghost margins wide");
    if (enable && !fn && !sh.rccl) return fail(MI_ERR_INVALID_ARGUMENT, "exact seam: with the caller's transport a sweep exchange callback is needed");
    if (enable) {   // ... also the tiles a load balance has cut (borders in force and pending): a body must never lie within the margin of two borders
        const float m2 = 2.f * sh.desc.ghost_margin;
        for (const std::vector<float>* b : {&sh.bordersX, &sh.bordersZ, &sh.nextX, &sh.nextZ})
            for (size_t i = 1; i < b->size(); ++i) if (!((*b)[i] - (*b)[i - 1] > m2)) return fail(MI_ERR_INVALID_ARGUMENT, "exact seam: a tile of the current borders is narrower than two ghost margins");
    }
    HIP_TRY(hipSetDevice(w->device));
    if (sh.exact != (enable != 0u)) { w->tabValid = false; w->haveEstimates = false; }   // the colour ranges mean something else from here on
    sh.exact = enable != 0u; sh.sweepFn = fn; sh.sweepUser = user; sh.sweepFullSteps = 2; sh.sweepRecvValid = false;
    if (sh.exact) { HIP_TRY(sh.sweepImport.ensure(sh.sweepFloats())); HIP_TRY(w->seamId.ensure(std::max<size_t>(w->bodies.size(), 1))); }
    return MI_OK;
}
MI_API int mi_world_shard_sweep_message_bytes(mi_world* w, uint64_t* out) {
    if (!w || !out || !w->shard.enabled) return fail(MI_ERR_INVALID_ARGUMENT, "not a sharded world");
    *out = (uint64_t)w->shard.sweepFloats() * sizeof(float); return MI_OK;
}
MI_API int mi_world_shard_export_sweep(mi_world* w, uint32_t slot, void* out) {
    if (!w || !out || !w->shard.enabled || !w->shard.exact || slot >= w->shard.sp.numPeers || !w->shard.sweepSend[slot].p) return fail(MI_ERR_INVALID_ARGUMENT, "no sweep message for this slot");
    HIP_TRY(hipSetDevice(w->device));
    // (only what the message holds: its header and `count` records; the rest of the caller's buffer is not touched)
    HIP_TRY(hipMemcpyAsync(out, w->shard.sweepSend[slot].p, (size_t)(std::min(w->shard.sweepCounts[slot], w->shard.capacity) + 1u) * kSweepRecordFloats * sizeof(float), hipMemcpyDeviceToHost, w->stream));
    HIP_TRY(hipStreamSynchronize(w->stream));
    return MI_OK;
}
MI_API int mi_world_shard_import_sweep(mi_world* w, const void* msg) {
    if (!w || !msg || !w->shard.enabled || !w->shard.exact) return fail(MI_ERR_INVALID_ARGUMENT, "not an exact-seam world");
    if (w->shard.rccl) return fail(MI_ERR_INVALID_ARGUMENT, "the library transport exchanges the sweeps itself");
    mi_world::ShardState& sh = w->shard;
    uint32_t count; std::memcpy(&count, msg, 4);
    if (count > sh.capacity) return fail(MI_ERR_CAPACITY, "sweep message holds more records than max_records");
    HIP_TRY(hipSetDevice(w->device));
    HIP_TRY(sh.sweepImport.ensure(sh.sweepFloats()));
    HIP_TRY(hipMemcpyAsync(sh.sweepImport.p, msg, (size_t)(count + 1u) * kSweepRecordFloats * sizeof(float), hipMemcpyHostToDevice, w->stream));
    ShardBufs in{}; in.p[0] = sh.sweepImport.p;
    if (count) k_seam_sweep_unpack<<<dim3(divUp(count, 256), 1), 256, 0, w->stream>>>((uint32_t)w->bodies.size(), in, sh.capacity, sh.active.p, w->gVel.p);
    HIP_TRY(hipStreamSynchronize(w->stream));   // the staging buffer is free again
    return MI_OK;
}
MI_API int mi_world_seam_stats(mi_world* w, uint32_t* manifolds, uint32_t* colors, uint32_t* violations) {
    if (!w) return fail(MI_ERR_INVALID_ARGUMENT, "null");
    if (manifolds) *manifolds = w->seamLast[0];
    if (colors) *colors = w->seamLast[1];
    if (violations) *violations = (uint32_t)std::min<uint64_t>(w->seamViolations, 0xFFFFFFFFull);
    return MI_OK;
}
// sapAxis (host) <- the device word, when a library-transport exchange has moved it on
int mi_world::shardSyncAxis() {
    if (!shard.enabled || shard.axisHostCurrent || !shard.axisDev.p) return MI_OK;
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipMemcpyAsync(&sapAxis, shard.axisDev.p, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    shard.axisHostCurrent = true;
    return MI_OK;
}

MI_API int mi_shard_tile_of_rank(uint32_t tx, uint32_t tz, uint32_t rank, uint32_t* out) {
    if (!out || !tx || !tz || tx > 65535u || tz > 65535u || rank >= tx * tz) return fail(MI_ERR_INVALID_ARGUMENT, "bad tile grid / rank");
    *out = tilesInRankOrder(tx, tz)[rank]; return MI_OK;
}
MI_API int mi_shard_rank_of_tile(uint32_t tx, uint32_t tz, uint32_t tile, uint32_t* out) {
    if (!out || !tx || !tz || tx > 65535u || tz > 65535u || tile >= tx * tz) return fail(MI_ERR_INVALID_ARGUMENT, "bad tile grid / tile");
    const std::vector<uint32_t> t = tilesInRankOrder(tx, tz);
    *out = (uint32_t)(std::find(t.begin(), t.end(), tile) - t.begin()); return MI_OK;
}
MI_API int mi_world_shard_enable(mi_world* w, const mi_shard_desc* d) {
    if (!w || !d) return fail(MI_ERR_INVALID_ARGUMENT, "null");
    if (!d->tiles_x || !d->tiles_z || d->tiles_x > 65535u || d->tiles_z > 65535u || d->num_ranks != d->tiles_x * d->tiles_z || d->rank >= d->num_ranks) return fail(MI_ERR_INVALID_ARGUMENT, "num_ranks must equal tiles_x * tiles_z");
    if (!(d->tile_size_x > 0.f) || !(d->tile_size_z > 0.f) || !(d->ghost_margin > 0.f) || d->ghost_margin >= d->tile_size_x || d->ghost_margin >= d->tile_size_z) return fail(MI_ERR_INVALID_ARGUMENT, "0 < ghost_margin < tile size");
    HIP_TRY(hipSetDevice(w->device));
    mi_world::ShardState& sh = w->shard;
    if (w->seamTiling.on) { w->seamTiling.on = false; w->tabValid = false; w->haveEstimates = false; }   // a told tiling (mi_world_set_seam_tiling) ends here: a sharded world takes its seam colouring from mi_world_shard_set_exact_seam only
    sh.desc = *d; sh.blocksAll = true;
    const std::vector<uint32_t> order = tilesInRankOrder(d->tiles_x, d->tiles_z);
    ShardParams& sp = sh.sp;
    sp.margin = d->ghost_margin;
    sp.tilesX = d->tiles_x; sp.tilesZ = d->tiles_z; sp.myTile = order[d->rank]; sp.numPeers = 0; sh.peerRanks.clear();
    sh.bordersX.clear(); sh.bordersZ.clear(); sh.bordersPending = false; sh.flagsOfAStep = false;
    for (uint32_t i = 1; i < d->tiles_x; ++i) sh.bordersX.push_back((float)((double)d->origin_x + (double)i * (double)d->tile_size_x));
    for (uint32_t i = 1; i < d->tiles_z; ++i) sh.bordersZ.push_back((float)((double)d->origin_z + (double)i * (double)d->tile_size_z));
    w->shardFillBorders(sp, sh.bordersX, sh.bordersZ);
    const int mx = (int)(sp.myTile % sp.tilesX), mz = (int)(sp.myTile / sp.tilesX);
    for (int z = mz - 1; z <= mz + 1; ++z) for (int x = mx - 1; x <= mx + 1; ++x) {          // ascending tile index
        if ((x == mx && z == mz) || x < 0 || z < 0 || x >= (int)sp.tilesX || z >= (int)sp.tilesZ) continue;
        const uint32_t t = (uint32_t)z * sp.tilesX + (uint32_t)x;
        sp.peers[sp.numPeers++] = t;
        sh.peerRanks.push_back((uint32_t)(std::find(order.begin(), order.end(), t) - order.begin()));
    }
    const uint32_t nb = (uint32_t)w->bodies.size();
    sh.capacity = d->max_records ? d->max_records : std::max(4096u, nb / d->num_ranks / 4u);   // a message always travels whole: (capacity + 1) records of 56 bytes
    { int rc = w->shardBuildRoots(); if (rc != MI_OK) return rc; }
    for (HBody& b : w->bodies) b.shardKnown = 1;                     // every rank was given the same scene
    HIP_TRY(sh.known.ensure(std::max(nb, 1u))); HIP_TRY(hipMemset(sh.known.p, 1, std::max(nb, 1u)));
    for (uint32_t k = 0; k < sp.numPeers; ++k) {
        HIP_TRY(sh.sendBuf[k].ensure(sh.messageFloats())); HIP_TRY(sh.recvBuf[k].ensure(sh.messageFloats()));
        HIP_TRY(hipMemset(sh.sendBuf[k].p, 0, sh.messageFloats() * sizeof(float))); HIP_TRY(hipMemset(sh.recvBuf[k].p, 0, sh.messageFloats() * sizeof(float)));
    }
    if (!sh.sentHost && hipHostMalloc((void**)&sh.sentHost, 8 * sizeof(uint32_t), hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) { (void)hipGetLastError(); HIP_TRY(hipHostMalloc((void**)&sh.sentHost, 8 * sizeof(uint32_t))); }   // (written by k_shard_pack_headers)
    std::memset(sh.sentHost, 0, 8 * sizeof(uint32_t)); sh.sentPending = false; sh.exchangeTimed = false;
    sh.fullExchanges = 2; sh.recvValid = false; sh.sweepFullSteps = 2; sh.sweepRecvValid = false; sh.adaptive = w->knobs.shardAdaptive;
    HIP_TRY(sh.axisDev.ensure(1)); HIP_TRY(sh.axisGlobal.ensure(kAxisSums)); HIP_TRY(sh.importBuf.ensure(sh.messageFloats()));
    HIP_TRY(hipMemcpy(sh.axisDev.p, &w->sapAxis, sizeof(uint32_t), hipMemcpyHostToDevice)); sh.axisHostCurrent = true;
    sh.enabled = true;
    w->haveEstimates = false;   // the first sharded step sizes itself exactly
    return MI_OK;
}
MI_API int mi_world_shard_neighbours(mi_world* w, uint32_t* out, uint32_t* count) {
    if (!w || !count || !w->shard.enabled) return fail(MI_ERR_INVALID_ARGUMENT, "not a sharded world");
    *count = w->shard.sp.numPeers;
    if (out) for (uint32_t k = 0; k < w->shard.sp.numPeers; ++k) out[k] = w->shard.peerRanks[k];
    return MI_OK;
}
MI_API int mi_world_shard_counts(mi_world* w, uint32_t* bodies, uint32_t* manifolds, uint32_t* contacts) {
    if (!w || !w->shard.enabled) return fail(MI_ERR_INVALID_ARGUMENT, "not a sharded world");
    if (bodies) *bodies = w->shard.owned[0];
    if (manifolds) *manifolds = w->shard.owned[1];
    if (contacts) *contacts = w->shard.owned[2];
    return w->shardCheckOverflow(true);   // (an overflow in the LAST exchange of a run is reported here at the latest)
}
// ---- load balance: the tile borders follow the bodies
extern "C++" {
namespace {
// What ONE change of the borders may do.  A body's new owner, and every rank that newly holds it as a ghost, must be the old owner's tile or one of
// its neighbours (only those exchange messages): new border i stays within [old border i-1 + margin, old border i+1 - margin]; and a tile stays
// wider than the margin (its ghost region must not reach past its neighbours).
bool shardBordersValid(const std::vector<float>& cur, const float* nb, uint32_t n, float m, float minWidth) {   // minWidth: m, or 2 m under the exact seam (a body within the margin of TWO borders has no seam class)
    for (uint32_t i = 0; i < n; ++i) {
        if (!(nb[i] == nb[i])) return false;
        if (i > 0 && !(nb[i] - nb[i - 1] > minWidth)) return false;
        if (i > 0 && nb[i] < cur[i - 1] + m) return false;
        if (i + 1 < n && nb[i] > cur[i + 1] - m) return false;
    }
    return true;
}
}
}
void mi_world::shardFillBorders(ShardParams& sp, const std::vector<float>& bx, const std::vector<float>& bz) const {
    const float inf = std::numeric_limits<float>::infinity();
    auto lower = [&](const std::vector<float>& b, int tile) { return tile <= 0 ? -inf : tile > (int)b.size() ? inf : b[(size_t)tile - 1]; };   // lower border of `tile`
    const int mx = (int)(sp.myTile % sp.tilesX), mz = (int)(sp.myTile / sp.tilesX);
    for (int k = 0; k < 4; ++k) { sp.bx[k] = lower(bx, mx - 1 + k); sp.bz[k] = lower(bz, mz - 1 + k); }
}
MI_API int mi_world_shard_set_borders(mi_world* w, const float* bx, const float* bz) {
    if (!w || !w->shard.enabled) return fail(MI_ERR_INVALID_ARGUMENT, "not a sharded world");
    mi_world::ShardState& sh = w->shard;
    const float m = sh.desc.ghost_margin;
    const float minWidth = sh.exact ? 2.f * m : m;
    if ((bx && !shardBordersValid(sh.bordersX, bx, (uint32_t)sh.bordersX.size(), m, minWidth)) || (bz && !shardBordersValid(sh.bordersZ, bz, (uint32_t)sh.bordersZ.size(), m, minWidth)))
        return fail(MI_ERR_INVALID_ARGUMENT, "borders: ascending, tiles wider than ghost_margin (two margins under the exact seam), and border i within [old border i-1 + margin, old border i+1 - margin]");
    sh.nextX = bx ? std::vector<float>(bx, bx + sh.bordersX.size()) : sh.bordersX;
    sh.nextZ = bz ? std::vector<float>(bz, bz + sh.bordersZ.size()) : sh.bordersZ;
    sh.spNext = sh.sp; w->shardFillBorders(sh.spNext, sh.nextX, sh.nextZ);
    sh.bordersPending = true;
    return MI_OK;
}
MI_API int mi_world_shard_get_borders(mi_world* w, float* bx, float* bz) {
    if (!w || !w->shard.enabled) return fail(MI_ERR_INVALID_ARGUMENT, "not a sharded world");
    if (bx) std::copy(w->shard.bordersX.begin(), w->shard.bordersX.end(), bx);
    if (bz) std::copy(w->shard.bordersZ.begin(), w->shard.bordersZ.end(), bz);
    return MI_OK;
}
MI_API int mi_world_shard_histogram(mi_world* w, uint32_t axis, float lo, float hi, uint32_t bins, uint32_t* out) {
    if (!w || !out || !w->shard.enabled || axis > 1u || !bins || !(hi > lo)) return fail(MI_ERR_INVALID_ARGUMENT, "axis 0 | 1, bins > 0, lo < hi");
    HIP_TRY(hipSetDevice(w->device));
    const uint32_t nb = (uint32_t)w->bodies.size();
    std::fill(out, out + bins, 0u);
    if (!nb || w->topologyDirty || !w->shard.flagsOfAStep) return MI_OK;   // no step since the scene was (re)built: nothing is owned yet
    HIP_TRY(w->shard.hist.ensure(bins));
    HIP_TRY(hipMemsetAsync(w->shard.hist.p, 0, bins * sizeof(uint32_t), w->stream));
    k_shard_histogram<<<divUp(nb, 256), 256, 0, w->stream>>>(nb, axis, lo, (float)bins / (hi - lo), bins, w->shard.active.p, w->bPos.p, w->bRot.p, w->bCogInvMass.p, w->shard.root.p, w->shard.hist.p);
    HIP_TRY(hipMemcpyAsync(out, w->shard.hist.p, bins * sizeof(uint32_t), hipMemcpyDeviceToHost, w->stream));
    HIP_TRY(hipStreamSynchronize(w->stream));
    return MI_OK;
}
// Borders that even out the body counts: hist = bodies per bin of [lo, hi) along one axis, summed over all ranks.  Border i goes where the cumulative
// count reaches i / tiles of the total (linear inside a bin), clamped to what one change may do; pure arithmetic, the same on every rank.
MI_API int mi_shard_balance_borders(const uint64_t* hist, uint32_t bins, float lo, float hi, uint32_t tiles, const float* cur, float margin, float* out) {
    if (!hist || !bins || !(hi > lo) || !tiles || (tiles > 1 && (!cur || !out))) return fail(MI_ERR_INVALID_ARGUMENT, "null / empty");
    const uint32_t n = tiles - 1u;
    if (!n) return MI_OK;
    const std::vector<float> c(cur, cur + n);
    std::vector<float> nb(c);
    double total = 0; for (uint32_t b = 0; b < bins; ++b) total += (double)hist[b];
    if (total > 0) {
        const double width = ((double)hi - (double)lo) / (double)bins;
        uint32_t b = 0; double below = 0;
        for (uint32_t i = 0; i < n; ++i) {
            const double target = total * (double)(i + 1u) / (double)tiles;
            while (b + 1u < bins && below + (double)hist[b] < target) { below += (double)hist[b]; ++b; }
            const double frac = hist[b] ? std::min(1.0, std::max(0.0, (target - below) / (double)hist[b])) : 0.5;
            double v = (double)lo + ((double)b + frac) * width;
            if (i > 0) v = std::max(v, std::max((double)c[i - 1] + (double)margin, (double)nb[i - 1] + 1.25 * (double)margin));   // (x 1.25: room to move next time)
            if (i + 1u < n) v = std::min(v, (double)c[i + 1] - (double)margin);
            // ... and move by at most two margins: the hand-over rides in ONE neighbour message, whose capacity is sized in margin strips
            v = std::min(std::max(v, (double)c[i] - 2.0 * (double)margin), (double)c[i] + 2.0 * (double)margin);
            if (i > 0) v = std::max(v, (double)nb[i - 1] + 1.25 * (double)margin);
            nb[i] = (float)v;
        }
    }
    const bool ok = shardBordersValid(c, nb.data(), n, margin, margin);
    for (uint32_t i = 0; i < n; ++i) out[i] = ok ? nb[i] : c[i];
    return MI_OK;
}
// Sum of n 64-bit counters over all ranks: ONE ncclAllReduce on the world's stream (global counts; the histograms of the load balance)
MI_API int mi_world_shard_allreduce_u64(mi_world* w, uint64_t* inout, uint32_t n) {
    if (!w || !w->shard.enabled || (n && !inout)) return fail(MI_ERR_INVALID_ARGUMENT, "not a sharded world / null");
    if (!w->shard.rccl) return fail(MI_ERR_UNSUPPORTED, "the library's all-reduce needs the library transport (mi_world_shard_attach_rccl); with the caller's transport reduce the values yourself");
    Rccl* r = rccl(); if (!r || !r->AllReduce) return fail(MI_ERR_UNSUPPORTED, "ncclAllReduce not found");
    if (!n) return MI_OK;
    HIP_TRY(hipSetDevice(w->device));
    HIP_TRY(w->shard.reduceBuf.ensure(n));
    HIP_TRY(hipMemcpyAsync(w->shard.reduceBuf.p, inout, n * sizeof(uint64_t), hipMemcpyHostToDevice, w->stream));
    const int e = r->AllReduce(w->shard.reduceBuf.p, w->shard.reduceBuf.p, n, kNcclUint64, kNcclSum, w->shard.comm, w->stream);
    if (e) return fail(MI_ERR_DEVICE, r->GetErrorString ? r->GetErrorString(e) : "ncclAllReduce failed");
    HIP_TRY(hipMemcpyAsync(inout, w->shard.reduceBuf.p, n * sizeof(uint64_t), hipMemcpyDeviceToHost, w->stream));
    HIP_TRY(hipStreamSynchronize(w->stream));
    return MI_OK;
}
// One rebalancing round in one call (library transport): histograms of both axes over the extent of the tile grid as enabled, all-reduced, balanced, set.
MI_API int mi_world_shard_rebalance(mi_world* w, uint32_t bins) {
    if (!w || !w->shard.enabled || !bins || bins > 65536u) return fail(MI_ERR_INVALID_ARGUMENT, "not a sharded world / bins");
    if (!w->shard.rccl) return fail(MI_ERR_UNSUPPORTED, "mi_world_shard_rebalance needs the library transport; with the caller's transport: mi_world_shard_histogram, your all-reduce, mi_shard_balance_borders, mi_world_shard_set_borders");
    const mi_shard_desc& d = w->shard.desc;
    const float lo[2] = {d.origin_x, d.origin_z};
    const float hi[2] = {(float)((double)d.origin_x + (double)d.tiles_x * (double)d.tile_size_x), (float)((double)d.origin_z + (double)d.tiles_z * (double)d.tile_size_z)};
    std::vector<uint32_t> h32(bins); std::vector<uint64_t> h((size_t)2 * bins);
    for (uint32_t a = 0; a < 2; ++a) {
        int rc = mi_world_shard_histogram(w, a, lo[a], hi[a], bins, h32.data()); if (rc != MI_OK) return rc;
        for (uint32_t b = 0; b < bins; ++b) h[(size_t)a * bins + b] = h32[b];
    }
    int rc = mi_world_shard_allreduce_u64(w, h.data(), 2u * bins); if (rc != MI_OK) return rc;
    std::vector<float> nx(w->shard.bordersX), nz(w->shard.bordersZ);
    rc = mi_shard_balance_borders(h.data(), bins, lo[0], hi[0], d.tiles_x, w->shard.bordersX.data(), d.ghost_margin, nx.data()); if (rc != MI_OK) return rc;
    rc = mi_shard_balance_borders(h.data() + bins, bins, lo[1], hi[1], d.tiles_z, w->shard.bordersZ.data(), d.ghost_margin, nz.data()); if (rc != MI_OK) return rc;
    if (w->shard.exact) {   // exact seam: a tile stays wider than TWO margins (a body within the margin of two borders has no seam class); a proposal that would not is not taken
        const float m2 = 2.f * d.ghost_margin;
        auto wide = [&](const std::vector<float>& b) { for (size_t i = 1; i < b.size(); ++i) if (!(b[i] - b[i - 1] > m2)) return false; return true; };
        if (!wide(nx)) nx = w->shard.bordersX;
        if (!wide(nz)) nz = w->shard.bordersZ;
    }
    return mi_world_shard_set_borders(w, nx.empty() ? nullptr : nx.data(), nz.empty() ? nullptr : nz.data());
}
MI_API int mi_world_shard_owned_entities(mi_world* w, uint32_t* out, uint32_t cap, uint32_t* count) {
    if (!w || !count || !w->shard.enabled) return fail(MI_ERR_INVALID_ARGUMENT, "not a sharded world");
    HIP_TRY(hipSetDevice(w->device));
    const uint32_t nb = (uint32_t)w->bodies.size();
    std::vector<uint8_t> act(nb, 0);
    HIP_TRY(hipStreamSynchronize(w->stream));
    { int rc = w->shardCheckOverflow(false); if (rc != MI_OK) return rc; }
    if (nb && w->shard.flagsOfAStep && !w->topologyDirty) HIP_TRY(hipMemcpy(act.data(), w->shard.active.p, nb, hipMemcpyDeviceToHost));   // (no step since the scene was (re)built: nothing is owned yet)
    uint32_t n = 0;
    for (uint32_t b = 0; b < nb; ++b) if (act[b] == 1u) { if (out && n < cap) out[n] = w->bodies[b].entity; ++n; }
    *count = n;
    return (out && n > cap) ? fail(MI_ERR_CAPACITY, "capacity < owned bodies") : MI_OK;
}
MI_API int mi_shard_get_unique_id(void* out) {
    if (!out) return fail(MI_ERR_INVALID_ARGUMENT, "null");
    Rccl* r = rccl(); if (!r) return fail(MI_ERR_UNSUPPORTED, "librccl.so.1 not found");
    return r->GetUniqueId(out) == 0 ? MI_OK : fail(MI_ERR_DEVICE, "ncclGetUniqueId failed");
}
MI_API int mi_shard_library_transport_available(void) { Rccl* r = rccl(); return r && r->AllReduce && r->CommDestroy ? 1 : 0; }
MI_API int mi_world_shard_attach_rccl(mi_world* w, const void* id) {
    if (!w || !id || !w->shard.enabled) return fail(MI_ERR_INVALID_ARGUMENT, "enable sharding first");
    Rccl* r = rccl(); if (!r) return fail(MI_ERR_UNSUPPORTED, "librccl.so.1 not found");
    HIP_TRY(hipSetDevice(w->device));
    Id128 uid; std::memcpy(uid.bytes, id, sizeof(uid.bytes));
    const int e = r->CommInitRank(&w->shard.comm, (int)w->shard.desc.num_ranks, uid, (int)w->shard.desc.rank);
    if (e) return fail(MI_ERR_DEVICE, r->GetErrorString ? r->GetErrorString(e) : "ncclCommInitRank failed");
    w->shard.rccl = true; w->shard.fullExchanges = 2; w->shard.recvValid = false; w->shard.sweepFullSteps = 2; w->shard.sweepRecvValid = false;
    return MI_OK;
}
// Development / tests: the library transport on ONE rank.  A one-rank communicator whose every neighbour is this rank itself: the exchange then runs
// ncclGroupStart / ncclSend / ncclRecv / ncclGroupEnd, the unpack kernels and the all-reduce with real records on one GPU — each message comes back to its sender.
// (What a rank receives are the records it packed for the neighbouring tile: states of bodies it holds anyway, so the world goes on exactly like one on the
// caller's transport that is handed its own messages back: tests/test_gpu_sharding.py.)
MI_API int mi_debug_shard_attach_loopback(mi_world* w) {
    if (!w || !w->shard.enabled) return fail(MI_ERR_INVALID_ARGUMENT, "enable sharding first");
    Rccl* r = rccl(); if (!r) return fail(MI_ERR_UNSUPPORTED, "librccl.so.1 not found");
    HIP_TRY(hipSetDevice(w->device));
    Id128 uid; std::memset(&uid, 0, sizeof(uid));
    int e = r->GetUniqueId(&uid);
    if (!e) e = r->CommInitRank(&w->shard.comm, 1, uid, 0);
    if (e) return fail(MI_ERR_DEVICE, r->GetErrorString ? r->GetErrorString(e) : "ncclCommInitRank failed");
    for (uint32_t& p : w->shard.peerRanks) p = 0u;
    w->shard.rccl = true; w->shard.fullExchanges = 2; w->shard.recvValid = false; w->shard.sweepFullSteps = 2; w->shard.sweepRecvValid = false;
    return MI_OK;
}
// ... and the message last RECEIVED in slot `slot` (library transport), so a test can hold it against what was sent
MI_API int mi_debug_shard_peek_received(mi_world* w, uint32_t slot, uint32_t sweep_message, void* out) {
    if (!w || !out || !w->shard.enabled || slot >= w->shard.sp.numPeers) return fail(MI_ERR_INVALID_ARGUMENT, "bad slot");
    HIP_TRY(hipSetDevice(w->device));
    HIP_TRY(hipStreamSynchronize(w->stream));
    const DBuf<float>& b = sweep_message ? w->shard.sweepRecv[slot] : w->shard.recvBuf[slot];
    const size_t n = sweep_message ? w->shard.sweepFloats() : w->shard.messageFloats();
    if (!b.p || b.cap < n) return fail(MI_ERR_INVALID_ARGUMENT, "nothing received in this slot yet");
    HIP_TRY(hipMemcpy(out, b.p, n * sizeof(float), hipMemcpyDeviceToHost));
    return MI_OK;
}
MI_API int mi_world_shard_detach_rccl(mi_world* w) {
    if (!w || !w->shard.enabled) return fail(MI_ERR_INVALID_ARGUMENT, "not a sharded world");
    HIP_TRY(hipSetDevice(w->device));
    HIP_TRY(hipStreamSynchronize(w->stream));
    if (w->shard.exact && !w->shard.sweepFn) return fail(MI_ERR_INVALID_ARGUMENT, "exact seam: detaching the library transport needs a sweep exchange callback (mi_world_shard_set_exact_seam) first");
    w->shardReleaseComm(); w->shard.rccl = false;
    { int rc = w->shardSyncAxis(); if (rc != MI_OK) return rc; }
    return w->shardCheckOverflow(false);
}
MI_API int mi_world_shard_message_bytes(mi_world* w, uint64_t* out) {
    if (!w || !out || !w->shard.enabled) return fail(MI_ERR_INVALID_ARGUMENT, "not a sharded world");
    *out = (uint64_t)w->shard.messageFloats() * sizeof(float); return MI_OK;
}
MI_API int mi_world_shard_export(mi_world* w, uint32_t slot, void* out) {
    if (!w || !out || !w->shard.enabled || slot >= w->shard.sp.numPeers) return fail(MI_ERR_INVALID_ARGUMENT, "bad slot");
    HIP_TRY(hipSetDevice(w->device));
    HIP_TRY(hipMemcpy(out, w->shard.sendBuf[slot].p, w->shard.messageFloats() * sizeof(float), hipMemcpyDeviceToHost));
    return MI_OK;
}
MI_API int mi_world_shard_import(mi_world* w, const void* msg) {
    if (!w || !msg || !w->shard.enabled) return fail(MI_ERR_INVALID_ARGUMENT, "not a sharded world");
    if (w->shard.rccl) return fail(MI_ERR_INVALID_ARGUMENT, "mi_world_shard_import belongs to the caller's transport; this world exchanges through the library's (mi_world_shard_detach_rccl first)");
    HIP_TRY(hipSetDevice(w->device));
    uint32_t count; std::memcpy(&count, msg, 4);
    if (count > w->shard.capacity) return fail(MI_ERR_CAPACITY, "shard message overflow: raise mi_shard_desc::max_records (equal on all ranks)");
    w->scalarsClean = false;   // (a kernel on the step scalars outside a step: the next step starts with its own reset)
    const uint32_t nb = (uint32_t)w->bodies.size();
    HIP_TRY(w->shard.importBuf.ensure(w->shard.messageFloats()));   // its own staging: a tile without neighbours (1 x 1 grid) has no receive buffer
    HIP_TRY(hipMemcpyAsync(w->shard.importBuf.p, msg, (size_t)(count + 1u) * kShardRecordFloats * sizeof(float), hipMemcpyHostToDevice, w->stream));
    ShardBufs one{}; one.p[0] = w->shard.importBuf.p;
    ++w->poseEpoch;
    if (count) k_shard_unpack<<<dim3(divUp(count, 256), 1), 256, 0, w->stream>>>(nb, one, w->shard.capacity, w->bPos.p, w->bRot.p, w->bLinVel.p, w->bAngVel.p, w->shard.known.p, ShardCaps{{0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}}, nullptr, 0u,
                                                                                   w->shard.blockStamp.p, (uint32_t)w->totalSteps + 1u);
    HIP_TRY(hipStreamSynchronize(w->stream));     // `msg` is the caller's (possibly pageable) memory
    w->hostStale = true;
    return MI_OK;
}

// Global sweep axis with the caller's transport: this rank's centre statistics of the last internal step (the colliders of the bodies it owned;
// rank 0 also the colliders without a rigid body) — add them over all ranks and hand the sums to every rank before its next step.
MI_API int mi_world_shard_axis_sums(mi_world* w, uint64_t* out9) {
    if (!w || !out9 || !w->shard.enabled) return fail(MI_ERR_INVALID_ARGUMENT, "not a sharded world");
    for (uint32_t c = 0; c < kAxisSums; ++c) out9[c] = w->hs.axisSums[c];
    return MI_OK;
}
MI_API int mi_world_shard_set_axis_sums(mi_world* w, const uint64_t* global9) {
    if (!w || !global9 || !w->shard.enabled) return fail(MI_ERR_INVALID_ARGUMENT, "not a sharded world");
    if (w->shard.rccl) return fail(MI_ERR_INVALID_ARGUMENT, "with the library transport the exchange sums the statistics itself (ncclAllReduce)");
    HIP_TRY(hipSetDevice(w->device));
    unsigned long long s9[kAxisSums]; for (uint32_t c = 0; c < kAxisSums; ++c) s9[c] = global9[c];
    w->sapAxis = axisFromSums(s9, (uint32_t)w->colliders.size());
    HIP_TRY(hipMemcpyAsync(w->shard.axisDev.p, &w->sapAxis, sizeof(uint32_t), hipMemcpyHostToDevice, w->stream));
    HIP_TRY(hipStreamSynchronize(w->stream));
    w->shard.axisHostCurrent = true;
    return MI_OK;
}
// What the exchanges cost and moved (bench.py's N > 1 line): device time between the pack kernel and the end of the unpack / axis kernels.
MI_API int mi_world_shard_exchange_stats(mi_world* w, mi_shard_exchange_stats* out, uint32_t reset) {
    if (!w || !out || !w->shard.enabled) return fail(MI_ERR_INVALID_ARGUMENT, "not a sharded world");
    HIP_TRY(hipSetDevice(w->device));
    mi_world::ShardState& sh = w->shard;
    int rc = w->shardCheckOverflow(true);
    std::memset(out, 0, sizeof(*out));
    out->exchanges = sh.exchangesTimed; out->device_ms_sum = sh.exchangeMsSum; out->num_neighbours = sh.sp.numPeers;
    out->message_bytes = (uint64_t)sh.messageFloats() * sizeof(float); out->library_transport = sh.rccl ? 1u : 0u;
    for (uint32_t k = 0; k < 8u; ++k) out->message_records_last[k] = k < sh.sp.numPeers ? (sh.rccl ? sh.sizedLast[k] : sh.capacity) : 0u;
    out->message_bytes_sum = sh.bytesSentSum;
    for (uint32_t k = 0; k < sh.sp.numPeers; ++k) { out->neighbour_rank[k] = sh.peerRanks[k]; out->records_last[k] = sh.sentLast[k]; out->records_sum[k] = sh.sentSum[k]; }
    const uint32_t nb = (uint32_t)w->bodies.size();
    if (nb && sh.flagsOfAStep && !w->topologyDirty) {
        std::vector<uint8_t> act(nb);
        HIP_TRY(hipMemcpy(act.data(), sh.active.p, nb, hipMemcpyDeviceToHost));
        for (uint8_t a : act) { out->owned_bodies += a == 1u; out->ghost_bodies += a == 2u; }
    }
    out->sweep_exchanges = sh.sweepExchanges; out->sweep_message_bytes = sh.exact ? (uint64_t)((sh.rccl && sh.sp.numPeers ? sh.sweepSized[0] : sh.capacity) + 1u) * kSweepRecordFloats * sizeof(float) : 0ull;
    for (uint32_t k = 0; k < sh.sp.numPeers; ++k) out->sweep_records_last[k] = sh.exact ? sh.sweepCounts[k] : 0u;
    if (reset) { sh.exchangesTimed = 0; sh.exchangeMsSum = 0.0; for (uint64_t& v : sh.sentSum) v = 0; sh.sweepExchanges = 0; sh.bytesSentSum = 0; }
    return rc;
}
