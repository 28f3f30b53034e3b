// Part of world.hip (one translation unit; #included there, in this order): checkpoints, body states on the device, stage dumps, debug entry points.

// ---- checkpoint / resume (SURVEY §5: the solver-relevant state of a world)
// Everything a bit-identical continuation needs that is not the scene description itself: body states (physics_transform1,
// velocities, accumulators), physics_transform0 + the interpolated entity transforms, the step accumulator, the SAP axis chosen
// for the next step, the colour history (pair -> colour, which is also the previous step's collision list of the events), the
// previous step's trigger overlaps and the constraint PODs (motors / limits may have been edited).  The blob is tied to the
// topology: it can only be loaded into a world built from the same scene (same bodies, colliders, constraints).
extern "C++" {
namespace {
struct CheckpointHeader { uint32_t magic, version, numEntities, numBodies, numColliders, numHistory, numTriggerOverlaps, sapAxis; float timer; uint32_t eventsEnabled, jointCounts[6], reserved; };
constexpr uint32_t kCheckpointMagic = 0x4350494Du;   // "MIPC"
// CheckpointHeader::reserved bit 0: a SHARD SECTION follows the cloths — the blob is ONE RANK's view of a sharded world (include/mi_shard.h): which of
// its body copies are current (a rank only trusts a copy it owned in the last step or got a record for), the tile borders in force and the pending
// ones of a load-balance round.  Without it a restore to an earlier step would classify with the flags and borders of the LATER moment: bodies that
// migrated in between would be owned by nobody (or by two ranks) and silently drop out.  Such a blob only loads into the same rank of the same grid.
constexpr uint32_t kCheckpointHasShard = 1u;
struct CheckpointShard { uint32_t numRanks, rank, tilesX, tilesZ, bordersPending, knownBytes; };
template <class T> void put(std::vector<uint8_t>& out, const T* p, size_t n) { const uint8_t* b = reinterpret_cast<const uint8_t*>(p); out.insert(out.end(), b, b + n * sizeof(T)); }
template <class T> bool take(const uint8_t*& p, const uint8_t* end, T* out, size_t n) { if ((size_t)(end - p) < n * sizeof(T)) return false; std::memcpy(out, p, n * sizeof(T)); p += n * sizeof(T); return true; }
}
}
MI_API int mi_world_save_checkpoint(mi_world* w, void* out, uint64_t capacity, uint64_t* out_size) {
    if (!w || !out_size) return fail(MI_ERR_INVALID_ARGUMENT, "null");
    HIP_TRY(hipSetDevice(w->device));
    int rc = w->download(); if (rc != MI_OK) return rc;
    rc = w->joints.pullDeviceWrites(); if (rc != MI_OK) return rc;   // (the blob holds the PODs as the next step would see them)
    if (w->shard.enabled) { rc = w->shardCheckOverflow(true); if (rc != MI_OK) return rc; rc = w->shardSyncAxis(); if (rc != MI_OK) return rc; }
    std::vector<unsigned long long> keys; std::vector<uint32_t> vals;
    if (w->tabValid) {   // also with a pending topology edit: the keys are creation indices, the live world keeps the history across it
        const size_t cap = (size_t)w->tabMask[w->tabCur] + 1;
        std::vector<HistSlot> t(cap);
        HIP_TRY(hipMemcpy(t.data(), w->tab[w->tabCur].p, cap * sizeof(HistSlot), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < cap; ++i) if (t[i].key) { keys.push_back(t[i].key); vals.push_back((uint32_t)t[i].val); }
    }
    CheckpointHeader h{};
    h.magic = kCheckpointMagic; h.version = 1; h.numEntities = (uint32_t)w->entities.size(); h.numBodies = (uint32_t)w->bodies.size();
    h.numColliders = (uint32_t)w->colliders.size(); h.numHistory = (uint32_t)keys.size(); h.numTriggerOverlaps = (uint32_t)w->prevTriggerOverlaps.size();
    h.sapAxis = w->sapAxis; h.timer = w->timer; h.eventsEnabled = w->eventsEnabled ? 1u : 0u;
    h.reserved = w->shard.enabled ? kCheckpointHasShard : 0u;
    const JointSet& j = w->joints;
    j.each([&](uint32_t type, const auto& l) { h.jointCounts[type] = (uint32_t)l.pods.size(); });
    std::vector<uint8_t> blob;
    put(blob, &h, 1);
    for (const HEntity& e : w->entities) { put(blob, &e.pos, 1); put(blob, &e.rot, 1); }
    for (const HBody& b : w->bodies) { put(blob, &b.p0, 1); put(blob, &b.r0, 1); put(blob, &b.p1, 1); put(blob, &b.r1, 1); put(blob, &b.linVel, 1); put(blob, &b.angVel, 1); put(blob, &b.force, 1); put(blob, &b.torque, 1); }
    if (!keys.empty()) { put(blob, keys.data(), keys.size()); put(blob, vals.data(), vals.size()); }
    if (!w->prevTriggerOverlaps.empty()) put(blob, w->prevTriggerOverlaps.data(), w->prevTriggerOverlaps.size());
    j.each([&](uint32_t, const auto& l) { if (!l.pods.empty()) put(blob, l.pods.data(), l.pods.size()); });
    {   // cloths: particle state (positions incl. inverse mass, previous positions, velocities, force accumulators) and the editable properties
        const uint32_t numCloths = (uint32_t)w->cloths.size();
        put(blob, &numCloths, 1);
        HIP_TRY(hipStreamSynchronize(w->stream));
        for (mi_world::HCloth* c : w->cloths) {
            const uint32_t n = c->desc.grid_size_x * c->desc.grid_size_y;
            put(blob, &c->desc, 1); put(blob, &c->oldTotalMass, 1); put(blob, &c->oldStiffness, 1);
            std::vector<float4> buf(4 * (size_t)n);
            HIP_TRY(hipMemcpy(buf.data(), c->pos.p, n * sizeof(float4), hipMemcpyDeviceToHost)); HIP_TRY(hipMemcpy(buf.data() + n, c->prev.p, n * sizeof(float4), hipMemcpyDeviceToHost));
            HIP_TRY(hipMemcpy(buf.data() + 2 * (size_t)n, c->vel.p, n * sizeof(float4), hipMemcpyDeviceToHost)); HIP_TRY(hipMemcpy(buf.data() + 3 * (size_t)n, c->force.p, n * sizeof(float4), hipMemcpyDeviceToHost));
            put(blob, buf.data(), buf.size());
            put(blob, c->restInvMass.data(), c->restInvMass.size());
        }
    }
    if (w->shard.enabled) {   // this rank's view: current copies, borders (download() has mirrored the device's `known` flags into the host bodies)
        const mi_world::ShardState& sh = w->shard;
        const uint32_t nb = (uint32_t)w->bodies.size();
        CheckpointShard cs{sh.desc.num_ranks, sh.desc.rank, sh.desc.tiles_x, sh.desc.tiles_z, sh.bordersPending ? 1u : 0u, (nb + 3u) & ~3u};
        put(blob, &cs, 1);
        std::vector<uint8_t> known(cs.knownBytes, 0); for (uint32_t i = 0; i < nb; ++i) known[i] = w->bodies[i].shardKnown;
        put(blob, known.data(), known.size());
        const std::vector<float>& nx = sh.bordersPending ? sh.nextX : sh.bordersX; const std::vector<float>& nz = sh.bordersPending ? sh.nextZ : sh.bordersZ;
        if (!sh.bordersX.empty()) { put(blob, sh.bordersX.data(), sh.bordersX.size()); put(blob, nx.data(), nx.size()); }
        if (!sh.bordersZ.empty()) { put(blob, sh.bordersZ.data(), sh.bordersZ.size()); put(blob, nz.data(), nz.size()); }
    }
    *out_size = blob.size();
    if (!out) return MI_OK;
    if (capacity < blob.size()) return fail(MI_ERR_CAPACITY, "capacity < checkpoint size");
    std::memcpy(out, blob.data(), blob.size());
    return MI_OK;
}
MI_API int mi_world_load_checkpoint(mi_world* w, const void* data, uint64_t size) {
    if (!w || !data) return fail(MI_ERR_INVALID_ARGUMENT, "null");
    HIP_TRY(hipSetDevice(w->device));
    // Transactional: the blob is validated against the scene and its own header BEFORE anything is allocated from its counts,
    // parsed into temporaries, and only committed to the world once it has been consumed completely.  Nothing throws across the ABI.
    try {
        const uint8_t* p = static_cast<const uint8_t*>(data); const uint8_t* end = p + size;
        CheckpointHeader h;
        if (!take(p, end, &h, 1) || h.magic != kCheckpointMagic || h.version != 1) return fail(MI_ERR_INVALID_ARGUMENT, "not a checkpoint of this library version");
        JointSet& j = w->joints;
        { int prc = j.pullDeviceWrites(); if (prc != MI_OK) return prc; }   // (the blob's PODs replace the mirror; nothing newer may be pulled over them later)
        uint32_t jc[6]; uint64_t podBytes = 0;   // the POD section: the types' arrays one after the other
        j.each([&](uint32_t type, const auto& l) { jc[type] = (uint32_t)l.pods.size(); podBytes += (uint64_t)l.pods.size() * sizeof(l.pods[0]); });
        if (h.numEntities != w->entities.size() || h.numBodies != w->bodies.size() || h.numColliders != w->colliders.size() || std::memcmp(jc, h.jointCounts, sizeof(jc)) != 0)
            return fail(MI_ERR_INVALID_ARGUMENT, "checkpoint belongs to a different scene (entity / body / collider / constraint counts differ)");
        // exact size the header implies (64-bit arithmetic; the cloth section is checked against the world's own cloths)
        const uint64_t entityBytes = sizeof(w->entities[0].pos) + sizeof(w->entities[0].rot);
        const uint64_t bodyBytes = sizeof(HBody::p0) + sizeof(HBody::r0) + sizeof(HBody::p1) + sizeof(HBody::r1) + sizeof(HBody::linVel) + sizeof(HBody::angVel) + sizeof(HBody::force) + sizeof(HBody::torque);
        uint64_t expect = sizeof(CheckpointHeader) + (uint64_t)h.numEntities * entityBytes + (uint64_t)h.numBodies * bodyBytes
                        + (uint64_t)h.numHistory * (sizeof(unsigned long long) + sizeof(uint32_t)) + (uint64_t)h.numTriggerOverlaps * sizeof(w->prevTriggerOverlaps[0])
                        + podBytes + sizeof(uint32_t);
        for (const mi_world::HCloth* c : w->cloths) {
            const uint64_t n = (uint64_t)c->desc.grid_size_x * c->desc.grid_size_y;
            expect += sizeof(mi_cloth_desc) + 2 * sizeof(float) + 4 * n * sizeof(float4) + (uint64_t)c->restInvMass.size() * sizeof(c->restInvMass[0]);
        }
        const bool hasShard = (h.reserved & kCheckpointHasShard) != 0u;
        if (h.reserved & ~kCheckpointHasShard) return fail(MI_ERR_INVALID_ARGUMENT, "not a checkpoint of this library version");
        if (hasShard) {
            if (!w->shard.enabled) return fail(MI_ERR_INVALID_ARGUMENT, "the checkpoint is one rank's view of a sharded world: enable sharding (same grid, same rank) before loading it");
            expect += sizeof(CheckpointShard) + (((uint64_t)h.numBodies + 3u) & ~3ull) + 2ull * sizeof(float) * (w->shard.bordersX.size() + w->shard.bordersZ.size());
        }
        if (expect != size) return fail(MI_ERR_INVALID_ARGUMENT, "truncated or oversized checkpoint (size does not match its header and this scene)");
        // ---- parse into temporaries
        struct EntityState { decltype(HEntity::pos) pos; decltype(HEntity::rot) rot; };
        struct BodyState { decltype(HBody::p0) p0; decltype(HBody::r0) r0; decltype(HBody::p1) p1; decltype(HBody::r1) r1; decltype(HBody::linVel) linVel, angVel, force, torque; };
        std::vector<EntityState> es(h.numEntities); std::vector<BodyState> bs(h.numBodies);
        bool okay = true;
        for (EntityState& e : es) okay = okay && take(p, end, &e.pos, 1) && take(p, end, &e.rot, 1);
        for (BodyState& b : bs) okay = okay && take(p, end, &b.p0, 1) && take(p, end, &b.r0, 1) && take(p, end, &b.p1, 1) && take(p, end, &b.r1, 1) && take(p, end, &b.linVel, 1) && take(p, end, &b.angVel, 1) && take(p, end, &b.force, 1) && take(p, end, &b.torque, 1);
        std::vector<unsigned long long> keys(h.numHistory); std::vector<uint32_t> vals(h.numHistory);
        okay = okay && take(p, end, keys.data(), keys.size()) && take(p, end, vals.data(), vals.size());
        auto overlaps = w->prevTriggerOverlaps; overlaps.resize(h.numTriggerOverlaps);
        okay = okay && take(p, end, overlaps.data(), overlaps.size());
        std::vector<uint8_t> podSection((size_t)podBytes);   // staged whole (sized by the world's own pools, which the header's counts equal); copied into the pools type by type at commit
        okay = okay && take(p, end, podSection.data(), podSection.size());
        uint32_t numCloths = 0;
        okay = okay && take(p, end, &numCloths, 1);
        if (!okay) return fail(MI_ERR_INVALID_ARGUMENT, "truncated checkpoint");
        if (numCloths != w->cloths.size()) return fail(MI_ERR_INVALID_ARGUMENT, "checkpoint belongs to a different scene (cloth count differs)");
        struct ClothState { mi_cloth_desc d; float oldMass, oldStiff; std::vector<float4> buf; std::vector<float2> rest; };
        std::vector<ClothState> cs(w->cloths.size());
        for (size_t k = 0; k < cs.size(); ++k) {
            const mi_world::HCloth* c = w->cloths[k]; ClothState& t = cs[k];
            okay = take(p, end, &t.d, 1) && take(p, end, &t.oldMass, 1) && take(p, end, &t.oldStiff, 1);
            if (!okay) return fail(MI_ERR_INVALID_ARGUMENT, "truncated checkpoint");
            if (t.d.grid_size_x != c->desc.grid_size_x || t.d.grid_size_y != c->desc.grid_size_y) return fail(MI_ERR_INVALID_ARGUMENT, "checkpoint belongs to a different scene (cloth grid differs)");
            const size_t n = (size_t)c->desc.grid_size_x * c->desc.grid_size_y;
            t.buf.resize(4 * n); t.rest.resize(c->restInvMass.size());
            if (!take(p, end, t.buf.data(), t.buf.size()) || !take(p, end, t.rest.data(), t.rest.size())) return fail(MI_ERR_INVALID_ARGUMENT, "truncated checkpoint");
        }
        CheckpointShard shardHdr{}; std::vector<uint8_t> known; std::vector<float> curX, nextX, curZ, nextZ;
        if (hasShard) {
            const mi_world::ShardState& sh = w->shard;
            if (!take(p, end, &shardHdr, 1)) return fail(MI_ERR_INVALID_ARGUMENT, "truncated checkpoint");
            if (shardHdr.numRanks != sh.desc.num_ranks || shardHdr.rank != sh.desc.rank || shardHdr.tilesX != sh.desc.tiles_x || shardHdr.tilesZ != sh.desc.tiles_z || shardHdr.knownBytes != ((h.numBodies + 3u) & ~3u))
                return fail(MI_ERR_INVALID_ARGUMENT, "the checkpoint belongs to another rank or another tile grid of the sharded world");
            known.resize(shardHdr.knownBytes); curX.resize(sh.bordersX.size()); nextX.resize(sh.bordersX.size()); curZ.resize(sh.bordersZ.size()); nextZ.resize(sh.bordersZ.size());
            bool ok2 = take(p, end, known.data(), known.size());
            if (!curX.empty()) ok2 = ok2 && take(p, end, curX.data(), curX.size()) && take(p, end, nextX.data(), nextX.size());
            if (!curZ.empty()) ok2 = ok2 && take(p, end, curZ.data(), curZ.size()) && take(p, end, nextZ.data(), nextZ.size());
            if (!ok2) return fail(MI_ERR_INVALID_ARGUMENT, "truncated checkpoint");
            auto ascending = [](const std::vector<float>& b) { for (size_t i = 0; i < b.size(); ++i) { if (!(b[i] == b[i])) return false; if (i && !(b[i] > b[i - 1])) return false; } return true; };
            if (!ascending(curX) || !ascending(curZ) || !ascending(nextX) || !ascending(nextZ)) return fail(MI_ERR_INVALID_ARGUMENT, "corrupt checkpoint (tile borders)");
        }
        if (p != end) return fail(MI_ERR_INVALID_ARGUMENT, "oversized checkpoint");
        // colour history table: same open-addressing layout the kernels probe (tableSlot / linear probing)
        uint32_t cap = 1024; while ((uint64_t)cap < 2ull * h.numHistory) cap <<= 1;
        std::vector<unsigned long long> tk; std::vector<uint32_t> tv, th;   // th: the probe hints of the table as rebuilt here (kernels_narrow.hpp, tableFind)
        if (h.numHistory) {
            tk.assign(cap, 0ull); tv.assign(cap, 0u); th.assign(cap, 0u);
            for (uint32_t i = 0; i < h.numHistory; ++i) {
                if (!keys[i]) return fail(MI_ERR_INVALID_ARGUMENT, "corrupt checkpoint (null history key)");
                uint32_t s_ = (uint32_t)((keys[i] * 0x9E3779B97F4A7C15ull) >> 40) & (cap - 1u);
                const uint32_t home = s_; uint32_t disp = 0;
                while (tk[s_]) { s_ = (s_ + 1u) & (cap - 1u); ++disp; }
                tk[s_] = keys[i]; tv[s_] = vals[i]; th[home] = std::max(th[home], disp);
            }
        }
        // ---- commit
        int rc = w->download(); if (rc != MI_OK) return rc;   // the host copy becomes authoritative; everything is re-sent before the next step
        if (h.numHistory) { const int c = w->tabCur; HIP_TRY(w->tab[c].ensure(cap)); }
        for (size_t i = 0; i < es.size(); ++i) { w->entities[i].pos = es[i].pos; w->entities[i].rot = es[i].rot; }
        for (size_t i = 0; i < bs.size(); ++i) { HBody& b = w->bodies[i]; b.p0 = bs[i].p0; b.r0 = bs[i].r0; b.p1 = bs[i].p1; b.r1 = bs[i].r1; b.linVel = bs[i].linVel; b.angVel = bs[i].angVel; b.force = bs[i].force; b.torque = bs[i].torque; }
        w->prevTriggerOverlaps = std::move(overlaps);
        const uint8_t* podAt = podSection.data();
        j.each([&](uint32_t, auto& l) { const size_t n = l.pods.size() * sizeof(l.pods[0]); if (n) std::memcpy(l.pods.data(), podAt, n); podAt += n; });
        for (size_t k = 0; k < cs.size(); ++k) {
            mi_world::HCloth* c = w->cloths[k]; ClothState& t = cs[k];
            const uint32_t n = c->desc.grid_size_x * c->desc.grid_size_y;
            c->desc = t.d; c->oldTotalMass = t.oldMass; c->oldStiffness = t.oldStiff; c->restInvMass.assign(t.rest.begin(), t.rest.end());
            for (uint32_t i = 0; i < n; ++i) c->invMasses[i] = t.buf[i].w;
            HIP_TRY(hipMemcpy(c->pos.p, t.buf.data(), n * sizeof(float4), hipMemcpyHostToDevice)); HIP_TRY(hipMemcpy(c->prev.p, t.buf.data() + n, n * sizeof(float4), hipMemcpyHostToDevice));
            HIP_TRY(hipMemcpy(c->vel.p, t.buf.data() + 2 * (size_t)n, n * sizeof(float4), hipMemcpyHostToDevice)); HIP_TRY(hipMemcpy(c->force.p, t.buf.data() + 3 * (size_t)n, n * sizeof(float4), hipMemcpyHostToDevice));
            c->constraintsDirty = true;
        }
        w->clothsDirty = true;
        w->timer = h.timer; w->sapAxis = h.sapAxis; w->eventsEnabled = h.eventsEnabled != 0; w->pendingEvents.clear();
        w->topologyDirty = true; w->haveEstimates = false; w->scalarsClean = false; ++w->poseEpoch;
        if (w->shard.enabled) {   // the rank's view of that moment (or, from a blob of an unsharded / fully synchronised world: every copy is current)
            mi_world::ShardState& sh = w->shard;
            for (size_t i = 0; i < w->bodies.size(); ++i) w->bodies[i].shardKnown = hasShard ? (known[i] ? 1 : 0) : 1;
            if (hasShard) {
                sh.bordersX = curX; sh.bordersZ = curZ; w->shardFillBorders(sh.sp, sh.bordersX, sh.bordersZ);
                sh.bordersPending = shardHdr.bordersPending != 0u;
                if (sh.bordersPending) { sh.nextX = nextX; sh.nextZ = nextZ; sh.spNext = sh.sp; w->shardFillBorders(sh.spNext, sh.nextX, sh.nextZ); }
            }
            sh.flagsOfAStep = false; sh.prevValid = false; sh.sentPending = false; sh.exchangeTimed = false;
            sh.rearmFullSize(); sh.recvValid = false; sh.sweepRecvValid = false;   // (the counts of the exchange before the restore say nothing about the one after it)
            HIP_TRY(hipMemcpy(sh.axisDev.p, &w->sapAxis, sizeof(uint32_t), hipMemcpyHostToDevice)); sh.axisHostCurrent = true;
        }
        w->tabValid = h.numHistory != 0;
        if (w->tabValid) {
            const int c = w->tabCur; w->tabMask[c] = cap - 1u;
            std::vector<HistSlot> t(cap);
            for (uint32_t i = 0; i < cap; ++i) { t[i].key = tk[i]; t[i].val = tv[i]; }
            HIP_TRY(hipMemcpy(w->tab[c].p, t.data(), cap * sizeof(HistSlot), hipMemcpyHostToDevice));
            w->hintOf[c] = 0; HIP_TRY(w->histHint[0].ensure(cap));
            HIP_TRY(hipMemcpy(w->histHint[0].p, th.data(), (size_t)cap * sizeof(uint32_t), hipMemcpyHostToDevice));   // the probe hints of the table as rebuilt here
            w->last.numManifolds = h.numHistory;
        }
        return MI_OK;
    } catch (const std::bad_alloc&) {
        return fail(MI_ERR_OUT_OF_MEMORY, "out of host memory while loading a checkpoint");
    } catch (...) {
        return fail(MI_ERR_INVALID_ARGUMENT, "checkpoint could not be loaded");
    }
}

MI_API int mi_world_enable_events(mi_world* w, uint32_t enable) {
    if (!w) return fail(MI_ERR_INVALID_ARGUMENT, "null");
    w->eventsEnabled = enable != 0; w->pendingEvents.clear(); w->prevTriggerOverlaps.clear();
    w->tabValid = false;           // the event diff starts from an empty previous frame (so does the colour history, once)
    w->haveEstimates = false;
    return MI_OK;
}
MI_API int mi_world_poll_events(mi_world* w, mi_event* out, uint32_t cap, uint32_t* count) {
    if (!w || !count) return fail(MI_ERR_INVALID_ARGUMENT, "null");
    *count = (uint32_t)w->pendingEvents.size();
    if (!out) return MI_OK;
    if (cap < w->pendingEvents.size()) return fail(MI_ERR_CAPACITY, "capacity < pending events");
    std::memcpy(out, w->pendingEvents.data(), w->pendingEvents.size() * sizeof(mi_event));
    w->pendingEvents.clear();
    return MI_OK;
}
MI_API int mi_world_get_step_mode_stats(mi_world* w, uint32_t* steps, uint32_t* spec, uint32_t* retries) {
    if (!w) return fail(MI_ERR_INVALID_ARGUMENT, "null");
    if (steps) *steps = w->totalSteps;
    if (spec) *spec = w->specSteps;
    if (retries) *retries = w->specRetries;
    return MI_OK;
}

MI_API int mi_world_num_entities(mi_world* w, uint32_t* out) { if (!w || !out) return fail(MI_ERR_INVALID_ARGUMENT, "null"); *out = (uint32_t)w->entities.size(); return MI_OK; }

static int getTransforms(mi_world* w, float* p, float* r, uint32_t cap, bool physics) {
    if (!w) return fail(MI_ERR_INVALID_ARGUMENT, "null");
    uint32_t n = (uint32_t)w->entities.size();
    if (cap < n) return fail(MI_ERR_CAPACITY, "capacity < num entities");
    {   // the poses produced on the device in the caller's layout, one copy (PoseStream)
        float t;
        if (w->posesPossible(physics, &t)) {
            mi_world::PoseStream& ps = w->pose;
            if (!(ps.valid && ps.steps == w->totalSteps && ps.t == t && ps.n == n && ps.tablesValid && ps.tableCount == n)) { ++ps.produced_on_demand; int rc = w->posesProduce(t, false, false); if (rc != MI_OK) return rc; }
            ps.askedPhysics = physics;
            return w->posesFetch(p, r, nullptr, nullptr);
        }
    }
    {   // The caller that reads the poses after every step (a renderer): positions and rotations come straight from the device — 2 arrays (4 while an
        // interpolation is pending) instead of the 6-8 of a full download() — and the host mirror of the bodies is left alone (still stale: whoever
        // needs it downloads it).  Same arithmetic as download(), which keeps producing the same values later.
        const uint32_t nb = (uint32_t)w->bodies.size();
        const bool follow = physics || w->transformsFollowPhysics, lerpNow = !follow && w->lerpPending;
        if (w->hostStale && !w->topologyDirty && nb && (follow || lerpNow)) {
            HIP_TRY(hipSetDevice(w->device));
            const bool p0Dev = lerpNow && w->p0OnDevice;
            const size_t rows = (p0Dev ? 4u : 2u) * (size_t)nb;
            if (rows > w->downloadStageCap) {
                if (w->downloadStage) (void)hipHostFree(w->downloadStage);
                w->downloadStage = nullptr; w->downloadStageCap = 0;
                HIP_TRY(hipHostMalloc((void**)&w->downloadStage, (8u * (size_t)nb + 2u * (size_t)nb) * sizeof(float4)));   // what download() will ask for, once
                w->downloadStageCap = 8u * (size_t)nb + 2u * (size_t)nb;
            }
            float4 *pos = w->downloadStage, *rot = pos + nb, *pos0 = rot + nb, *rot0 = pos0 + nb;
            HIP_TRY(hipMemcpyAsync(pos, w->bPos.p, (size_t)nb * 16, hipMemcpyDeviceToHost, w->stream));
            HIP_TRY(hipMemcpyAsync(rot, w->bRot.p, (size_t)nb * 16, hipMemcpyDeviceToHost, w->stream));
            if (p0Dev) {
                HIP_TRY(hipMemcpyAsync(pos0, w->bPos0.p, (size_t)nb * 16, hipMemcpyDeviceToHost, w->stream));
                HIP_TRY(hipMemcpyAsync(rot0, w->bRot0.p, (size_t)nb * 16, hipMemcpyDeviceToHost, w->stream));
            }
            HIP_TRY(hipStreamSynchronize(w->stream));
            const float t = w->lerpT;
            hostParallelFor(n, [&](uint32_t i) {
                const HEntity& e = w->entities[i];
                V3 ps = e.pos; Q4 rt = e.rot;
                if (e.rb >= 0) {
                    const uint32_t b = (uint32_t)e.rb;
                    const V3 p1(pos[b].x, pos[b].y, pos[b].z); const Q4 r1(rot[b].x, rot[b].y, rot[b].z, rot[b].w);
                    if (follow) { ps = p1; rt = r1; }
                    else {   // lerp(trs): nlerp on the quaternion (src/core/math.h:673-682)
                        const V3 p0 = p0Dev ? V3(pos0[b].x, pos0[b].y, pos0[b].z) : w->bodies[b].p0;
                        const Q4 r0 = p0Dev ? Q4(rot0[b].x, rot0[b].y, rot0[b].z, rot0[b].w) : w->bodies[b].r0;
                        ps = lerp(p0, p1, t);
                        rt = normalize(Q4(r0.x + t * (r1.x - r0.x), r0.y + t * (r1.y - r0.y), r0.z + t * (r1.z - r0.z), r0.w + t * (r1.w - r0.w)));
                    }
                }
                if (p) { p[3 * i] = ps.x; p[3 * i + 1] = ps.y; p[3 * i + 2] = ps.z; }
                if (r) { r[4 * i] = rt.x; r[4 * i + 1] = rt.y; r[4 * i + 2] = rt.z; r[4 * i + 3] = rt.w; }
            });
            return MI_OK;
        }
    }
    int rc = w->download(); if (rc != MI_OK) return rc;
    hostParallelFor(n, [&](uint32_t i) {
        const HEntity& e = w->entities[i];
        V3 pos = e.pos; Q4 rot = e.rot;
        if (physics && e.rb >= 0) { pos = w->bodies[e.rb].p1; rot = w->bodies[e.rb].r1; }
        if (p) { p[3 * i] = pos.x; p[3 * i + 1] = pos.y; p[3 * i + 2] = pos.z; }
        if (r) { r[4 * i] = rot.x; r[4 * i + 1] = rot.y; r[4 * i + 2] = rot.z; r[4 * i + 3] = rot.w; }
    });
    return MI_OK;
}
MI_API int mi_world_get_transforms(mi_world* w, float* p, float* r, uint32_t cap) { return getTransforms(w, p, r, cap, false); }
MI_API int mi_world_get_physics_transforms(mi_world* w, float* p, float* r, uint32_t cap) { return getTransforms(w, p, r, cap, true); }
// The same values without the last copy: pointers to the library's pinned rows ([n][3] positions, [n][4] rotations), valid until the
// SECOND next stepping call on this world (two sets alternate).  MI_ERR_UNSUPPORTED when the poses are not coming from the device right now
// (nothing stepped since the last download, topology changed, sharded world): mi_world_get_transforms covers every case.
static int viewTransforms(mi_world* w, const float** p, const float** r, uint32_t* count, bool physics) {
    if (!w || (!p && !r)) return fail(MI_ERR_INVALID_ARGUMENT, "null");
    const uint32_t n = (uint32_t)w->entities.size();
    float t;
    if (!w->posesPossible(physics, &t)) return fail(MI_ERR_UNSUPPORTED, "no device-side poses to view (nothing stepped since the last download, topology change pending, or sharded world): mi_world_get_transforms");
    mi_world::PoseStream& ps = w->pose;
    if (!(ps.valid && ps.steps == w->totalSteps && ps.t == t && ps.n == n && ps.tablesValid && ps.tableCount == n)) { ++ps.produced_on_demand; int rc = w->posesProduce(t, false, false); if (rc != MI_OK) return rc; }
    ps.askedPhysics = physics;
    if (count) *count = n;
    const float *vp = nullptr, *vr = nullptr;
    int rc = w->posesFetch(nullptr, nullptr, &vp, &vr); if (rc != MI_OK) return rc;
    if (p) *p = vp;
    if (r) *r = vr;
    return MI_OK;
}
MI_API int mi_world_view_transforms(mi_world* w, const float** p, const float** r, uint32_t* count) { return viewTransforms(w, p, r, count, false); }
MI_API int mi_world_view_physics_transforms(mi_world* w, const float** p, const float** r, uint32_t* count) { return viewTransforms(w, p, r, count, true); }
// The same rows WITHOUT waiting for a copy still on the bus: the newest set that is complete in host memory (include/mi_physics.h)
MI_API int mi_world_view_transforms_landed(mi_world* w, uint32_t physics, const float** p, const float** r, uint32_t* count, uint64_t* of_step) {
    if (!w || (!p && !r)) return fail(MI_ERR_INVALID_ARGUMENT, "null");
    float t;
    if (!w->posesPossible(physics != 0u, &t)) return fail(MI_ERR_UNSUPPORTED, "no device-side poses to view (nothing stepped since the last download, topology change pending, or sharded world): mi_world_get_transforms");
    mi_world::PoseStream& ps = w->pose;
    const uint32_t n = (uint32_t)w->entities.size();
    // nothing produced for the current state yet (the first frame, or a caller that had stopped asking): produce it now — it is on its way while the previous rows are handed out
    if (!(ps.valid && ps.steps == w->totalSteps && ps.t == t && ps.n == n && ps.tablesValid && ps.tableCount == n)) { ++ps.produced_on_demand; int rc = w->posesProduce(t, false, false); if (rc != MI_OK) return rc; }
    int rc = w->posesViewLanded(physics != 0u, p, r, count, of_step);
    if (rc == MI_ERR_UNSUPPORTED) {   // nothing has landed at all yet (the very first request): wait for the rows just produced
        g_lastError.clear();
        const float *vp = nullptr, *vr = nullptr;
        ps.askedPhysics = physics != 0u;
        rc = w->posesFetch(nullptr, nullptr, &vp, &vr); if (rc != MI_OK) return rc;
        if (p) *p = vp;
        if (r) *r = vr;
        if (count) *count = n;
        if (of_step) *of_step = w->totalSteps;
    }
    return rc;
}
// ... and the velocities of every entity's rigid body (zero without one), [n][3] each, from the same rows: they ride along from the frame after the first request on
MI_API int mi_world_view_velocities(mi_world* w, const float** lin, const float** ang, uint32_t* count) {
    if (!w || (!lin && !ang)) return fail(MI_ERR_INVALID_ARGUMENT, "null");
    const uint32_t n = (uint32_t)w->entities.size();
    mi_world::PoseStream& ps = w->pose;
    float t;
    if (!w->posesPossible(ps.askedPhysics, &t)) return fail(MI_ERR_UNSUPPORTED, "no device-side rows to view (nothing stepped since the last download, topology change pending, or sharded world): mi_world_get_velocities");
    ps.wantVel = true;
    const bool current = ps.valid && ps.steps == w->totalSteps && ps.n == n && ps.tablesValid && ps.tableCount == n;
    if (!(current && ps.hasVel)) { ++ps.produced_on_demand; int rc = w->posesProduce(current ? ps.t : t, false, false); if (rc != MI_OK) return rc; }
    if (count) *count = n;
    const float *vl = nullptr, *va = nullptr;
    int rc = w->posesFetch(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &vl, &va); if (rc != MI_OK) return rc;
    if (lin) *lin = vl;
    if (ang) *ang = va;
    return MI_OK;
}
MI_API int mi_debug_color_tail_stats(mi_world* w, uint64_t* steps, uint64_t* rounds) {
    if (!w || !steps || !rounds) return fail(MI_ERR_INVALID_ARGUMENT, "null argument");
    *steps = w->tailSteps; *rounds = w->tailRoundsSum; return MI_OK;
}
MI_API int mi_debug_step_ahead_stats(mi_world* w, uint64_t* enqueued, uint64_t* adopted) {
    if (!w) return fail(MI_ERR_INVALID_ARGUMENT, "null");
    if (enqueued) *enqueued = w->aheadEnqueued;
    if (adopted) *adopted = w->aheadUsed;
    return MI_OK;
}
MI_API int mi_debug_pose_stream_stats(mi_world* w, uint32_t* ahead, uint32_t* on_demand) {
    if (!w) return fail(MI_ERR_INVALID_ARGUMENT, "null");
    if (ahead) *ahead = w->pose.produced_ahead;
    if (on_demand) *on_demand = w->pose.produced_on_demand;
    return MI_OK;
}
MI_API int mi_world_get_velocities(mi_world* w, float* lin, float* ang, uint32_t cap) {
    if (!w) return fail(MI_ERR_INVALID_ARGUMENT, "null");
    uint32_t n = (uint32_t)w->entities.size();
    if (cap < n) return fail(MI_ERR_CAPACITY, "capacity < num entities");
    const uint32_t nb = (uint32_t)w->bodies.size();
    if (w->pose.enabled && w->hostStale && !w->topologyDirty && nb && !w->shard.enabled) {   // a caller that reads poses AND velocities every frame: they ride in the pose rows from the next frame on
        mi_world::PoseStream& ps = w->pose;
        ps.wantVel = true;
        if (ps.valid && ps.hasVel && ps.steps == w->totalSteps && ps.n == n) return w->posesFetch(nullptr, nullptr, nullptr, nullptr, lin, ang);
    }
    if (w->hostStale && !w->topologyDirty && nb) {   // straight from the device, like the poses (getTransforms): two arrays, host mirror left alone
        HIP_TRY(hipSetDevice(w->device));
        if (2u * (size_t)nb > w->downloadStageCap) {
            if (w->downloadStage) (void)hipHostFree(w->downloadStage);
            w->downloadStage = nullptr; w->downloadStageCap = 0;
            HIP_TRY(hipHostMalloc((void**)&w->downloadStage, 10u * (size_t)nb * sizeof(float4)));
            w->downloadStageCap = 10u * (size_t)nb;
        }
        float4 *lv = w->downloadStage, *av = lv + nb;
        HIP_TRY(hipMemcpyAsync(lv, w->bLinVel.p, (size_t)nb * 16, hipMemcpyDeviceToHost, w->stream));
        HIP_TRY(hipMemcpyAsync(av, w->bAngVel.p, (size_t)nb * 16, hipMemcpyDeviceToHost, w->stream));
        HIP_TRY(hipStreamSynchronize(w->stream));
        hostParallelFor(n, [&](uint32_t i) {
            V3 v, a;
            const int b = w->entities[i].rb;
            if (b >= 0) { v = V3(lv[b].x, lv[b].y, lv[b].z); a = V3(av[b].x, av[b].y, av[b].z); }
            if (lin) { lin[3 * i] = v.x; lin[3 * i + 1] = v.y; lin[3 * i + 2] = v.z; }
            if (ang) { ang[3 * i] = a.x; ang[3 * i + 1] = a.y; ang[3 * i + 2] = a.z; }
        });
        return MI_OK;
    }
    int rc = w->download(); if (rc != MI_OK) return rc;
    hostParallelFor(n, [&](uint32_t i) {
        V3 v, a;
        if (w->entities[i].rb >= 0) { v = w->bodies[w->entities[i].rb].linVel; a = w->bodies[w->entities[i].rb].angVel; }
        if (lin) { lin[3 * i] = v.x; lin[3 * i + 1] = v.y; lin[3 * i + 2] = v.z; }
        if (ang) { ang[3 * i] = a.x; ang[3 * i + 1] = a.y; ang[3 * i + 2] = a.z; }
    });
    return MI_OK;
}
MI_API int mi_world_get_mass_properties(mi_world* w, float* invMass, float* invInertia, float* cog, uint32_t cap) {
    if (!w) return fail(MI_ERR_INVALID_ARGUMENT, "null");
    w->recalcProperties();
    uint32_t n = (uint32_t)w->entities.size();
    if (cap < n) return fail(MI_ERR_CAPACITY, "capacity < num entities");
    for (uint32_t i = 0; i < n; ++i) {
        float im = 0.f; M3 ii = M3::zero(); V3 c;
        if (w->entities[i].rb >= 0) { const HBody& b = w->bodies[w->entities[i].rb]; im = b.invMass; ii = b.invInertia; c = b.localCOG; }
        if (invMass) invMass[i] = im;
        if (invInertia) {   // column-major like the reference's mat3 (src/core/math.h:390-397)
            float* o = invInertia + 9 * i;
            o[0] = ii.m00; o[1] = ii.m10; o[2] = ii.m20; o[3] = ii.m01; o[4] = ii.m11; o[5] = ii.m21; o[6] = ii.m02; o[7] = ii.m12; o[8] = ii.m22;
        }
        if (cog) { cog[3 * i] = c.x; cog[3 * i + 1] = c.y; cog[3 * i + 2] = c.z; }
    }
    return MI_OK;
}
MI_API int mi_world_get_counts(mi_world* w, mi_step_counts* out) { if (!w || !out) return fail(MI_ERR_INVALID_ARGUMENT, "null"); *out = w->counts; return MI_OK; }
MI_API int mi_world_get_accumulated_stage_times(mi_world* w, mi_stage_times* out_sum, uint32_t* out_steps, uint64_t* out_contact_updates, uint32_t reset) {
    if (!w) return fail(MI_ERR_INVALID_ARGUMENT, "null");
    w->finishTimes();
    if (out_sum) *out_sum = w->timesSum;
    if (out_steps) *out_steps = w->timesSteps;
    if (out_contact_updates) *out_contact_updates = w->contactUpdatesSum;
    if (reset) { w->timesSum = mi_stage_times{}; w->timesSteps = 0; w->contactUpdatesSum = 0; }
    return MI_OK;
}
// Which contact-solver kernel the last internal step ran: 0 k_contact_solve (one launch per colour per sweep), 1 k_contact_solve_flow,
// 2 k_contact_solve_persist, 3 k_solve_flow_islands (contacts + joint islands fused), 4 k_contact_solve_persist XCD-partitioned, 5 the same on one XCD.
MI_API int mi_debug_step_graph_stats(mi_world* w, uint32_t* out4) {
    if (!w || !out4) return fail(MI_ERR_INVALID_ARGUMENT, "null");
    out4[0] = w->graphsEnabled ? 1u : 0u; out4[1] = w->graphHits; out4[2] = w->graphCaptures; out4[3] = w->graphPlain;
    return MI_OK;
}
// Tests (tests/test_gpu_scan.py): k_exclusive_scan over a host array, enqueued on the world's stream through the step's OWN scan sites (width_bits 32: the cell histogram's,
// 64: the pair scan's) — behind whatever records, tickets and generations the steps and calls so far have left there.  zero_input != 0: `in` comes back as the kernel left it.
MI_API int mi_debug_exclusive_scan(mi_world* w, uint32_t widthBits, void* in, uint32_t n, uint32_t zeroInput, void* out) {
    if (!w || (widthBits != 32u && widthBits != 64u) || (n && (!in || !out))) return fail(MI_ERR_INVALID_ARGUMENT, "width_bits is 32 or 64; null array");
    HIP_TRY(hipSetDevice(w->device));
    if (!n) return MI_OK;
    const size_t bytes = (size_t)n * (widthBits / 8u), words = (bytes + 7u) / 8u;
    HIP_TRY(w->dbgScanIn.ensure(words)); HIP_TRY(w->dbgScanOut.ensure(words));
    HIP_TRY(hipMemcpyAsync(w->dbgScanIn.p, in, bytes, hipMemcpyHostToDevice, w->stream));
    Launcher& L = w->query.L;
    L.begin(false, false);
    if (widthBits == 32u) HIP_TRY(w->scanCells.run(L, reinterpret_cast<uint32_t*>(w->dbgScanIn.p), reinterpret_cast<uint32_t*>(w->dbgScanOut.p), n, w->stream, zeroInput != 0u));
    else HIP_TRY(w->scanPairs.run(L, w->dbgScanIn.p, w->dbgScanOut.p, n, w->stream, zeroInput != 0u));
    HIP_TRY(hipMemcpyAsync(out, w->dbgScanOut.p, bytes, hipMemcpyDeviceToHost, w->stream));
    if (zeroInput) HIP_TRY(hipMemcpyAsync(in, w->dbgScanIn.p, bytes, hipMemcpyDeviceToHost, w->stream));
    HIP_TRY(hipStreamSynchronize(w->stream));
    return MI_OK;
}
MI_API int mi_world_get_solver_kind(mi_world* w, uint32_t* out) {
    if (!w || !out) return fail(MI_ERR_INVALID_ARGUMENT, "null");
    *out = w->usedFused ? 3u : w->usedPersist ? (w->usedXcdSingle ? 5u : w->usedXcd ? 4u : 2u) : w->usedFlow ? 1u : 0u;
    return MI_OK;
}
// Host-side evaluation of the tile -> XCD assignment the XCD-partitioned solver uses on the device (tests: the per-XCD shares of
// a bin must add up, and (owner, rank) must enumerate every tile of a bin exactly once).  out = { owner, rank inside the owner's share, share of `query_xcd` }.
MI_API int mi_debug_tile_owner(uint32_t tile_in_bin, uint32_t tiles_in_bin, uint32_t bin, uint32_t query_xcd, uint32_t* out) {
    if (!out || tile_in_bin >= tiles_in_bin || query_xcd >= 8u) return fail(MI_ERR_INVALID_ARGUMENT, "tile_in_bin < tiles_in_bin, query_xcd < 8");
    out[0] = tileOwner(tile_in_bin, tiles_in_bin, bin); out[1] = tileOwnerRank(tile_in_bin, tiles_in_bin, bin); out[2] = tileOwnerCount(query_xcd, tiles_in_bin, bin);
    return MI_OK;
}
// Event pairs around every stage cost a few microseconds of device time per step each: NOTHING is timed by default (level 0: the stage times read 0, the
// accumulated step and contact-update counts still count every valid step); level 2 = the whole step and the solve stage, level 3 = the solve stage alone, level 1 = every stage.
MI_API int mi_world_set_stage_timing(mi_world* w, uint32_t level) {
    if (!w || level > 3u) return fail(MI_ERR_INVALID_ARGUMENT, "level: 0 off, 1 every stage, 2 the whole step and the solve stage, 3 the solve stage alone");
    w->timingLevel = level; return MI_OK;
}
MI_API int mi_world_get_stage_times(mi_world* w, mi_stage_times* out) { if (!w || !out) return fail(MI_ERR_INVALID_ARGUMENT, "null"); w->finishTimes(); *out = w->times; return MI_OK; }

MI_API int mi_world_get_contacts(mi_world* w, mi_contact* out, uint32_t cap, uint32_t* count) {
    if (!w || !count) return fail(MI_ERR_INVALID_ARGUMENT, "null");
    uint32_t nm = w->manifoldsLast, nc = w->counts.num_contacts;
    *count = nc;
    if (!out) return MI_OK;
    if (cap < nc) return fail(MI_ERR_CAPACITY, "capacity < num contacts");
    if (!nm) return MI_OK;
    uint32_t np = w->hs.numPairs;
    std::vector<uint32_t> mp(nm); std::vector<uint2> mb(nm), mi_(nm); std::vector<uint64_t> keys(np); std::vector<float4> nrm(np), pts(4 * (size_t)np);
    HIP_TRY(hipMemcpy(mp.data(), w->manPair.p, nm * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(mb.data(), w->manBodies.p, nm * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(mi_.data(), w->manInfo.p, nm * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(keys.data(), w->pairsIn, np * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(nrm.data(), w->npNormal.p, np * 16, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(pts.data(), w->npPoints.p, 4 * (size_t)np * 16, hipMemcpyDeviceToHost));
    // device manifolds are stored in arrival order; report them in ascending (bucket, colliderA, colliderB) key order
    std::vector<uint32_t> ord(nm);
    for (uint32_t m = 0; m < nm; ++m) ord[m] = m;
    std::sort(ord.begin(), ord.end(), [&](uint32_t x, uint32_t y) { return keys[mp[x]] < keys[mp[y]]; });
    uint32_t ci = 0;
    for (uint32_t mo = 0; mo < nm; ++mo) {
        uint32_t m = ord[mo];
        uint32_t p = mp[m], cnt = mi_[m].x & 7u;
        const bool terrain = (mi_[m].x >> 31) != 0u;   // contact k and its own normal in pair record p + k
        for (uint32_t k = 0; k < cnt && ci < nc; ++k, ++ci) {
            mi_contact& o = out[ci];
            float4 pd = terrain ? pts[4 * ((size_t)p + k)] : pts[4 * (size_t)p + k];
            const float4 nk = terrain ? nrm[p + k] : nrm[p];
            o.point[0] = pd.x; o.point[1] = pd.y; o.point[2] = pd.z; o.penetration_depth = pd.w;
            o.normal[0] = nk.x; o.normal[1] = nk.y; o.normal[2] = nk.z;
            o.friction_restitution = mi_[m].y;
            o.collider_a = (uint32_t)((keys[p] >> 29) & 0x1FFFFFFFu); o.collider_b = (uint32_t)(keys[p] & 0x1FFFFFFFu);
            if (o.collider_b >= kHeightmapVirtualBase) o.collider_b = 0xFFFFFFFFu;   // terrain contact
            o.body_a = mb[m].x; o.body_b = mb[m].y;
        }
    }
    return MI_OK;
}

// ---- ghost-region exchange (multi-GPU sharding)
MI_API int mi_world_entities_to_bodies(mi_world* w, uint32_t n, const uint32_t* ents, uint32_t* out) {
    if (!w || (n && (!ents || !out))) return fail(MI_ERR_INVALID_ARGUMENT, "null");
    for (uint32_t i = 0; i < n; ++i) {
        if (ents[i] >= w->entities.size() || w->entities[ents[i]].rb < 0) return fail(MI_ERR_INVALID_ARGUMENT, "not a rigid body");
        out[i] = (uint32_t)w->entities[ents[i]].rb;
    }
    return MI_OK;
}
static int statesDevice(mi_world* w, uint32_t n, const uint32_t* idsDev, float* outDev, const float* inDev, bool sync) {
    if (!w || (n && (!idsDev || (!outDev && !inDev)))) return fail(MI_ERR_INVALID_ARGUMENT, "null");
    int rc = ensureUploaded(w); if (rc != MI_OK) return rc;
    if (n && outDev) k_gather_states<<<divUp(n, 256), 256, 0, w->stream>>>(n, idsDev, w->bPos.p, w->bRot.p, w->bLinVel.p, w->bAngVel.p, outDev);
    if (n && inDev) { w->ahead.stale = true; ++w->poseEpoch;   // (what ran ahead of the next step read the poses this call replaces)
                      k_scatter_states<<<divUp(n, 256), 256, 0, w->stream>>>(n, idsDev, inDev, w->bPos.p, w->bRot.p, w->bLinVel.p, w->bAngVel.p, w->shard.enabled ? w->shard.known.p : nullptr); w->hostStale = true; w->shard.prevValid = false; w->shard.rearmFullSize(); w->pose.valid = false; }   // (pose rows produced before this write are stale)
    if (sync) HIP_TRY(hipStreamSynchronize(w->stream));
    return MI_OK;
}
MI_API int mi_world_get_body_states_device(mi_world* w, uint32_t n, const uint32_t* idsDev, float* outDev) { return statesDevice(w, n, idsDev, outDev, nullptr, true); }
MI_API int mi_world_set_body_states_device(mi_world* w, uint32_t n, const uint32_t* idsDev, const float* inDev) { return statesDevice(w, n, idsDev, nullptr, inDev, true); }
// The same without a host synchronisation: the copy kernels are only ENQUEUED on the world's stream (mi_world_get_stream).  A
// caller that runs its collective on that stream (e.g. torch.cuda.ExternalStream + RCCL) gets gather -> exchange -> scatter ->
// next step ordered on the device with no host round trip in between.
MI_API int mi_world_get_body_states_device_async(mi_world* w, uint32_t n, const uint32_t* idsDev, float* outDev) { return statesDevice(w, n, idsDev, outDev, nullptr, false); }
MI_API int mi_world_set_body_states_device_async(mi_world* w, uint32_t n, const uint32_t* idsDev, const float* inDev) { return statesDevice(w, n, idsDev, nullptr, inDev, false); }
// mi_world_set_body_states_device_async with the choice of rows left to the device: the same bookkeeping (the call may write any of the rows)
MI_API int mi_world_set_body_states_masked_device_async(mi_world* w, uint32_t n, const uint32_t* idsDev, const float* inDev, const uint32_t* maskDev, uint32_t group) {
    if (!w || (n && (!idsDev || !inDev || !maskDev)) || !group) return fail(MI_ERR_INVALID_ARGUMENT, "null argument, or group = 0");
    if (w->shard.enabled) return fail(MI_ERR_UNSUPPORTED, "mi_world_set_body_states_masked_device_async: not on a sharded world");
    int rc = ensureUploaded(w); if (rc != MI_OK) return rc;
    if (!n) return MI_OK;
    w->ahead.stale = true; ++w->poseEpoch;
    k_scatter_states_masked<<<divUp(n, 256), 256, 0, w->stream>>>(n, idsDev, inDev, maskDev, group, (uint32_t)w->bodies.size(), w->bPos.p, w->bRot.p, w->bLinVel.p, w->bAngVel.p);
    HIP_TRY(hipGetLastError());
    w->hostStale = true; w->shard.prevValid = false; w->shard.rearmFullSize(); w->pose.valid = false;
    return MI_OK;
}
// The rows of mi_world_get_transforms / mi_world_get_physics_transforms / mi_world_get_velocities in the caller's DEVICE buffers: k_entity_poses, which the
// pinned pose stream uses too, launched straight into them.  The pose stream itself (its rows, `valid`, `wanted`, the host sets) is not touched; only the
// entity -> body table is shared.
MI_API int mi_world_get_transforms_device_async(mi_world* w, uint32_t physics, float* posDev, float* rotDev, float* linDev, float* angDev) {
    if (!w) return fail(MI_ERR_INVALID_ARGUMENT, "null");
    if ((reinterpret_cast<uintptr_t>(rotDev) & 15u) != 0u) return fail(MI_ERR_INVALID_ARGUMENT, "rotations4_dev must be 16-byte aligned");
    if (w->shard.enabled) return fail(MI_ERR_UNSUPPORTED, "mi_world_get_transforms_device_async: not on a sharded world");
    int rc = ensureUploaded(w); if (rc != MI_OK) return rc;
    const uint32_t n = (uint32_t)w->entities.size(), nb = (uint32_t)w->bodies.size();
    if (!n || !nb || (!posDev && !rotDev && !linDev && !angDev)) return MI_OK;
    rc = w->posesEnsureTables(); if (rc != MI_OK) return rc;
    const bool follow = physics != 0u || w->transformsFollowPhysics, lerpNow = !follow && w->lerpPending;
    const float4 *pos = w->bPos.p, *rot = w->bRot.p; float t = -1.f;
    if (w->hostStale && (follow || (lerpNow && w->p0OnDevice))) { if (!follow) t = w->lerpT; }
    else {   // the host holds the transforms (nothing stepped since the last download, or physics_transform0 lives there): exactly what the host calls would do, then up in body order
        rc = w->download(); if (rc != MI_OK) return rc;
        std::vector<float4> hp(nb), hr(nb);
        for (uint32_t b = 0; b < nb; ++b) {
            const HBody& hb = w->bodies[b]; const HEntity& e = w->entities[hb.entity];
            const V3 p = physics ? hb.p1 : e.pos; const Q4 q = physics ? hb.r1 : e.rot;
            hp[b] = make_float4(p.x, p.y, p.z, 0.f); hr[b] = make_float4(q.x, q.y, q.z, q.w);
        }
        HIP_TRY(w->poseStagePos.ensure(nb)); HIP_TRY(w->poseStageRot.ensure(nb));
        HIP_TRY(hipMemcpyAsync(w->poseStagePos.p, hp.data(), (size_t)nb * 16, hipMemcpyHostToDevice, w->stream));
        HIP_TRY(hipMemcpyAsync(w->poseStageRot.p, hr.data(), (size_t)nb * 16, hipMemcpyHostToDevice, w->stream));
        HIP_TRY(hipStreamSynchronize(w->stream));   // (hp / hr are locals)
        pos = w->poseStagePos.p; rot = w->poseStageRot.p;
    }
    // k_entity_poses writes positions AND rotations, and the velocities when both of their rows are given: a missing row goes to a scratch row of the library
    float *oP = posDev, *oR = rotDev, *oL = linDev, *oA = angDev;
    const bool vel = linDev || angDev;
    if (!oP || !oR || (vel && (!oL || !oA))) {
        HIP_TRY(w->poseScratch.ensure(4u * (size_t)n));
        if (!oP) oP = w->poseScratch.p; if (!oR) oR = w->poseScratch.p; if (vel && !oL) oL = w->poseScratch.p; if (vel && !oA) oA = w->poseScratch.p;
    }
    hipLaunchKernelGGL(k_entity_poses, dim3(divUp(n, 256u)), dim3(256), 0, w->stream, n, w->pose.entBody.p, pos, rot, w->bPos0.p, w->bRot0.p, t, oP, oR,
                       w->bLinVel.p, w->bAngVel.p, vel ? oL : nullptr, vel ? oA : nullptr);
    HIP_TRY(hipGetLastError());
    return MI_OK;
}
MI_API int mi_world_get_stream(mi_world* w, void** out) {
    if (!w || !out) return fail(MI_ERR_INVALID_ARGUMENT, "null");
    *out = (void*)w->stream;
    return MI_OK;
}
static int statesHost(mi_world* w, uint32_t n, const uint32_t* ents, float* out, const float* in) {
    if (!w || (n && !ents)) return fail(MI_ERR_INVALID_ARGUMENT, "null");
    if (!n) return MI_OK;
    std::vector<uint32_t> ids(n);
    int rc = mi_world_entities_to_bodies(w, n, ents, ids.data()); if (rc != MI_OK) return rc;
    rc = ensureUploaded(w); if (rc != MI_OK) return rc;
    DBuf<uint32_t> dIds; DBuf<float> dSt;
    HIP_TRY(dIds.ensure(n)); HIP_TRY(dSt.ensure(13 * (size_t)n));
    HIP_TRY(hipMemcpy(dIds.p, ids.data(), n * 4, hipMemcpyHostToDevice));
    if (in) {
        HIP_TRY(hipMemcpy(dSt.p, in, 13 * (size_t)n * 4, hipMemcpyHostToDevice));
        return mi_world_set_body_states_device(w, n, dIds.p, dSt.p);
    }
    rc = mi_world_get_body_states_device(w, n, dIds.p, dSt.p); if (rc != MI_OK) return rc;
    HIP_TRY(hipMemcpy(out, dSt.p, 13 * (size_t)n * 4, hipMemcpyDeviceToHost));
    return MI_OK;
}
MI_API int mi_world_get_body_states(mi_world* w, uint32_t n, const uint32_t* ents, float* out) { return statesHost(w, n, ents, out, nullptr); }
MI_API int mi_world_set_body_states(mi_world* w, uint32_t n, const uint32_t* ents, const float* in) { return statesHost(w, n, ents, nullptr, in); }

// Stage dumps for parity bisecting.
MI_API int mi_world_get_aabbs(mi_world* w, float* out6, uint32_t cap) {
    if (!w || !out6) return fail(MI_ERR_INVALID_ARGUMENT, "null");
    uint32_t nc = w->counts.num_colliders;
    if (cap < nc) return fail(MI_ERR_CAPACITY, "capacity < num colliders");
    std::vector<float4> mn(nc), mx(nc);
    if (nc) { HIP_TRY(hipMemcpy(mn.data(), w->aabbMin.p, nc * 16, hipMemcpyDeviceToHost)); HIP_TRY(hipMemcpy(mx.data(), w->aabbMax.p, nc * 16, hipMemcpyDeviceToHost)); }
    for (uint32_t i = 0; i < nc; ++i) { out6[6 * i] = mn[i].x; out6[6 * i + 1] = mn[i].y; out6[6 * i + 2] = mn[i].z; out6[6 * i + 3] = mx[i].x; out6[6 * i + 4] = mx[i].y; out6[6 * i + 5] = mx[i].z; }
    return MI_OK;
}
MI_API int mi_world_get_manifold_colors(mi_world* w, uint32_t* out, uint32_t cap) {
    if (!w || !out) return fail(MI_ERR_INVALID_ARGUMENT, "null");
    uint32_t nm = w->manifoldsLast;
    if (cap < nm) return fail(MI_ERR_CAPACITY, "capacity < num manifolds");
    if (!nm) return MI_OK;
    // same manifold order as mi_world_get_contacts: ascending (bucket, colliderA, colliderB)
    uint32_t np = w->hs.numPairs;
    std::vector<uint32_t> col(nm), mp(nm), ord(nm); std::vector<uint64_t> keys(np);
    HIP_TRY(hipMemcpy(col.data(), w->color.p, nm * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(mp.data(), w->manPair.p, nm * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(keys.data(), w->pairsIn, np * 8, hipMemcpyDeviceToHost));
    for (uint32_t m = 0; m < nm; ++m) ord[m] = m;
    std::sort(ord.begin(), ord.end(), [&](uint32_t x, uint32_t y) { return keys[mp[x]] < keys[mp[y]]; });
    for (uint32_t m = 0; m < nm; ++m) out[m] = col[ord[m]];
    return MI_OK;
}

}  // extern "C"
