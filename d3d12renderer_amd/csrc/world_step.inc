// Part of world.hip (one translation unit; #included there, in this order): one internal step: enqueue, read-back, validation, fallback ladder; poses for the caller.

// ------------------------------------------------------------------------------------------------
// One internal step (physicsStepInternal, src/physics/physics.cpp:1180-1362)
// ------------------------------------------------------------------------------------------------
// what a step expects to find cleared when it starts (by every thread of ONE workgroup of nt threads)
__device__ __forceinline__ void resetStepState(uint32_t t, uint32_t nt, StepScalars* sc, Shards* sh, uint32_t* roundFlags, uint32_t* keyCount) {
    for (uint32_t i = t; i < kSpatialKeys; i += nt) keyCount[i] = 0u;
    for (uint32_t i = t; i < sizeof(Shards) / 4u; i += nt) reinterpret_cast<uint32_t*>(sh)[i] = 0u;
    for (uint32_t i = t; i < kRoundFlagWords; i += nt) roundFlags[i] = 0u;
    if (t == 0) {
        sc->numDead = 0; sc->shardOwned[0] = sc->shardOwned[1] = sc->shardOwned[2] = 0;
        for (int q = 0; q < 8; ++q) sc->shardSent[q] = 0;
        sc->seamStats[0] = sc->seamStats[1] = sc->seamStats[2] = 0;
        sc->extentSum = 0.0; sc->largeThreshold = 0.f; sc->numLarge = 0; sc->numPairs = 0; sc->numOverlaps = 0; sc->numManifolds = 0; sc->numContacts = 0; sc->solveError = 0;
        sc->tailRounds = 0; sc->specOverflow = 0; sc->totalTiles = 0; sc->totalCt = 0; sc->colorPending = 0; sc->partitioned = 0; sc->gjkLo = 0; sc->gjkHi = 0; sc->numCells = 0; sc->numPairsFound = 0; sc->numEvents = 0; sc->numInterPairs = 0; sc->numInteractions = 0; sc->numHmContacts = 0; sc->numHmColliders = 0; sc->numHmManifolds = 0; sc->numEpa = 0;
        for (int q = 0; q < 8; ++q) { sc->xcdCount[q] = 0; sc->xccOf[q] = 0xFFFFFFFFu; }
        for (int a = 0; a < 3; ++a) { sc->boundsMin[a] = 0x7FFFFFFF; sc->boundsMax[a] = (int)0x80000000; }
    }
    if (t < 24) { sc->bucketHist[t] = 0; sc->bucketCursor[t] = 0; }
}
__global__ void k_reset_scalars(StepScalars* sc, Shards* sh, uint32_t* roundFlags, uint32_t* keyCount) { resetStepState(threadIdx.x, blockDim.x, sc, sh, roundFlags, keyCount); }
// End-of-step read-back without a copy engine round trip and without a driver wake-up: one workgroup writes the scalars and the
// colouring round flags straight into pinned host memory, fences at system scope and then publishes the step's sequence number,
// which the host thread spins on.
// `resetSc` (non-null): the same workgroup then clears what the NEXT step expects cleared (k_reset_scalars' work): that launch — 4 us at the very start of a step, plus the
// gap until the host has the second launch out — disappears from the step (the host reads the pinned copy, never these device words again).
__global__ __launch_bounds__(256) void k_publish_readback(const uint32_t* __restrict__ src, uint32_t words, uint32_t* dstHost, uint32_t seqWord, uint32_t* seqDev,
                                                          StepScalars* resetSc, Shards* resetSh, uint32_t* resetFlags, uint32_t* resetKeys) {
    for (uint32_t i = threadIdx.x; i < words; i += blockDim.x) dstHost[i] = src[i];
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t seq = *seqDev + 1u; if (seq == 0u) seq = 1u;   // never 0 (the host counts the same way)
        *seqDev = seq;
        __hip_atomic_store(dstHost + seqWord, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    if (resetSc) resetStepState(threadIdx.x, blockDim.x, resetSc, resetSh, resetFlags, resetKeys);   // (every word was copied out before the barrier above)
}
__global__ void k_reset_pair_counters(StepScalars* sc, Shards* sh) {
    uint32_t t = threadIdx.x;
    if (t == 0) { sc->numPairs = 0; sc->numOverlaps = 0; sc->numInterPairs = 0; }
    if (t < 24) sc->bucketHist[t] = 0;
    for (uint32_t k = 0; k < kShards; ++k) { if (t == 0) sh->c[k].numOverlaps = 0; if (t < 24) sh->c[k].bucketHist[t] = 0; }   // the pair pass's counters only (owned[] of a sharded world stays)
}

// One internal step.  Two ways to run it:
//   * synchronous: the host reads the pair count, the manifold count and the schedule back as they appear and sizes
//     every buffer and launch exactly (first step, after a topology change, per-colour solver path, or as the retry);
//   * speculative (default for every later step): no read-back until the very end.  Every kernel takes its sizes from
//     StepScalars on the device; the host only needs UPPER BOUNDS for launch grids, scan lengths and capacities, and
//     takes them from the previous step's counts (+12.5 %).  The end-of-step read-back validates the bounds (and that
//     the colouring converged, no overflow colour appeared, ...).  Nothing persistent is modified before
//     k_integrate_velocities, which writes into the second body-state buffer set, so an invalid speculation is simply
//     re-run synchronously from the untouched state.  This removes ~0.35 ms of idle GPU time per step at 262144 bodies.
enum { STEP_RETRY = 1 };

int mi_world::stepInternal(const mi_step_settings& settings, float dt) {
    HIP_TRY(hipSetDevice(device));
    ++poseEpoch;
    if (topologyDirty) { int rc = download(); if (rc != MI_OK) return rc; rc = upload(); if (rc != MI_OK) return rc; haveEstimates = false; }
    else if (joints.podsDirty()) { int rc = joints.uploadPods(stream); if (rc != MI_OK) return rc; HIP_TRY(hipStreamSynchronize(stream)); }
    if (bodies.empty()) return cloths.empty() ? MI_OK : stepCloths(dt);   // physics.cpp:1184-1189: cloth alone still steps
    if (shard.stepOpen) shard.prevValid = false;   // the previous step ended in an error: what its kernels left behind is not what the flags describe
    shard.stepOpen = true;
    if (debugOrderPending && (heightmap || shard.enabled)) { debugOrderPending = false; debugOrder.clear(); shard.stepOpen = false; return fail(MI_ERR_UNSUPPORTED, "mi_debug_set_solve_order: not with heightmap terrain or sharding"); }   // (terrain / sharding came after the order was set: the order is dropped, later steps run)
    const bool exactSeam = shard.enabled && shard.exact;   // every rank must take the same path through the step (its sweeps end in an exchange): no speculation
    shard.sweepsDone = 0;
    const bool spec = specEnabled && haveEstimates && flowSolver && !launchFallbackSteps && !debugOrderPending && !exactSeam && (!usesInteractions || last.numInteractions <= 32768u);   // (triggers / force fields: ordered and applied on the device while there are at most 32 k interactions)
    ++totalSteps; if (spec) ++specSteps;
    int rc = runStep(settings, dt, spec);
    // a step that asks to be re-run has written nothing persistent; each re-run is synchronous and one rung further down the ladder
    // speculative -> exact sizes -> unpartitioned -> dispatch-ordered dataflow kernel -> one launch per colour
    for (int attempt = 0; rc == STEP_RETRY && attempt < 6; ++attempt) {
        if (poseArm.done) { poseArm.done = false; pose.valid = false; pose.retrySameStep = true; --pose.produced_ahead; }
        if (exactSeam && shard.sweepsDone) return fail(MI_ERR_DEVICE, "exact seam: the step would have to be re-run after sweeps were already exchanged with the neighbours");
        ++specRetries; rc = runStep(settings, dt, false);
    }
    if (rc == STEP_RETRY) return fail(MI_ERR_DEVICE, "step could not be completed on any solver path");
    if (rc == MI_OK && launchFallbackSteps) --launchFallbackSteps;
    debugOrderDepthLast = debugOrderPending && debugOrderLevelled ? debugOrderDepth : 0u;
    debugOrderPending = false; debugOrder.clear(); debugOrderLevelled = false;   // (one step only, whatever became of it)
    if (rc == MI_OK && shard.enabled) rc = shardExchange();
    if (rc == MI_OK && !cloths.empty()) rc = stepCloths(dt);   // after the rigid bodies (physics.cpp:1352-1358); once per VALID step: cloth state is updated in place
    return rc;
}

// cloth_component::applyWindForce(globalForceField) + simulate(...) for every cloth: one launch, one workgroup per cloth.
int mi_world::stepCloths(float dt) {
    for (HCloth* c : cloths) {
        if (c->desc.total_mass != c->oldTotalMass || c->desc.stiffness != c->oldStiffness) {   // recalculateProperties (cloth.cpp:299-317)
            const uint32_t n = c->desc.grid_size_x * c->desc.grid_size_y;
            const float invMassPerParticle = (float)n / c->desc.total_mass;
            for (float& im : c->invMasses) im = (im != 0.f) ? invMassPerParticle : 0.f;
            c->desc.stiffness = clampr(c->desc.stiffness, 0.01f, 1.f);
            const float invStiffness = 1.f / c->desc.stiffness;
            for (size_t k = 0; k < c->pairs.size(); ++k) c->restInvMass[k].y = (c->invMasses[c->pairs[k].x] + c->invMasses[c->pairs[k].y]) * invStiffness;
            c->oldTotalMass = c->desc.total_mass; c->oldStiffness = c->desc.stiffness;
            c->constraintsDirty = true;
            // the inverse masses ride in pos.w
            std::vector<float4> p(n);
            HIP_TRY(hipMemcpyAsync(p.data(), c->pos.p, n * sizeof(float4), hipMemcpyDeviceToHost, stream)); HIP_TRY(hipStreamSynchronize(stream));
            for (uint32_t i = 0; i < n; ++i) p[i].w = c->invMasses[i];
            HIP_TRY(hipMemcpyAsync(c->pos.p, p.data(), n * sizeof(float4), hipMemcpyHostToDevice, stream)); HIP_TRY(hipStreamSynchronize(stream));
        }
        if (c->constraintsDirty) {
            HIP_TRY(hipMemcpyAsync(c->dRestInvMass.p, c->restInvMass.data(), c->restInvMass.size() * sizeof(float2), hipMemcpyHostToDevice, stream));
            HIP_TRY(hipStreamSynchronize(stream));
            c->constraintsDirty = false; clothsDirty = true;
        }
    }
    if (clothsDirty) {
        std::vector<ClothDev> d(cloths.size());
        for (size_t i = 0; i < cloths.size(); ++i) {
            HCloth& c = *cloths[i];
            ClothDev& o = d[i];
            o.pos = c.pos.p; o.prev = c.prev.p; o.vel = c.vel.p; o.force = c.force.p; o.pairs = c.dPairs.p; o.restInvMass = c.dRestInvMass.p; o.temp = c.temp.p; o.order = c.dOrder.p;
            std::memcpy(o.colourOffsets, c.colourOffsets, sizeof(o.colourOffsets));
            o.gridX = c.desc.grid_size_x; o.gridY = c.desc.grid_size_y; o.numConstraints = (uint32_t)c.pairs.size();
            o.gravityFactor = c.desc.gravity_factor; o.damping = c.desc.damping;
        }
        HIP_TRY(clothDescs.ensure(d.size()));
        HIP_TRY(hipMemcpyAsync(clothDescs.p, d.data(), d.size() * sizeof(ClothDev), hipMemcpyHostToDevice, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        clothsDirty = false;
    }
    k_cloth_step<<<(uint32_t)cloths.size(), 256, 0, stream>>>(clothDescs.p, make_float3(globalForce.x, globalForce.y, globalForce.z), dt, clothIterations[0], clothIterations[1], clothIterations[2]);
    HIP_TRY(hipGetLastError());
    return MI_OK;
}

// handleNonCollisionInteractions (physics.cpp:952-1039) for the AABB overlaps the pair pass collected between rigid-body colliders
// and trigger / force-field colliders.  Synchronous: the (few) interactions come back to the host, which puts them into the
// canonical order (body, other collider, body collider); localized force fields then add up per body on the device in that
// order, trigger overlaps are de-duplicated per (trigger entity, body entity) and diffed against the previous step.
int mi_world::interactions(std::vector<mi_event>& out) {
    const uint32_t nb = (uint32_t)bodies.size();
    hipStream_t st = stream;
    HIP_TRY(hipMemcpyAsync(bForceStep.p, bForce.p, (size_t)nb * sizeof(float4), hipMemcpyDeviceToDevice, st));
    std::vector<DeviceInteraction> list;
    if (hs.numInterPairs) {
        HIP_TRY(interList.ensure(hs.numInterPairs));
        HullSet hset{hullVerts.p, hullRanges.p};
        k_overlap<<<divUp(hs.numInterPairs, 64), 64, 0, st>>>(scalarsPtr(), hs.numInterPairs, interKeys.p, wShape.p, aabbMin.p, aabbMax.p, hset, interList.p);
        HIP_TRY(hipMemcpyAsync(&hs, scalarsPtr(), sizeof(StepScalars), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        list.resize(hs.numInteractions);
        if (!list.empty()) {
            HIP_TRY(hipMemcpyAsync(list.data(), interList.p, list.size() * sizeof(DeviceInteraction), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
        }
        std::sort(list.begin(), list.end(), [](const DeviceInteraction& x, const DeviceInteraction& y) {
            if (x.body != y.body) return x.body < y.body;
            if (x.otherCollider != y.otherCollider) return x.otherCollider < y.otherCollider;
            return x.rbCollider < y.rbCollider;
        });
    }
    std::vector<uint2> fields;
    for (const DeviceInteraction& in : list) if ((in.other >> 28) == OBJ_FORCE_FIELD) fields.push_back(make_uint2(in.body, in.other & 0x0FFFFFFFu));
    if (!fields.empty()) {
        HIP_TRY(fieldList.ensure(fields.size()));
        HIP_TRY(hipMemcpyAsync(fieldList.p, fields.data(), fields.size() * sizeof(uint2), hipMemcpyHostToDevice, st));
        k_apply_fields<<<divUp((uint32_t)fields.size(), 256), 256, 0, st>>>((uint32_t)fields.size(), fieldList.p, localForce.p, bForceStep.p);
        HIP_TRY(hipStreamSynchronize(st));   // `fields` is pageable host memory
    }
    return triggerEventsFrom(list, out);
}
int mi_world::triggerEventsFrom(const std::vector<DeviceInteraction>& list, std::vector<mi_event>& out) {
    nextTriggerOverlaps.clear();
    for (const DeviceInteraction& in : list) {
        const uint32_t type = in.other >> 28, index = in.other & 0x0FFFFFFFu;
        if (type == OBJ_TRIGGER) nextTriggerOverlaps.push_back(((uint64_t)triggerEntities[index] << 32) | (uint64_t)bodies[in.body].entity);
    }
    std::sort(nextTriggerOverlaps.begin(), nextTriggerOverlaps.end());
    nextTriggerOverlaps.erase(std::unique(nextTriggerOverlaps.begin(), nextTriggerOverlaps.end()), nextTriggerOverlaps.end());
    if (!eventsEnabled) { nextTriggerOverlaps.clear(); return MI_OK; }
    auto emit = [&](uint64_t key, uint32_t type) {
        mi_event e{}; e.type = type; e.entity_a = (uint32_t)(key >> 32); e.entity_b = (uint32_t)key; e.collider_a = e.collider_b = 0xFFFFFFFFu;
        out.push_back(e);
    };
    const std::vector<uint64_t>& prev = prevTriggerOverlaps;
    size_t p = 0, t = 0;
    while (p < prev.size() && t < nextTriggerOverlaps.size()) {
        uint64_t pk = prev[p], tk = nextTriggerOverlaps[t];
        if (pk == tk) { ++p; ++t; }
        else if (pk < tk) { emit(pk, MI_EVENT_TRIGGER_LEAVE); ++p; }
        else { emit(tk, MI_EVENT_TRIGGER_ENTER); ++t; }
    }
    while (p < prev.size()) emit(prev[p++], MI_EVENT_TRIGGER_LEAVE);
    while (t < nextTriggerOverlaps.size()) emit(nextTriggerOverlaps[t++], MI_EVENT_TRIGGER_ENTER);
    return MI_OK;
}
// Speculative form: k_overlap over the bound of the candidate pairs, canonical order by a device rank sort, force fields applied from the
// sorted list — nothing comes back to the host inside the step; the trigger overlaps are taken from the sorted list after the read-back.
int mi_world::interactionsDevice(uint32_t interPairBound) {
    const uint32_t nb = (uint32_t)bodies.size();
    hipStream_t st = stream;
    HIP_TRY(L.memcpyAsync(bForceStep.p, bForce.p, (size_t)nb * sizeof(float4), hipMemcpyDeviceToDevice, st));
    if (!interPairBound) return MI_OK;
    const uint32_t cap = (uint32_t)interList.cap;
    HullSet hset{hullVerts.p, hullRanges.p};
    L.launch(k_overlap, dim3(divUp(interPairBound, 64)), dim3(64), 0, st, scalarsPtr(), cap, interKeys.p, wShape.p, aabbMin.p, aabbMax.p, hset, interList.p);
    L.launch(k_inter_sort, dim3(divUp(cap, 256)), dim3(256), 0, st, scalarsPtr(), cap, interList.p, interSorted.p);
    L.launch(k_apply_fields_sorted, dim3(divUp(cap, 256)), dim3(256), 0, st, scalarsPtr(), cap, interSorted.p, localForce.p, bForceStep.p);
    return MI_OK;
}

// The nine event slots of a step (ev[]): the boundaries of mi_stage_times' stages, in the order they are passed.
enum StepEvent { EV_STEP_BEGIN, EV_PREPARED, EV_BROAD, EV_NARROW, EV_FORCES, EV_SCHEDULE, EV_SOLVE_BEGIN, EV_SOLVE_END, EV_STEP_END };
static bool isStepEnd(int id) { return id == EV_STEP_BEGIN || id == EV_STEP_END; }
static bool isSolveEnd(int id) { return id == EV_SOLVE_BEGIN || id == EV_SOLVE_END; }
// Passes over enqueueStep (launcher.hpp): a speculative step of a small scene first runs it DRY (signature only); a known
// signature is replayed from its captured graph, one seen in the previous step as well is captured now, anything else runs plainly.
enum StepPass { PASS_PLAIN, PASS_DRY, PASS_CAPTURE };

// What one attempt at a step (one runStep call) knows: decided by planStep once, or by an enqueue stage for the stages behind it (every pass runs every stage and
// finds the same values).  Plain data on runStep's stack.  No device pointer is kept here: buffers are (re)allocated on the way through a step, every launch reads x.p itself.
struct StepAttempt {
    mi_step_settings settings; float dt; bool spec; uint32_t nb, nc;
    // planStep
    bool graphStep, fuseResetStep, skipReset, useAhead;
    int pass; bool attached;   // attached: this pass's EV_STEP_BEGIN / SOLVE_BEGIN / SOLVE_END / STEP_END ride on kernel dispatches (a graph cannot hold that form, it gets recorded events)
    // stagePrepare
    bool blockSkip, seamOn, prepared;
    // stageBroad
    uint32_t pairBound;       // upper bound of this step's collision pairs that launches / scans are sized for
    bool skippedPartition, finishInNarrow;  // finishInNarrow: k_narrow derives the pair list's final counts itself (no k_pair_finish launch)
    GridParams* statsGridNext; uint32_t statsCellCap, statsBlocks;   // (speculative steps: pairFinishStats runs beside k_narrow_clip)
    // stageInteractions
    uint32_t interPairBound; std::vector<mi_event> triggerEvents;
    // stageForces
    bool keysWithForces;
    // stageSchedule
    uint32_t nmBound, conBound, tilesCap, ctCap, eventCap, xcdListCap;
    bool xcdSingle, xcdPlan;
    bool shardCounted;   // sharded world: this rank's manifolds / contacts are counted inside k_manifold_keys when that runs, else by k_shard_count
    // stageConstraintInit
    uint32_t tilesLaunch, persistMaxSlots; bool useFlow, fused, persistPlan; IslandPrivate islandPriv;
    // stageSolve
    bool solveAttached; uint64_t mainContacts;
};
static uint32_t specBound(uint32_t last, uint32_t slack) { return last + last / 8u + slack; }
// sharded world: the per-body / per-collider passes run a fixed number of workgroups that stride over the blocks of 256 and skip those with nothing simulated in them
static uint32_t bodyGrid(const StepAttempt& a, uint32_t blocks) { return a.blockSkip ? std::min(blocks, kShardGrid) : blocks; }

int mi_world::readScalars() { HIP_TRY(hipMemcpyAsync(&hs, scalarsPtr(), sizeof(StepScalars), hipMemcpyDeviceToHost, stream)); HIP_TRY(hipStreamSynchronize(stream)); return MI_OK; }
// The step (EV_STEP_BEGIN / EV_STEP_END) and the solve stage (EV_SOLVE_BEGIN / EV_SOLVE_END) are always timed.  A recorded event is a barrier packet of its own (~6 us of
// idle device per event: 24 us per step); where the stage is ONE kernel the events ride on that kernel's dispatch instead
// (Launcher::launchTimed: start / stop events): no packet, no gap.  `a.attached` = this pass's four are attached ones.
// Timing is opt-in (mi_world_set_stage_timing): even ATTACHED events are not free — the start / stop events riding on the solver's dispatch cost ~11 us of idle
// device per step (the kernels before / after wait for the signals), the step's two ~1.5 us: 12 us of a 1.0 ms step for numbers nobody asked for.
void mi_world::mark(const StepAttempt& a, int id) {
    if (knobs.debugSync && !L.dry) { std::fprintf(stderr, "[mi_physics] step %llu: waiting for the stage ending at mark %d\n", (unsigned long long)totalSteps, id); std::fflush(stderr);   // (a memory fault ends the process inside the wait: the last line names the stage)
        hipError_t e = hipStreamSynchronize(stream); if (e != hipSuccess) std::fprintf(stderr, "[mi_physics] step %llu (%s): stage ending at mark %d: %s\n", (unsigned long long)totalSteps, a.spec ? "speculative" : "synchronous", id, hipGetErrorString(e)); }
    if (!timingLevel) return;
    if (a.attached && (isStepEnd(id) || isSolveEnd(id))) return;
    if (!timesEnds(timingLevel) && isStepEnd(id)) return;   // level 3: the solve stage alone (the step's own start / stop events cost two more gaps)
    if (!timesStages(timingLevel) && !isStepEnd(id) && !isSolveEnd(id)) return;   // levels 2 and 3: no stage boundaries
    L.eventRecord(ev[id], stream);
}
// XCD partitioning pays once the pile is big enough to keep eight L2s busy; it needs the persistent kernel (no joints)
bool mi_world::xcdAble() const { return flowSolver && persistSolver && persistXcd && joints.count() == 0 && (persistWaves & 7u) == 0u && !debugOrderPending && !exactSeamStep(); }
// small piles: the 128 waves of ONE XCD run the whole solve, every body hand-over goes through that XCD's L2 (tileOwner(..., single))
bool mi_world::xcdSingleFor(uint32_t nm) const { return xcdAble() && persistXcdSingle && nm && nm < xcdMinManifolds && divUp(divUp(nm, 64) + kSchedBins + 8, persistWaves / 8u) <= 16u; }
bool mi_world::xcdPlanFor(uint32_t nm) const { return xcdAble() && (nm >= xcdMinManifolds || xcdSingleFor(nm)); }
// per-launch HIP events around the solver's launches (mi_world_step_profiled): a pair per launch, created as needed
int mi_world::profileBegin() {
    if (!profileSolve) return MI_OK;
    const size_t e = 2 * (size_t)profLaunches;
    while (profEvents.size() < e + 2) { hipEvent_t ev_; HIP_TRY(hipEventCreate(&ev_)); profEvents.push_back(ev_); }
    (void)hipEventRecord(profEvents[e], stream);
    return MI_OK;
}
void mi_world::profileEnd() { if (profileSolve) { (void)hipEventRecord(profEvents[2 * (size_t)profLaunches + 1], stream); ++profLaunches; } }

int mi_world::runStep(const mi_step_settings& settings, float dt, bool spec) {
    StepAttempt a{};
    a.settings = settings; a.dt = dt; a.spec = spec; a.nb = (uint32_t)bodies.size(); a.nc = (uint32_t)colliders.size();
    L.traceEach = knobs.debugSync; L.traceOrdinal = 0;   // development: find the stage a device fault comes from
    int rc = planStep(a); if (rc != MI_OK) return rc;
    for (bool again = true; again;) {
        rc = enqueueStep(a); if (rc != MI_OK) return rc;
        rc = submitPass(a, again); if (rc != MI_OK) return rc;
    }
    if (poseArm.armed) {   // the poses of the state this step is producing, enqueued behind it (a step that turns out void produces them again)
        ++pose.produced_ahead; poseArm.done = false;
        int rcp = posesProduce(poseArm.t, true, true); if (rcp != MI_OK) return rcp;
        poseArm.done = true;
    }
    rc = awaitReadback(); if (rc != MI_OK) return rc;
    rc = validateStep(a); if (rc != MI_OK) return rc;   // (STEP_RETRY among them)
    rc = collectEvents(a); if (rc != MI_OK) return rc;
    commitStep(a);
    return MI_OK;
}

// What is decided once per attempt, before any pass: whether the step goes through the graph passes, whether the reset rides in the publish kernel, and whether
// what ran ahead of this step is adopted.
int mi_world::planStep(StepAttempt& a) {
    const uint32_t nb = a.nb, nc = a.nc;
    const bool debugSync = knobs.debugSync;
    constexpr uint32_t kGraphMaxColliders = 32768;   // larger scenes are not launch-bound (MI_GRAPH=all replays them too)
    a.graphStep = a.spec && graphsEnabled && !profileSolve && !xcdFaultTest && !flowFaultTest && !debugSync && !launchFallbackSteps &&
                  (graphsForAll || nc <= kGraphMaxColliders) && readbackSeqDev.p;
    a.pass = a.graphStep ? PASS_DRY : PASS_PLAIN;
    // k_reset_scalars' work rides at the end of k_publish_readback (`scalarsClean`: the previous attempt's publish has done it): the step then starts with k_bp_prepare, whose 27 us
    // give the host time to get the next launches out — the 4 us launch and the ~8 us gap behind it are gone.  Not for worlds whose host side looks at the device words again after
    // the read-back (events: the "every collision ended" pass), nor where another kernel would have to carry the step's start event.  (A sharded world's exchange runs
    // behind the reset: k_shard_pack counts its records from zero, and nothing of the next step minds the counts it leaves.)
    a.fuseResetStep = knobs.fuseReset && spinReadback && readbackSeqDev.p && !eventsEnabled && !seamMode() && nc && gridValid && knobs.fuseWorld && !debugSync;
    a.skipReset = a.fuseResetStep && scalarsClean;
    scalarsClean = false;
    // step-ahead (world.hip): the previous speculative step has already run this step's k_bp_prepare on the state it produced.  Adopted only if this step would launch exactly that
    // kernel on exactly those inputs; otherwise what it counted is cleared (cell histogram here, the scalars / counter shards by k_reset_scalars) and the step starts as usual.
    const bool aheadFits = ahead.pending && !ahead.stale && a.spec && a.pass == PASS_PLAIN && a.skipReset && !shard.enabled && nc && gridValid && knobs.fuseWorld && !heightmap && !usesInteractions &&
                           ahead.nc == nc && ahead.nb == nb && ahead.gridIdx == gridCur && ahead.axis == sapAxis && ahead.pos == bPos.p && ahead.rot == bRot.p && ahead.shape == cShape.p &&
                           !timesEnds(timingLevel) && !debugSync && !debugOrderPending;
    if (ahead.pending && !aheadFits) {
        a.skipReset = false;
        if (cellCount.p) HIP_TRY(hipMemsetAsync(cellCount.p, 0, cellCount.cap * sizeof(uint32_t), stream));   // (16 MB; this path is rare: an outside write, a void step, another step mode)
    }
    a.useAhead = ahead.pending && aheadFits;
    ahead.pending = false; ahead.stale = false;
    if (a.useAhead) { wShape.swap(wShapeAlt); aabbMin.swap(aabbMinAlt); aabbMax.swap(aabbMaxAlt); ++aheadUsed; }
    return MI_OK;
}

// Everything a step puts on the stream, in stage order; every pass runs exactly this.
int mi_world::enqueueStep(StepAttempt& a) {
    L.trace = graphDebug;
    L.begin(a.pass == PASS_DRY, a.pass != PASS_PLAIN);
    a.attached = !knobs.debugSync && a.pass == PASS_PLAIN;
    mark(a, EV_STEP_BEGIN);
    int rc = stagePrepare(a); if (rc != MI_OK) return rc;
    mark(a, EV_PREPARED);
    rc = stageBroad(a); if (rc != MI_OK) return rc;
    if (a.pass == PASS_PLAIN) finishTimes();   // the previous step's event times, now that this step's first kernels keep the device busy
    mark(a, EV_BROAD);
    rc = stageNarrow(a); if (rc != MI_OK) return rc;
    rc = stageInteractions(a); if (rc != MI_OK) return rc;
    mark(a, EV_NARROW);
    rc = stageForces(a); if (rc != MI_OK) return rc;
    mark(a, EV_FORCES);
    rc = stageSchedule(a); if (rc != MI_OK) return rc;
    mark(a, EV_SCHEDULE);
    rc = stageConstraintInit(a); if (rc != MI_OK) return rc;
    mark(a, EV_SOLVE_BEGIN);
    rc = stageSolve(a); if (rc != MI_OK) return rc;
    mark(a, EV_SOLVE_END);
    if (a.attached && !a.solveAttached) (void)hipEventRecord(ev[EV_SOLVE_END], stream);
    rc = stageIntegrate(a); if (rc != MI_OK) return rc;
    mark(a, EV_STEP_END);
    return stagePublish(a);
}

// What becomes of the pass just enqueued.  A signature pass: replay the captured graph of that signature, or capture (signature seen within the last two steps), or
// run plainly; a capture pass: instantiate and launch.  `again`: enqueueStep is to run once more, as a.pass.
int mi_world::submitPass(StepAttempt& a, bool& again) {
    hipStream_t st = stream;
    again = false;
    auto plainAgain = [&]() { a.pass = PASS_PLAIN; again = true; };
    if (a.pass == PASS_DRY) {
        const uint64_t sig = L.h ^ ((uint64_t)L.ops << 48);
        StepGraph* hit = nullptr;
        for (StepGraph& g : stepGraphs) if (g.sig == sig && g.exec) { hit = &g; break; }
        if (graphDebug) {
            if (!hit && !graphPrevOps2.empty()) {   // compare with the step before the previous one (same buffer parity)
                size_t k = 0; while (k < graphPrevOps2.size() && k < L.opHashes.size() && graphPrevOps2[k] == L.opHashes[k]) ++k;
                std::fprintf(stderr, "[mi_physics] step %llu: graph signature differs from that of two steps ago at operation %zu of %zu (then %zu)\n", (unsigned long long)totalSteps, k, L.opHashes.size(), graphPrevOps2.size());
            }
            graphPrevOps2 = graphPrevOps; graphPrevOps = L.opHashes;
        }
        if (hit) {
            hit->lastUse = ++graphUseClock; ++graphHits;
            if (hipGraphLaunch(hit->exec, st) != hipSuccess) { (void)hipGetLastError(); graphsEnabled = false; dropStepGraphs(); plainAgain(); }
        } else if (sig == graphLastSig || sig == graphPrevSig) {      // seen within the last two steps as well: capture it
            if (stepGraphs.size() >= kMaxStepGraphs) { HIP_TRY(hipStreamSynchronize(st)); dropStepGraphs(); }   // a long-lived scene keeps changing shape: start over (all at once, with the stream idle)
            graphPrevSig = graphLastSig; graphLastSig = sig;
            if (hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal) != hipSuccess) { (void)hipGetLastError(); graphsEnabled = false; plainAgain(); }
            else { a.pass = PASS_CAPTURE; again = true; }
        } else { graphPrevSig = graphLastSig; graphLastSig = sig; ++graphPlain; plainAgain(); }
    } else if (a.pass == PASS_CAPTURE) {
        hipGraph_t graph = nullptr; hipGraphExec_t exec = nullptr;
        bool ok = hipStreamEndCapture(st, &graph) == hipSuccess && graph && L.firstError == hipSuccess;
        if (ok) ok = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) == hipSuccess;
        if (graph) (void)hipGraphDestroy(graph);
        if (ok) ok = hipGraphLaunch(exec, st) == hipSuccess;
        if (!ok) {   // this runtime cannot hold the step in a graph: plain launches from now on (nothing has been enqueued yet)
            (void)hipGetLastError();
            if (exec) (void)hipGraphExecDestroy(exec);
            graphsEnabled = false; dropStepGraphs(); plainAgain();
            return MI_OK;
        }
        stepGraphs.push_back(StepGraph{graphLastSig, exec, ++graphUseClock}); ++graphCaptures;
    }
    return MI_OK;
}

// Reset of the step's scalars, shard / seam classification, world-space colliders (with the grid pass in the same kernel where a grid is ready), terrain contact counts.
int mi_world::stagePrepare(StepAttempt& a) {
    const uint32_t nb = a.nb, nc = a.nc, B = 256;
    StepScalars* sc = scalarsPtr(); hipStream_t st = stream;
    const bool startTimed = a.attached && timesEnds(timingLevel);   // the step's first kernel carries the start event
    if (!a.skipReset) L.launchTimed(startTimed, ev[EV_STEP_BEGIN], nullptr, k_reset_scalars, dim3(1), dim3(128), 0, st, sc, shards.p, roundFlagsPtr(), keyCount.p);   // (else the start event rides on k_bp_prepare below)
    a.blockSkip = shard.enabled && nb && knobs.shardBlockSkip;
    if (shard.enabled && nb) {
        HIP_TRY(shard.activePrev.ensure(std::max(nb, 1u)));
        if (shard.flagsSwapPending) { shard.active.swap(shard.activePrev); shard.flagsSwapPending = false; }   // (not on the synchronous re-run of a step)
        const uint32_t bodyBlocks = divUp(nb, B), colliderBlocks = divUp(std::max(nc, 1u), B);
        HIP_TRY(shard.blockStamp.ensure(bodyBlocks)); HIP_TRY(shard.blockLive.ensure(bodyBlocks)); HIP_TRY(shard.cbLive.ensure(colliderBlocks));
        if (!shard.stepHost) { HIP_TRY(hipHostMalloc((void**)&shard.stepHost, sizeof(uint32_t))); HIP_TRY(shard.stepDev.ensure(4)); }
        *shard.stepHost = (uint32_t)totalSteps;     // (read by the copy below when it EXECUTES — pinned memory —, also when a replayed step graph executes it: written in the signature pass too)
        HIP_TRY(L.memcpyAsync(shard.stepDev.p, shard.stepHost, sizeof(uint32_t), hipMemcpyHostToDevice, st));
        if (a.blockSkip && (!shard.prevValid || shard.blocksAll)) {   // every block is recent (and counts as live) for this step: it classifies them all and finds out
            L.launch(k_fill_u32_from, dim3(divUp(bodyBlocks, B)), dim3(B), 0, st, shard.blockStamp.p, shard.stepDev.p, bodyBlocks);
            HIP_TRY(L.memsetAsync(shard.blockLive.p, 1, bodyBlocks, st)); HIP_TRY(L.memsetAsync(shard.cbLive.p, 1, colliderBlocks, st));
            if (!L.dry) shard.blocksAll = false;
        }
        if (!shard.prevValid) { HIP_TRY(L.memsetAsync(shard.activePrev.p, 1, nb, st)); if (!L.dry) shard.prevValid = true; }   // after an upload / an outside write: every body is copied once
        L.launch(k_shard_classify, dim3(bodyGrid(a, bodyBlocks)), dim3(B), 0, st, nb, shard.sp, bPos.p, bRot.p, bCogInvMass.p, shard.active.p, shards.p, shard.root.p, shard.known.p,
                 shard.activePrev.p, a.blockSkip ? shard.blockStamp.p : nullptr, shard.blockLive.p, shard.stepDev.p);
    }
    a.seamOn = seamMode() && nb;
    if (a.seamOn) {   // exact seam: which tile border every body is shared across (decides the class of its manifolds)
        HIP_TRY(seamId.ensure(nb));
        if (shard.enabled) L.launch(k_seam_classify_shard, dim3(divUp(nb, B)), dim3(B), 0, st, nb, shard.sp, bPos.p, bRot.p, bCogInvMass.p, shard.root.p, shard.active.p, seamId.p);
        else L.launch(k_seam_classify_tiling, dim3(divUp(nb, B)), dim3(B), 0, st, nb, seamTiling.dBx.p, (uint32_t)seamTiling.bx.size(), seamTiling.dBz.p, (uint32_t)seamTiling.bz.size(), seamTiling.margin,
                      bPos.p, bRot.p, bCogInvMass.p, shard.root.p, seamId.p);
    }
    if (exactSeamStep() && nb) {   // ... and the bodies whose velocities go to each neighbour after every sweep
        HIP_TRY(shard.sweepCount.ensure(8));
        HIP_TRY(L.memsetAsync(shard.sweepCount.p, 0, 8 * sizeof(uint32_t), st));
        SweepLists lists{}; for (uint32_t k = 0; k < shard.sp.numPeers; ++k) { HIP_TRY(shard.sweepList[k].ensure(shard.capacity)); lists.p[k] = shard.sweepList[k].p; }
        L.launch(k_seam_sweep_list, dim3(divUp(nb, B)), dim3(B), 0, st, nb, shard.sp, shard.active.p, bPos.p, bRot.p, bCogInvMass.p, shard.root.p, lists, shard.capacity, shard.sweepCount.p);
    }
    a.prepared = false;
    if (!nc) return MI_OK;
    // with a grid prepared by the previous step the world colliders are computed INSIDE k_bp_prepare (one launch, one pass over the AABB rows less)
    if (gridValid && knobs.fuseWorld) {   // (the cell histogram is all zero here: cleared once at upload, and every scan clears the cells it has read)
        // Not launched if the previous step ran it (step-ahead).  Behind a skipped reset it is the first kernel of the step and carries the start event (sharded: k_shard_classify before it is not in the step's time).
        if (!a.useAhead)
            L.launchTimed(a.skipReset && startTimed, ev[EV_STEP_BEGIN], nullptr, a.blockSkip ? k_bp_prepare<true> : k_bp_prepare<false>, dim3(bodyGrid(a, divUp(nc, 256))), dim3(256), 0, st,
                          nc, colliderRows(bPos.p, bRot.p, wShape.p, aabbMin.p, aabbMax.p), grid.p + gridCur, axisPartials.p, shards.p, sc, largeList.p, isLarge.p, blockBounds.p, cellKeys.p, cellRanks.p,
                          cellCount.p, countUnowned(), sapAxis, shard.enabled ? shard.axisDev.p : nullptr, a.blockSkip ? BlockSkip{cbRange.p, shard.blockLive.p, shard.cbLive.p} : BlockSkip{});
        a.prepared = true;
    } else
        L.launch(k_world_colliders, dim3(divUp(nc, B)), dim3(B), 0, st, nc, colliderRows(bPos.p, bRot.p, wShape.p, aabbMin.p, aabbMax.p), sc, sapAxis, shard.enabled ? shard.axisDev.p : nullptr);
    if (heightmap) {   // terrain contacts per collider, their offsets and totals (they join the pair list after the collider-pair narrow phase)
        const HullSet hmHulls{hullVerts.p, hullRanges.p};
        L.launch(k_hm_lowest<HmOut>, dim3(divUp(nc, 256)), dim3(256), 0, st, nc, hmParams, wShape.p, aabbMin.p, aabbMax.p, hmSlow.p, hmHulls);
        L.launch(k_hm_contacts<false, false, HmOut>, dim3(divUp(nc, 4)), dim3(256), 0, st, nc, hmParams, wShape.p, aabbMin.p, aabbMax.p, hmPacked.p, hmSlow.p, nullptr, HmOut{}, hmHulls, hmStash.p);
        L.launch(k_hm_contacts<false, true, HmOut>, dim3(std::min(divUp(nc, 256), kHmScanBlocks)), dim3(256), 0, st, nc, hmParams, wShape.p, aabbMin.p, aabbMax.p, hmPacked.p, hmSlow.p, nullptr, HmOut{}, hmHulls, hmStash.p);   // (the colliders the first pass flagged: a cell window beyond 64 cells)
        HIP_TRY(scanTerrain.run(L, hmPacked.p, hmScan.p, nc, st));
        L.launch(k_hm_totals, dim3(1), dim3(1), 0, st, nc, hmPacked.p, hmScan.p, sc);
    }
    return MI_OK;
}

// Broad phase: cell table, sorted colliders, the pair pass (redone with a larger list while a synchronous step overflows it), the pair list's final counts and the next step's grid.
int mi_world::stageBroad(StepAttempt& a) {
    const uint32_t nb = a.nb, nc = a.nc, B = 256;
    StepScalars* sc = scalarsPtr(); hipStream_t st = stream;
    const bool spec = a.spec;
    a.pairBound = 0; a.skippedPartition = false; a.finishInNarrow = false;
    a.statsGridNext = nullptr; a.statsCellCap = 0; a.statsBlocks = 0;
    if (!nc) return MI_OK;
    uint32_t nblk = divUp(nc, 256);
    // the cell table (histogram + scan) covers cellCap cells; k_bp_grid_setup enlarges the cells if the grid would need more
    const uint32_t cellCapNext = std::min<uint32_t>(kMaxCells, std::max<uint32_t>(1u << 16, 4u * nc));
    const uint32_t cellCap = gridValid ? (lastCellCap = std::min<uint32_t>(kMaxCells, (lastCellCap > gridNextCells && lastCellCap - gridNextCells <= 8192u) ? lastCellCap : ((gridNextCells + 1u + 4095u) & ~4095u))) : spec ? std::min<uint32_t>(kMaxCells, std::max<uint32_t>(1u << 16, 2u * last.numCells)) : kMaxCells;
    GridParams* gridUse = grid.p + gridCur; GridParams* gridNext = grid.p + (gridCur ^ 1u);
    a.statsGridNext = gridNext; a.statsCellCap = cellCapNext; a.statsBlocks = nblk;
    if (a.prepared) {}   // k_bp_prepare ran with the world colliders
    else if (gridValid) {
        // the grid prepared at the end of the previous step (k_pair_finish): one fused kernel instead of five launches; the cell histogram
        // is all zero here (cleared once at upload, and every scan clears the cells it has read)
        ColliderRows given{};   // no collider table: k_world_colliders has written this step's rows, the kernel reads them (and the shard flags)
        given.aabbMin = aabbMin.p; given.aabbMax = aabbMax.p; given.bodyActive = shard.enabled ? shard.active.p : nullptr; given.bodyActivePrev = shard.enabled ? shard.activePrev.p : nullptr;
        L.launch(k_bp_prepare<false>, dim3(nblk), dim3(256), 0, st, nc, given, gridUse, axisPartials.p, shards.p, sc, largeList.p, isLarge.p, blockBounds.p, cellKeys.p, cellRanks.p, cellCount.p,
                 countUnowned(), 0u, nullptr, BlockSkip{});
    } else {
        L.launch(k_axis_partials, dim3(nblk), dim3(256), 0, st, nc, aabbMin.p, aabbMax.p, axisPartials.p, shards.p, shard.enabled ? shard.active.p : nullptr, countUnowned());
        L.launch(k_bp_threshold, dim3(1), dim3(256), 0, st, nc, shards.p, sc);
        L.launch(k_bp_classify, dim3(divUp(nc, B)), dim3(B), 0, st, nc, aabbMin.p, aabbMax.p, sc, largeList.p, isLarge.p, blockBounds.p);
        L.launch(k_bp_grid_setup, dim3(1), dim3(256), 0, st, nc, nblk, cellCap, blockBounds.p, sc, gridUse);
        L.launch(k_bp_cell_ids, dim3(divUp(nc, B)), dim3(B), 0, st, nc, aabbMin.p, aabbMax.p, isLarge.p, gridUse, cellKeys.p, cellRanks.p, cellCount.p);
    }
    HIP_TRY(scanCells.run(L, cellCount.p, cellLower.p, cellCap, st, true));
    const bool skipBlocks = a.blockSkip && a.prepared;   // (the dead blocks' flags come from k_bp_prepare)
    L.launch(skipBlocks ? k_bp_scatter_sorted<true> : k_bp_scatter_sorted<false>, dim3(skipBlocks ? bodyGrid(a, divUp(nc, B)) : divUp(nc, B)), dim3(B), 0, st,
             nc, cellKeys.p, cellRanks.p, cellLower.p, aabbMin.p, aabbMax.p, cellKeysS.p, cellValsS.p, sMin.p, sMax.p, gridUse, sRow.p, skipBlocks ? shard.cbLive.p : nullptr);
    if (pairKeys.cap == 0) { HIP_TRY(pairKeys.ensure(std::max<size_t>(1u << 16, 8 * (size_t)nc))); }
    if (spec) { HIP_TRY(pairKeys.ensure(specBound(last.numPairs, 4096))); }
    if (usesInteractions && interKeys.cap == 0) HIP_TRY(interKeys.ensure(4096));
    if (usesInteractions && spec) HIP_TRY(interKeys.ensure(specBound(last.numInterPairs, 1024)));
    for (int attempt = 0; attempt < 3; ++attempt) {
        uint32_t cap = (uint32_t)std::min<size_t>(pairKeys.cap, 0x7FFFFFFFu);
        const InterSink inter{usesInteractions ? interKeys.p : nullptr, (uint32_t)interKeys.cap, &sc->numInterPairs};
        // sized for the small (grid) colliders expected — in a sharded world most colliders are dead and in no list; more than expected: the workgroups loop
        const uint32_t smallBound = spec ? std::min(nc, specBound(last.numSmall, 4096)) : nc;
        const uint32_t bpc = (divUp(smallBound, kGridChunks * 256u) + 7u) & ~7u;   // a multiple of 8 (XCD-contiguous block order in k_bp_pairs_grid)
        const uint32_t largeGx = std::min(divUp(smallBound + 1024u, B), 4096u), largeGy = std::min(16u, std::max(1u, divUp(spec ? last.numLarge + last.numLarge / 4u : 1024u, 64u)));
#ifdef MI_DBG_KNOCKOUT
        if (attempt == 0) { int rck = dbgKnockBroad(bpc, cap, gridUse); if (rck != MI_OK) return rck; }
#endif
        if (knobs.fuseLarge) {   // both passes in one launch, the large one in its first workgroups (k_bp_pairs)
            const uint32_t largeBlocks = (largeGx * largeGy + 7u) & ~7u;
            L.launch(k_bp_pairs, dim3(largeBlocks + 5u * bpc), dim3(B), 0, st, largeBlocks, largeGx, largeGy, nc, bpc, cellKeysS.p, cellValsS.p, sRow.p, sMin.p, sMax.p, cellLower.p, gridUse, largeList.p, aabbMin.p, aabbMax.p, pairKeys.p, cap, sc, shards.p, inter);
        } else {
            L.launch(k_bp_pairs_grid, dim3(5u * bpc), dim3(B), 0, st, nc, bpc, cellKeysS.p, sRow.p, sMin.p, sMax.p, cellLower.p, gridUse, pairKeys.p, cap, sc, shards.p, inter);
            L.launch(k_bp_pairs_large, dim3(largeGx, largeGy), dim3(B), 0, st, nc, largeList.p, aabbMin.p, aabbMax.p, cellValsS.p, sMin.p, sMax.p, cellLower.p, gridUse, pairKeys.p, cap, sc, shards.p, inter);
        }
        // (a box pile: nearly every pair is of one type and k_pair_finish decides against partitioning — k_pair_partition then does nothing but cost its
        // launch slot: a speculative step whose predecessor was not partitioned leaves it out; if this step wants it after all, k_pair_finish voids the step)
        a.skippedPartition = spec && havePartitionFlag && !lastPartitioned;
        // (and without k_pair_partition nothing needs the list's final counts before k_narrow: its workgroups derive them themselves — one launch less)
        a.finishInNarrow = a.skippedPartition && knobs.finishInNarrow && std::min(cap, specBound(last.numPairs, 4096)) != 0u;
        if (!a.finishInNarrow)
        L.launch(k_pair_finish, dim3(1), dim3(256), 0, st, shards.p, sc, spec ? std::min(cap, specBound(last.numPairs, 4096)) : 0xFFFFFFFFu, nc, nblk, attempt == 0 ? axisPartials.p : nullptr, blockBounds.p, attempt == 0 ? gridNext : nullptr, cellCapNext,
                 a.skippedPartition ? 0u : 1u, spec ? 0u : 1u /* speculative: an extra workgroup of k_narrow_clip does the statistics, off the critical path */);
        if (spec) { a.pairBound = std::min(cap, specBound(last.numPairs, 4096)); break; }
        int rc = readScalars(); if (rc != MI_OK) return rc;
        a.pairBound = hs.numPairs + hs.numHmContacts;   // the terrain contacts are appended to the pair list after the narrow phase
        if (a.pairBound <= cap && hs.numInterPairs <= interKeys.cap) { if (debugOrderPending) { int rco = orientPairsLikeDebugOrder(); if (rco != MI_OK) return rco; } break; }
        if (attempt == 2) return fail(MI_ERR_DEVICE, "pair pass did not settle");
        if (a.pairBound > cap) HIP_TRY(pairKeys.ensure((size_t)a.pairBound + a.pairBound / 4));   // overflow: grow and redo the pair pass
        if (hs.numInterPairs > interKeys.cap) HIP_TRY(interKeys.ensure((size_t)hs.numInterPairs + hs.numInterPairs / 4));
        L.launch(k_reset_pair_counters, dim3(1), dim3(32), 0, st, sc, shards.p);
    }
    return MI_OK;
}

// Narrow phase: contacts per pair (boxes / spheres directly and through the clip queues, GJK / EPA, terrain), their scan, and the manifolds with the colours they keep.
int mi_world::stageNarrow(StepAttempt& a) {
    const uint32_t nb = a.nb, nc = a.nc, B = 256, pairBound = a.pairBound;
    StepScalars* sc = scalarsPtr(); hipStream_t st = stream;
    const bool spec = a.spec;
    if (!pairBound) return MI_OK;
    HIP_TRY(pairKeysS.ensure(pairKeys.cap));
    if (!a.skippedPartition) L.launch(k_pair_partition, dim3(divUp(pairBound, 1024)), dim3(256), 0, st, pairKeys.p, pairKeysS.p, sc);
    HIP_TRY(npPacked.ensure(pairBound)); HIP_TRY(npScan.ensure(pairBound)); HIP_TRY(npNormal.ensure(pairBound)); HIP_TRY(npPoints.ensure(4 * (size_t)pairBound));
    HIP_TRY(manPair.ensure(pairBound)); HIP_TRY(manBodies.ensure(pairBound)); HIP_TRY(manInfo.ensure(pairBound));
    HIP_TRY(colWork.ensure(pairBound)); HIP_TRY(color.ensure(pairBound));
    // bodyUsed is all zero here (k_integrate_velocities of the previous step / upload cleared it); k_emit_manifolds seeds it with the kept colours
    HullSet hset{hullVerts.p, hullRanges.p};
    const uint32_t narrowBlocks = divUp(pairBound, B);
    const uint32_t queueRegion = divUp(narrowBlocks, kBoxQueues) * B;   // a queue can hold every pair of the workgroups that feed it
    HIP_TRY(boxQueue.ensure((size_t)kBoxQueues * queueRegion));
    uint32_t histCap = 1024;
    {   // the NEXT step's colour history: sized here, cleared by k_narrow on the side (k_emit_manifolds already enters the manifolds that keep their colour)
        const uint32_t histBound = spec ? std::min(pairBound, specBound(last.numManifolds, 1024)) : pairBound;
        const int nt = tabCur ^ 1;
        while (histCap < 2u * histBound) histCap <<= 1;
        HIP_TRY(tab[nt].ensure(histCap)); HIP_TRY(manKept.ensure(pairBound));
        tabMask[nt] = histCap - 1u;
        // probe hints: the next table goes on with the previous table's array while the size stays (kept entries keep their slots, hence their displacements); a table
        // of another size — or the first one — starts on the other array, zeroed
        if (tabValid && tabMask[nt] == tabMask[tabCur] && histHint[hintOf[tabCur]].cap >= histCap) hintOf[nt] = hintOf[tabCur];
        else {
            hintOf[nt] = tabValid ? hintOf[tabCur] ^ 1 : 0;
            HIP_TRY(histHint[hintOf[nt]].ensure(histCap));
            HIP_TRY(L.memsetAsync(histHint[hintOf[nt]].p, 0, (size_t)histCap * sizeof(uint32_t), st));
        }
    }
    L.launch(k_narrow, dim3(narrowBlocks), dim3(B), 0, st, pairBound, queueRegion, sc, pairKeys.p, pairKeysS.p, wShape.p, hset, npPacked.p, npNormal.p, npPoints.p, boxQueue.p,
             reinterpret_cast<ulonglong2*>(tab[tabCur ^ 1].p), histCap, a.finishInNarrow ? shards.p : nullptr, pairBound, shards.p);
    const bool statsInClip = spec && a.statsGridNext != nullptr;   // (a synchronous step: k_pair_finish did it)
    L.launch(k_narrow_clip, dim3(kBoxQueues * (queueRegion / B) + (statsInClip ? 1u : 0u)), dim3(B), 0, st, queueRegion, sc, pairKeys.p, pairKeysS.p, wShape.p, boxQueue.p, npPacked.p, npNormal.p, npPoints.p, shards.p,
             statsInClip ? shards.p : nullptr, sc, nc, a.statsBlocks, axisPartials.p, blockBounds.p, a.statsGridNext, a.statsCellCap, a.blockSkip && a.prepared ? shard.cbLive.p : nullptr);
    // (a GJK-only kernel feeding a queue of hits to an EPA kernel was measured: no gain — the GJK half already needs ~250 VGPRs)
    if (usesGjk) {
        HIP_TRY(epaQueue.ensure(pairBound)); HIP_TRY(epaSimplex.ensure((size_t)pairBound * kEpaSimplexRows));
        // few GJK pairs (vehicles on hull tiles, a handful of capsules): one WAVE per pair for GJK as well; many: GJK by lanes, EPA by waves
        const int gjkWaveMode = knobs.gjkWave;   // 0 / 1 force a variant (tests, tuning)
        const bool gjkWave = gjkWaveMode >= 0 ? gjkWaveMode != 0 : (spec ? last.gjkSpan <= gjkWaveMaxPairs : false);
        if (gjkWave) L.launch(k_narrow_gjk_wave, dim3(std::min(pairBound, 16384u)), dim3(64), 0, st, sc, pairKeys.p, pairKeysS.p, wShape.p, hset, npPacked.p, npNormal.p, npPoints.p);
        else {
            L.launch(k_narrow_gjk, dim3(divUp(pairBound, 64)), dim3(64), 0, st, sc, pairKeys.p, pairKeysS.p, wShape.p, hset, npPacked.p, npNormal.p, npPoints.p, epaQueue.p, epaSimplex.p, pairBound);
            L.launch(k_narrow_epa, dim3(std::min(pairBound, 8192u)), dim3(64), 0, st, sc, pairKeys.p, pairKeysS.p, wShape.p, hset, epaQueue.p, epaSimplex.p, pairBound, npPacked.p, npNormal.p, npPoints.p);
        }
    }
    if (heightmap) {
        const HmOut hmOut{sc, pairBound, pairKeys.p, pairKeysS.p, npPacked.p, npNormal.p, npPoints.p};
        L.launch(k_hm_contacts<true, false, HmOut>, dim3(std::min(divUp(nc, 256), kHmScanBlocks)), dim3(256), 0, st, nc, hmParams, wShape.p, aabbMin.p, aabbMax.p, hmPacked.p, hmSlow.p, hmScan.p, hmOut, hset, hmStash.p);
        L.launch(k_hm_contacts<true, true, HmOut>, dim3(std::min(divUp(nc, 256), kHmScanBlocks)), dim3(256), 0, st, nc, hmParams, wShape.p, aabbMin.p, aabbMax.p, hmPacked.p, hmSlow.p, hmScan.p, hmOut, hset, hmStash.p);
        L.launch(k_hm_write_stashed<HmOut>, dim3(divUp(pairBound, B)), dim3(B), 0, st, nc, hmParams, wShape.p, aabbMin.p, aabbMax.p, hmPacked.p, hmSlow.p, hmScan.p, hmOut, hset, hmStash.p);   // (sized for all pairs: the terrain contacts are among them)
        L.launch(k_hm_finish, dim3(1), dim3(1), 0, st, sc, pairBound);
    }
    HIP_TRY(scanPairs.run(L, reinterpret_cast<unsigned long long*>(npPacked.p), reinterpret_cast<unsigned long long*>(npScan.p), pairBound, st));
    if (eventsEnabled) HIP_TRY(manIsNew.ensure(pairBound));
    const bool round0InEmit = emitsRound0();
#ifdef MI_DBG_KNOCKOUT
    { int rck = dbgKnockEmit(a); if (rck != MI_OK) return rck; }
#endif
    L.launch(k_emit_manifolds, dim3(divUp(pairBound, B)), dim3(B), 0, st, nc, nb, pairKeys.p, pairKeysS.p, npPacked.p, npScan.p, cEmit.p,
                                                    manPair.p, manBodies.p, manInfo.p, colWork.p, color.p,
                                                    tabValid ? tab[tabCur].p : nullptr, tabMask[tabCur], bodyUsed.p, eventsEnabled ? manIsNew.p : nullptr, sc,
                                                    heightmap ? make_float2(hmParams.restitution, hmParams.friction) : make_float2(0.f, 0.f),
                                                    tab[tabCur ^ 1].p, tabMask[tabCur ^ 1], manKept.p, tabValid ? histHint[hintOf[tabCur]].p : nullptr, histHint[hintOf[tabCur ^ 1]].p,
                                                    a.seamOn ? seamId.p : nullptr, round0InEmit ? bodyTop.p + (nb + 1) : nullptr, roundFlagsPtr());
    return MI_OK;
}

// Triggers / force fields: a speculative step orders and applies them on the device; a synchronous one brings the (few) interactions to the host.
int mi_world::stageInteractions(StepAttempt& a) {
    a.interPairBound = 0; a.triggerEvents.clear();
    if (usesInteractions && a.spec) {
        a.interPairBound = (uint32_t)std::min<size_t>(interKeys.cap, specBound(last.numInterPairs, 1024));
        HIP_TRY(interList.ensure(specBound(last.numInteractions, 1024))); HIP_TRY(interSorted.ensure(interList.cap));
        return interactionsDevice(a.interPairBound);
    }
    return usesInteractions ? interactions(a.triggerEvents) : MI_OK;
}

// Gravity, damping and the external forces into the solver's body arrays (+ the manifolds' spatial keys for the XCD-partitioned layout, in the same launch).
int mi_world::stageForces(StepAttempt& a) {
    const uint32_t nb = a.nb, B = 256;
    hipStream_t st = stream;
    // (speculative step of a pile that gets the XCD-partitioned layout: the spatial keys of the manifolds ride in the same launch — k_forces_keys)
    const uint32_t specNmBound = a.spec && a.pairBound ? std::min(a.pairBound, specBound(last.numManifolds, 1024)) : 0u;
    a.keysWithForces = knobs.fuseKeys && specNmBound && xcdPlanFor(specNmBound) && !xcdSingleFor(specNmBound);
    const dim3 bodyBlocks(bodyGrid(a, divUp(nb + 1, B)));
    if (a.keysWithForces) {
        HIP_TRY(sortKeys[0].ensure(specNmBound)); HIP_TRY(sortVals[0].ensure(specNmBound));
        const uint32_t keyBlocks = divUp(specNmBound, kKeyItems);
        L.launch(a.blockSkip ? k_forces_keys<true> : k_forces_keys<false>, dim3(keyBlocks + bodyBlocks.x), dim3(B), 0, st, keyBlocks, forcesArgs(a), keysArgs(specNmBound));
    } else L.launch(a.blockSkip ? k_integrate_forces<true> : k_integrate_forces<false>, bodyBlocks, dim3(B), 0, st, forcesArgs(a));
    return MI_OK;
}
// (evaluated where it is launched: buffers may still be (re)allocated on the way there)
ForcesArgs mi_world::forcesArgs(const StepAttempt& a) {
    return ForcesArgs{bPos.p, bRot.p, bCogInvMass.p, bInvI.p, bParams.p, bLinVel.p, bAngVel.p, usesInteractions ? bForceStep.p : bForce.p, bTorque.p,
                      gPos.p, gInvI.p, gVel.p, gVelL.p, bodyOwner.p, shard.enabled ? shard.active.p : nullptr, a.blockSkip ? shard.blockLive.p : nullptr, a.nb, a.dt, {globalForce.x, globalForce.y, globalForce.z}, 0u};
}
KeysArgs mi_world::keysArgs(uint32_t nm) {
    return KeysArgs{nm, (uint32_t)bodies.size(), scalarsPtr(), grid.p + gridCur, manBodies.p, bPos.p, bCogInvMass.p, sortKeys[0].p, sortVals[0].p, keyCount.p, shard.enabled ? shard.active.p : nullptr, manInfo.p, shards.p};
}

// Colouring rounds a step enqueues before k_bin_hist.
// Converged rounds exit at once, but every enqueued round costs its launch slot (~4.6 us): a scene that replays its steps as graphs wants the same
// launches step after step (a multiple of 4), a large one exactly what the previous step needed plus the margin
// ... or, with the colouring tail (k_bin_hist runs whatever rounds are missing: colorTail in kernels.hpp), what the previous step needed + 1: the tail's rounds are slow (a device-wide barrier with cache write-back each), it is there for the
// step that outgrows its predecessor by more, not for every other step
uint32_t mi_world::colorBatchFor(const StepAttempt& a, bool colorTailOn) {
    constexpr uint32_t kColorMargin = 3, kColorTailMargin = 1;   // extra rounds enqueued beyond the previous step's count, without / with the tail
    if (a.graphStep && colorTailOn) {   // a scene that replays its steps as graphs: the same launches step after step — the count only moves when the need outgrows it or falls 2 below
        const uint32_t need = std::min<uint32_t>(96u, last.colorRounds + kColorTailMargin);
        if (need > colorBatchSticky || need + 2u < colorBatchSticky) colorBatchSticky = need;
    }
    uint32_t colorBatch = !a.spec ? 20u : a.graphStep ? (colorTailOn ? colorBatchSticky : std::min<uint32_t>(96u, (last.colorRounds + std::max(kColorMargin, last.colorRounds / 4u) + 3u) & ~3u))
                                        : colorTailOn ? std::min<uint32_t>(96u, last.colorRounds + kColorTailMargin)
                                                      : std::min<uint32_t>(96u, last.colorRounds + std::max(kColorMargin, last.colorRounds / 4u));
    if (colorTailOn && knobs.colorRoundsMax) colorBatch = std::min(colorBatch, knobs.colorRoundsMax);
    return colorBatch;
}

// Schedule: bounds of the manifolds / contacts, spatial placement for the XCD layout, graph colouring, colour bins -> tiles, the next step's colour history, collision events.
int mi_world::stageSchedule(StepAttempt& a) {
    const uint32_t nb = a.nb, nc = a.nc, B = 256, pairBound = a.pairBound;
    StepScalars* sc = scalarsPtr(); hipStream_t st = stream;
    const bool spec = a.spec, seamOn = a.seamOn, round0InEmit = emitsRound0();
    uint32_t nmBound = 0, conBound = 0;
    if (pairBound) {
        if (spec) { nmBound = std::min(pairBound, specBound(last.numManifolds, 1024)); conBound = specBound(last.numContacts, 4096); }
        else { int rc = readScalars(); if (rc != MI_OK) return rc; nmBound = hs.numManifolds; conBound = hs.numContacts; }
    }
    a.nmBound = nmBound; a.conBound = conBound;
    a.tilesCap = a.ctCap = a.eventCap = a.xcdListCap = 0; a.shardCounted = false;
    const bool xcdSingle = a.xcdSingle = xcdSingleFor(nmBound), xcdPlan = a.xcdPlan = xcdPlanFor(nmBound);
    if (spec && colorTailHold) --colorTailHold;
    const bool colorTailOn = spec && knobs.colorTail && !colorTailHold;   // (colorTailHold: the tail's device-wide barrier timed out recently — a margin of enqueued rounds instead, like the other fault paths)
    uint32_t colorBatch = colorBatchFor(a, colorTailOn);
    if (nmBound) {
        uint32_t tilesCap = divUp(nmBound, 64) + kSchedBins + 8, ctCap = divUp(conBound, 64) + 4 * kSchedBins + 8, xcdListCap = 0;
        // the sequential (overflow) bin's tiles take 4 contact-tiles each whatever their contact counts.  A synchronous step must hold whatever the colouring puts there — in the
        // caller's order that is EVERY manifold, and a heap of bodies spawned into one another fills it with one-contact manifolds (tools/gpu_fuzz.py: MI_ERR_CAPACITY out of a
        // synchronous step) —; a speculative step with anything in that bin is void anyway and sized for none.
        if (debugOrderPending || !spec) ctCap = std::max(ctCap, 4u * (divUp(nmBound, 64) + 1u) + 4u * kSchedBins + 8u);
        const uint32_t binBlocks = divUp(nmBound, kBinItems);
        HIP_TRY(order.ensure(std::max((size_t)binBlocks * kBinItems, (size_t)tilesCap * 64u))); HIP_TRY(orderTmp.ensure((size_t)binBlocks * kBinItems));
        HIP_TRY(blockHist.ensure((size_t)kColorBins * binBlocks)); HIP_TRY(blockScan.ensure((size_t)kColorBins * binBlocks));
        HIP_TRY(tileInfo.ensure(tilesCap)); HIP_TRY(tileDesc.ensure(tilesCap));
        if (xcdPlan) {   // slots in spatial order inside every bin + per-XCD tile lists (k_contact_solve_persist<.., true>)
            xcdListCap = xcdSingle ? tilesCap + kSchedBins : divUp(tilesCap, 8) + kSchedBins;
            HIP_TRY(sortKeys[0].ensure(nmBound)); for (int k = 0; k < 2; ++k) HIP_TRY(sortVals[k].ensure(nmBound));
            HIP_TRY(xcdTiles.ensure((size_t)8 * xcdListCap)); HIP_TRY(xcdInfo.ensure((size_t)8 * xcdListCap));
            if (!xcdSingle) {   // (one XCD: nothing to keep apart, the emission order will do)
                if (!a.keysWithForces) L.launch(k_manifold_keys, dim3(divUp(nmBound, kKeyItems)), dim3(256), 0, st, keysArgs(nmBound));
                a.shardCounted = shard.enabled;
                L.launch(k_manifold_place, dim3(divUp(nmBound, kKeyItems)), dim3(256), 0, st, nmBound, sc, sortKeys[0].p, sortVals[0].p, keyCount.p, sortVals[1].p);
            }
        }
        a.tilesCap = tilesCap; a.ctCap = ctCap; a.xcdListCap = xcdListCap;
        const uint32_t* perm = xcdPlan && !xcdSingle ? sortVals[1].p : nullptr;
        unsigned long long* top[2] = {bodyTop.p, bodyTop.p + (nb + 1)};
        if (debugOrderPending) { int rc = applyDebugOrder(); if (rc != MI_OK) return rc; }   // (synchronous step: hs holds this step's counts) every manifold -> the sequential colour
        uint32_t round = round0InEmit ? 1u : 0u;
        while (true) {
            for (uint32_t r = (round0InEmit && round == 1u) ? 1u : 0u; r < colorBatch; ++r, ++round)
                L.launch(k_color_round, dim3(divUp(nmBound, B)), dim3(B), 0, st, sc, round, colWork.p, color.p, top[round & 1], top[(round + 1) & 1], bodyUsed.p, roundFlagsPtr(), seamOn ? 1u : 0u);
            // schedule bins -> tiles (valid once the last round left nothing uncoloured: StepScalars::colorPending)
            L.launch(k_bin_hist, dim3(binBlocks), dim3(256), 0, st, sc, binBlocks, perm, color.p, manInfo.p, blockHist.p,
                     ColorTail{colWork.p, color.p, top[0], top[1], bodyUsed.p, roundFlagsPtr(), colorTailOn ? round : 0u, seamOn ? 1u : 0u}, sc);
            HIP_TRY(scanBins.run(L, blockHist.p, blockScan.p, kColorBins * binBlocks, st));
            {   // slots, colour history of the new manifolds, bins -> tiles, tile tables: one launch (k_schedule_finish)
                const int ntab = tabCur ^ 1;   // the NEXT step's colour history (sized and cleared in the narrow-phase stage; current only if this step turns out valid)
                L.launch(k_schedule_finish, dim3(binBlocks + divUp(tilesCap, B)), dim3(256), 0, st, round - 1, roundFlagsPtr(), binBlocks, perm, color.p, manInfo.p, blockHist.p, blockScan.p, order.p, sc,
                         nc, manPair.p, pairKeys.p, pairKeysS.p, tab[ntab].p, tabMask[ntab], manKept.p, histHint[hintOf[ntab]].p,
                         tilesCap, ctCap, binInfo.p, xcdPlan ? xcdBase.p : nullptr, xcdSingle ? 1u : 0u, tileInfo.p, tileDesc.p, xcdPlan ? xcdTiles.p : nullptr, xcdInfo.p, xcdListCap);
            }
            if (spec) break;
            int rc = readScalars(); if (rc != MI_OK) return rc;
            if (hs.numManifolds && hs.totalTiles == 0u) return fail(MI_ERR_CAPACITY, "the schedule's tile tables outgrew their (exactly sized) capacity");   // (k_schedule_finish wrote no tile table: nothing may be launched over it)
            if (hs.colorPending == 0) break;
            if (round + 8 > kMaxColorRounds) return fail(MI_ERR_DEVICE, "colouring did not converge");
            colorBatch = 8;
        }
        colorRoundsLaunched = round;
        // a caller-ordered step leaves the overflow colour for every one of its manifolds in the history (its colours were levels of the order, or 64, mixed with
        // the kept manifolds' old colours: together no valid colouring); the next free step colours them afresh, as the oracle does
        if (debugOrderPending) L.launch(k_history_overflow, dim3(divUp(tabMask[tabCur ^ 1] + 1u, B)), dim3(B), 0, st, tab[tabCur ^ 1].p, tabMask[tabCur ^ 1]);
        if (seamOn) L.launch(k_seam_stats, dim3(divUp(nmBound, B)), dim3(B), 0, st, sc, colWork.p, color.p, shard.enabled ? shard.active.p : nullptr);
        if (eventsEnabled) {   // begins: manifolds not in the previous table; ends: previous pairs not in this step's table
            const int nt = tabCur ^ 1;   // colour history for the next step, the OTHER table (sized and cleared before k_emit_manifolds; it becomes current only if this step turns out valid)
            const uint32_t eventCap = a.eventCap = nmBound + (tabValid ? last.numManifolds : 0u) + 1024u;
            HIP_TRY(devEvents.ensure(eventCap));
            L.launch(k_events_begin, dim3(divUp(nmBound, B)), dim3(B), 0, st, nc, eventCap, sc, manIsNew.p, manPair.p, manBodies.p, manInfo.p, pairKeys.p, pairKeysS.p,
                                                           npNormal.p, npPoints.p, gPos.p, gVel.p, devEvents.p);
            if (tabValid) L.launch(k_events_end, dim3(divUp(tabMask[tabCur] + 1u, B)), dim3(B), 0, st, eventCap, sc, tab[tabCur].p, tabMask[tabCur], tab[nt].p, tabMask[nt], devEvents.p, histHint[hintOf[nt]].p);
        }
        if (!spec) { int rc = orderSequentialBin(); if (rc != MI_OK) return rc; }
    }
    if (debugOrderPending && !nmBound && !debugOrder.empty()) return fail(MI_ERR_INVALID_ARGUMENT, "mi_debug_set_solve_order: the step found no contact manifold, the list holds " + std::to_string(debugOrder.size()));
    return MI_OK;
}
// Synchronous step, schedule known (hs): the host mirror of it, and the slot order of the sequential (overflow) bin.
int mi_world::orderSequentialBin() {
    hipStream_t st = stream;
    mirrorSchedule();
    const BinInfo& ob = bins[kSchedBins - 1];
    if (debugOrderPending && debugOrderLevelled) {
        if (ob.count) return fail(MI_ERR_DEVICE, "mi_debug_set_solve_dataflow: the levelled schedule put a manifold into the sequential bin");
    } else
    if (debugOrderPending) {   // the caller's order (applyDebugOrder left every manifold's rank in debugRank)
        if (ob.count != hs.numManifolds) return fail(MI_ERR_DEVICE, "mi_debug_set_solve_order: schedule did not put every manifold into the sequential bin");
        if (ob.count) {
            std::vector<uint32_t> ord(ob.count);
            for (uint32_t m = 0; m < ob.count; ++m) ord[debugRank[m]] = m;
            HIP_TRY(hipMemcpyAsync(order.p + ob.slotStart, ord.data(), ob.count * sizeof(uint32_t), hipMemcpyHostToDevice, st));
            HIP_TRY(hipStreamSynchronize(st));
        }
    } else
    if (ob.count > 1) {   // overflow colour: sequential solve in ascending pair-key order
        HIP_TRY(L.memcpyAsync(orderTmp.p + ob.slotStart, order.p + ob.slotStart, ob.count * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
        L.launch(k_sort_overflow, dim3(1), dim3(256), 0, st, ob.slotStart, ob.count, manPair.p, hs.partitioned ? pairKeysS.p : pairKeys.p, orderTmp.p, order.p);
    }
    return MI_OK;
}

// slots (tiles) one persistent workgroup must hold: exact in a synchronous step, from the previous step's lists (+ slack) in a speculative one
uint32_t mi_world::persistSlots(const StepAttempt& a) {
    if (!a.xcdPlan) return divUp(a.tilesLaunch, persistWaves);
    uint32_t longest = 0;
    if (a.spec) longest = (haveXcdEstimate && lastXcdSingle == a.xcdSingle) ? lastXcdMax + lastXcdMax / 8u + 16u : a.xcdSingle ? a.tilesLaunch + 16u : divUp(a.tilesLaunch, 8) + 64u;
    else for (uint32_t x = 0; x < 8u; ++x) { uint32_t n = 0; for (uint32_t bn = 0; bn < kSchedBins; ++bn) n += tileOwnerCount(x, divUp(bins[bn].count, 64), bn, a.xcdSingle ? 1u : 0u); longest = std::max(longest, n); }
    return divUp(std::max(longest, 1u), persistWaves / 8u);
}

// Constraints: which solver this step gets, and the contact rows / slot data (k_contact_init) and joint rows it starts from.
int mi_world::stageConstraintInit(StepAttempt& a) {
    const uint32_t nb = a.nb, B = 256, nmBound = a.nmBound, tilesCap = a.tilesCap, ctCap = a.ctCap, xcdListCap = a.xcdListCap;
    StepScalars* sc = scalarsPtr(); hipStream_t st = stream;
    const bool xcdPlan = a.xcdPlan;
    const uint32_t tilesLaunch = a.tilesLaunch = a.spec ? tilesCap : totalTiles;   // sync mode knows the exact tile count (mirrorSchedule)
    a.useFlow = flowSolver && !launchFallbackSteps && (!debugOrderPending || debugOrderLevelled) && (a.spec || bins[kSchedBins - 1].count == 0 || !nmBound);   // the overflow colour needs the sequential kernel
    const bool fused = a.fused = a.useFlow && joints.allInIslands() && !exactSeamStep();   // joints of all sweeps inside the dataflow launch
    // the persistent kernel keeps the accumulated impulses in LDS while they fit: k_contact_init then need not write the impulse granules
    a.persistPlan = !fused && a.useFlow && persistSolver && joints.count() == 0 && tilesLaunch && !exactSeamStep();
    a.persistMaxSlots = a.persistPlan ? persistSlots(a) : 0u;
    const bool privateIslands = fused && privateIslandsEnabled && !shard.enabled && joints.dBodyIsland.p && nmBound && tilesLaunch;
    const IslandPrivate islandPriv = a.islandPriv = privateIslands ? joints.islandPrivate() : IslandPrivate{nullptr, nullptr, nullptr, nullptr, nullptr};
    const bool impNeeded = !(a.persistPlan && persistImpLds && a.persistMaxSlots * (4u * 512u + 24u) <= 38u * 1024u);
    if (nmBound) {
        HIP_TRY(slotMeta.ensure((size_t)tilesCap * 64)); HIP_TRY(slotNormal.ensure((size_t)tilesCap * 64)); HIP_TRY(slotMass.ensure((size_t)tilesCap * 64));
        HIP_TRY(rows.ensure((size_t)ctCap * kRows * 64)); HIP_TRY(imp.ensure((size_t)ctCap * 64));
        if (privateIslands) {   // which joint islands are private this step (joints.hpp "PRIVATE islands"): their manifolds go to the island's own workgroup
            HIP_TRY(L.memsetAsync(joints.dIslState.p, 0, 3 * (size_t)joints.numIslands * sizeof(uint32_t), st));
            L.launch(k_island_classify, dim3(divUp(nmBound, B)), dim3(B), 0, st, sc, colWork.p, color.p, islandPriv);
        }
        if (tilesLaunch)
            L.launch(k_contact_init, dim3(xcdPlan ? 8u * xcdListCap : tilesLaunch), dim3(64), 0, st, sc, nb, a.dt, xcdPlan ? xcdInfo.p : tileInfo.p, order.p, manPair.p, manBodies.p, manInfo.p, npNormal.p, npPoints.p,
                                                      gPos.p, gInvI.p, xcdPlan ? gVelL.p : gVel.p /* same content here; the cached copy */, color.p, bodyUsed.p, fused ? joints.dBodyJ.p : nullptr, rows.p, impNeeded ? imp.p : nullptr, slotMeta.p, slotNormal.p, slotMass.p,
                                                      xcdPlan ? reinterpret_cast<uint8_t*>(bodyOwner.p) : nullptr, xcdListCap, xcdPlan ? 8u * xcdListCap : tilesCap, islandPriv);
    }
    return joints.initialize(*this, a.dt, st);   // (through L)
}

// The solve stage: one of four solver paths (stepInternal's ladder walks down them), then a sharded world's counts.
int mi_world::stageSolve(StepAttempt& a) {
    const bool persist = !a.fused && a.persistPlan && a.persistMaxSlots * 24u <= 38u * 1024u;
    a.solveAttached = false; a.mainContacts = 0;
    if (a.attached && !persist) (void)hipEventRecord(ev[EV_SOLVE_BEGIN], stream);   // another solver path (several launches): classic recorded events
    usedFlow = a.useFlow; usedPersist = false; usedFused = a.fused; usedXcd = false; usedXcdSingle = false;
    int rc = a.fused ? solveFused(a) : persist ? solvePersistent(a) : a.useFlow ? solveFlow(a) : solvePerColour(a);
    if (rc != MI_OK) return rc;
    if (shard.enabled && a.pairBound && !a.shardCounted) L.launch(k_shard_count, dim3(divUp(a.nmBound ? a.nmBound : 1u, 256)), dim3(256), 0, stream, a.nb, manBodies.p, manInfo.p, bCogInvMass.p, shard.active.p, scalarsPtr(), shards.p);
    return MI_OK;
}
// contacts and joint islands of every sweep in one launch (k_solve_flow_islands)
int mi_world::solveFused(StepAttempt& a) {
    const uint32_t iters = a.settings.num_rigid_solver_iterations;
    const uint64_t per = (uint64_t)joints.numIslands + a.tilesLaunch;
    const uint32_t perLaunch = per * iters < 0x7FFFFFFFull ? iters : 1u;
    solveLaunches = (iters + perLaunch - 1) / perLaunch;
    BodyView bv{gPos.p, gInvI.p, gVel.p, bRot.p, bCogInvMass.p, shard.enabled ? shard.active.p : nullptr};
    const IslandUpd iu = joints.islandUpd();
    const IslandAcc ia = joints.islandAcc();
    for (uint32_t it = 0; it < iters; it += perLaunch) {
        int rc = profileBegin(); if (rc != MI_OK) return rc;
        L.launch(k_solve_flow_islands, dim3((uint32_t)(per * perLaunch)), dim3(64), 0, stream, it, perLaunch, joints.numIslands, joints.dIslands.p, joints.dSteps.p, joints.dIslandBodies.p, iu, ia, bv, bodyUsed.p,
                                                                               tileDesc.p, slotMeta.p, slotNormal.p, slotMass.p, rows.p, imp.p, scalarsPtr(), a.islandPriv, iters);
        profileEnd();
    }
    return MI_OK;
}
// persistent waves: one workgroup per SIMD owns its tiles through all sweeps, impulses (and, while they fit, the constant slot data) in LDS (k_contact_solve_persist)
int mi_world::solvePersistent(StepAttempt& a) {
    const uint32_t iters = a.settings.num_rigid_solver_iterations, maxSlots = a.persistMaxSlots;
    const bool metaLds = persistMetaLds && maxSlots * (64u * 40u + 4u * 512u + 24u) <= 38u * 1024u;
    usedXcd = a.xcdPlan; usedXcdSingle = a.xcdPlan && a.xcdSingle;
    const uint32_t xcdFault = xcdFaultTest && usedXcd && !xcdFaultFired ? 1u : 0u;   // tests: one workgroup reports a placement mismatch once
    if (xcdFault) xcdFaultFired = true;
    solveLaunches = 1; usedPersist = true;
    int rc = profileBegin(); if (rc != MI_OK) return rc;
    const bool impLds = persistImpLds && maxSlots * (4u * 512u + 24u) <= 38u * 1024u;   // beyond that the impulses travel as granules in `imp` (no size limit)
    const uint32_t ldsMeta = maxSlots * (64u * 40u + 4u * 512u + 24u) + 16u, ldsImp = maxSlots * (4u * 512u + 24u) + 16u, ldsDesc = maxSlots * 24u + 16u;
    // the solve stage IS this launch: its timing events ride on the dispatch (when this path is not taken they are recorded in stageSolve / enqueueStep)
    hipEvent_t e6 = a.attached && timingLevel ? ev[EV_SOLVE_BEGIN] : nullptr, e7 = a.attached && timingLevel ? ev[EV_SOLVE_END] : nullptr;
    a.solveAttached = a.attached;
#ifdef MI_DBG_KNOCKOUT
    if (usedXcd && metaLds && impLds) { int rck = dbgKnockSolve(a, ldsMeta); if (rck != MI_OK) return rck; }
#endif
    // <slot data in LDS, per-XCD tile lists, impulses in LDS>: the six instantiations that exist
    const bool allLds = metaLds && impLds;
    auto* solver = usedXcd ? (allLds ? k_contact_solve_persist<true, true, true> : impLds ? k_contact_solve_persist<false, true, true> : k_contact_solve_persist<false, true, false>)
                           : (allLds ? k_contact_solve_persist<true, false, true> : impLds ? k_contact_solve_persist<false, false, true> : k_contact_solve_persist<false, false, false>);
    L.launchTimed(a.attached, e6, e7, solver, dim3(persistWaves), dim3(64), allLds ? ldsMeta : impLds ? ldsImp : ldsDesc, stream,
                  iters, maxSlots, tileDesc.p, slotMeta.p, slotNormal.p, slotMass.p, rows.p, gVel.p, scalarsPtr(), xcdTiles.p, a.xcdListCap, bodyOwner.p, gVelL.p, slotMeta.p, imp.p, xcdFault, knobs.persistResident ? 1u : 0u);
    profileEnd();
    return MI_OK;
}
// the dispatch-ordered dataflow kernel: no joints between the sweeps -> all sweeps in one launch; otherwise one launch per sweep (joints run in between)
int mi_world::solveFlow(StepAttempt& a) {
    const uint32_t iters = a.settings.num_rigid_solver_iterations, tilesLaunch = a.tilesLaunch;
    hipStream_t st = stream;
    const bool exactSeam = exactSeamStep();   // every sweep ends in an exchange with the neighbours: one launch per sweep
    const uint32_t perLaunch = joints.count() == 0 && !exactSeam && (uint64_t)std::max(tilesLaunch, 1u) * iters < 0x7FFFFFFFull ? iters : 1u;
    solveLaunches = tilesLaunch ? (iters + perLaunch - 1) / perLaunch : 0;
    for (uint32_t it = 0; it < iters; it += perLaunch) {
        if (perLaunch == 1) joints.solveIteration(*this, st);   // the six types in JointSet's order (constraints.cpp:3764-3769)
        if (!tilesLaunch) { if (exactSeam) { int rcx = shardSweepExchange(it); if (rcx != MI_OK) return rcx; } continue; }
        int rc = profileBegin(); if (rc != MI_OK) return rc;
        L.launch(k_contact_solve_flow, dim3(tilesLaunch * perLaunch), dim3(64), 0, st, it, perLaunch, tileDesc.p, slotMeta.p, slotNormal.p, slotMass.p, rows.p, imp.p, gVel.p, scalarsPtr());
        profileEnd();
        if (exactSeam) { int rcx = shardSweepExchange(it); if (rcx != MI_OK) return rcx; }   // exact seam: the owners' velocities of the shared bodies replace the ghost copies
    }
    return MI_OK;
}
// one launch per colour per sweep (MI_SOLVER=launch, or an overflow colour is present); synchronous mode only
int mi_world::solvePerColour(StepAttempt& a) {
    const uint32_t iters = a.settings.num_rigid_solver_iterations;
    hipStream_t st = stream;
    auto colorCount = [&](uint32_t c) { return bins[4 * c].count + bins[4 * c + 1].count + bins[4 * c + 2].count + bins[4 * c + 3].count; };
    // colours [tailStart, tailEnd) are small (<= 512 manifolds each, a suffix of the used colours): one launch for all of them
    if (!a.nmBound) { numColorsUsed = 0; for (BinInfo& b : bins) b.count = 0; }   // no manifolds this step: the mirrored schedule is the previous step's
    uint32_t tailEnd = std::min(numColorsUsed, kOverflowColor), tailStart = tailEnd;
    while (tailStart > 0 && colorCount(tailStart - 1) <= 512u) --tailStart;
    if (tailEnd - tailStart < 2) tailStart = tailEnd;
    std::vector<ColorLaunch> launches(tailStart);
    for (uint32_t c = 0; c < tailStart; ++c) {
        ColorLaunch& cl = launches[c];
        uint32_t acc = 0;
        for (uint32_t k = 0; k < 4; ++k) { cl.tileStart[k] = bins[4 * c + k].tileStart; cl.ctStart[k] = bins[4 * c + k].ctStart; a.mainContacts += (uint64_t)bins[4 * c + k].count * (k + 1); }
        for (uint32_t i = 0; i < 4; ++i) { acc += divUp(bins[4 * c + (3 - i)].count, 64); cl.blockEnd[i] = acc; }
        cl.numBlocks = acc;
    }
    solveLaunches = iters * (tailStart + (tailStart < tailEnd ? 1u : 0u));
    for (uint32_t it = 0; it < iters; ++it) {
        if (debugOrderPending) { int rcj = joints.solveIterationReference(*this, st); if (rcj != MI_OK) return rcj; }
        else joints.solveIteration(*this, st);
        for (uint32_t c = 0; c < tailStart; ++c) {
            const ColorLaunch& cl = launches[c];
            if (!cl.numBlocks) continue;
            int rc = profileBegin(); if (rc != MI_OK) return rc;
            L.launch(k_contact_solve, dim3(cl.numBlocks), dim3(64), 0, st, cl, slotMeta.p, slotNormal.p, slotMass.p, rows.p, imp.p, gVel.p);
            profileEnd();
        }
        if (tailStart < tailEnd) L.launch(k_contact_solve_tail, dim3(1), dim3(256), 0, st, binInfo.p, tailStart, tailEnd, slotMeta.p, slotNormal.p, slotMass.p, rows.p, imp.p, gVel.p);
        if (bins[kSchedBins - 1].count) L.launch(k_contact_solve_serial, dim3(1), dim3(64), 0, st, bins[kSchedBins - 1], slotMeta.p, slotNormal.p, slotMass.p, rows.p, imp.p, gVel.p);
        if (exactSeamStep()) { int rcx = shardSweepExchange(it); if (rcx != MI_OK) return rcx; }
    }
    return MI_OK;
}

// Velocities -> the new body state (the "N" set; nothing persistent is written before this kernel).  Last kernel of the step's time: it carries the stop event.
int mi_world::stageIntegrate(StepAttempt& a) {
    const uint32_t nb = a.nb, B = 256;
    L.launchTimed(a.attached && timesEnds(timingLevel), nullptr, ev[EV_STEP_END], a.blockSkip ? k_integrate_velocities<true> : k_integrate_velocities<false>, dim3(bodyGrid(a, divUp(nb + 1, B))), dim3(B), 0, stream,
                  nb, a.dt, gPos.p, gVel.p, bCogInvMass.p, bRot.p, bPosN.p, bRotN.p, bLinVelN.p, bAngVelN.p, bForceN.p, bTorqueN.p, gVelL.p, usedXcd ? bodyOwner.p : nullptr, bodyUsed.p, bodyTop.p,
                  shard.enabled ? shard.active.p : nullptr, bPos.p, bLinVel.p, bAngVel.p, bForce.p, bTorque.p, shard.activePrev.p, shards.p, scalarsPtr(), a.blockSkip ? shard.blockLive.p : nullptr);
    return MI_OK;
}

// End of step: the one read-back (and, behind it, the next step's first kernel: step-ahead).
int mi_world::stagePublish(StepAttempt& a) {
    const uint32_t nb = a.nb, nc = a.nc;
    StepScalars* sc = scalarsPtr(); hipStream_t st = stream;
    const uint32_t words = (uint32_t)(offsetof(Readback, seq) / 4u);
    if (spinReadback) L.launch(k_publish_readback, dim3(1), dim3(256), 0, st, reinterpret_cast<const uint32_t*>(sc), words, reinterpret_cast<uint32_t*>(hsPinned), words, readbackSeqDev.p,
                               a.fuseResetStep ? sc : nullptr, shards.p, roundFlagsPtr(), keyCount.p);
    else HIP_TRY(L.memcpyAsync(hsPinned, sc, offsetof(Readback, seq), hipMemcpyDeviceToHost, st));   // scalars + round flags are contiguous
    // step-ahead: the next step's k_bp_prepare, on the state this step has just written (the "N" set, current once the step is valid), the grid this step prepared and the
    // axis it chose (read from the device: StepScalars::axisNext survives the reset inside k_publish_readback), into the other set of world-shape / AABB rows
    if (knobs.stepAhead && a.spec && a.pass == PASS_PLAIN && spinReadback && a.fuseResetStep && !shard.enabled && nc && gridValid && knobs.fuseWorld && !a.graphStep && !knobs.debugSync &&
        !timesEnds(timingLevel) && !debugOrderPending && !heightmap && !usesInteractions) {
        HIP_TRY(wShapeAlt.ensure(wShape.cap)); HIP_TRY(aabbMinAlt.ensure(aabbMin.cap)); HIP_TRY(aabbMaxAlt.ensure(aabbMax.cap));
        hipLaunchKernelGGL(k_bp_prepare<false>, dim3(divUp(nc, 256)), dim3(256), 0, st, nc, colliderRows(bPosN.p, bRotN.p, wShapeAlt.p, aabbMinAlt.p, aabbMaxAlt.p), grid.p + (gridCur ^ 1u),
                           axisPartials.p, shards.p, sc, largeList.p, isLarge.p, blockBounds.p, cellKeys.p, cellRanks.p, cellCount.p, 1u, sapAxis, &sc->axisNext, BlockSkip{});
        ++aheadEnqueued;
        ahead.pending = true; ahead.stale = true /* until this step is known to be valid */; ahead.nc = nc; ahead.nb = nb; ahead.gridIdx = gridCur ^ 1u; ahead.pos = bPosN.p; ahead.rot = bRotN.p; ahead.shape = cShape.p; ahead.axis = 0xFFFFFFFFu;
    }
    return MI_OK;
}

// The host's one wait per step: for the sequence number k_publish_readback writes behind the scalars (or for the stream, on the copy path).
int mi_world::awaitReadback() {
    if (spinReadback) {
        const uint32_t seq = readbackSeq + 1u ? readbackSeq + 1u : 1u;   // never 0; the device counts the same way (k_publish_readback)
        readbackSeq = seq;
        volatile uint32_t* flag = &hsPinned->seq;
        const auto t0 = std::chrono::steady_clock::now();
        uint32_t spins = 0;
        while (__atomic_load_n(flag, __ATOMIC_ACQUIRE) != seq) {
            __builtin_ia32_pause();
            if ((++spins & 0xFFFu) == 0u && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(200)) {
                HIP_TRY(hipStreamSynchronize(stream));   // a long step, a device fault or a lost store: let the runtime report it
                if (__atomic_load_n(flag, __ATOMIC_ACQUIRE) != seq) return fail(MI_ERR_DEVICE, "end-of-step read-back did not arrive");
                break;
            }
        }
    } else {
        HIP_TRY(hipStreamSynchronize(stream));
    }
    hs = hsPinned->sc;
    HIP_TRY(hipGetLastError());
    return MI_OK;
}

// Was the attempt valid?  MI_OK, an error, or STEP_RETRY with whatever the next attempt must know already set (nothing persistent has been written: stepInternal
// runs the same step again, synchronously, one rung further down its ladder).
int mi_world::validateStep(StepAttempt& a) {
    scalarsClean = a.fuseResetStep;   // (the publish kernel of THIS attempt cleared the device words for whatever runs next: the next step, or this one again)
    if (a.spec) {
        const uint32_t ovfCount = hs.binStart[kColorBins] - hs.binStart[kSchedBins - 1];
        const bool valid = hs.numPairs <= a.pairBound && hs.numManifolds <= a.nmBound && hs.specOverflow == 0 && hs.colorPending == 0 && ovfCount == 0 &&
                           (!usesInteractions || (hs.numInterPairs <= a.interPairBound && hs.numInteractions <= interList.cap && hs.numInteractions <= 32768u));
        if (hs.tailRounds == kTailTimedOut) colorTailHold = 256u;
        if (!valid) return STEP_RETRY;   // nothing persistent was modified: run the same step synchronously (what ran ahead of the next step stays marked stale)
        mirrorSchedule();
    }
#ifdef MI_DBG_TIMELINE
    { int rct = dbgTimelineDump(); if (rct != MI_OK) return rct; }
#endif
    if (usedXcd && !hs.solveError) {
        // partitioning is only trusted when the eight residue classes of blockIdx really sat on eight DIFFERENT XCDs (a device
        // that exposes fewer XCDs, or hides the id, runs unpartitioned)
        bool distinct = true;
        for (int x = 0; x < 8 && distinct; ++x) for (int y = x + 1; y < 8; ++y) if (hs.xccOf[x] == hs.xccOf[y]) { distinct = false; break; }
        if (!distinct) { persistXcd = false; return STEP_RETRY; }
    }
    if (hs.solveError && usedPersist) {
        // nothing persistent has been written yet, the step is simply run again:
        //   2 with XCD lists: a list outgrew the speculative LDS sizing -> the synchronous run sizes it exactly;
        //   3: blockIdx % 8 does not identify the XCD on this device -> no XCD partitioning from now on;
        //   otherwise: the persistent kernel needs all its workgroups resident at once and the device did not grant that (or
        //   a wait ran out of budget) -> the dispatch-ordered dataflow kernel for good
        if (hs.solveError == 2u && usedXcd && a.spec) { haveXcdEstimate = false; return STEP_RETRY; }
        if (usedXcd) persistXcd = false; else persistSolver = false;
        return STEP_RETRY;
    }
    if (flowFaultTest && !flowFaultFired && a.useFlow && !usedPersist && !hs.solveError) { flowFaultFired = true; hs.solveError = 1u; }   // test injection
    if (hs.solveError && a.useFlow) {
        // the dispatch-ordered kernels rely on workgroups being started in index order on a device that is not shared; when a wait
        // runs out of budget nothing persistent has been written: run the step again with one launch per colour, and stay there a while
        launchFallbackSteps = 256u; ++flowFallbacks;
        return STEP_RETRY;
    }
    if (hs.solveError) return fail(MI_ERR_DEVICE, "contact solver reported an error on the per-colour path");
    return MI_OK;
}

// What a valid step reports besides the new state: the solver profile, trigger enter / leave and collision begin / end events.
int mi_world::collectEvents(StepAttempt& a) {
    const uint32_t B = 256;
    StepScalars* sc = scalarsPtr(); hipStream_t st = stream;
    if (profileSolve) {
        if (a.useFlow) { a.mainContacts = 0; for (uint32_t bn = 0; bn + 1 < kSchedBins; ++bn) a.mainContacts += (uint64_t)bins[bn].count * ((bn & 3u) + 1u); }
        profContacts = a.mainContacts * a.settings.num_rigid_solver_iterations;
        profKernelMs = 0.f;
        for (uint32_t l = 0; l < profLaunches; ++l) profKernelMs += elapsedMs(profEvents[2 * l], profEvents[2 * l + 1]);
    }
    if (a.spec && usesInteractions) {   // the trigger overlaps of this step, from the device-sorted interaction list (force fields were applied in-stream)
        std::vector<DeviceInteraction> list(eventsEnabled ? hs.numInteractions : 0u);
        if (!list.empty()) { HIP_TRY(hipMemcpyAsync(list.data(), interSorted.p, list.size() * sizeof(DeviceInteraction), hipMemcpyDeviceToHost, st)); HIP_TRY(hipStreamSynchronize(st)); }
        int rc = triggerEventsFrom(list, a.triggerEvents); if (rc != MI_OK) return rc;
    }
    if (!eventsEnabled) return MI_OK;
    pendingEvents.insert(pendingEvents.end(), a.triggerEvents.begin(), a.triggerEvents.end());   // handleNonCollisionInteractions runs before the collision events
    if (!a.nmBound && tabValid) {   // no manifolds at all this step: every collision of the previous step ended
        uint32_t cap = last.numManifolds + 1024u;
        HIP_TRY(devEvents.ensure(cap));
        const int nt = tabCur ^ 1;
        HIP_TRY(tab[nt].ensure(1024)); tabMask[nt] = 1023u;
        HIP_TRY(hipMemsetAsync(tab[nt].p, 0, 1024 * sizeof(HistSlot), st));
        hintOf[nt] = hintOf[tabCur] ^ 1; HIP_TRY(histHint[hintOf[nt]].ensure(1024)); HIP_TRY(hipMemsetAsync(histHint[hintOf[nt]].p, 0, 1024 * sizeof(uint32_t), st));
        k_events_end<<<divUp(tabMask[tabCur] + 1u, B), B, 0, st>>>(cap, sc, tab[tabCur].p, tabMask[tabCur], tab[nt].p, tabMask[nt], devEvents.p, histHint[hintOf[nt]].p);
        HIP_TRY(hipMemcpyAsync(hsPinned, sc, offsetof(Readback, seq), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        hs = hsPinned->sc;
    }
    if (hs.numEvents) {
        std::vector<DeviceEvent> ev_(hs.numEvents);
        HIP_TRY(hipMemcpyAsync(ev_.data(), devEvents.p, (size_t)hs.numEvents * sizeof(DeviceEvent), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        std::sort(ev_.begin(), ev_.end(), [](const DeviceEvent& x, const DeviceEvent& y) { return x.colliderA != y.colliderA ? x.colliderA < y.colliderA : x.colliderB < y.colliderB; });
        for (const DeviceEvent& d : ev_) {   // the reference's sorted merge visits the pairs in ascending (a, b) order
            mi_event e{}; e.type = d.type; e.collider_a = d.colliderA; e.collider_b = d.colliderB;
            e.entity_a = colliders[d.colliderA].entity; e.entity_b = colliders[d.colliderB].entity;
            for (int k = 0; k < 3; ++k) { e.point[k] = d.point[k]; e.normal[k] = d.normal[k]; e.relative_velocity[k] = d.relVel[k]; }
            pendingEvents.push_back(e);
        }
    }
    return MI_OK;
}

// The next step's launch sizes derive from the counts of the last valid step; they are kept as snug, STICKY upper bounds (12.5 % granules, unchanged while
// they still fit) so that consecutive steps of a scene in a steady state enqueue identical work — which a captured graph can replay.
static uint32_t stickyBound(uint32_t x, uint32_t prev, uint32_t minGranule) {
    const uint32_t g = std::max(minGranule, (x ? 1u << (31 - __builtin_clz(x)) : 1u) >> 3);
    if (prev >= x && prev - x <= 2u * g) return prev;
    return (x / g + 1u) * g;
}
// The step is valid: the freshly integrated state becomes the current one, its counts the next step's estimates.
void mi_world::commitStep(const StepAttempt& a) {
    const uint32_t nb = a.nb, nc = a.nc;
    bPos.swap(bPosN); bRot.swap(bRotN); bLinVel.swap(bLinVelN); bAngVel.swap(bAngVelN); bForce.swap(bForceN); bTorque.swap(bTorqueN);
    if (usesInteractions) prevTriggerOverlaps.swap(nextTriggerOverlaps);
    sapAxis = hs.axisNext; ahead.axis = hs.axisNext; ahead.stale = false;   // (the step is valid: what ran ahead of the next step ran on the state that is now current)
    if (nc) { gridCur ^= 1u; gridValid = true; gridNextCells = hs.numCellsNext; }   // the grid k_pair_finish prepared becomes the next step's
    if (a.nmBound) { tabCur ^= 1; tabValid = true; } else tabValid = false;
    hostStale = true;
    last.numPairs = stickyBound(hs.numPairs, last.numPairs, 256); last.numManifolds = stickyBound(hs.numManifolds, last.numManifolds, 256);
    last.numContacts = stickyBound(hs.numContacts, last.numContacts, 256); last.numCells = stickyBound(hs.numCells, last.numCells, 1024);
    last.numSmall = stickyBound(nc - std::min(nc, hs.numLarge + hs.numDead), last.numSmall, 256); last.numLarge = stickyBound(hs.numLarge, last.numLarge, 16);
    last.gjkSpan = stickyBound(hs.gjkHi - hs.gjkLo, last.gjkSpan, 256);
    last.numInterPairs = stickyBound(hs.numInterPairs, last.numInterPairs, 256); last.numInteractions = stickyBound(hs.numInteractions, last.numInteractions, 256);
    for (int k = 0; k < 3; ++k) shard.owned[k] = hs.shardOwned[k];
    if (seamMode()) { seamLast[0] = hs.seamStats[0]; seamLast[1] = hs.seamStats[1]; seamViolations += hs.seamStats[2]; }
    shard.flagsSwapPending = shard.enabled; shard.stepOpen = false; shard.flagsOfAStep = shard.enabled;
    haveXcdEstimate = usedXcd; lastXcdSingle = usedXcdSingle;
    if (usedXcd) { uint32_t m = 0; for (int x = 0; x < 8; ++x) m = std::max(m, hs.xcdCount[x]); lastXcdMax = stickyBound(m, lastXcdMax, 16); }
    if (hs.tailRounds) { ++tailSteps; tailRoundsSum += hs.tailRounds; }
    const uint32_t* flagsHost = hsPinned->flags;
    last.colorRounds = 0;
    while (last.colorRounds < 96u && flagsHost[last.colorRounds]) ++last.colorRounds;   // rounds that still had work (+1 to commit) this step
    ++last.colorRounds;
    haveEstimates = true;
    pairsIn = hs.partitioned ? pairKeysS.p : pairKeys.p;
    lastPartitioned = hs.partitioned != 0u; havePartitionFlag = a.pairBound != 0u;

    counts.num_rigid_bodies = nb; counts.num_colliders = nc; counts.num_broadphase_overlaps = nc ? hs.numOverlaps : 0;
#ifdef MI_DBG_BP_COUNT
    fprintf(stderr, "bp_count: candidates tested %u, passed the quantised test %u, AABB overlaps (both passes) %u, small colliders %u\n", hs.reserved14[0], hs.reserved14[1], hs.numOverlaps, nc - hs.numLarge - hs.numDead);
#endif
    manifoldsLast = a.pairBound ? hs.numManifolds : 0;
    counts.num_collisions = manifoldsLast - (manifoldsLast ? hs.numHmManifolds - hs.numHmColliders : 0u);   // terrain: one collision per collider (heightmap_collision.cpp:582-594)
    counts.num_contacts = a.pairBound ? hs.numContacts : 0;
    counts.num_colors = manifoldsLast ? numColorsUsed : 0u /* (a step without manifolds builds no schedule: the mirrored one is an earlier step's) */; counts.sorting_axis = hs.axisCur; counts.reserved = solveLaunches;
    // the step's device times: read from its events LATER (finishTimes), the next step records into the other set
    finishTimes();   // (normally done already, at the start of this step)
    timesPending = timingLevel != 0u; timesPendingSet = evSet; timesPendingLevel = timingLevel; timesPendingUpdates = (uint64_t)counts.num_contacts * a.settings.num_rigid_solver_iterations;
    if (!timesPending) { times = mi_stage_times{}; ++timesSteps; contactUpdatesSum += timesPendingUpdates; }   // timing off: no stale times, and the step / contact-update counts still add up
    evSet ^= 1; ev = evSets[evSet];
}
// (the host gets here after the published read-back of the step the events belong to — but the HIP 7.0 runtime now and then still reports an event
// attached to a kernel as not ready, ~1 step in 1000: elapsedMs waits for it then instead of reporting 0 ms)
void mi_world::finishTimes() {
    if (!timesPending) return;
    timesPending = false;
    hipEvent_t* e = evSets[timesPendingSet];
    auto el = [&](int a, int b) { return elapsedMs(e[a], e[b]); };
    if (timesStages(timesPendingLevel)) {
        times.world_colliders = el(EV_STEP_BEGIN, EV_PREPARED); times.broadphase = el(EV_PREPARED, EV_BROAD); times.narrowphase = el(EV_BROAD, EV_NARROW); times.integrate_forces = el(EV_NARROW, EV_FORCES);
        times.schedule = el(EV_FORCES, EV_SCHEDULE); times.init_constraints = el(EV_SCHEDULE, EV_SOLVE_BEGIN);
    } else { times.world_colliders = times.broadphase = times.narrowphase = times.integrate_forces = times.schedule = times.init_constraints = 0.f; }
    times.solve = el(EV_SOLVE_BEGIN, EV_SOLVE_END);
    if (timesEnds(timesPendingLevel)) { times.integrate_velocities = el(EV_SOLVE_END, EV_STEP_END); times.total = el(EV_STEP_BEGIN, EV_STEP_END); } else times.integrate_velocities = times.total = 0.f;   // (level 3: the step's ends were not timed)
    { float* a = &timesSum.world_colliders; const float* b = &times.world_colliders; for (int i = 0; i < 9; ++i) a[i] += b[i]; ++timesSteps;
      contactUpdatesSum += timesPendingUpdates; }
}

#if defined(MI_DBG_KNOCKOUT) || defined(MI_DBG_TIMELINE)
// ------------------------------------------------------------------------------------------------
// Development builds only (tools/build_variant.py): knock-out launches and the persistent solver's timeline
// ------------------------------------------------------------------------------------------------
#ifdef MI_DBG_KNOCKOUT
// A knock-out site (tools/gpu_knockout.sh) launches one kernel of the step a FIRST time with parts of it removed (g_dbgKnock, kernels.hpp) and whatever it modifies
// redirected to scratch; the real launch behind it starts from untouched data and the step goes on from ITS results.  Device time of the knock-out launches -> knockMsSum / knockLaunches.
int mi_world::dbgKnockWait(KnockSite& s) {   // the previous step's launch of this site
    if (!s.k0) { HIP_TRY(hipEventCreate(&s.k0)); HIP_TRY(hipEventCreate(&s.k1)); }
    if (s.pending) { HIP_TRY(hipEventSynchronize(s.k1)); float ms = 0.f; if (hipEventElapsedTime(&ms, s.k0, s.k1) == hipSuccess && timingLevel >= 2u) { knockMsSum += ms; ++knockLaunches; } s.pending = false; }   // (counted while the caller times steps: mi_world_set_stage_timing)
    return MI_OK;
}
template <class F> int mi_world::dbgKnockLaunch(KnockSite& s, uint32_t word, F&& launch) {
    s.word = word;
    HIP_TRY(hipMemcpyToSymbolAsync(HIP_SYMBOL(g_dbgKnock), &s.word, sizeof(s.word), 0, hipMemcpyHostToDevice, stream));
    (void)hipEventRecord(s.k0, stream);
    launch();
    (void)hipEventRecord(s.k1, stream);
    HIP_TRY(hipMemcpyToSymbolAsync(HIP_SYMBOL(g_dbgKnock), &knockZero, sizeof(knockZero), 0, hipMemcpyHostToDevice, stream));
    s.pending = true;
    return MI_OK;
}
// the grid part of the pair pass, on a scratch pair list and scratch counters (g_dbgKnock bits 16-18)
int mi_world::dbgKnockBroad(uint32_t bpc, uint32_t cap, GridParams* gridUse) {
    if (!(knobs.knockout >> 16) || L.dry) return MI_OK;
    hipStream_t st = stream;
    int rc = dbgKnockWait(knockBp); if (rc != MI_OK) return rc;
    HIP_TRY(knockPairs.ensure(pairKeys.cap)); HIP_TRY(knockSc.ensure(sizeof(StepScalars))); HIP_TRY(knockSh.ensure(sizeof(Shards)));
    HIP_TRY(hipMemcpyAsync(knockSc.p, scalarsPtr(), sizeof(StepScalars), hipMemcpyDeviceToDevice, st)); HIP_TRY(hipMemsetAsync(knockSh.p, 0, sizeof(Shards), st));
    const uint32_t word = (knobs.knockout >> 16) >= 0x80u ? 0u : (knobs.knockout & 0xFF0000u);   // (0x800000: nothing removed)
    return dbgKnockLaunch(knockBp, word, [&]() {
        hipLaunchKernelGGL(k_bp_pairs_grid, dim3(5u * bpc), dim3(256), 0, st, (uint32_t)colliders.size(), bpc, cellKeysS.p, sRow.p, sMin.p, sMax.p, cellLower.p, gridUse, knockPairs.p, cap, reinterpret_cast<StepScalars*>(knockSc.p), reinterpret_cast<Shards*>(knockSh.p), InterSink{nullptr, 0u, nullptr});
    });
}
// k_emit_manifolds (g_dbgKnock bits 8-12), its read-modify-write targets (per-body colour masks, the next history table, round-0 proposals, round flags) redirected
// to scratch; everything else it writes the real launch behind it writes again.
int mi_world::dbgKnockEmit(const StepAttempt& a) {
    if (!((knobs.knockout >> 8) & 0xFFu) || L.dry || !tabValid) return MI_OK;
    const uint32_t nb = a.nb, nc = a.nc, B = 256;
    hipStream_t st = stream;
    int rc = dbgKnockWait(knockEmit); if (rc != MI_OK) return rc;
    HIP_TRY(knockUsed.ensure(bodyUsed.cap)); HIP_TRY(knockTop.ensure(bodyTop.cap)); HIP_TRY(knockTab.ensure(tab[tabCur ^ 1].cap)); HIP_TRY(knockFlags.ensure(64));
    HIP_TRY(hipMemsetAsync(knockUsed.p, 0, knockUsed.cap * 8, st)); HIP_TRY(hipMemsetAsync(knockTab.p, 0, knockTab.cap * sizeof(HistSlot), st)); HIP_TRY(hipMemsetAsync(knockTop.p, 0, knockTop.cap * 8, st));
    const uint32_t word = ((knobs.knockout >> 8) & 0xFFu) >= 0x80u ? 0u : (knobs.knockout & 0xFF00u);   // (0x8000: nothing removed = the harness itself)
    return dbgKnockLaunch(knockEmit, word, [&]() {
        hipLaunchKernelGGL(k_emit_manifolds, dim3(divUp(a.pairBound, B)), dim3(B), 0, st, nc, nb, pairKeys.p, pairKeysS.p, npPacked.p, npScan.p, cEmit.p,
                           manPair.p, manBodies.p, manInfo.p, colWork.p, color.p, tab[tabCur].p, tabMask[tabCur], knockUsed.p, eventsEnabled ? manIsNew.p : nullptr, scalarsPtr(),
                           heightmap ? make_float2(hmParams.restitution, hmParams.friction) : make_float2(0.f, 0.f), knockTab.p, tabMask[tabCur ^ 1], manKept.p, histHint[hintOf[tabCur]].p, histHint[hintOf[tabCur ^ 1]].p /* (a fresh insertion may raise a hint: harmless, they only ever grow) */,
                           a.seamOn ? seamId.p : nullptr, emitsRound0() ? knockTop.p + (nb + 1) : nullptr, knockFlags.p);
    });
}
// the persistent solver (all-LDS, XCD-partitioned variant) on scratch copies of the velocity arrays, with parts of the tile visit removed
int mi_world::dbgKnockSolve(const StepAttempt& a, uint32_t ldsMeta) {
    if (!(knobs.knockout & 0xFFu) || L.dry) return MI_OK;
    hipStream_t st = stream;
    int rc = dbgKnockWait(knockSolve); if (rc != MI_OK) return rc;
    knockVel.flags = gVel.flags;
    HIP_TRY(knockVel.ensure(gVel.cap)); HIP_TRY(knockVelL.ensure(gVelL.cap));
    HIP_TRY(hipMemcpyAsync(knockVel.p, gVel.p, gVel.cap * sizeof(float4), hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(knockVelL.p, gVelL.p, gVelL.cap * sizeof(float4), hipMemcpyDeviceToDevice, st));
#ifdef MI_DBG_TIMELINE
    dbgTimelineKnock = dbgTimelineBuf ? dbgTimelineBuf + (size_t)persistWaves * 256 * 8 : nullptr;   // (the knock-out launch stamps into the second half)
    if (dbgTimelineBuf) HIP_TRY(hipMemcpyToSymbolAsync(HIP_SYMBOL(g_dbgTimeline), &dbgTimelineKnock, sizeof(dbgTimelineKnock), 0, hipMemcpyHostToDevice, st));
#endif
    const uint32_t word = (knobs.knockout & 0xFFu) >= 8u ? 0u : (knobs.knockout & 0xFFu);   // (8: the unmodified kernel through the harness — what the harness itself costs)
    rc = dbgKnockLaunch(knockSolve, word, [&]() {
        hipLaunchKernelGGL((k_contact_solve_persist<true, true, true>), dim3(persistWaves), dim3(64), ldsMeta, st,
                           a.settings.num_rigid_solver_iterations, a.persistMaxSlots, tileDesc.p, slotMeta.p, slotNormal.p, slotMass.p, rows.p, knockVel.p, scalarsPtr(), xcdTiles.p, a.xcdListCap, bodyOwner.p, knockVelL.p, slotMeta.p, imp.p, 0u, knobs.persistResident ? 1u : 0u);
    });
    if (rc != MI_OK) return rc;
#ifdef MI_DBG_TIMELINE
    if (dbgTimelineBuf) HIP_TRY(hipMemcpyToSymbolAsync(HIP_SYMBOL(g_dbgTimeline), &dbgTimelineBuf, sizeof(dbgTimelineBuf), 0, hipMemcpyHostToDevice, st));
#endif
    return MI_OK;
}
#endif
#ifdef MI_DBG_TIMELINE
// per-visit wall-clock stamps of the persistent solver, dumped after step MI_DBG_TIMELINE_STEP (tools/gpu_timeline2.sh, tools/visit_stamps.py)
int mi_world::dbgTimelineDump() {
    if (!usedPersist || knobs.timelineOut.empty()) return MI_OK;
    const size_t words = (size_t)persistWaves * 256 * 8;      // (second half: the stamps of the knock-out launch of a -DMI_DBG_KNOCKOUT build)
    if (dbgTimelineBuf && totalSteps == (unsigned long long)knobs.timelineStep) {
        std::vector<unsigned long long> h(2 * words);
        HIP_TRY(hipMemcpy(h.data(), dbgTimelineBuf, 2 * words * 8, hipMemcpyDeviceToHost));
        FILE* f = fopen(knobs.timelineOut.c_str(), "wb"); if (f) { fwrite(h.data(), 8, words, f); fclose(f); }
        f = fopen((knobs.timelineOut + ".knock").c_str(), "wb"); if (f) { fwrite(h.data() + words, 8, words, f); fclose(f); }
    }
    if (!dbgTimelineBuf) {
        HIP_TRY(hipMalloc(&dbgTimelineBuf, 2 * words * 8)); HIP_TRY(hipMemset(dbgTimelineBuf, 0, 2 * words * 8));
        HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_dbgTimeline), &dbgTimelineBuf, sizeof(dbgTimelineBuf)));
    }
    return MI_OK;
}
#endif
#endif

// mi_debug_set_solve_order, inside a synchronous step after the manifolds are known (hs = this step's counts): every manifold is given the
// sequential colour (kOverflowColor: one lane solves that bin slot by slot), and its rank in the caller's list is remembered for the slot order.
int mi_world::applyDebugOrder() {
    const uint32_t nm = hs.numManifolds;
    if (nm != debugOrder.size()) return fail(MI_ERR_INVALID_ARGUMENT, "mi_debug_set_solve_order: the step found " + std::to_string(nm) + " contact manifolds, the list holds " + std::to_string(debugOrder.size()));
    debugRank.assign(nm, 0u);
    if (!nm) return MI_OK;
    std::vector<uint32_t> mp(nm), col(nm, kOverflowColor);
    HIP_TRY(hipMemcpyAsync(mp.data(), manPair.p, nm * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    std::vector<uint64_t> keys(hs.numPairs);
    HIP_TRY(hipMemcpyAsync(keys.data(), hs.partitioned ? pairKeysS.p : pairKeys.p, keys.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    std::unordered_map<uint64_t, uint32_t> rank; rank.reserve(2 * (size_t)nm);
    for (uint32_t i = 0; i < nm; ++i) if (!rank.emplace(debugOrder[i], i).second) return fail(MI_ERR_INVALID_ARGUMENT, "mi_debug_set_solve_order: a collider pair is listed twice");
    for (uint32_t m = 0; m < nm; ++m) {
        if (mp[m] >= keys.size()) return fail(MI_ERR_DEVICE, "mi_debug_set_solve_order: manifold without a pair");
        const uint64_t k = keys[mp[m]] & ((1ull << 58) - 1ull);   // (bucket bits dropped: a << 29 | b)
        auto it = rank.find(k);
        if (it == rank.end()) return fail(MI_ERR_INVALID_ARGUMENT, "mi_debug_set_solve_order: the step found a contact manifold (colliders " + std::to_string(k >> 29) + ", " + std::to_string(k & 0x1FFFFFFFull) + ") that is not in the list");
        debugRank[m] = it->second;
    }
    debugOrderLevelled = false;
    if (debugOrderDataflow && joints.count() == 0) {
        // mi_debug_set_solve_dataflow: the caller's order through the PRODUCTION solver.  A manifold's colour = its level in the order's dependency graph (1 + the highest
        // level among the earlier manifolds of its two bodies): manifolds of one level share no dynamic body, and along every body the levels ascend in the caller's
        // order — so the colour-major dataflow schedule (bins, tiles, k_contact_init's version bookkeeping from the per-body colour masks, the persistent kernel's
        // processTile) performs exactly the caller's sequence of updates on every body, i.e. the caller's sequential result, bit for bit.  Orders deeper than the 64
        // colours (large scenes: 160-265 levels at 16 384 bodies) keep the sequential kernel.
        std::vector<uint2> mb(nm);
        HIP_TRY(hipMemcpy(mb.data(), manBodies.p, nm * sizeof(uint2), hipMemcpyDeviceToHost));
        std::vector<uint4> cw(nm);
        HIP_TRY(hipMemcpy(cw.data(), colWork.p, nm * sizeof(uint4), hipMemcpyDeviceToHost));
        const uint32_t nb = (uint32_t)bodies.size();
        std::vector<uint32_t> byRank(nm); for (uint32_t m = 0; m < nm; ++m) byRank[debugRank[m]] = m;
        std::vector<uint32_t> top(nb + 1, 0u); std::vector<unsigned long long> used(nb + 1, 0ull);
        uint32_t depth = 0;
        for (uint32_t r = 0; r < nm; ++r) {
            const uint32_t m = byRank[r];
            const bool dynA = (cw[m].x & 0x80000000u) != 0u, dynB = (cw[m].y & 0x80000000u) != 0u;
            const uint32_t a = mb[m].x, b = mb[m].y;
            const uint32_t lvl = std::max(dynA ? top[a] : 0u, dynB ? top[b] : 0u);
            col[m] = lvl; depth = std::max(depth, lvl + 1u);
            if (dynA) top[a] = lvl + 1u;
            if (dynB) top[b] = lvl + 1u;
        }
        if (depth <= kOverflowColor) {
            for (uint32_t m = 0; m < nm; ++m) {
                if (cw[m].x & 0x80000000u) used[mb[m].x] |= 1ull << col[m];
                if (cw[m].y & 0x80000000u) used[mb[m].y] |= 1ull << col[m];
            }
            HIP_TRY(hipMemcpy(bodyUsed.p, used.data(), (nb + 1) * sizeof(unsigned long long), hipMemcpyHostToDevice));
            debugOrderLevelled = true; debugOrderDepth = depth;
        } else std::fill(col.begin(), col.end(), kOverflowColor);
    }
    HIP_TRY(hipMemcpyAsync(color.p, col.data(), nm * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return MI_OK;
}
// mi_debug_set_solve_order also ORIENTS: a pair of equal shape type whose AABB starts tie exactly on the sweep axis is oriented by the reference
// according to the history of its persistent, stably sorted endpoint array (collision_broad.cpp:386-398) — no rule of the current state reproduces
// that, the canonical rule (later created = new) is only the first frame's.  Synchronous step, right after the pair pass: pairs that the list holds
// the other way round (and not this way) are turned before the narrow phase sees them.
int mi_world::orientPairsLikeDebugOrder() {
    const uint32_t np = hs.numPairs;
    if (!np || debugOrder.empty()) return MI_OK;
    std::vector<uint64_t> keys(np);
    HIP_TRY(hipMemcpyAsync(keys.data(), pairKeys.p, (size_t)np * sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    std::unordered_map<uint64_t, uint32_t> listed; listed.reserve(2 * debugOrder.size());
    for (uint64_t k : debugOrder) listed.emplace(k, 0u);
    bool turned = false;
    for (uint64_t& k : keys) {
        const uint64_t bucket = k >> 58, a = (k >> 29) & 0x1FFFFFFFull, b = k & 0x1FFFFFFFull;
        uint32_t ta = 0, rem = (uint32_t)bucket; while (rem >= 6u - ta) { rem -= 6u - ta; ++ta; }
        if (rem != 0u) continue;                                      // different shape types: ordered by type on both sides
        if (!listed.count((a << 29) | b) && listed.count((b << 29) | a)) { k = (bucket << 58) | (b << 29) | a; turned = true; }
    }
    if (turned) { HIP_TRY(hipMemcpyAsync(pairKeys.p, keys.data(), (size_t)np * sizeof(uint64_t), hipMemcpyHostToDevice, stream)); HIP_TRY(hipStreamSynchronize(stream)); }
    return MI_OK;
}
extern "C" {
MI_API int mi_debug_set_sweep_axis(mi_world* w, uint32_t axis) {
    if (!w || axis > 2u) return fail(MI_ERR_INVALID_ARGUMENT, "axis 0 | 1 | 2");
    w->sapAxis = axis;
    if (w->shard.enabled && w->shard.axisDev.p) { HIP_TRY(hipSetDevice(w->device)); HIP_TRY(hipMemcpy(w->shard.axisDev.p, &axis, sizeof(uint32_t), hipMemcpyHostToDevice)); w->shard.axisHostCurrent = true; }
    return MI_OK;
}
MI_API int mi_debug_set_solve_order(mi_world* w, const uint32_t* pairs, uint32_t count) {
    if (!w || (count && !pairs)) return fail(MI_ERR_INVALID_ARGUMENT, "null");
    if (w->heightmap || w->shard.enabled) return fail(MI_ERR_UNSUPPORTED, "mi_debug_set_solve_order: not with heightmap terrain or sharding");   // (here, not in the step: a pending order would fail every later step)
    w->debugOrder.resize(count);
    for (uint32_t i = 0; i < count; ++i) {
        if (pairs[2 * i] >= (1u << 29) || pairs[2 * i + 1] >= (1u << 29)) return fail(MI_ERR_INVALID_ARGUMENT, "collider index out of range");
        w->debugOrder[i] = ((uint64_t)pairs[2 * i] << 29) | (uint64_t)pairs[2 * i + 1];
    }
    w->debugOrderPending = true;
    return MI_OK;
}
MI_API int mi_debug_set_solve_dataflow(mi_world* w, uint32_t enable) {
    if (!w) return fail(MI_ERR_INVALID_ARGUMENT, "null");
    w->debugOrderDataflow = enable != 0u;
    return MI_OK;
}
MI_API int mi_debug_solve_order_depth(mi_world* w, uint32_t* out_depth) {
    if (!w || !out_depth) return fail(MI_ERR_INVALID_ARGUMENT, "null");
    *out_depth = w->debugOrderDepthLast;
    return MI_OK;
}
}


// Host mirror of the device schedule (bins -> tiles), from the binStart table read back in StepScalars.
void mi_world::mirrorSchedule() {
    numColorsUsed = 0;
    uint32_t tiles = 0, ct = 0;
    for (uint32_t bn = 0; bn < kSchedBins; ++bn) {
        bool ovf = bn == kSchedBins - 1;
        uint32_t s0 = hs.binStart[bn], s1 = ovf ? hs.binStart[kColorBins] : hs.binStart[bn + 1];
        uint32_t stride = ovf ? 4u : (bn & 3u) + 1u;
        BinInfo bi{s0, s1 - s0, tiles, ct};
        uint32_t nt = divUp(bi.count, 64);
        tiles += nt; ct += nt * stride;
        bins[bn] = bi;
        if (bi.count) numColorsUsed = std::max(numColorsUsed, (ovf ? kOverflowColor : bn / 4u) + 1u);
    }
    totalTiles = tiles;
}
