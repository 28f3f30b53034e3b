// Part of world.hip (one translation unit; #included there, in this order): the C ABI of include/mi_physics.h and include/mi_constraints.h.

// ================================================================================================
// C ABI
// ================================================================================================
extern "C" {

MI_API const char* mi_last_error(void) { return g_lastError.c_str(); }
MI_API int mi_version(void) { return 1; }

MI_API int mi_world_create(const mi_world_desc* desc, mi_world** out) {
    if (!out) return fail(MI_ERR_INVALID_ARGUMENT, "out_world is null");
    mi_world* w = new mi_world();
    int rc = w->init(desc ? desc->device : 0);
    if (rc != MI_OK) { delete w; *out = nullptr; return rc; }
    *out = w;
    return MI_OK;
}
MI_API void mi_world_destroy(mi_world* w) {
#ifdef MI_DBG_KNOCKOUT
    if (w && w->knockLaunches) fprintf(stderr, "knockout %u: %u launches, mean %.2f us\n", w->knobs.knockout, w->knockLaunches, w->knockMsSum * 1e3 / w->knockLaunches);
#endif
    delete w;
}

MI_API int mi_entities_create(mi_world* w, uint32_t count, const mi_entity_desc* descs, uint32_t* out_first) {
    if (!w || (count && !descs)) return fail(MI_ERR_INVALID_ARGUMENT, "null argument");
    int rc = w->download(); if (rc != MI_OK) return rc;
    if (out_first) *out_first = (uint32_t)w->entities.size();
    for (uint32_t i = 0; i < count; ++i) {
        const mi_entity_desc& d = descs[i];
        HEntity e; e.pos = V3(d.position[0], d.position[1], d.position[2]); e.rot = Q4(d.rotation[0], d.rotation[1], d.rotation[2], d.rotation[3]); e.kind = d.kind;
        if (d.kind > MI_ENTITY_FORCE_FIELD) return fail(MI_ERR_INVALID_ARGUMENT, "bad entity kind");
        if (d.kind == MI_ENTITY_FORCE_FIELD) { e.kindIndex = (uint32_t)w->ffEntities.size(); w->ffEntities.push_back((uint32_t)w->entities.size()); }
        if (d.kind == MI_ENTITY_TRIGGER) { e.kindIndex = (uint32_t)w->triggerEntities.size(); w->triggerEntities.push_back((uint32_t)w->entities.size()); }
        if (d.kind == MI_ENTITY_DYNAMIC || d.kind == MI_ENTITY_KINEMATIC) {
            HBody b;
            b.entity = (uint32_t)w->entities.size();
            bool kin = d.kind == MI_ENTITY_KINEMATIC;   // rigid_body_component ctor, rigid_body.cpp:6-27
            b.invMass = kin ? 0.f : 1.f; b.invInertia = kin ? M3::zero() : M3::identity();
            b.gravityFactor = d.gravity_factor; b.linDamp = d.linear_damping; b.angDamp = d.angular_damping;
            b.linVel = V3(d.linear_velocity[0], d.linear_velocity[1], d.linear_velocity[2]);
            b.angVel = V3(d.angular_velocity[0], d.angular_velocity[1], d.angular_velocity[2]);
            b.p0 = b.p1 = e.pos; b.r0 = b.r1 = e.rot;
            e.rb = (int)w->bodies.size();
            w->bodies.push_back(b);
        }
        w->entities.push_back(e);
    }
    w->topologyDirty = true;
    return MI_OK;
}
MI_API int mi_entity_create(mi_world* w, const mi_entity_desc* d, uint32_t* out) { return mi_entities_create(w, 1, d, out); }
// game_scene::deleteEntity — src/scene/scene.cpp:124-150.  Host-side pool bookkeeping with EnTT's swap-and-pop (the LAST collider /
// rigid body / trigger / force field moves into the freed slot: world indices follow the pools, so the order downstream stages
// see changes exactly like the reference's); the scene is re-uploaded before the next step.  The colour history and the previous
// collision / trigger-overlap lists are keyed by pool positions and restart.
MI_API int mi_entity_destroy(mi_world* w, uint32_t entity) {
    if (!w || entity >= w->entities.size() || w->entities[entity].kind == MI_ENTITY_DESTROYED) return fail(MI_ERR_INVALID_ARGUMENT, "bad entity");
    int rc = w->download(); if (rc != MI_OK) return rc;
    const size_t mine = w->entities[entity].colliders.size();
    for (size_t k = 0; k < mine; ++k) {                       // the entity's colliders, newest first (removeColliderFromBroadphase + destroy)
        HEntity& e = w->entities[entity];
        const uint32_t id = e.colliders[0], last = (uint32_t)w->colliders.size() - 1u;
        e.colliders.erase(e.colliders.begin());
        if (id != last) {
            w->colliders[id] = w->colliders[last];
            for (uint32_t& c : w->entities[w->colliders[id].entity].colliders) if (c == last) c = id;
        }
        w->colliders.pop_back();
    }
    w->joints.destroyOfEntity(entity);                         // deleteAllConstraintsFromEntity
    HEntity& e = w->entities[entity];
    if (e.rb >= 0) {
        const uint32_t p = (uint32_t)e.rb, last = (uint32_t)w->bodies.size() - 1u;
        if (p != last) {
            w->bodies[p] = w->bodies[last]; w->entities[w->bodies[p].entity].rb = (int)p;
            // the reference derives body pairs from the entities every step (physics.cpp:789-806): re-point the cached ones
            w->joints.each([&](uint32_t, auto& t) { for (uint2& b : t.bodies) { if (b.x == last) b.x = p; if (b.y == last) b.y = p; } });
        }
        w->bodies.pop_back();
    }
    auto dropFrom = [&](std::vector<uint32_t>& pool) {
        const uint32_t p = e.kindIndex, last = (uint32_t)pool.size() - 1u;
        if (p != last) { pool[p] = pool[last]; w->entities[pool[p]].kindIndex = p; }
        pool.pop_back();
    };
    if (e.kind == MI_ENTITY_TRIGGER) dropFrom(w->triggerEntities);
    if (e.kind == MI_ENTITY_FORCE_FIELD) dropFrom(w->ffEntities);
    e.kind = MI_ENTITY_DESTROYED; e.rb = -1; e.colliders.clear(); e.pos = V3(0.f, 0.f, 0.f); e.rot = Q4(0.f, 0.f, 0.f, 1.f);
    w->tabValid = false; w->prevTriggerOverlaps.clear();
    w->topologyDirty = true; w->haveEstimates = false;
    return MI_OK;
}
// ---- cloth (cloth_component, src/physics/cloth.h:5-60)
static V3 clothParticlePosition(const mi_cloth_desc& d, float relX, float relY) {   // getParticlePosition, cloth.cpp:126-132
    V3 p(relX * d.width, -relY * d.height, 0.f);
    p.x -= d.width * 0.5f;
    float t = p.y; p.y = p.z; p.z = t;
    return p;
}
MI_API int mi_cloth_create(mi_world* w, const mi_cloth_desc* d, uint32_t* out) {   // cloth_component ctor, cloth.cpp:7-85
    if (!w || !d) return fail(MI_ERR_INVALID_ARGUMENT, "null argument");
    if (d->grid_size_x < 2 || d->grid_size_y < 2 || !(d->total_mass > 0.f) || !(d->stiffness > 0.f)) return fail(MI_ERR_INVALID_ARGUMENT, "bad cloth description");
    HIP_TRY(hipSetDevice(w->device));
    mi_world::HCloth* c = new mi_world::HCloth();
    c->desc = *d; c->oldTotalMass = d->total_mass; c->oldStiffness = d->stiffness;
    const uint32_t gx = d->grid_size_x, gy = d->grid_size_y, n = gx * gy;
    const float invMassPerParticle = (float)n / d->total_mass;
    std::vector<float4> pos(n);
    c->invMasses.resize(n);
    for (uint32_t y = 0; y < gy; ++y)
        for (uint32_t x = 0; x < gx; ++x) {
            const float im = (y == 0) ? 0.f : invMassPerParticle;   // upper row locked
            V3 p = clothParticlePosition(*d, (float)x / (float)(gx - 1), (float)y / (float)(gy - 1));
            pos[y * gx + x] = make_float4(p.x, p.y, p.z, im); c->invMasses[y * gx + x] = im;
        }
    std::vector<uint32_t> colours;
    auto add = [&](uint32_t a, uint32_t b, uint32_t colour) {
        V3 d_ = V3(pos[a].x, pos[a].y, pos[a].z) - V3(pos[b].x, pos[b].y, pos[b].z);
        c->pairs.push_back(make_uint2(a, b));
        c->restInvMass.push_back(make_float2(len(d_), (c->invMasses[a] + c->invMasses[b]) / d->stiffness));
        colours.push_back(colour);
    };
    for (uint32_t y = 0; y < gy; ++y)
        for (uint32_t x = 0; x < gx; ++x) {   // creation order of cloth.cpp:46-80; colour = family x parity (cloth.hpp)
            const uint32_t i = y * gx + x;
            if (x < gx - 1) add(i, i + 1, 0 + (x & 1u));
            if (y < gy - 1) add(i, i + gx, 2 + (y & 1u));
            if (x < gx - 1 && y < gy - 1) { add(i, i + gx + 1, 4 + (x & 1u)); add(i + gx, i + 1, 6 + (x & 1u)); }
            if (x < gx - 2) add(i, i + 2, 8 + ((x >> 1) & 1u));
            if (y < gy - 2) add(i, i + gx * 2, 10 + ((y >> 1) & 1u));
        }
    const uint32_t nc = (uint32_t)c->pairs.size();
    c->order.resize(nc);
    for (uint32_t k = 0; k < nc; ++k) c->order[k] = k;
    std::stable_sort(c->order.begin(), c->order.end(), [&](uint32_t a, uint32_t b) { return colours[a] < colours[b]; });
    std::memset(c->colourOffsets, 0, sizeof(c->colourOffsets));
    for (uint32_t k = 0; k < nc; ++k) c->colourOffsets[colours[k] + 1]++;
    for (int k = 0; k < 12; ++k) c->colourOffsets[k + 1] += c->colourOffsets[k];
    int rc = MI_OK;
    auto up = [&]() -> int {
        HIP_TRY(c->pos.ensure(n)); HIP_TRY(c->prev.ensure(n)); HIP_TRY(c->vel.ensure(n)); HIP_TRY(c->force.ensure(n)); HIP_TRY(c->temp.ensure(nc));
        HIP_TRY(c->dPairs.ensure(nc)); HIP_TRY(c->dRestInvMass.ensure(nc)); HIP_TRY(c->dOrder.ensure(nc));
        HIP_TRY(hipMemcpy(c->pos.p, pos.data(), n * sizeof(float4), hipMemcpyHostToDevice)); HIP_TRY(hipMemcpy(c->prev.p, pos.data(), n * sizeof(float4), hipMemcpyHostToDevice));
        HIP_TRY(hipMemset(c->vel.p, 0, n * sizeof(float4))); HIP_TRY(hipMemset(c->force.p, 0, n * sizeof(float4)));
        HIP_TRY(hipMemcpy(c->dPairs.p, c->pairs.data(), nc * sizeof(uint2), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(c->dOrder.p, c->order.data(), nc * sizeof(uint32_t), hipMemcpyHostToDevice));
        return MI_OK;
    };
    rc = up();
    if (rc != MI_OK) { delete c; return rc; }
    if (out) *out = (uint32_t)w->cloths.size();
    w->cloths.push_back(c); w->clothsDirty = true;
    return MI_OK;
}
MI_API int mi_cloth_set_fixed_vertices(mi_world* w, uint32_t cloth, const float* p3, const float* r4, uint32_t moveRigid) {   // cloth.cpp:87-124
    if (!w || cloth >= w->cloths.size() || !p3 || !r4) return fail(MI_ERR_INVALID_ARGUMENT, "bad cloth / null argument");
    HIP_TRY(hipSetDevice(w->device));
    mi_world::HCloth& c = *w->cloths[cloth];
    const uint32_t gx = c.desc.grid_size_x, gy = c.desc.grid_size_y, n = gx * gy;
    std::vector<float4> pos(n);
    HIP_TRY(hipStreamSynchronize(w->stream));
    HIP_TRY(hipMemcpy(pos.data(), c.pos.p, n * sizeof(float4), hipMemcpyDeviceToHost));
    const V3 tp(p3[0], p3[1], p3[2]); const Q4 tr(r4[0], r4[1], r4[2], r4[3]);
    auto xf = [&](V3 p) { return rotate(tr, p) + tp; };
    auto at = [&](uint32_t i) { return V3(pos[i].x, pos[i].y, pos[i].z); };
    if (moveRigid) {
        V3 pivot = (gx % 2 == 1) ? at(gx / 2) : (at(gx / 2) + at(gx / 2 - 1)) * 0.5f;
        V3 currentAxis = normalize(at(gx - 1) - at(0));
        V3 newAxis = normalize(xf(clothParticlePosition(c.desc, 1.f, 0.f)) - xf(clothParticlePosition(c.desc, 0.f, 0.f)));
        V3 newPivot = xf(clothParticlePosition(c.desc, 0.5f, 0.f));
        Q4 deltaRotation = rotateFromTo(currentAxis, newAxis);
        for (uint32_t y = 1; y < gy; ++y)
            for (uint32_t x = 0; x < gx; ++x) { V3 q = rotate(deltaRotation, at(y * gx + x) - pivot) + newPivot; float4& o = pos[y * gx + x]; o.x = q.x; o.y = q.y; o.z = q.z; }
    }
    for (uint32_t x = 0; x < gx; ++x) { V3 q = xf(clothParticlePosition(c.desc, (float)x / (float)(gx - 1), 0.f)); pos[x].x = q.x; pos[x].y = q.y; pos[x].z = q.z; }
    HIP_TRY(hipMemcpy(c.pos.p, pos.data(), n * sizeof(float4), hipMemcpyHostToDevice));
    return MI_OK;
}
MI_API int mi_cloth_set_properties(mi_world* w, uint32_t cloth, float totalMass, float stiffness, float damping, float gravityFactor) {
    if (!w || cloth >= w->cloths.size()) return fail(MI_ERR_INVALID_ARGUMENT, "bad cloth");
    mi_cloth_desc& d = w->cloths[cloth]->desc;
    d.total_mass = totalMass; d.stiffness = stiffness; d.damping = damping; d.gravity_factor = gravityFactor;
    w->clothsDirty = true;
    return MI_OK;
}
MI_API int mi_cloth_get_state(mi_world* w, uint32_t cloth, float* outPos, float* outVel, uint32_t cap) {
    if (!w || cloth >= w->cloths.size()) return fail(MI_ERR_INVALID_ARGUMENT, "bad cloth");
    HIP_TRY(hipSetDevice(w->device));
    mi_world::HCloth& c = *w->cloths[cloth];
    const uint32_t n = c.desc.grid_size_x * c.desc.grid_size_y;
    if (cap < n) return fail(MI_ERR_CAPACITY, "capacity < particles");
    std::vector<float4> buf(n);
    HIP_TRY(hipStreamSynchronize(w->stream));
    if (outPos) { HIP_TRY(hipMemcpy(buf.data(), c.pos.p, n * sizeof(float4), hipMemcpyDeviceToHost)); for (uint32_t i = 0; i < n; ++i) { outPos[3 * i] = buf[i].x; outPos[3 * i + 1] = buf[i].y; outPos[3 * i + 2] = buf[i].z; } }
    if (outVel) { HIP_TRY(hipMemcpy(buf.data(), c.vel.p, n * sizeof(float4), hipMemcpyDeviceToHost)); for (uint32_t i = 0; i < n; ++i) { outVel[3 * i] = buf[i].x; outVel[3 * i + 1] = buf[i].y; outVel[3 * i + 2] = buf[i].z; } }
    return MI_OK;
}
MI_API int mi_world_set_cloth_iterations(mi_world* w, uint32_t v, uint32_t p, uint32_t d) {
    if (!w) return fail(MI_ERR_INVALID_ARGUMENT, "null");
    w->clothIterations[0] = v; w->clothIterations[1] = p; w->clothIterations[2] = d;
    return MI_OK;
}

// ---- heightmap terrain (heightmap_collider_component, src/terrain/heightmap_collider.h:126-151)
MI_API int mi_heightmap_create(mi_world* w, uint32_t chunksPerDim, float chunkSize, float restitution, float friction) {
    if (!w || !chunksPerDim || !(chunkSize > 0.f)) return fail(MI_ERR_INVALID_ARGUMENT, "bad heightmap parameters");
    if (w->heightmap) return fail(MI_ERR_INVALID_ARGUMENT, "a world holds one heightmap");
    if (w->colliders.size() >= kHeightmapVirtualBase) return fail(MI_ERR_CAPACITY, "collider index space");
    w->heightmap = new mi_world::HHeightmap();
    w->heightmap->chunksPerDim = chunksPerDim; w->heightmap->chunkSize = chunkSize; w->heightmap->restitution = restitution; w->heightmap->friction = friction;
    w->heightmap->heights.resize((size_t)chunksPerDim * chunksPerDim);
    w->topologyDirty = true;
    return MI_OK;
}
MI_API int mi_heightmap_set_chunk_heights(mi_world* w, uint32_t x, uint32_t z, const uint16_t* heights) {
    if (!w || !w->heightmap || !heights) return fail(MI_ERR_INVALID_ARGUMENT, "no heightmap / null heights");
    if (x >= w->heightmap->chunksPerDim || z >= w->heightmap->chunksPerDim) return fail(MI_ERR_INVALID_ARGUMENT, "chunk out of range");
    w->heightmap->heights[(size_t)z * w->heightmap->chunksPerDim + x].assign(heights, heights + kHmVerts * kHmVerts);
    w->heightmap->dirty = true; w->topologyDirty = true;
    return MI_OK;
}
MI_API int mi_heightmap_update(mi_world* w, const float* minCorner, float amplitudeScale) {
    if (!w || !w->heightmap || !minCorner) return fail(MI_ERR_INVALID_ARGUMENT, "no heightmap / null corner");
    w->heightmap->minCorner = V3(minCorner[0], minCorner[1], minCorner[2]); w->heightmap->amplitudeScale = amplitudeScale;
    w->topologyDirty = true;
    return MI_OK;
}
MI_API int mi_heightmap_get_height(mi_world* w, float x, float z, float* out) {
    if (!w || !w->heightmap || !out) return fail(MI_ERR_INVALID_ARGUMENT, "no heightmap / null out");
    HIP_TRY(hipSetDevice(w->device));
    int rc = w->uploadHeightmap(); if (rc != MI_OK) return rc;   // refreshes the host mirror + parameters if needed
    HeightmapParams q = w->hmParams;
    q.heights = w->hmHostHeights.data(); q.chunkSlot = w->hmHostSlots.data(); q.mips = nullptr;
    *out = hmHeightAt(q, x, z);
    return MI_OK;
}
MI_API int mi_entity_set_force(mi_world* w, uint32_t entity, const float* force) {   // force_field_component::force (physics.h:35-38)
    if (!w || !force) return fail(MI_ERR_INVALID_ARGUMENT, "null argument");
    if (entity >= w->entities.size() || w->entities[entity].kind != MI_ENTITY_FORCE_FIELD) return fail(MI_ERR_INVALID_ARGUMENT, "not a force-field entity");
    w->entities[entity].force = V3(force[0], force[1], force[2]);
    w->topologyDirty = true;   // the rotated forces are part of the uploaded topology
    return MI_OK;
}

MI_API int mi_colliders_add(mi_world* w, uint32_t count, const uint32_t* ents, const mi_collider_desc* descs) {
    if (!w || (count && (!ents || !descs))) return fail(MI_ERR_INVALID_ARGUMENT, "null argument");
    int rc = w->download(); if (rc != MI_OK) return rc;
    for (uint32_t i = 0; i < count; ++i) {
        if (ents[i] >= w->entities.size()) return fail(MI_ERR_INVALID_ARGUMENT, "entity out of range");
        if (descs[i].type >= MI_COLLIDER_TYPE_COUNT) return fail(MI_ERR_INVALID_ARGUMENT, "bad collider type");
        if (descs[i].type == MI_COLLIDER_HULL && descs[i].hull_geometry >= w->hulls.size()) return fail(MI_ERR_INVALID_ARGUMENT, "bad hull geometry");
        HCollider c; c.entity = ents[i]; c.desc = descs[i];
        uint32_t id = (uint32_t)w->colliders.size();
        w->colliders.push_back(c);
        HEntity& e = w->entities[ents[i]];
        e.colliders.insert(e.colliders.begin(), id);   // linked-list prepend (src/scene/scene.h:52-54)
    }
    if (w->colliders.size() >= (1u << kIndexBits)) return fail(MI_ERR_CAPACITY, "collider index space is 26 bits per world");
    w->topologyDirty = true;
    return MI_OK;
}
MI_API int mi_collider_add(mi_world* w, uint32_t entity, const mi_collider_desc* d, uint32_t* out) {
    if (out && w) *out = (uint32_t)w->colliders.size();
    return mi_colliders_add(w, 1, &entity, d);
}

MI_API int mi_hull_geometry_create(mi_world* w, const float* v, uint32_t nv, const uint32_t* t, uint32_t nt, uint32_t* out) {
    if (!w || !v || !nv || !out) return fail(MI_ERR_INVALID_ARGUMENT, "null argument");
    HHull g; g.mn = V3(FLT_MAX); g.mx = V3(-FLT_MAX);
    for (uint32_t i = 0; i < nv; ++i) { V3 p(v[3 * i], v[3 * i + 1], v[3 * i + 2]); g.verts.push_back(p); g.mn = vmin(g.mn, p); g.mx = vmax(g.mx, p); }
    if (t) g.tris.assign(t, t + 3 * (size_t)nt);
    *out = (uint32_t)w->hulls.size();
    w->hulls.push_back(std::move(g));
    w->topologyDirty = true;
    return MI_OK;
}

MI_API int mi_constraint_create(mi_world* w, uint32_t type, uint32_t ea, uint32_t eb, const void* pod, uint32_t bytes, uint32_t* out) {
    if (!w || !pod) return fail(MI_ERR_INVALID_ARGUMENT, "null argument");
    int rc = w->joints.add(*w, type, ea, eb, pod, bytes, out);
    if (rc == MI_OK) w->topologyDirty = true;
    return rc;
}
MI_API int mi_constraint_update(mi_world* w, uint32_t type, uint32_t id, const void* pod, uint32_t bytes) {
    if (!w || !pod) return fail(MI_ERR_INVALID_ARGUMENT, "null argument");
    return w->joints.update(type, id, pod, bytes);   // motors / limits: the POD array is re-sent before the next step, nothing else changes
}
// Many constraints of one type at once (a policy writing the motor targets of thousands of ragdolls per step).
MI_API int mi_constraints_update(mi_world* w, uint32_t type, uint32_t count, const uint32_t* ids, const void* pods, uint32_t podBytes) {
    if (!w || (count && (!ids || !pods))) return fail(MI_ERR_INVALID_ARGUMENT, "null argument");
    for (uint32_t i = 0; i < count; ++i) {
        int rc = w->joints.update(type, ids[i], (const char*)pods + (size_t)i * podBytes, podBytes);
        if (rc != MI_OK) return rc;
    }
    return MI_OK;
}
MI_API int mi_constraint_destroy(mi_world* w, uint32_t type, uint32_t id) {
    if (!w) return fail(MI_ERR_INVALID_ARGUMENT, "null argument");
    int rc = w->joints.destroy(type, id);
    if (rc == MI_OK) w->topologyDirty = true;
    return rc;
}
MI_API int mi_constraints_destroy_all(mi_world* w) {
    if (!w) return fail(MI_ERR_INVALID_ARGUMENT, "null argument");
    w->joints.destroyAll(); w->topologyDirty = true;
    return MI_OK;
}
MI_API int mi_entity_destroy_constraints(mi_world* w, uint32_t entity) {
    if (!w || entity >= w->entities.size()) return fail(MI_ERR_INVALID_ARGUMENT, "bad entity");
    w->joints.destroyOfEntity(entity); w->topologyDirty = true;
    return MI_OK;
}
MI_API int mi_constraint_get(mi_world* w, uint32_t type, uint32_t id, void* pod, uint32_t bytes) {
    if (!w || !pod) return fail(MI_ERR_INVALID_ARGUMENT, "null argument");
    return w->joints.get(type, id, pod, bytes);
}
MI_API int mi_constraint_create_from_global(mi_world* w, uint32_t type, uint32_t ea, uint32_t eb, const float* anchor, const float* axis,
                                            float l0, float l1, uint32_t* out) {
    if (!w || !anchor) return fail(MI_ERR_INVALID_ARGUMENT, "null argument");
    int rc = w->download(); if (rc != MI_OK) return rc;
    rc = w->joints.addFromGlobal(*w, type, ea, eb, anchor, axis, l0, l1, out);
    if (rc == MI_OK) w->topologyDirty = true;
    return rc;
}

__global__ void k_add_forces(uint32_t n, const uint32_t* __restrict__ bodies, const float* __restrict__ ft, float4* __restrict__ bForce, float4* __restrict__ bTorque) {
    // one lane, in order: several entries may name the same body and the sums must not depend on scheduling
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t b = bodies[i];
        if (b == 0xFFFFFFFFu) continue;   // a ray that hit nothing
        float4 f = bForce[b], t = bTorque[b];
        f.x += ft[6 * i]; f.y += ft[6 * i + 1]; f.z += ft[6 * i + 2]; t.x += ft[6 * i + 3]; t.y += ft[6 * i + 4]; t.z += ft[6 * i + 5];
        bForce[b] = f; bTorque[b] = t;
    }
}
static int ensureUploaded(mi_world* w) {
    HIP_TRY(hipSetDevice(w->device));
    if (w->topologyDirty) { int rc = w->download(); if (rc != MI_OK) return rc; return w->upload(); }
    return MI_OK;
}
// rb.forceAccumulator += f; rb.torqueAccumulator += tau for many bodies.  While the host copy is authoritative (topology edits
// pending) the sums go there; otherwise they are added on the device without a download / re-upload.
MI_API int mi_entities_apply_forces(mi_world* w, uint32_t count, const uint32_t* ents, const float* forces3, const float* torques3) {
    if (!w || (count && !ents)) return fail(MI_ERR_INVALID_ARGUMENT, "null argument");
    for (uint32_t i = 0; i < count; ++i)
        if (ents[i] >= w->entities.size() || w->entities[ents[i]].rb < 0) return fail(MI_ERR_INVALID_ARGUMENT, "not a rigid body");
    if (!count) return MI_OK;
    if (w->topologyDirty) {
        int rc = w->download(); if (rc != MI_OK) return rc;
        for (uint32_t i = 0; i < count; ++i) {
            HBody& b = w->bodies[w->entities[ents[i]].rb];
            if (forces3) b.force = b.force + V3(forces3[3 * i], forces3[3 * i + 1], forces3[3 * i + 2]);
            if (torques3) b.torque = b.torque + V3(torques3[3 * i], torques3[3 * i + 1], torques3[3 * i + 2]);
        }
        return MI_OK;
    }
    HIP_TRY(hipSetDevice(w->device));
    std::vector<uint32_t> ids(count); std::vector<float> ft(6 * (size_t)count, 0.f);
    for (uint32_t i = 0; i < count; ++i) {
        ids[i] = (uint32_t)w->entities[ents[i]].rb;
        for (int k = 0; k < 3; ++k) { if (forces3) ft[6 * i + k] = forces3[3 * i + k]; if (torques3) ft[6 * i + 3 + k] = torques3[3 * i + k]; }
    }
    DBuf<uint32_t> dIds; DBuf<float> dFt;
    HIP_TRY(dIds.ensure(count)); HIP_TRY(dFt.ensure(6 * (size_t)count));
    HIP_TRY(hipMemcpyAsync(dIds.p, ids.data(), count * sizeof(uint32_t), hipMemcpyHostToDevice, w->stream));
    HIP_TRY(hipMemcpyAsync(dFt.p, ft.data(), ft.size() * sizeof(float), hipMemcpyHostToDevice, w->stream));
    k_add_forces<<<1, 1, 0, w->stream>>>(count, dIds.p, dFt.p, w->bForce.p, w->bTorque.p);
    w->shard.prevValid = false;
    HIP_TRY(hipStreamSynchronize(w->stream));
    w->hostStale = true;
    return MI_OK;
}
MI_API int mi_entity_apply_force(mi_world* w, uint32_t entity, const float* f, const float* t) { return mi_entities_apply_forces(w, 1, &entity, f, t); }
// testPhysicsInteraction(scene, ray, strength) (src/physics/physics.cpp:555-629) for `count` rays, applied in order.
MI_API int mi_world_test_interactions(mi_world* w, uint32_t count, const float* origins, const float* directions, const float* strengths, const uint32_t* ranges) {
    if (!w || (count && (!origins || !directions))) return fail(MI_ERR_INVALID_ARGUMENT, "null argument");
    if (!count) return MI_OK;
    int rc = ensureUploaded(w); if (rc != MI_OK) return rc;
    const uint32_t nc = (uint32_t)w->colliders.size();
    if (!nc || w->bodies.empty()) return MI_OK;
    std::vector<float> rays(8 * (size_t)count, 0.f); std::vector<uint32_t> rg(2 * (size_t)count);
    for (uint32_t r = 0; r < count; ++r) {
        for (int k = 0; k < 3; ++k) { rays[8 * r + k] = origins[3 * r + k]; rays[8 * r + 3 + k] = directions[3 * r + k]; }
        rays[8 * r + 6] = strengths ? strengths[r] : 1000.f;
        rg[2 * r] = ranges ? ranges[2 * r] : 0u; rg[2 * r + 1] = ranges ? ranges[2 * r + 1] : 0xFFFFFFFFu;
    }
    DBuf<float> dRays, dFT; DBuf<uint32_t> dRanges, dBody;
    HIP_TRY(dRays.ensure(rays.size())); HIP_TRY(dRanges.ensure(rg.size())); HIP_TRY(dBody.ensure(count)); HIP_TRY(dFT.ensure(6 * (size_t)count));
    HIP_TRY(hipMemcpyAsync(dRays.p, rays.data(), rays.size() * sizeof(float), hipMemcpyHostToDevice, w->stream));
    HIP_TRY(hipMemcpyAsync(dRanges.p, rg.data(), rg.size() * sizeof(uint32_t), hipMemcpyHostToDevice, w->stream));
    HullFaces hf{w->hullVerts.p, w->hullRanges.p, w->hullTris.p, w->hullTriRanges.p};
    k_ray_interactions<<<count, 256, 0, w->stream>>>(nc, dRays.p, dRanges.p, w->cTypeBody.p, w->cEntity.p, w->cShape.p, w->bPos.p, w->bRot.p, w->bCogInvMass.p, hf, dBody.p, dFT.p);
    k_add_forces<<<1, 1, 0, w->stream>>>(count, dBody.p, dFT.p, w->bForce.p, w->bTorque.p);
    HIP_TRY(hipStreamSynchronize(w->stream));
    w->hostStale = true;
    return MI_OK;
}

// mi_world_test_interactions on rays that already live on the device (k_ray_interactions' own layout): only enqueued.
MI_API int mi_world_test_interactions_device_async(mi_world* w, uint32_t count, const float* rays8Dev, const uint32_t* ranges2Dev) {
    if (!w || (count && !rays8Dev)) return fail(MI_ERR_INVALID_ARGUMENT, "null argument");
    if (w->shard.enabled) return fail(MI_ERR_UNSUPPORTED, "mi_world_test_interactions_device_async: not on a sharded world");
    if (!count) return MI_OK;
    int rc = ensureUploaded(w); if (rc != MI_OK) return rc;
    const uint32_t nc = (uint32_t)w->colliders.size();
    if (!nc || w->bodies.empty()) return MI_OK;
    HIP_TRY(w->interBody.ensure(count)); HIP_TRY(w->interFT.ensure(6 * (size_t)count));
    HullFaces hf{w->hullVerts.p, w->hullRanges.p, w->hullTris.p, w->hullTriRanges.p};
    k_ray_interactions<<<count, 256, 0, w->stream>>>(nc, rays8Dev, ranges2Dev, w->cTypeBody.p, w->cEntity.p, w->cShape.p, w->bPos.p, w->bRot.p, w->bCogInvMass.p, hf, w->interBody.p, w->interFT.p);
    k_add_forces_sparse<<<1, 1024, 0, w->stream>>>(count, w->interBody.p, w->interFT.p, w->bForce.p, w->bTorque.p);
    HIP_TRY(hipGetLastError());
    w->hostStale = true;
    return MI_OK;
}

// ---- constraint PODs written on the device
extern "C++" {
template <class JT> static int podIndices(JT& l, uint32_t count, const uint32_t* ids, uint32_t* out) {
    for (uint32_t i = 0; i < count; ++i) { const int d = l.dense(ids[i]); if (d < 0) return fail(MI_ERR_INVALID_ARGUMENT, "bad constraint id"); out[i] = (uint32_t)d; }
    return MI_OK;
}
}
MI_API int mi_constraints_to_device_indices(mi_world* w, uint32_t type, uint32_t count, const uint32_t* ids, uint32_t* out) {
    if (!w || (count && (!ids || !out))) return fail(MI_ERR_INVALID_ARGUMENT, "null argument");
    int rc = MI_OK;
    return w->joints.withType(type, [&](auto& l) { rc = podIndices(l, count, ids, out); }) ? rc : fail(MI_ERR_INVALID_ARGUMENT, "bad constraint type");
}
extern "C++" {
template <class JT> static int podsScatter(mi_world* w, JT& l, uint32_t count, const uint32_t* idxDev, const void* podsDev, uint32_t podBytes) {
    typedef typename std::remove_reference<decltype(l.pods[0])>::type P;
    static_assert(sizeof(P) % 4 == 0, "PODs are arrays of 32-bit words");
    if (podBytes != sizeof(P)) return fail(MI_ERR_INVALID_ARGUMENT, "constraint pod size mismatch (the packed mi_*_constraint)");
    if (l.pods.empty() || !l.dPods.p) return fail(MI_ERR_INVALID_ARGUMENT, "no constraint of this type");
    if (l.podsDirty) { HIP_TRY(l.uploadPods(w->stream)); HIP_TRY(hipStreamSynchronize(w->stream)); }   // a host update still waiting for the next step: it goes first, or that step's re-upload would undo this call
    const uint32_t words = (uint32_t)(sizeof(P) / 4u);
    const size_t total = (size_t)count * words;
    k_scatter_pods<<<(uint32_t)((total + 255u) / 256u), 256, 0, w->stream>>>(count, words, idxDev, static_cast<const uint32_t*>(podsDev), (uint32_t)l.pods.size(), reinterpret_cast<uint32_t*>(l.dPods.p));
    HIP_TRY(hipGetLastError());
    l.deviceNewer = true;
    return MI_OK;
}
}
MI_API int mi_constraints_update_device_async(mi_world* w, uint32_t type, uint32_t count, const uint32_t* idxDev, const void* podsDev, uint32_t podBytes) {
    if (!w || (count && (!idxDev || !podsDev))) return fail(MI_ERR_INVALID_ARGUMENT, "null argument");
    if (w->shard.enabled) return fail(MI_ERR_UNSUPPORTED, "mi_constraints_update_device_async: not on a sharded world");
    if (!count) return MI_OK;
    int rc = ensureUploaded(w); if (rc != MI_OK) return rc;
    return w->joints.withType(type, [&](auto& l) { rc = podsScatter(w, l, count, idxDev, podsDev, podBytes); }) ? rc : fail(MI_ERR_INVALID_ARGUMENT, "bad constraint type");
}

MI_API int mi_world_step_fixed(mi_world* w, const mi_step_settings* s, float dt, uint32_t n) {
    if (!w || !s) return fail(MI_ERR_INVALID_ARGUMENT, "null argument");
    if (n > 1 && w->shard.enabled && !w->shard.rccl) return fail(MI_ERR_INVALID_ARGUMENT, "a sharded world with the caller's transport takes one internal step per call (exchange in between)");
    if (n) w->transformsFollowPhysics = true;
    for (uint32_t i = 0; i < n; ++i) { if (i + 1 == n) w->posesArm(false, 0.f); int rc = w->stepInternal(*s, dt); if (rc != MI_OK) { w->posesAbort(); return rc; } }
    return n ? w->posesAfterStep() : MI_OK;
}

// One internal step with a HIP event pair around every k_contact_solve launch (roofline measurement; bench.py).
// out: number of profiled launches, their summed kernel time (ms), and the contact updates (contacts x iterations) they performed.
MI_API int mi_world_step_profiled(mi_world* w, const mi_step_settings* s, float dt, uint32_t* out_launches, float* out_kernel_ms, uint64_t* out_contact_updates) {
    if (!w || !s) return fail(MI_ERR_INVALID_ARGUMENT, "null argument");
    w->profileSolve = true; w->profLaunches = 0; w->profSlots = 0; w->profKernelMs = 0.f; w->profContacts = 0;
    int rc = w->stepInternal(*s, dt);
    w->profileSolve = false;
    if (out_launches) *out_launches = w->profLaunches;
    if (out_kernel_ms) *out_kernel_ms = w->profKernelMs;
    if (out_contact_updates) *out_contact_updates = w->profContacts;
    return rc;
}

// physicsStep (src/physics/physics.cpp:1364-1413): accumulator, <= maxPhysicsIterationsPerFrame sub-steps, pose interpolation.
MI_API int mi_world_step(mi_world* w, const mi_step_settings* s, float dt) {
    if (!w || !s) return fail(MI_ERR_INVALID_ARGUMENT, "null argument");
    if (w->shard.enabled && !w->shard.rccl && s->fixed_frame_rate && s->max_physics_iterations_per_frame > 1u)
        return fail(MI_ERR_INVALID_ARGUMENT, "a sharded world with the caller's transport takes ONE internal step per call (the exchange lies in between): max_physics_iterations_per_frame = 1, or mi_world_step_fixed");
    if (w->transformsFollowPhysics) { int rc = w->download(); if (rc != MI_OK) return rc; w->transformsFollowPhysics = false; }   // settle what mi_world_step_fixed left pending
    if (s->fixed_frame_rate) {
        const float fixedDt = 1.f / (float)s->frame_rate;
        w->timer += dt;
        uint32_t iterations = 0;
        if (w->timer >= fixedDt) {
            // physics_transform0 = physics_transform1 (physics.cpp:1380-1384), on the device
            HIP_TRY(hipSetDevice(w->device));
            if (w->topologyDirty) { int rc = w->download(); if (rc != MI_OK) return rc; rc = w->upload(); if (rc != MI_OK) return rc; w->haveEstimates = false; }
            const uint32_t nb = (uint32_t)w->bodies.size();
            if (nb) {
                HIP_TRY(w->bPos0.ensure(nb)); HIP_TRY(w->bRot0.ensure(nb));
                HIP_TRY(hipMemcpyAsync(w->bPos0.p, w->bPos.p, (size_t)nb * sizeof(float4), hipMemcpyDeviceToDevice, w->stream));
                HIP_TRY(hipMemcpyAsync(w->bRot0.p, w->bRot.p, (size_t)nb * sizeof(float4), hipMemcpyDeviceToDevice, w->stream));
                w->p0OnDevice = true; w->hostStale = true;
            }
            uint32_t willRun = 0; float timerAfter = w->timer;   // the loop below, run ahead: how many internal steps, and the interpolation factor they leave
            { uint32_t it = 0; while (timerAfter >= fixedDt && it++ < s->max_physics_iterations_per_frame) { timerAfter -= fixedDt; ++willRun; } if (timerAfter >= fixedDt) timerAfter = fmodf(timerAfter, fixedDt); }
            while (w->timer >= fixedDt && iterations++ < s->max_physics_iterations_per_frame) {
                if (iterations == willRun && nb) w->posesArm(true, timerAfter / fixedDt);
                int rc = w->stepInternal(*s, fixedDt); if (rc != MI_OK) { w->posesAbort(); return rc; }
                w->timer -= fixedDt;
            }
        }
        if (w->timer >= fixedDt) w->timer = fmodf(w->timer, fixedDt);
        // the interpolated transforms lerp(transform0, transform1, timer / fixedDt) are produced when somebody asks for them (download)
        w->lerpT = w->timer / fixedDt;
        if (w->hostStale) { w->lerpPending = true; return w->posesAfterStep(); }
        const float t = w->lerpT;   // nothing newer on the device (no sub-step in this call, host state current): interpolate right here
        for (HBody& b : w->bodies) {
            HEntity& e = w->entities[b.entity];
            e.pos = lerp(b.p0, b.p1, t);
            e.rot = normalize(Q4(b.r0.x + t * (b.r1.x - b.r0.x), b.r0.y + t * (b.r1.y - b.r0.y), b.r0.z + t * (b.r1.z - b.r0.z), b.r0.w + t * (b.r1.w - b.r0.w)));
        }
        return MI_OK;
    }
    w->posesArm(false, 0.f);
    int rc = w->stepInternal(*s, dt); if (rc != MI_OK) { w->posesAbort(); return rc; }
    w->transformsFollowPhysics = true;   // transform = physics_transform1, at the next download
    return w->posesAfterStep();
}
