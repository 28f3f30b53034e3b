// Part of world.hip (one translation unit; #included there, in this order): mass properties (setup time), upload / download.

// ------------------------------------------------------------------------------------------------
// Mass properties (setup time; src/physics/physics.cpp:1416-1588, src/physics/rigid_body.cpp:29-81)
// ------------------------------------------------------------------------------------------------
static float sphereVol(float r) { float sq = r * r; float sqpi = kPi * sq; return 4.f / 3.f * sqpi * r; }

static MassProps colliderMassProps(const mi_world& w, const mi_collider_desc& d) {
    MassProps r; r.inertia = M3::zero(); r.mass = 0.f;
    const float* f = d.shape;
    float density = d.density;
    switch (d.type) {
        case T_SPHERE: {
            float rad = f[3];
            r.mass = sphereVol(rad) * density;
            r.cog = V3(f[0], f[1], f[2]);
            r.inertia = scale(M3::identity(), 2.f / 5.f * r.mass * rad * rad);
        } break;
        case T_CAPSULE: case T_CYLINDER: {
            V3 a(f[0], f[1], f[2]), b(f[3], f[4], f[5]); float rad = f[6];
            V3 axis = a - b;
            if (axis.y < 0.f) axis = axis * -1.f;
            float height = len(axis);
            axis = axis * (1.f / height);
            M3 rot = quatToMat(rotateFromTo(V3(0.f, 1.f, 0.f), axis));
            float sqR = rad * rad;
            M3 I = M3::zero();
            if (d.type == T_CAPSULE) {
                float sqRpi = kPi * sqR;
                float volume = (4.f / 3.f * sqRpi * rad) + (sqRpi * len(a - b));
                r.mass = volume * density;
                float cylMass = density * sqRpi * height;
                float hemiMass = density * 2.f / 3.f * sqRpi * rad;
                float sqH = height * height;
                I.m11 = sqR * cylMass * 0.5f;
                I.m00 = I.m22 = I.m11 * 0.5f + cylMass * sqH / 12.f;
                float t0 = hemiMass * 2.f * sqR / 5.f;
                I.m11 += t0 * 2.f;
                float t1 = height * 0.5f;
                float t2 = t0 + hemiMass * (t1 * t1 + 3.f / 8.f * sqH);
                I.m00 += t2 * 2.f;
                I.m22 += t2 * 2.f;
            } else {
                float volume = (kPi * rad * rad) * len(a - b);
                r.mass = volume * density;
                float sqH = height * height;
                I.m11 = sqR * r.mass * 0.5f;
                I.m00 = I.m22 = 1.f / 12.f * r.mass * (3.f * sqR + sqH);
            }
            r.cog = (a + b) * 0.5f;
            r.inertia = mul(mul(transpose(rot), I), rot);
        } break;
        case T_AABB: {
            V3 mn(f[0], f[1], f[2]), mx(f[3], f[4], f[5]);
            V3 d0 = mx - mn;
            r.mass = (d0.x * d0.y * d0.z) * density;
            r.cog = (mn + mx) * 0.5f;
            V3 dia = ((mx - mn) * 0.5f) * 2.f;
            r.inertia.m00 = 1.f / 12.f * r.mass * (dia.y * dia.y + dia.z * dia.z);
            r.inertia.m11 = 1.f / 12.f * r.mass * (dia.x * dia.x + dia.z * dia.z);
            r.inertia.m22 = 1.f / 12.f * r.mass * (dia.x * dia.x + dia.y * dia.y);
        } break;
        case T_OBB: {
            Q4 q(f[0], f[1], f[2], f[3]); V3 c(f[4], f[5], f[6]), rad(f[7], f[8], f[9]);
            V3 dia = rad * 2.f;
            r.mass = (dia.x * dia.y * dia.z) * density;
            r.cog = c;
            M3 I = M3::zero();
            I.m00 = 1.f / 12.f * r.mass * (dia.y * dia.y + dia.z * dia.z);
            I.m11 = 1.f / 12.f * r.mass * (dia.x * dia.x + dia.z * dia.z);
            I.m22 = 1.f / 12.f * r.mass * (dia.x * dia.x + dia.y * dia.y);
            M3 rot = quatToMat(q);
            r.inertia = mul(mul(transpose(rot), I), rot);
        } break;
        default: {  // hull: tetrahedron covariance sum (physics.cpp:1517-1579)
            Q4 q(f[0], f[1], f[2], f[3]); V3 pos(f[4], f[5], f[6]);
            const HHull& g = w.hulls[d.hull_geometry];
            const float s60 = 1.f / 60.f, s120 = 1.f / 120.f;
            M3 Cc; Cc.m00 = s60; Cc.m01 = s120; Cc.m02 = s120; Cc.m10 = s120; Cc.m11 = s60; Cc.m12 = s120; Cc.m20 = s120; Cc.m21 = s120; Cc.m22 = s60;
            float totalMass = 0.f; M3 totalCov = M3::zero(); V3 totalCOG;
            for (size_t t = 0; t + 2 < g.tris.size(); t += 3) {
                V3 w1 = pos + rotate(q, g.verts[g.tris[t]]), w2 = pos + rotate(q, g.verts[g.tris[t + 1]]), w3 = pos + rotate(q, g.verts[g.tris[t + 2]]);
                M3 A; A.m00 = w1.x; A.m01 = w2.x; A.m02 = w3.x; A.m10 = w1.y; A.m11 = w2.y; A.m12 = w3.y; A.m20 = w1.z; A.m21 = w2.z; A.m22 = w3.z;
                float dA = det(A);
                M3 cov = mul(mul(scale(A, dA), Cc), transpose(A));
                float mass = 1.f / 6.f * dA;
                V3 cog = (w1 + w2 + w3) * 0.25f;
                totalMass += mass;
                totalCov = add(totalCov, cov);
                totalCOG = totalCOG + cog * mass;
            }
            totalCOG = totalCOG / totalMass;
            M3 Cp = sub(totalCov, scale(outer(totalCOG, totalCOG), totalMass));
            r.cog = totalCOG;
            r.mass = totalMass * density;
            float tr = Cp.m00 + Cp.m11 + Cp.m22;
            r.inertia = sub(scale(M3::identity(), tr), Cp);
            r.inertia = scale(r.inertia, density);
        } break;
    }
    return r;
}

int mi_world::recalcProperties() {
    for (HBody& rb : bodies) {
        if (entities[rb.entity].kind == MI_ENTITY_KINEMATIC) continue;
        const HEntity& e = entities[rb.entity];
        size_t n = e.colliders.size();
        if (!n) { rb.invMass = 1.f; rb.invInertia = M3::identity(); rb.localCOG = V3(); continue; }
        std::vector<MassProps> props(n);
        for (size_t i = 0; i < n; ++i) props[i] = colliderMassProps(*this, colliders[e.colliders[i]].desc);
        M3 inertia = M3::zero(); V3 cog; float mass = 0.f;
        for (size_t i = 0; i < n; ++i) { mass += props[i].mass; cog = cog + props[i].cog * props[i].mass; }
        rb.invMass = 1.f / mass;
        rb.localCOG = cog = cog * rb.invMass;
        for (size_t i = 0; i < n; ++i) {
            V3 r = props[i].cog - cog;
            M3 shift = scale(sub(scale(M3::identity(), dot(r, r)), outer(r, r)), props[i].mass);
            inertia = add(inertia, add(props[i].inertia, shift));
        }
        rb.invInertia = invert(inertia);
    }
    return MI_OK;
}

// ------------------------------------------------------------------------------------------------
// Upload / download
// ------------------------------------------------------------------------------------------------
static float4 h4(V3 v, float w) { return make_float4(v.x, v.y, v.z, w); }

int mi_world::upload() {
    recalcProperties();
    dropStepGraphs();
    ahead.stale = true;     // (what ran ahead of the next step ran on arrays that are being replaced)
    scalarsClean = false;   // (whatever the last step's publish kernel left cleared: anything may have touched the device since — the next step resets for itself)
    pose.valid = false; pose.tablesValid = false;
    shard.prevValid = false; shard.flagsSwapPending = false; shard.flagsOfAStep = false;
    shard.rearmFullSize();
    uint32_t nb = (uint32_t)bodies.size(), nc = (uint32_t)colliders.size();
    std::vector<float4> pos(nb), rot(nb), lv(nb), av(nb), fo(nb), to(nb), cim(nb), ii(3 * (size_t)nb), prm(nb);
    for (uint32_t i = 0; i < nb; ++i) {
        const HBody& b = bodies[i];
        pos[i] = h4(b.p1, 0.f); rot[i] = make_float4(b.r1.x, b.r1.y, b.r1.z, b.r1.w);
        lv[i] = h4(b.linVel, 0.f); av[i] = h4(b.angVel, 0.f); fo[i] = h4(b.force, 0.f); to[i] = h4(b.torque, 0.f);
        cim[i] = h4(b.localCOG, b.invMass);
        const M3& m = b.invInertia;
        ii[3 * i] = make_float4(m.m00, m.m01, m.m02, 0.f); ii[3 * i + 1] = make_float4(m.m10, m.m11, m.m12, 0.f); ii[3 * i + 2] = make_float4(m.m20, m.m21, m.m22, 0.f);
        prm[i] = make_float4(b.gravityFactor, b.linDamp, b.angDamp, 0.f);
    }
#define UP(buf, vec, count)                                                                                  \
    do {                                                                                                      \
        HIP_TRY(buf.ensure(std::max<size_t>((count), 1)));                                                    \
        if (count) HIP_TRY(hipMemcpyAsync(buf.p, vec.data(), (count) * sizeof(vec[0]), hipMemcpyHostToDevice, stream)); \
    } while (0)
    UP(bPos, pos, nb); UP(bRot, rot, nb); UP(bLinVel, lv, nb); UP(bAngVel, av, nb); UP(bForce, fo, nb); UP(bTorque, to, nb);
    UP(bCogInvMass, cim, nb); UP(bInvI, ii, 3 * (size_t)nb); UP(bParams, prm, nb);
    { size_t n1 = std::max<size_t>(nb, 1);
      HIP_TRY(bPosN.ensure(n1)); HIP_TRY(bRotN.ensure(n1)); HIP_TRY(bLinVelN.ensure(n1)); HIP_TRY(bAngVelN.ensure(n1)); HIP_TRY(bForceN.ensure(n1)); HIP_TRY(bTorqueN.ensure(n1)); }
    HIP_TRY(gPos.ensure(nb + 1)); HIP_TRY(gInvI.ensure(3 * ((size_t)nb + 1))); HIP_TRY(gVel.ensure(2 * ((size_t)nb + 1)));
    HIP_TRY(bodyTop.ensure(2 * ((size_t)nb + 1))); HIP_TRY(bodyUsed.ensure(nb + 1));
    HIP_TRY(hipMemsetAsync(bodyTop.p, 0, 2 * ((size_t)nb + 1) * sizeof(unsigned long long), stream));   // from here on k_integrate_velocities leaves both cleared for the next step
    HIP_TRY(hipMemsetAsync(bodyUsed.p, 0, ((size_t)nb + 1) * sizeof(unsigned long long), stream));
    HIP_TRY(gVelL.ensure(2 * ((size_t)nb + 1))); HIP_TRY(bodyOwner.ensure(nb + 1)); HIP_TRY(xcdBase.ensure(kSchedBins * 8)); HIP_TRY(keyCount.ensure(kSpatialKeys));

    usesGjk = false;
    for (const HCollider& c : colliders) if (c.desc.type == T_CAPSULE || c.desc.type == T_CYLINDER || c.desc.type == T_HULL) usesGjk = true;
    std::vector<uint32_t> tb(2 * (size_t)nc), obj(nc), cent(nc); std::vector<float4> sh(3 * (size_t)nc), sp(nc), sr(nc), emit(nc);
    // force fields (getForceFieldStates, physics.cpp:759-787): rotated force per field; fields without colliders are global
    usesInteractions = false; globalForce = V3();
    std::vector<float4> lf(ffEntities.size());
    for (size_t i = ffEntities.size(); i-- > 0;) {   // EnTT view order: back to front
        const HEntity& e = entities[ffEntities[i]];
        V3 f = rotate(e.rot, e.force);
        if (!e.colliders.empty()) lf[i] = h4(f, 0.f); else { lf[i] = make_float4(0, 0, 0, 0); globalForce = globalForce + f; }   // (a global field needs no interaction pass: k_integrate_forces adds it)
    }
    for (uint32_t k = 0; k < nc; ++k) {   // world index k <-> creation index nc-1-k (EnTT iterates back to front, physics.cpp:635-641)
        const HCollider& c = colliders[nc - 1 - k];
        const HEntity& e = entities[c.entity];
        tb[2 * k] = c.desc.type; tb[2 * k + 1] = e.rb >= 0 ? (uint32_t)e.rb : kNoBody;
        cent[k] = c.entity;
        obj[k] = e.kind == MI_ENTITY_FORCE_FIELD ? (OBJ_FORCE_FIELD | e.kindIndex << 8) : e.kind == MI_ENTITY_TRIGGER ? (OBJ_TRIGGER | e.kindIndex << 8) : OBJ_STATIC;
        if (e.kind == MI_ENTITY_FORCE_FIELD || e.kind == MI_ENTITY_TRIGGER) usesInteractions = true;
        float s[12]; std::memcpy(s, c.desc.shape, sizeof(s));
        if (c.desc.type == T_HULL) std::memcpy(&s[7], &c.desc.hull_geometry, 4);
        sh[3 * k] = make_float4(s[0], s[1], s[2], s[3]); sh[3 * k + 1] = make_float4(s[4], s[5], s[6], s[7]); sh[3 * k + 2] = make_float4(s[8], s[9], s[10], s[11]);
        sp[k] = h4(e.pos, 0.f); sr[k] = make_float4(e.rot.x, e.rot.y, e.rot.z, e.rot.w);
        // what k_emit_manifolds needs of a collider in one gather (objIndex as k_world_colliders writes it: the body, or the static dummy `nb`)
        const uint32_t obj = e.rb >= 0 ? (uint32_t)e.rb : e.kind == MI_ENTITY_FORCE_FIELD || e.kind == MI_ENTITY_TRIGGER ? e.kindIndex : nb;
        const uint32_t dyn = e.rb >= 0 && bodies[e.rb].invMass != 0.f ? 1u : 0u;
        emit[k] = make_float4(c.desc.restitution, c.desc.friction, 0.f, 0.f);
        std::memcpy(&emit[k].z, &obj, 4); std::memcpy(&emit[k].w, &dyn, 4);
    }
    UP(cObject, obj, nc); UP(localForce, lf, lf.size()); UP(cEntity, cent, nc);
    if (usesInteractions) HIP_TRY(bForceStep.ensure(std::max<size_t>(nb, 1)));
    {   // sharded worlds: which body blocks each collider block refers to (k_bp_prepare skips a collider block none of whose body blocks is live)
        const uint32_t numCb = divUp(std::max(nc, 1u), 256);
        std::vector<uint2> cbr(numCb, make_uint2(0xFFFFFFFFu, 0u));
        for (uint32_t k = 0; k < nc; ++k) {
            uint2& r = cbr[k >> 8];
            const uint32_t body = tb[2 * k + 1];
            if (body == kNoBody || body >= nb) { r.x = 1u; r.y = 0u; continue; }    // a collider without a rigid body is never "not simulated here"
            if (r.x == 1u && r.y == 0u) continue;
            r.x = std::min(r.x, body >> 8); r.y = std::max(r.y, body >> 8);
        }
        for (uint2& r : cbr) if (r.x <= r.y && r.y - r.x > 15u) { r.x = 1u; r.y = 0u; }     // bodies scattered over many blocks: not worth asking
        UP(cbRange, cbr, numCb);
    }
    UP(cTypeBody, tb, 2 * (size_t)nc); UP(cShape, sh, 3 * (size_t)nc); UP(cStaticPos, sp, nc); UP(cStaticRot, sr, nc); UP(cEmit, emit, nc);
    HIP_TRY(wShape.ensure(3 * (size_t)nc + 1)); HIP_TRY(aabbMin.ensure(nc + 1)); HIP_TRY(aabbMax.ensure(nc + 1));
    HIP_TRY(sMin.ensure(nc + 1)); HIP_TRY(sMax.ensure(nc + 1)); HIP_TRY(sRow.ensure(nc + 1));
    HIP_TRY(largeList.ensure(nc + 1)); HIP_TRY(isLarge.ensure(nc + 1));
    HIP_TRY(cellKeys.ensure(nc + 1)); HIP_TRY(cellRanks.ensure(nc + 1)); HIP_TRY(cellKeysS.ensure(nc + 1)); HIP_TRY(cellValsS.ensure(nc + 1));
    HIP_TRY(cellCount.ensure(kMaxCells)); HIP_TRY(cellLower.ensure(kMaxCells));
    HIP_TRY(hipMemsetAsync(cellCount.p, 0, (size_t)kMaxCells * sizeof(uint32_t), stream));   // from here on every scan clears what it read
    HIP_TRY(blockBounds.ensure(6 * (size_t)divUp(std::max(nc, 1u), 256)));
    HIP_TRY(axisPartials.ensure(kAxisSums * (size_t)divUp(std::max(nc, 1u), 256)));
    // hull geometry pool
    std::vector<float4> ha(2 * hulls.size() + 1), hv; std::vector<uint32_t> hr(2 * hulls.size() + 2);
    for (size_t h = 0; h < hulls.size(); ++h) {
        ha[2 * h] = h4(hulls[h].mn, 0.f); ha[2 * h + 1] = h4(hulls[h].mx, 0.f);
        hr[2 * h] = (uint32_t)hv.size(); hr[2 * h + 1] = (uint32_t)hulls[h].verts.size();
        for (const V3& v : hulls[h].verts) hv.push_back(h4(v, 0.f));
    }
    if (hv.empty()) hv.push_back(make_float4(0, 0, 0, 0));
    std::vector<uint32_t> ht, htr(2 * hulls.size() + 2);
    for (size_t h = 0; h < hulls.size(); ++h) { htr[2 * h] = (uint32_t)(ht.size() / 3); htr[2 * h + 1] = (uint32_t)(hulls[h].tris.size() / 3); ht.insert(ht.end(), hulls[h].tris.begin(), hulls[h].tris.end()); }
    if (ht.empty()) ht.push_back(0u);
    UP(hullTris, ht, ht.size()); UP(hullTriRanges, htr, htr.size());
    UP(hullAabb, ha, ha.size()); UP(hullVerts, hv, hv.size()); UP(hullRanges, hr, hr.size());
#undef UP
    int rc = joints.upload(*this, stream);
    if (rc != MI_OK) return rc;
    if (heightmap) {
        HIP_TRY(hmPacked.ensure(nc + 1)); HIP_TRY(hmScan.ensure(nc + 1)); HIP_TRY(hmSlow.ensure(nc + 1)); HIP_TRY(hmStash.ensure((size_t)(nc + 1) * kHmStash));
        rc = uploadHeightmap(); if (rc != MI_OK) return rc;
    }
    HIP_TRY(hipStreamSynchronize(stream));
    topologyDirty = false; hostStale = false; haveEstimates = false; gridValid = false;
    ++poseEpoch;
    if (seamTiling.on && !shard.enabled) { int rc = shardBuildRoots(); if (rc != MI_OK) return rc; }
    if (shard.enabled) {   // the previous step's counts say nothing about the new topology
        int rc = shardBuildRoots(); if (rc != MI_OK) return rc;
        std::vector<uint8_t> kn(std::max(nb, 1u), 1u);
        for (uint32_t i = 0; i < nb; ++i) kn[i] = bodies[i].shardKnown;
        HIP_TRY(shard.known.ensure(kn.size())); HIP_TRY(hipMemcpy(shard.known.p, kn.data(), kn.size(), hipMemcpyHostToDevice));
    }
    return MI_OK;
}

// heightmap_collider_chunk::setHeights (heightmap_collider.cpp:42-114): the min/max pyramid of every chunk that has heights,
// built on the host at upload time (setup cost, not per step) and pooled on the device next to the heights.
int mi_world::uploadHeightmap() {
    HHeightmap& h = *heightmap;
    const uint32_t nchunks = h.chunksPerDim * h.chunksPerDim;
    if (h.dirty) {
        hmHostSlots.assign(nchunks, 0xFFFFFFFFu);
        uint32_t used = 0;
        for (uint32_t c = 0; c < nchunks; ++c) if (!h.heights[c].empty()) hmHostSlots[c] = used++;
        hmHostHeights.assign((size_t)std::max(used, 1u) * kHmVerts * kHmVerts, 0);
        std::vector<uint32_t> mips((size_t)std::max(used, 1u) * kHmMipEntries, 0u);
        for (uint32_t c = 0; c < nchunks; ++c) {
            if (hmHostSlots[c] == 0xFFFFFFFFu) continue;
            const uint16_t* src = h.heights[c].data();
            std::copy(src, src + kHmVerts * kHmVerts, hmHostHeights.begin() + (size_t)hmHostSlots[c] * kHmVerts * kHmVerts);
            uint32_t* mp = mips.data() + (size_t)hmHostSlots[c] * kHmMipEntries;
            for (uint32_t z = 0; z < kHmSegs; ++z)
                for (uint32_t x = 0; x < kHmSegs; ++x) {
                    uint16_t v[4] = {src[kHmVerts * z + x], src[kHmVerts * (z + 1) + x], src[kHmVerts * z + x + 1], src[kHmVerts * (z + 1) + x + 1]};
                    mp[z * kHmSegs + x] = (uint32_t)*std::min_element(v, v + 4) | ((uint32_t)*std::max_element(v, v + 4) << 16);
                }
            for (uint32_t mip = 1; mip < 8; ++mip) {
                const uint32_t n = kHmSegs >> mip, rs = n * 2;
                const uint32_t* rd = mp + hmMipOffset(mip - 1); uint32_t* wr = mp + hmMipOffset(mip);
                for (uint32_t z = 0; z < n; ++z)
                    for (uint32_t x = 0; x < n; ++x) {
                        uint32_t q[4] = {rd[rs * (2 * z) + 2 * x], rd[rs * (2 * z + 1) + 2 * x], rd[rs * (2 * z) + 2 * x + 1], rd[rs * (2 * z + 1) + 2 * x + 1]};
                        uint32_t mn = 0xFFFFu, mx = 0u;
                        for (uint32_t k = 0; k < 4; ++k) { mn = std::min(mn, q[k] & 0xFFFFu); mx = std::max(mx, q[k] >> 16); }
                        wr[z * n + x] = mn | (mx << 16);
                    }
            }
        }
        HIP_TRY(hmHeights.ensure(hmHostHeights.size())); HIP_TRY(hmMips.ensure(mips.size())); HIP_TRY(hmChunkSlot.ensure(nchunks));
        HIP_TRY(hipMemcpyAsync(hmHeights.p, hmHostHeights.data(), hmHostHeights.size() * sizeof(uint16_t), hipMemcpyHostToDevice, stream));
        HIP_TRY(hipMemcpyAsync(hmMips.p, mips.data(), mips.size() * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
        HIP_TRY(hipMemcpyAsync(hmChunkSlot.p, hmHostSlots.data(), nchunks * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
        HIP_TRY(hipStreamSynchronize(stream));   // `mips` is a local
        h.dirty = false;
    }
    HeightmapParams& q = hmParams;   // heightmap_collider_component ctor + update (heightmap_collider.cpp:5-19)
    q.heights = hmHeights.p; q.mips = hmMips.p; q.chunkSlot = hmChunkSlot.p; q.chunksPerDim = h.chunksPerDim;
    q.chunkSize = h.chunkSize; q.invChunkSize = 1.f / h.chunkSize; q.chunkScale = h.chunkSize / (float)kHmSegs;
    q.heightScale = h.amplitudeScale / 65535.f; q.invAmplitudeScale = 1.f / h.amplitudeScale;
    q.minX = h.minCorner.x; q.minY = h.minCorner.y; q.minZ = h.minCorner.z; q.restitution = h.restitution; q.friction = h.friction;
    return MI_OK;
}

// ---- poses for the caller (PoseStream)
bool mi_world::posesPossible(bool physics, float* t) const {
    const bool follow = physics || transformsFollowPhysics, lerpNow = !follow && lerpPending;
    if (!pose.enabled || !hostStale || topologyDirty || bodies.empty() || shard.enabled) return false;
    if (!follow && !(lerpNow && p0OnDevice)) return false;
    *t = follow ? -1.f : lerpT;
    return true;
}
// entity -> rigid body (or -1) on the device, and the entities without one: rebuilt after an upload
int mi_world::posesEnsureTables() {
    PoseStream& ps = pose;
    const uint32_t n = (uint32_t)entities.size();
    if (!ps.tablesValid || ps.tableCount != n) {
        std::vector<int> eb(n); ps.noBody.clear();
        for (uint32_t i = 0; i < n; ++i) { eb[i] = entities[i].rb; if (eb[i] < 0) ps.noBody.push_back(i); }
        HIP_TRY(ps.entBody.ensure(std::max<size_t>(n, 1)));
        HIP_TRY(hipMemcpyAsync(ps.entBody.p, eb.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, stream));
        HIP_TRY(hipStreamSynchronize(stream));   // (eb is pageable and goes away)
        ps.tablesValid = true; ps.tableCount = n;
    }
    return MI_OK;
}
int mi_world::posesProduce(float t, bool fromNextState, bool ahead) {
    HIP_TRY(hipSetDevice(device));
    PoseStream& ps = pose;
    const uint32_t n = (uint32_t)entities.size();
    if (!ps.copyStream) {
        HIP_TRY(hipStreamCreateWithFlags(&ps.copyStream, hipStreamNonBlocking));
        HIP_TRY(hipEventCreateWithFlags(&ps.produced, hipEventDisableTiming));
        for (hipEvent_t& e : ps.chunkEv) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        for (auto& ff : ps.sets) for (auto& si : ff) HIP_TRY(hipEventCreateWithFlags(&si.landed, hipEventDisableTiming));
    }
    if (ps.copyInFlight) { HIP_TRY(hipStreamWaitEvent(stream, ps.chunkEv[kPoseChunks - 1], 0)); ps.copyInFlight = false; }   // the device-side rows are about to be rewritten
    { int rc = posesEnsureTables(); if (rc != MI_OK) return rc; }
    if (ahead && ps.valid && ps.hasVel && !ps.velConsumed) ps.wantVel = false;   // nobody read the velocities of the last frame: they stop riding along
    const bool vel = ps.wantVel;
    const size_t floats = (vel ? 13u : 7u) * (size_t)n;   // [n][4] rotations, [n][3] positions (, [n][3] linear, [n][3] angular velocities)
    HIP_TRY(ps.out.ensure(std::max<size_t>(floats, 4)));
    if (13u * (size_t)n > ps.hostCap) {   // (sized for the rows WITH velocities from the start: growing later would pull the rows out from under a view a caller still holds; entities added = topology change, views are void then anyway)
        HIP_TRY(hipStreamSynchronize(ps.copyStream));
        for (auto& hh : ps.host) for (float*& h : hh) { if (h) (void)hipHostFree(h); h = nullptr; }
        ps.hostCap = 0;
        const size_t cap = 13u * (size_t)n + 13u * (size_t)n / 4 + 16;
        for (auto& hh : ps.host) for (float*& h : hh) HIP_TRY(hipHostMalloc((void**)&h, cap * sizeof(float)));
        ps.hostCap = cap;
        for (auto& ff : ps.sets) for (auto& si : ff) si.valid = false;   // (fresh memory: nothing has landed in it)
    }
    const int fl = t < 0.f ? 1 : 0;
    const bool again = (!ps.valid && ps.retrySameStep && ps.flavour == fl) ||                       // a step that is re-run,
                       (ps.valid && ps.steps == totalSteps && ps.flavour == fl && ps.t == t && ps.n == n);   // or the same rows once more (now with the velocities): into the same set, the same bytes —
    if (!again) ps.cur[fl] ^= 1;                                                                         // the other set may still be in a caller's hands
    ps.retrySameStep = false;
    float* outR = ps.out.p; float* outP = ps.out.p + 4u * (size_t)n;
    hipLaunchKernelGGL(k_entity_poses, dim3(divUp(n, 256u)), dim3(256), 0, stream, n, ps.entBody.p, fromNextState ? bPosN.p : bPos.p, fromNextState ? bRotN.p : bRot.p, bPos0.p, bRot0.p, t, outP, outR,
                       fromNextState ? bLinVelN.p : bLinVel.p, fromNextState ? bAngVelN.p : bAngVel.p, vel ? ps.out.p + 7u * (size_t)n : nullptr, vel ? ps.out.p + 10u * (size_t)n : nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ps.produced, stream));
    HIP_TRY(hipStreamWaitEvent(ps.copyStream, ps.produced, 0));
    const size_t bytes = floats * sizeof(float);
    for (uint32_t k = 0; k <= kPoseChunks; ++k) ps.chunkOff[k] = k == kPoseChunks ? bytes : std::min(bytes, ((bytes * k / kPoseChunks) + 4095u) & ~(size_t)4095u);
    for (uint32_t k = 0; k < kPoseChunks; ++k) {
        const size_t off = ps.chunkOff[k], len = ps.chunkOff[k + 1] - off;
        if (len) HIP_TRY(hipMemcpyAsync(reinterpret_cast<char*>(ps.host[fl][ps.cur[fl]]) + off, reinterpret_cast<const char*>(ps.out.p) + off, len, hipMemcpyDeviceToHost, ps.copyStream));
        HIP_TRY(hipEventRecord(ps.chunkEv[k], ps.copyStream));
    }
    {   // the set's own "landed" event (behind its last piece) and what it holds
        PoseStream::SetInfo& si = ps.sets[fl][ps.cur[fl]];
        HIP_TRY(hipEventRecord(si.landed, ps.copyStream));
        si.valid = true; si.steps = totalSteps; si.t = t; si.n = n;
    }
    ps.flavour = fl; ps.hasVel = vel; ps.velConsumed = false;
    ps.valid = true; ps.copyInFlight = true; ps.steps = totalSteps; ps.t = t; ps.n = n; ps.consumed = false;
    return MI_OK;
}
// p / r (/ lin / ang): the caller's arrays ([n][3], [n][4], [n][3], [n][3]; any may be null) — a few threads copy each piece as it lands; view*: the pinned rows themselves
int mi_world::posesFetch(float* p, float* r, const float** viewP, const float** viewR, float* lin, float* ang, const float** viewL, const float** viewA) {
    PoseStream& ps = pose;
    const uint32_t n = ps.n;
    float* src = ps.host[ps.flavour][ps.cur[ps.flavour]];
    const size_t N = (size_t)n;
    const bool wantsVel = lin || ang || viewL || viewA;
    if (wantsVel && !ps.hasVel) return fail(MI_ERR_UNSUPPORTED, "the rows carry no velocities");
    if (viewP || viewR || viewL || viewA) {
        HIP_TRY(hipEventSynchronize(ps.chunkEv[kPoseChunks - 1]));
        for (uint32_t i : ps.noBody) {
            const HEntity& e = entities[i];
            float* rr = src + 4u * (size_t)i; float* pp = src + 4u * N + 3u * (size_t)i;
            rr[0] = e.rot.x; rr[1] = e.rot.y; rr[2] = e.rot.z; rr[3] = e.rot.w; pp[0] = e.pos.x; pp[1] = e.pos.y; pp[2] = e.pos.z;
            if (ps.hasVel) for (int k = 0; k < 3; ++k) { src[7u * N + 3u * (size_t)i + k] = 0.f; src[10u * N + 3u * (size_t)i + k] = 0.f; }
        }
        if (viewP) *viewP = src + 4u * N;
        if (viewR) *viewR = src;
        if (viewL) *viewL = src + 7u * N;
        if (viewA) *viewA = src + 10u * N;
    }
    if (p || r || lin || ang) {
        struct Region { size_t off, len; char* dst; };   // where the pieces of the rows go
        const Region regions[4] = {{0, 16u * N, reinterpret_cast<char*>(r)}, {16u * N, 12u * N, reinterpret_cast<char*>(p)},
                                   {28u * N, ps.hasVel ? 12u * N : 0u, reinterpret_cast<char*>(lin)}, {40u * N, ps.hasVel ? 12u * N : 0u, reinterpret_cast<char*>(ang)}};
        const size_t total = ps.chunkOff[kPoseChunks];
        const uint32_t threads = total >= (1u << 20) ? std::min<uint32_t>(4u, std::max(1u, std::thread::hardware_concurrency())) : 1u;
        std::atomic<int> err{0};
        auto work = [&](uint32_t tid) {
            for (uint32_t k = 0; k < kPoseChunks; ++k) {
                if (hipEventSynchronize(ps.chunkEv[k]) != hipSuccess) { err = 1; return; }
                const size_t lo0 = ps.chunkOff[k], len = ps.chunkOff[k + 1] - lo0;
                const size_t lo = lo0 + ((len * tid / threads) & ~(size_t)63), hi = tid + 1 == threads ? lo0 + len : lo0 + ((len * (tid + 1) / threads) & ~(size_t)63);
                for (const Region& g : regions) {
                    const size_t a = std::max(lo, g.off), e = std::min(hi, g.off + g.len);
                    if (g.dst && a < e) std::memcpy(g.dst + (a - g.off), reinterpret_cast<const char*>(src) + a, e - a);
                }
            }
        };
        std::vector<std::thread> pool;
        for (uint32_t tdx = 1; tdx < threads; ++tdx) { try { pool.emplace_back(work, tdx); } catch (...) { for (std::thread& th : pool) th.join(); pool.clear(); for (uint32_t q = 1; q < threads; ++q) work(q); break; } }
        work(0);
        for (std::thread& th : pool) th.join();
        if (err) return fail(MI_ERR_DEVICE, "pose copy");
        for (uint32_t i : ps.noBody) {
            const HEntity& e = entities[i];
            if (p) { p[3 * (size_t)i] = e.pos.x; p[3 * (size_t)i + 1] = e.pos.y; p[3 * (size_t)i + 2] = e.pos.z; }
            if (r) { r[4 * (size_t)i] = e.rot.x; r[4 * (size_t)i + 1] = e.rot.y; r[4 * (size_t)i + 2] = e.rot.z; r[4 * (size_t)i + 3] = e.rot.w; }
            if (lin) for (int k = 0; k < 3; ++k) lin[3 * (size_t)i + k] = 0.f;
            if (ang) for (int k = 0; k < 3; ++k) ang[3 * (size_t)i + k] = 0.f;
        }
    }
    if (wantsVel) ps.velConsumed = true;
    if (p || r || viewP || viewR) { ps.consumed = true; ps.wanted = true; }
    return MI_OK;
}
// end of mi_world_step / mi_world_step_fixed: a caller that asked for the poses after the previous step gets this step's under way now
bool mi_world::posesWantedAhead() {
    PoseStream& ps = pose;
    if (!ps.enabled || !ps.wanted) return false;
    if (ps.valid && !ps.consumed) { ps.wanted = false; return false; }   // nobody read the last ones
    return true;
}
// before the last internal step of a stepping call: what the poses will be afterwards is known (physics_transform1, or the lerp with the factor
// the accumulator will leave), so that step enqueues them itself — the host's ~0.1 ms of launches and copies hides behind the step's kernels
void mi_world::posesArm(bool lerpAfterwards, float lerpTAfterwards) {
    poseArm = PoseArm{};
    if (!posesWantedAhead() || topologyDirty || bodies.empty() || shard.enabled) return;
    const bool follow = pose.askedPhysics || !lerpAfterwards;
    poseArm.armed = true; poseArm.t = follow ? -1.f : lerpTAfterwards;
}
// The newest rows of this flavour that are COMPLETE in host memory, without waiting: the last production's if its copy has landed, else the one before (the other set).
// *ofStep = the internal step whose state they are.  What is handed out stays intact until the next stepping call produces into the same set: the rows of the step BEFORE the
// last one are overwritten by the NEXT stepping call (two sets alternate), those of the last step by the one after it.
int mi_world::posesViewLanded(bool physics, const float** p, const float** r, uint32_t* count, uint64_t* ofStep) {
    PoseStream& ps = pose;
    const int fl = physics ? 1 : 0;
    const uint32_t n = (uint32_t)entities.size();
    int pick = -1;
    for (int k = 0; k < 2 && pick < 0; ++k) {   // newest first: the current set of this flavour, then the other one
        const int set = k == 0 ? ps.cur[fl] : ps.cur[fl] ^ 1;
        const PoseStream::SetInfo& si = ps.sets[fl][set];
        if (!si.valid || si.n != n || !si.landed) continue;
        if (k == 0 && !(ps.valid && ps.flavour == fl)) continue;                     // (a voided production)
        const hipError_t q = hipEventQuery(si.landed);
        if (q == hipSuccess) pick = set;
        else if (q != hipErrorNotReady) return fail(MI_ERR_DEVICE, "pose copy");
        else (void)hipGetLastError();
    }
    if (pick < 0) return fail(MI_ERR_UNSUPPORTED, "no pose rows have landed yet: mi_world_view_transforms waits for the current ones");
    float* src = ps.host[fl][pick];
    const size_t N = (size_t)n;
    for (uint32_t i : ps.noBody) {   // entities without a rigid body: the host's transform
        const HEntity& e = entities[i];
        float* rr = src + 4u * (size_t)i; float* pp = src + 4u * N + 3u * (size_t)i;
        rr[0] = e.rot.x; rr[1] = e.rot.y; rr[2] = e.rot.z; rr[3] = e.rot.w; pp[0] = e.pos.x; pp[1] = e.pos.y; pp[2] = e.pos.z;
    }
    if (p) *p = src + 4u * N;
    if (r) *r = src;
    if (count) *count = n;
    if (ofStep) *ofStep = ps.sets[fl][pick].steps;
    ps.askedPhysics = physics; ps.consumed = true; ps.wanted = true;   // (the stepping calls keep producing ahead for this caller)
    return MI_OK;
}
// a stepping call that failed: rows the failed step enqueued for itself were computed from a state that was never swapped in — they must not be handed
// out as the current poses (ps.steps == totalSteps would still hold)
void mi_world::posesAbort() {
    if (poseArm.armed && poseArm.done && pose.produced_ahead) --pose.produced_ahead;
    if (poseArm.armed) pose.valid = false;
    poseArm = PoseArm{};
}
int mi_world::posesAfterStep() {
    PoseStream& ps = pose;
    const bool inside = poseArm.armed && poseArm.done;
    poseArm = PoseArm{};
    if (inside) return MI_OK;
    if (!posesWantedAhead()) return MI_OK;
    float t;
    if (!posesPossible(ps.askedPhysics, &t)) return MI_OK;
    if (ps.valid && ps.steps == totalSteps && ps.t == t && ps.n == (uint32_t)entities.size() && ps.tablesValid) return MI_OK;
    ++ps.produced_ahead;
    return posesProduce(t, false, true);
}

int mi_world::download() {
    if (!hostStale) return MI_OK;
    uint32_t nb = (uint32_t)bodies.size();
    if (nb) {
        // pinned staging, kept: pageable std::vectors made this 2.5 ms per call at 57 k bodies (allocation + staged copies), which was
        // the largest part of a batched learning step once mi_world_step stopped downloading
        const size_t rows = (p0OnDevice ? 8u : 6u) * (size_t)nb;
        if (rows > downloadStageCap) {
            if (downloadStage) (void)hipHostFree(downloadStage);
            downloadStage = nullptr; downloadStageCap = 0;
            HIP_TRY(hipHostMalloc((void**)&downloadStage, (rows + rows / 4) * sizeof(float4)));
            downloadStageCap = rows + rows / 4;
        }
        float4 *pos = downloadStage, *rot = pos + nb, *lv = rot + nb, *av = lv + nb, *fo = av + nb, *to = fo + nb, *pos0 = to + nb, *rot0 = pos0 + nb;
        HIP_TRY(hipMemcpyAsync(pos, bPos.p, nb * 16, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipMemcpyAsync(rot, bRot.p, nb * 16, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipMemcpyAsync(lv, bLinVel.p, nb * 16, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipMemcpyAsync(av, bAngVel.p, nb * 16, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipMemcpyAsync(fo, bForce.p, nb * 16, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipMemcpyAsync(to, bTorque.p, nb * 16, hipMemcpyDeviceToHost, stream));
        if (p0OnDevice) {
            HIP_TRY(hipMemcpyAsync(pos0, bPos0.p, nb * 16, hipMemcpyDeviceToHost, stream));
            HIP_TRY(hipMemcpyAsync(rot0, bRot0.p, nb * 16, hipMemcpyDeviceToHost, stream));
        }
        HIP_TRY(hipStreamSynchronize(stream));
        hostParallelFor(nb, [&](uint32_t i) {   // a body writes its own HBody and its own entity only
            HBody& b = bodies[i];
            if (p0OnDevice) { b.p0 = V3(pos0[i].x, pos0[i].y, pos0[i].z); b.r0 = Q4(rot0[i].x, rot0[i].y, rot0[i].z, rot0[i].w); }
            b.p1 = V3(pos[i].x, pos[i].y, pos[i].z); b.r1 = Q4(rot[i].x, rot[i].y, rot[i].z, rot[i].w);
            b.linVel = V3(lv[i].x, lv[i].y, lv[i].z); b.angVel = V3(av[i].x, av[i].y, av[i].z);
            b.force = V3(fo[i].x, fo[i].y, fo[i].z); b.torque = V3(to[i].x, to[i].y, to[i].z);
            // after n x physicsStepInternal without interpolation (mi_world_step_fixed) the transform is physics_transform1 (physics.cpp:1408-1411)
            if (transformsFollowPhysics) { HEntity& e = entities[b.entity]; e.pos = b.p1; e.rot = b.r1; }
            else if (lerpPending) {   // lerp(trs): nlerp on the quaternion (src/core/math.h:673-682)
                HEntity& e = entities[b.entity]; const float t = lerpT;
                e.pos = lerp(b.p0, b.p1, t);
                e.rot = normalize(Q4(b.r0.x + t * (b.r1.x - b.r0.x), b.r0.y + t * (b.r1.y - b.r0.y), b.r0.z + t * (b.r1.z - b.r0.z), b.r0.w + t * (b.r1.w - b.r0.w)));
            }
        });
        p0OnDevice = false; lerpPending = false;
        if (shard.enabled && shard.known.p && shard.known.cap >= nb) {
            std::vector<uint8_t> kn(nb);
            HIP_TRY(hipMemcpy(kn.data(), shard.known.p, nb, hipMemcpyDeviceToHost));
            for (uint32_t i = 0; i < nb; ++i) bodies[i].shardKnown = kn[i];
        }
    }
    hostStale = false;
    return MI_OK;
}
