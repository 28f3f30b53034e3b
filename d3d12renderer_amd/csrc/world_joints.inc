// Part of world.hip (one translation unit; #included there, in this order): joint storage on the host, islands.

// ------------------------------------------------------------------------------------------------
// Joint storage (host) — addConstraint / add*ConstraintFromGlobalPoints (src/physics/physics.cpp:128-333)
// ------------------------------------------------------------------------------------------------
// A constraint POD may be handed over packed (sizeof(mi_*_constraint)) or AS THE REFERENCE'S STRUCT LIES IN MEMORY (src/physics/constraints.h): the
// fields are the same in the same order; a leading quat makes fixed_constraint and slider_constraint 16-byte aligned, i.e. 8 bytes of tail
// padding (40 -> 48, 72 -> 80: MI_REF_SIZEOF_*).  Only the fields are read / written, the padding is ignored / left untouched.
template <class P> constexpr uint32_t refSizeof() { return (std::is_same<P, mi_fixed_constraint>::value || std::is_same<P, mi_slider_constraint>::value) ? (uint32_t)((sizeof(P) + 15u) & ~15u) : (uint32_t)sizeof(P); }
static_assert(refSizeof<mi_distance_constraint>() == MI_REF_SIZEOF_DISTANCE_CONSTRAINT && refSizeof<mi_ball_constraint>() == MI_REF_SIZEOF_BALL_CONSTRAINT && refSizeof<mi_fixed_constraint>() == MI_REF_SIZEOF_FIXED_CONSTRAINT &&
              refSizeof<mi_hinge_constraint>() == MI_REF_SIZEOF_HINGE_CONSTRAINT && refSizeof<mi_cone_twist_constraint>() == MI_REF_SIZEOF_CONE_TWIST_CONSTRAINT && refSizeof<mi_slider_constraint>() == MI_REF_SIZEOF_SLIDER_CONSTRAINT, "reference struct sizes");
template <class P> static bool podSizeOk(uint32_t bytes) { return bytes == sizeof(P) || bytes == refSizeof<P>(); }
template <class JT>
static int jointAddTo(mi_world& w, JT& l, uint32_t ea, uint32_t eb, const void* pod, uint32_t bytes, uint32_t* out) {
    typedef typename std::remove_reference<decltype(l.pods[0])>::type P;
    if (!podSizeOk<P>(bytes)) return fail(MI_ERR_INVALID_ARGUMENT, "constraint pod size mismatch");
    if (ea >= w.entities.size() || eb >= w.entities.size() || w.entities[ea].rb < 0 || w.entities[eb].rb < 0)
        return fail(MI_ERR_INVALID_ARGUMENT, "both constraint entities must be rigid bodies");
    P p; std::memcpy(&p, pod, sizeof(P));
    const uint32_t handle = (uint32_t)l.denseOf.size();
    if (out) *out = handle;
    l.denseOf.push_back((int32_t)l.pods.size()); l.handleAt.push_back(handle);
    l.ents.push_back(make_uint2(ea, eb)); l.seq.push_back(w.joints.nextSeq++);
    l.pods.push_back(p);
    l.bodies.push_back(make_uint2((uint32_t)w.entities[ea].rb, (uint32_t)w.entities[eb].rb));
    return MI_OK;
}
// deleteConstraint / deleteAllConstraints / deleteAllConstraintsFromEntity — src/physics/physics.cpp:443-539
int JointSet::destroy(uint32_t type, uint32_t id) {
    { int rc = pullDeviceWrites(); if (rc != MI_OK) return rc; }
    bool ok = false;
    withType(type, [&](auto& l) { ok = l.destroy(id); });
    return ok ? MI_OK : fail(MI_ERR_INVALID_ARGUMENT, "bad constraint type or id");
}
void JointSet::destroyAll() { (void)pullDeviceWrites(); each([](uint32_t, auto& l) { l.clearAll(); }); }
void JointSet::destroyOfEntity(uint32_t entity) {
    struct Hit { uint64_t seq; uint32_t type, handle; };
    std::vector<Hit> hits;
    each([&](uint32_t type, const auto& l) { for (size_t d = 0; d < l.pods.size(); ++d) if (l.ents[d].x == entity || l.ents[d].y == entity) hits.push_back(Hit{l.seq[d], type, l.handleAt[d]}); });
    std::sort(hits.begin(), hits.end(), [](const Hit& x, const Hit& y) { return x.seq > y.seq; });   // the entity's edge list is newest first
    for (const Hit& h : hits) (void)destroy(h.type, h.handle);
}
int JointSet::add(mi_world& w, uint32_t type, uint32_t ea, uint32_t eb, const void* pod, uint32_t bytes, uint32_t* out) {
    { int rc = pullDeviceWrites(); if (rc != MI_OK) return rc; }
    int rc = MI_OK;
    return withType(type, [&](auto& l) { rc = jointAddTo(w, l, ea, eb, pod, bytes, out); }) ? rc : fail(MI_ERR_INVALID_ARGUMENT, "bad constraint type");
}
template <class JT> static int jointCopy(JT& l, uint32_t id, void* dst, const void* src, uint32_t bytes) {
    typedef typename std::remove_reference<decltype(l.pods[0])>::type P;
    if (!podSizeOk<P>(bytes) || l.dense(id) < 0) return fail(MI_ERR_INVALID_ARGUMENT, "bad constraint id or pod size");
    if (src) std::memcpy(&l.pods[l.dense(id)], src, sizeof(P)); else std::memcpy(dst, &l.pods[l.dense(id)], sizeof(P));
    return MI_OK;
}
int JointSet::update(uint32_t type, uint32_t id, const void* pod, uint32_t bytes) {
    { int rc = pullDeviceWrites(); if (rc != MI_OK) return rc; }   // (the re-upload sends the WHOLE array: what the device wrote into other constraints must be in it)
    int rc = MI_OK;
    return withType(type, [&](auto& l) { l.podsDirty = true; rc = jointCopy(l, id, nullptr, pod, bytes); }) ? rc : fail(MI_ERR_INVALID_ARGUMENT, "bad constraint type");
}
// Brings the host mirror up to date with what mi_constraints_update_device_async wrote (per type; a no-op otherwise).  Positions in dPods are positions
// in `pods` as long as no constraint of the type was created or destroyed since the upload — and both pull first.
int JointSet::pullDeviceWrites() {
    if (!tryEach([](uint32_t, auto& t) { return t.deviceNewer; })) return MI_OK;
    HIP_TRY(hipSetDevice(mirrorDevice));
    auto pull = [&](uint32_t, auto& t) -> hipError_t {
        if (!t.deviceNewer) return hipSuccess;
        t.deviceNewer = false;
        if (t.pods.empty() || !t.dPods.p || t.pods.size() > t.dPods.cap) return hipSuccess;
        return hipMemcpyAsync(t.pods.data(), t.dPods.p, t.pods.size() * sizeof(t.pods[0]), hipMemcpyDeviceToHost, mirrorStream);
    };
    HIP_TRY(tryEach(pull));   // every pull enqueued, ONE wait
    HIP_TRY(hipStreamSynchronize(mirrorStream));
    return MI_OK;
}
int JointSet::uploadPods(hipStream_t st) {   // the host copy is authoritative for the PODs (unless pullDeviceWrites has something to fetch: the callers that dirty it pull first)
    HIP_TRY(tryEach([&](uint32_t, auto& l) { return l.podsDirty ? l.uploadPods(st) : hipSuccess; }));
    return MI_OK;
}
int JointSet::get(uint32_t type, uint32_t id, void* pod, uint32_t bytes) {
    { int rc = pullDeviceWrites(); if (rc != MI_OK) return rc; }
    int rc = MI_OK;
    return withType(type, [&](auto& l) { rc = jointCopy(l, id, pod, nullptr, bytes); }) ? rc : fail(MI_ERR_INVALID_ARGUMENT, "bad constraint type");
}
static void put3(float* f, V3 v) { f[0] = v.x; f[1] = v.y; f[2] = v.z; }
static void put4(float* f, Q4 q) { f[0] = q.x; f[1] = q.y; f[2] = q.z; f[3] = q.w; }
int JointSet::addFromGlobal(mi_world& w, uint32_t type, uint32_t ea, uint32_t eb, const float* anchor, const float* axisIn, float l0, float l1, uint32_t* out) {
    if (ea >= w.entities.size() || eb >= w.entities.size()) return fail(MI_ERR_INVALID_ARGUMENT, "entity out of range");
    const HEntity& A = w.entities[ea]; const HEntity& B = w.entities[eb];
    auto invPos = [](const HEntity& e, V3 p) { V3 r = rotate(conj(e.rot), p - e.pos); return V3(r.x / 1.f, r.y / 1.f, r.z / 1.f); };   // inverseTransformPosition (scale = 1)
    auto invDir = [](const HEntity& e, V3 d) { return rotate(conj(e.rot), d); };
    V3 ga(anchor[0], anchor[1], anchor[2]);
    V3 gx = axisIn ? V3(axisIn[0], axisIn[1], axisIn[2]) : V3();
    switch (type) {
        case MI_CONSTRAINT_DISTANCE: {   // anchor = globalAnchorA, axis = globalAnchorB (physics.cpp:147-156)
            mi_distance_constraint c; put3(c.local_anchor_a, invPos(A, ga)); put3(c.local_anchor_b, invPos(B, gx)); c.global_length = len(ga - gx);
            return add(w, type, ea, eb, &c, sizeof(c), out);
        }
        case MI_CONSTRAINT_BALL: {
            mi_ball_constraint c; put3(c.local_anchor_a, invPos(A, ga)); put3(c.local_anchor_b, invPos(B, ga));
            return add(w, type, ea, eb, &c, sizeof(c), out);
        }
        case MI_CONSTRAINT_FIXED: {
            mi_fixed_constraint c; put3(c.local_anchor_a, invPos(A, ga)); put3(c.local_anchor_b, invPos(B, ga));
            put4(c.initial_inv_rotation_difference, conj(B.rot) * A.rot);
            return add(w, type, ea, eb, &c, sizeof(c), out);
        }
        case MI_CONSTRAINT_HINGE: {
            mi_hinge_constraint c;
            put3(c.local_anchor_a, invPos(A, ga)); put3(c.local_anchor_b, invPos(B, ga));
            V3 axA = invDir(A, gx), axB = invDir(B, gx);
            put3(c.local_hinge_axis_a, axA); put3(c.local_hinge_axis_b, axB);
            V3 t = tangentOf(axA), bt = cross(axA, t);
            put3(c.local_hinge_tangent_a, t); put3(c.local_hinge_bitangent_a, bt);
            put3(c.local_hinge_tangent_b, rotate(conj(B.rot), rotate(A.rot, t)));
            c.min_rotation_limit = l0; c.max_rotation_limit = l1;
            c.motor_type = MI_MOTOR_VELOCITY; c.motor_velocity_or_target_angle = 0.f; c.max_motor_torque = -1.f;
            return add(w, type, ea, eb, &c, sizeof(c), out);
        }
        case MI_CONSTRAINT_CONE_TWIST: {
            mi_cone_twist_constraint c;
            put3(c.local_anchor_a, invPos(A, ga)); put3(c.local_anchor_b, invPos(B, ga));
            c.swing_limit = l0; c.twist_limit = l1;
            V3 axA = invDir(A, gx), axB = invDir(B, gx);
            put3(c.local_limit_axis_a, axA); put3(c.local_limit_axis_b, axB);
            V3 t = tangentOf(axA), bt = cross(axA, t);
            put3(c.local_limit_tangent_a, t); put3(c.local_limit_bitangent_a, bt);
            put3(c.local_limit_tangent_b, rotate(conj(B.rot), rotate(A.rot, t)));
            c.swing_motor_type = MI_MOTOR_VELOCITY; c.swing_motor_velocity_or_target_angle = 0.f; c.max_swing_motor_torque = -1.f; c.swing_motor_axis = 0.f;
            c.twist_motor_type = MI_MOTOR_VELOCITY; c.twist_motor_velocity_or_target_angle = 0.f; c.max_twist_motor_torque = -1.f;
            return add(w, type, ea, eb, &c, sizeof(c), out);
        }
        case MI_CONSTRAINT_SLIDER: {
            mi_slider_constraint c;
            put3(c.local_anchor_a, invPos(A, ga)); put3(c.local_anchor_b, invPos(B, ga));
            put3(c.local_axis_a, invDir(A, gx));
            put4(c.initial_inv_rotation_difference, conj(B.rot) * A.rot);
            c.neg_distance_limit = l0; c.pos_distance_limit = l1;
            c.motor_type = MI_MOTOR_VELOCITY; c.motor_velocity_or_target_distance = 0.f; c.max_motor_force = -1.f;
            return add(w, type, ea, eb, &c, sizeof(c), out);
        }
    }
    return fail(MI_ERR_INVALID_ARGUMENT, "bad constraint type");
}
int JointSet::upload(mi_world& w, hipStream_t st) {
    { int rc = pullDeviceWrites(); if (rc != MI_OK) return rc; }   // (a topology upload re-sends the mirror)
    mirrorStream = st; mirrorDevice = w.device;
    if (!count()) {   // the last constraint may just have been deleted: nothing of the previous topology may survive
        releaseIslands();
        each([](uint32_t, auto& l) { l.order.clear(); });
        return MI_OK;
    }
    std::vector<float> invMass(w.bodies.size());
    for (size_t i = 0; i < w.bodies.size(); ++i) invMass[i] = w.bodies[i].invMass;
    each([&](uint32_t, auto& l) { l.computeOrder(invMass); });
    {
        std::vector<IslandDesc> islands; std::vector<IslandStep> steps; std::vector<uint32_t> islandBodies;
        buildIslands(invMass, islands, steps, islandBodies);
        releaseIslands();
        if (!islands.empty()) {
            HIP_TRY(dIslands.ensure(islands.size())); HIP_TRY(dSteps.ensure(steps.size())); HIP_TRY(dIslandBodies.ensure(islandBodies.size()));
            HIP_TRY(hipMemcpyAsync(dIslands.p, islands.data(), islands.size() * sizeof(IslandDesc), hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(dSteps.p, steps.data(), steps.size() * sizeof(IslandStep), hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(dIslandBodies.p, islandBodies.data(), islandBodies.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
            std::vector<uint8_t> bodyJ(invMass.size() + 1, 0);
            for (uint32_t b : islandBodies) if (b < invMass.size() && invMass[b] != 0.f) bodyJ[b] = 1;
            HIP_TRY(dBodyJ.ensure(bodyJ.size()));
            HIP_TRY(hipMemcpyAsync(dBodyJ.p, bodyJ.data(), bodyJ.size(), hipMemcpyHostToDevice, st));
            // private islands (joints.hpp): island of every dynamic island body; per-step state and the islands' manifold lists
            std::vector<uint32_t> bodyIsland(invMass.size() + 1, 0xFFFFFFFFu);
            for (uint32_t i = 0; i < (uint32_t)islands.size(); ++i)
                for (uint32_t k = 0; k < islands[i].numBodies; ++k) { const uint32_t b = islandBodies[islands[i].bodyBegin + k]; if (b < invMass.size() && invMass[b] != 0.f) bodyIsland[b] = i; }
            HIP_TRY(dBodyIsland.ensure(bodyIsland.size()));
            HIP_TRY(hipMemcpyAsync(dBodyIsland.p, bodyIsland.data(), bodyIsland.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
            HIP_TRY(dIslState.ensure(3 * islands.size()));
            HIP_TRY(dIslEntries.ensure(islands.size() * (size_t)mi::kIslandMaxContacts));
            HIP_TRY(hipStreamSynchronize(st));   // the staging vectors are locals
            numIslands = (uint32_t)islands.size();
        }
    }
    each([](uint32_t, auto& l) { l.finishOrder(); });
    HIP_TRY(tryEach([&](uint32_t, auto& l) { return l.upload(st); }));
    each([](uint32_t, auto& l) { l.podsDirty = false; });
    return MI_OK;
}
// Connected components of the joint graph over DYNAMIC bodies; an island small enough for one wave gets a program of
// (type, colour) groups in canonical order, the rest stays with the per-colour kernels.
void JointSet::buildIslands(const std::vector<float>& invMass, std::vector<IslandDesc>& islands, std::vector<IslandStep>& steps, std::vector<uint32_t>& islandBodies) {
    const uint32_t nb = (uint32_t)invMass.size();
    std::vector<uint32_t> parent(nb);
    for (uint32_t i = 0; i < nb; ++i) parent[i] = i;
    auto find = [&](uint32_t x) { while (parent[x] != x) { parent[x] = parent[parent[x]]; x = parent[x]; } return x; };
    struct Ref { uint32_t type, joint, color; uint2 bodies; };
    std::vector<Ref> all;
    uint8_t* flags[6];   // by type: JointType::inIsland
    each([&](uint32_t type, auto& l) {
        flags[type] = l.inIsland.data();
        for (uint32_t j = 0; j < (uint32_t)l.bodies.size(); ++j) {
            uint2 b = l.bodies[j];
            bool dynA = b.x < nb && invMass[b.x] != 0.f, dynB = b.y < nb && invMass[b.y] != 0.f;
            if (dynA && dynB) parent[find(b.x)] = find(b.y);
            all.push_back(Ref{type, j, l.colorOf[j], b});
        }
    });
    // joints by island root (a joint between two non-dynamic bodies does nothing; it stays with the per-colour kernels)
    std::vector<std::vector<uint32_t>> byRoot(nb);
    for (uint32_t r = 0; r < (uint32_t)all.size(); ++r) {
        const Ref& ref = all[r];
        bool dynA = ref.bodies.x < nb && invMass[ref.bodies.x] != 0.f, dynB = ref.bodies.y < nb && invMass[ref.bodies.y] != 0.f;
        if (dynA || dynB) byRoot[find(dynA ? ref.bodies.x : ref.bodies.y)].push_back(r);
    }
    for (uint32_t root = 0; root < nb; ++root) {
        std::vector<uint32_t>& js = byRoot[root];
        if (js.empty()) continue;
        std::stable_sort(js.begin(), js.end(), [&](uint32_t x, uint32_t y) { return all[x].type != all[y].type ? all[x].type < all[y].type : all[x].color < all[y].color; });
        std::vector<uint32_t> slots;   // island-local body table (dynamic and static bodies alike; the static dummy is body index nb)
        auto slotOf = [&](uint32_t body) { for (uint32_t k = 0; k < (uint32_t)slots.size(); ++k) if (slots[k] == body) return k; slots.push_back(body); return (uint32_t)slots.size() - 1u; };
        bool fits = js.size() <= kIslandMaxJoints;
        std::vector<IslandStep> st;
        IslandDesc d{};
        uint32_t group = 0;   // groups are numbered type-major, colour-major within the island
        for (size_t k = 0; fits && k < js.size(); ++k) {
            const Ref& ref = all[js[k]];
            if (ref.color >= 64u) { fits = false; break; }
            if (k > 0 && (all[js[k - 1]].type != ref.type || all[js[k - 1]].color != ref.color)) ++group;
            st.push_back(IslandStep{ref.joint, (uint16_t)slotOf(ref.bodies.x), (uint16_t)slotOf(ref.bodies.y), (uint16_t)ref.type, (uint16_t)group});
            d.typeGroups[ref.type + 1] = group + 1;   // end of this type's groups so far
            if (slots.size() > kIslandMaxBodies) fits = false;
        }
        if (!fits) continue;
        for (uint32_t t = 1; t <= 6; ++t) d.typeGroups[t] = std::max(d.typeGroups[t], d.typeGroups[t - 1]);   // absent types: empty range
        d.bodyBegin = (uint32_t)islandBodies.size(); d.numBodies = (uint32_t)slots.size(); d.stepBegin = (uint32_t)steps.size(); d.numJoints = (uint32_t)st.size();
        steps.insert(steps.end(), st.begin(), st.end());
        islandBodies.insert(islandBodies.end(), slots.begin(), slots.end());
        islands.push_back(d);
        for (uint32_t r : js) flags[all[r].type][all[r].joint] = 1;
    }
}
static BodyView bodyView(mi_world& w) { return BodyView{w.gPos.p, w.gInvI.p, w.gVel.p, w.bRot.p, w.bCogInvMass.p, w.shard.enabled ? w.shard.active.p : nullptr}; }
int JointSet::initialize(mi_world& w, float dt, hipStream_t st) {
    if (!count()) return MI_OK;
    BodyView bv = bodyView(w);
    uint32_t dummy = (uint32_t)w.bodies.size();
    mi::Launcher& L = w.L;
    each([&](uint32_t, auto& l) { l.launchInit(L, dummy, bv, dt, st); });
    return MI_OK;
}
int JointSet::solveIterationReference(mi_world& w, hipStream_t st) {
    if (!count()) return MI_OK;
    BodyView bv = bodyView(w);
    mi::Launcher& L = w.L;
    HIP_TRY(tryEach([&](uint32_t, auto& l) { return l.launchSolveReference(L, bv, st); }));
    return MI_OK;
}
void JointSet::solveIteration(mi_world& w, hipStream_t st) {
    if (!count()) return;
    BodyView bv = bodyView(w);
    mi::Launcher& L = w.L;
    if (numIslands) L.launch(k_joint_islands, dim3(numIslands), dim3(64), 0, st, dIslands.p, dSteps.p, dIslandBodies.p, islandUpd(), bv);
    each([&](uint32_t, auto& l) { l.launchSolve(L, bv, st); });
}
