// learning_shared.hpp — the environment arithmetic of the learning library, stated ONCE for both of its translation units:
// learning.cpp (g++, the host path) and learning_device.hip (hipcc, the device path's kernels).  The little math of
// src/core/math.h, the xorshift64 generator, the humanoid's constant tables (src/physics/ragdoll.cpp:9-123) and state /
// part points / reward / push draw of src/learning/learned_locomotion.cpp — every expression in the reference's operation
// order.  Both units are built without FMA contraction and with correctly rounded division and square root, so whatever is
// made of + - * / sqrt gives the same bits on either side; only acos and exp (the reward) come from different maths libraries.
//
// Poses are read through PoseRows: per-entity rows [n][3] positions, [n][4] rotations, [n][3] linear and angular velocities —
// the host's cache (refreshTransforms) or the device's (mi_world_get_transforms_device_async).
#ifndef MI_LEARNING_SHARED_HPP
#define MI_LEARNING_SHARED_HPP
#include <cmath>
#include <cstdint>

#include "../../include/mi_constraints.h"

#if defined(__HIPCC__)
#define LEARN_HD __host__ __device__ inline
#else
#define LEARN_HD inline
#endif

namespace learn {

// ---- the little math the environment needs (src/core/math.h; operation order kept) ---------------------------------------
struct v3 { float x, y, z; };
struct q4 { float x, y, z, w; };
LEARN_HD v3 operator+(v3 a, v3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
LEARN_HD v3 operator-(v3 a, v3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
LEARN_HD v3 operator*(v3 a, float s) { return {a.x * s, a.y * s, a.z * s}; }
LEARN_HD v3 operator*(float s, v3 a) { return a * s; }
LEARN_HD float dot(v3 a, v3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
LEARN_HD v3 cross(v3 a, v3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
LEARN_HD float length(v3 a) { return std::sqrt(dot(a, a)); }
LEARN_HD v3 normalize(v3 a) { float l = length(a); return a * (1.f / l); }
LEARN_HD q4 conjugate(q4 a) { return {-a.x, -a.y, -a.z, a.w}; }
LEARN_HD q4 operator*(q4 a, q4 b) {   // math.h:627-633
    v3 av{a.x, a.y, a.z}, bv{b.x, b.y, b.z};
    float w = a.w * b.w - dot(av, bv);
    v3 v = av * b.w + bv * a.w + cross(av, bv);
    return {v.x, v.y, v.z, w};
}
LEARN_HD v3 operator*(q4 q, v3 v) { q4 p{v.x, v.y, v.z, 0.f}; q4 r = q * p * conjugate(q); return {r.x, r.y, r.z}; }   // math.h:642-646
LEARN_HD float lerpf(float l, float u, float t) { return l + t * (u - l); }
LEARN_HD float clampf(float v, float l, float u) { float r = l > v ? l : v; return u < r ? u : r; }
constexpr float kPi = 3.14159265359f;

// random_number_generator (src/core/random.h:5-52): xorshift64
struct Rng {
    uint64_t state;
    LEARN_HD uint64_t next64() { uint64_t x = state; x ^= x << 13; x ^= x >> 7; x ^= x << 17; state = x; return x; }
    LEARN_HD uint32_t next32() { return (uint32_t)next64(); }
    LEARN_HD uint32_t between(uint32_t lo, uint32_t hi) { return next32() % (hi - lo) + lo; }
    LEARN_HD float float01() { return (float)next32() / (float)0xFFFFFFFFu; }
    LEARN_HD float floatBetween(float lo, float hi) { return lerpf(lo, hi, (float01() - 0.f) / (1.f - 0.f)); }
};

// ---- the humanoid (src/physics/ragdoll.cpp:9-123) ------------------------------------------------------------------------
constexpr int kParts = 14, kCone = 7, kHinge = 6;
constexpr int kActionFloats = kCone * 3 + kHinge;          // learning_action: 27
constexpr int kStateFloats = 13 * 3 + kActionFloats;       // learning_state: 66
constexpr int kEntitiesPerEnv = kParts + 1;                // ground + body parts
constexpr float kScale = 0.42f;
enum Part { TORSO, HEAD, L_UPPER_ARM, L_LOWER_ARM, R_UPPER_ARM, R_LOWER_ARM, L_UPPER_LEG, L_LOWER_LEG, L_FOOT, L_TOES, R_UPPER_LEG, R_LOWER_LEG, R_FOOT, R_TOES };
// (the tables are host data: a kernel gets what it needs of them through EnvTables)
const int kParent[kParts] = {-1, TORSO, TORSO, L_UPPER_ARM, TORSO, R_UPPER_ARM, TORSO, L_UPPER_LEG, L_LOWER_LEG, L_FOOT, TORSO, R_UPPER_LEG, R_LOWER_LEG, R_FOOT};
struct PartDef { v3 pos; float zDeg; };
const PartDef kPartDefs[kParts] = {
    {{0.f, 0.f, 0.f}, 0.f}, {{0.f, 1.45f, 0.f}, 0.f},
    {{-0.6f, 0.75f, 0.f}, -30.f}, {{-0.884f, 0.044f, -0.043f}, -20.f}, {{0.6f, 0.75f, 0.f}, 30.f}, {{0.884f, 0.044f, -0.043f}, 20.f},
    {{-0.371f, -0.812f, 0.f}, -10.f}, {{-0.452f, -1.955f, 0.f}, -3.5f}, {{-0.498f, -2.585f, -0.18f}, 0.f}, {{-0.498f, -2.585f, -0.637f}, 0.f},
    {{0.371f, -0.812f, 0.f}, 10.f}, {{0.452f, -1.955f, 0.f}, 3.5f}, {{0.498f, -2.585f, -0.18f}, 0.f}, {{0.498f, -2.585f, -0.637f}, 0.f}};
struct ColDef { int part; bool box; v3 a, b; float r; };   // capsule (a, b, r) or AABB (centre a = 0, half extents b), before `scale *`
const ColDef kColDefs[] = {
    {TORSO, false, {-0.2f, 0.f, 0.f}, {0.2f, 0.f, 0.f}, 0.25f}, {TORSO, false, {-0.16f, 0.32f, 0.f}, {0.16f, 0.32f, 0.f}, 0.2f},
    {TORSO, false, {-0.14f, 0.62f, 0.f}, {0.14f, 0.62f, 0.f}, 0.22f}, {TORSO, false, {-0.14f, 0.92f, 0.f}, {0.14f, 0.92f, 0.f}, 0.2f},
    {HEAD, false, {0.f, -0.075f, 0.f}, {0.f, 0.075f, 0.f}, 0.25f},
    {L_UPPER_ARM, false, {0.f, -0.2f, 0.f}, {0.f, 0.2f, 0.f}, 0.15f}, {L_LOWER_ARM, false, {0.f, -0.2f, 0.f}, {0.f, 0.2f, 0.f}, 0.15f},
    {R_UPPER_ARM, false, {0.f, -0.2f, 0.f}, {0.f, 0.2f, 0.f}, 0.15f}, {R_LOWER_ARM, false, {0.f, -0.2f, 0.f}, {0.f, 0.2f, 0.f}, 0.15f},
    {L_UPPER_LEG, false, {0.f, -0.3f, 0.f}, {0.f, 0.3f, 0.f}, 0.25f}, {L_LOWER_LEG, false, {0.f, -0.3f, 0.f}, {0.f, 0.3f, 0.f}, 0.18f},
    {L_FOOT, true, {0.f, 0.f, 0.f}, {0.1587f, 0.1f, 0.3424f}, 0.f}, {L_TOES, false, {-0.0587f, 0.f, 0.f}, {0.0587f, 0.f, 0.f}, 0.1f},
    {R_UPPER_LEG, false, {0.f, -0.3f, 0.f}, {0.f, 0.3f, 0.f}, 0.25f}, {R_LOWER_LEG, false, {0.f, -0.3f, 0.f}, {0.f, 0.3f, 0.f}, 0.18f},
    {R_FOOT, true, {0.f, 0.f, 0.f}, {0.1587f, 0.1f, 0.3424f}, 0.f}, {R_TOES, false, {-0.0587f, 0.f, 0.f}, {0.0587f, 0.f, 0.f}, 0.1f}};
constexpr int kNumCols = sizeof(kColDefs) / sizeof(kColDefs[0]);
// joints in creation order (ragdoll.cpp:100-116); coneIndex / hingeIndex = slot in humanoid_ragdoll::coneTwistConstraints / hingeConstraints
struct JointDef { bool cone; int slot, a, b, anchorPart; v3 anchor; int axisPart; v3 axis; bool normalizeAxis; float l0, l1; };
const JointDef kJointDefs[] = {
    {true, 0, TORSO, HEAD, TORSO, {0.f, 1.2f, 0.f}, -1, {0.f, 1.f, 0.f}, false, 50.f, 90.f},
    {true, 1, TORSO, L_UPPER_ARM, TORSO, {-0.4f, 1.f, 0.f}, -1, {-1.f, 0.f, 0.f}, false, 130.f, 90.f},
    {false, 0, L_UPPER_ARM, L_LOWER_ARM, L_UPPER_ARM, {0.f, -0.42f, 0.f}, -1, {1.f, 0.f, 1.f}, true, -5.f, 85.f},
    {true, 2, TORSO, R_UPPER_ARM, TORSO, {0.4f, 1.f, 0.f}, -1, {1.f, 0.f, 0.f}, false, 130.f, 90.f},
    {false, 1, R_UPPER_ARM, R_LOWER_ARM, R_UPPER_ARM, {0.f, -0.42f, 0.f}, -1, {1.f, 0.f, -1.f}, true, -5.f, 85.f},
    {true, 3, TORSO, L_UPPER_LEG, TORSO, {-0.3f, -0.25f, 0.f}, L_UPPER_LEG, {0.f, -1.f, 0.f}, false, -1000.f, 30.f},
    {false, 2, L_UPPER_LEG, L_LOWER_LEG, L_UPPER_LEG, {0.f, -0.6f, 0.f}, -1, {1.f, 0.f, 0.f}, false, -90.f, 5.f},
    {true, 4, L_LOWER_LEG, L_FOOT, L_LOWER_LEG, {0.f, -0.52f, 0.f}, L_LOWER_LEG, {0.f, -1.f, 0.f}, false, 75.f, 20.f},
    {false, 3, L_FOOT, L_TOES, L_FOOT, {0.f, 0.f, -0.36f}, -1, {1.f, 0.f, 0.f}, false, -45.f, 45.f},
    {true, 5, TORSO, R_UPPER_LEG, TORSO, {0.3f, -0.25f, 0.f}, R_UPPER_LEG, {0.f, -1.f, 0.f}, false, -1000.f, 30.f},
    {false, 4, R_UPPER_LEG, R_LOWER_LEG, R_UPPER_LEG, {0.f, -0.6f, 0.f}, -1, {1.f, 0.f, 0.f}, false, -90.f, 5.f},
    {true, 6, R_LOWER_LEG, R_FOOT, R_LOWER_LEG, {0.f, -0.52f, 0.f}, R_LOWER_LEG, {0.f, -1.f, 0.f}, false, 75.f, 20.f},
    {false, 5, R_FOOT, R_TOES, R_FOOT, {0.f, 0.f, -0.36f}, -1, {1.f, 0.f, 0.f}, false, -45.f, 45.f}};

struct Target { v3 pos[6], vel[6]; q4 localRot; };   // learning_target
// one environment's episode state as the host keeps it (the device path holds the same fields in arrays of their own)
struct Env {
    float smoothed[kActionFloats];   // lastSmoothedAction
    float headTargetHeight;
    v3 torsoVelocityTarget;          // always kTorsoVelocityTarget (training_locomotion::reset); the device path keeps no copy of it
    Target targets[kParts];
    Rng rng;
    float totalReward;
    v3 origin;
};
constexpr v3 kTorsoVelocityTarget{0.f, 0.f, 0.f};
// what is the same for every environment and every step: the parent table, the parts' local centres of gravity (from the physics
// library's mass properties) and getLocalPositions (the 6 face centres of each part's local collider AABB)
struct EnvTables { int parent[kParts]; v3 localCOG[kParts]; v3 localPositions[kParts][6]; };

struct PoseRows { const float *pos, *rot, *lin, *ang; };
LEARN_HD uint32_t entityOf(int env, int part) { return (uint32_t)(env * kEntitiesPerEnv + 1 + part); }
LEARN_HD v3 entityPos(const PoseRows& r, uint32_t e) { return {r.pos[3 * e], r.pos[3 * e + 1], r.pos[3 * e + 2]}; }
LEARN_HD q4 entityRot(const PoseRows& r, uint32_t e) { return {r.rot[4 * e], r.rot[4 * e + 1], r.rot[4 * e + 2], r.rot[4 * e + 3]}; }
LEARN_HD v3 entityLin(const PoseRows& r, uint32_t e) { return {r.lin[3 * e], r.lin[3 * e + 1], r.lin[3 * e + 2]}; }
LEARN_HD v3 entityAng(const PoseRows& r, uint32_t e) { return {r.ang[3 * e], r.ang[3 * e + 1], r.ang[3 * e + 2]}; }
LEARN_HD v3 globalCOG(const PoseRows& r, uint32_t e, v3 localCOG) { return entityPos(r, e) + entityRot(r, e) * localCOG; }   // rigid_body_component::getGlobalCOGPosition

// learned_locomotion::updateConstraint x13 over the smoothed action (learned_locomotion.cpp:74-115): position motors, 200 Nm
LEARN_HD void smoothAction(float* smoothed, const float* action /* or null = zero */) {
    const float beta = 0.1f;
    for (int i = 0; i < kActionFloats; ++i) smoothed[i] = lerpf(smoothed[i], action ? action[i] : 0.f, beta);
}
LEARN_HD void armMotors(const float* smoothed, mi_cone_twist_constraint* cones /* [kCone] */, mi_hinge_constraint* hinges /* [kHinge] */) {
    for (int s = 0; s < kCone; ++s) {
        mi_cone_twist_constraint& c = cones[s];
        c.max_swing_motor_torque = 200.f; c.max_twist_motor_torque = 200.f;
        c.swing_motor_type = 1u; c.twist_motor_type = 1u;   // constraint_position_motor
        c.twist_motor_velocity_or_target_angle = smoothed[3 * s];        // cone_twist_action: twistTargetAngle, swingTargetAngle, swingAxisAngle
        c.swing_motor_velocity_or_target_angle = smoothed[3 * s + 1];
        c.swing_motor_axis = smoothed[3 * s + 2];
    }
    for (int s = 0; s < kHinge; ++s) {
        mi_hinge_constraint& h = hinges[s];
        h.max_motor_torque = 200.f; h.motor_type = 1u;
        h.motor_velocity_or_target_angle = smoothed[kCone * 3 + s];
    }
}

// the random push (learned_locomotion.cpp:458-468): with probability 0.02 a ray from 5 m away at a random body part.  The draws
// are made in this order whether or not anybody uses the ray.
LEARN_HD bool drawPush(Rng& rng, const PoseRows& rows, int e, v3& origin, v3& dir) {
    if (!(rng.float01() < 0.02f)) return false;
    uint32_t part = rng.between(0, kParts - 1);
    v3 target = entityPos(rows, entityOf(e, (int)part)) + v3{0.f, 0.2f, 0.f};
    float dx = rng.floatBetween(-1.f, 1.f), dz = rng.floatBetween(-1.f, 1.f);
    dir = normalize(v3{dx, 0.f, dz});
    origin = target - dir * 5.f;
    return true;
}

// learned_locomotion::getState (learned_locomotion.cpp:117-156); returns hasFallen (head below 1 m)
LEARN_HD bool stateOf(const PoseRows& rows, const v3* localCOG, int e, const float* smoothed, float* out) {
    v3 cog = globalCOG(rows, entityOf(e, TORSO), localCOG[TORSO]);
    cog.y = 0.f;
    auto part = [&](int p, float* posOut, float* velOut) {
        v3 lp = globalCOG(rows, entityOf(e, p), localCOG[p]) - cog, lv = entityLin(rows, entityOf(e, p));   // trs(cog, identity): conjugate(identity) * (p - cog) / 1
        posOut[0] = lp.x; posOut[1] = lp.y; posOut[2] = lp.z; velOut[0] = lv.x; velOut[1] = lv.y; velOut[2] = lv.z;
    };
    // learning_state layout (learned_locomotion.h:41-65)
    v3 cv = entityLin(rows, entityOf(e, TORSO));
    out[0] = cv.x; out[1] = cv.y; out[2] = cv.z;
    part(L_TOES, out + 3, out + 6); part(R_TOES, out + 9, out + 12); part(TORSO, out + 15, out + 18); part(HEAD, out + 21, out + 24);
    part(L_LOWER_ARM, out + 27, out + 30); part(R_LOWER_ARM, out + 33, out + 36);
    for (int i = 0; i < kActionFloats; ++i) out[39 + i] = smoothed[i];
    return out[21 + 1] < 1.f;
}

// training_locomotion::getBodyPartTarget / readPartDifference (learned_locomotion.cpp:248-317)
LEARN_HD void partPoints(const PoseRows& rows, const EnvTables& tb, int e, int p, v3 pos[6], v3 vel[6], q4& localRot) {
    const uint32_t ent = entityOf(e, p);
    const v3 tp = entityPos(rows, ent); const q4 tr = entityRot(rows, ent);
    const v3 cog = globalCOG(rows, ent, tb.localCOG[p]), lv = entityLin(rows, ent), av = entityAng(rows, ent);
    for (int i = 0; i < 6; ++i) {
        v3 gp = tr * tb.localPositions[p][i] + tp;            // transformPosition (scale 1)
        pos[i] = gp;
        vel[i] = lv + cross(av, gp - cog);                   // getGlobalPointVelocity
    }
    q4 parentRot = tb.parent[p] >= 0 ? entityRot(rows, entityOf(e, tb.parent[p])) : q4{0.f, 0.f, 0.f, 1.f};
    localRot = tr * conjugate(parentRot);
}
// one part's share of getReward's three sums (learned_locomotion.cpp:318-333)
LEARN_HD void partErrors(const v3 pos[6], const v3 vel[6], q4 localRot, const Target& target, float& pe, float& ve, float& re) {
    pe = 0.f; ve = 0.f;
    for (int i = 0; i < 6; ++i) { pe += length(pos[i] - target.pos[i]); ve += length(vel[i] - target.vel[i]); }
    q4 diff = target.localRot * conjugate(localRot);
    re = 2.f * std::acos(clampf(diff.w, -1.f, 1.f));
}
// ... and the reward from the sums over the 14 parts, added in part order (learned_locomotion.cpp:334-345)
LEARN_HD float rewardOfSums(float positionError, float velocityError, float rotationError, v3 torsoVelocity, v3 torsoVelocityTarget, float headTargetHeight, float headHeight) {
    float vcmError = length(torsoVelocity - torsoVelocityTarget);
    float rp = std::exp(-10.f / kParts * positionError), rv = std::exp(-1.f / kParts * velocityError);
    float rlocal = std::exp(-10.f / kParts * rotationError), rvcm = std::exp(-vcmError);
    float fall = clampf(1.3f - 1.4f * (headTargetHeight - headHeight), 0.f, 1.f);
    return fall * (rp + rv + rlocal + rvcm);
}

}  // namespace learn
#endif
