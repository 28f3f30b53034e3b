// learning_device.hip — the device-resident step of the batched learning environments (include/mi_learning.h:
// resetPhysicsBatchDevice / updatePhysicsBatchDevice / getPhysicsStream).
//
// updatePhysicsBatch (learning.cpp) crosses the host in both directions on every step: actions up as constraint PODs, push
// rays up, every entity's pose and velocity down, states and rewards computed in a host loop, resets up.  Here the same step
// keeps every per-environment byte on the device — actions come from a device buffer, states / rewards / done flags go to
// device buffers — through four device-side calls of the physics library (include/mi_physics.h: transforms, constraint PODs,
// interactions, masked body states) and two kernels:
//
//   k_learn_actions        one lane per environment: smooth the action, arm the 13 position motors in the environment's POD copy,
//                          draw the random push and write its ray (or an empty range) into the environment's ray slot
//   k_learn_state_reward   16 lanes per environment, one per body part (4 environments per wave): the part's 6 points, its errors
//                          against the target; one lane then adds the 14 parts in part order, writes the 66 state floats, the
//                          reward and the done flag; a fallen environment is reset in place by its 16 lanes
//
// The arithmetic is learning_shared.hpp, the very functions the host path runs, built with the same floating-point rules (no
// contraction, correctly rounded division and square root): states and done flags equal the host path's bit for bit, rewards up
// to the difference between the two maths libraries' acos and exp.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/mi_learning.h"
#include "learning_device.hpp"

#define EXPORT extern "C" __attribute__((visibility("default")))

namespace {
using namespace learn;

constexpr int kEnvsPerBlock = 16, kLanesPerEnv = 16;   // k_learn_state_reward: 256 lanes = 4 waves of 4 environments

// smoothing, motors, push draw (stepAll's first two phases)
__global__ __launch_bounds__(64) void k_learn_actions(int n, const float* __restrict__ actions, float* __restrict__ smoothed, mi_cone_twist_constraint* __restrict__ cones,
                                                      mi_hinge_constraint* __restrict__ hinges, uint64_t* __restrict__ rng, PoseRows rows, float* __restrict__ rays8, uint32_t* __restrict__ ranges2,
                                                      uint32_t* __restrict__ counters) {
    const int e = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (e >= n) return;
    float sm[kActionFloats];
    for (int i = 0; i < kActionFloats; ++i) sm[i] = smoothed[(size_t)e * kActionFloats + i];
    smoothAction(sm, actions + (size_t)e * kActionFloats);
    for (int i = 0; i < kActionFloats; ++i) smoothed[(size_t)e * kActionFloats + i] = sm[i];
    armMotors(sm, cones + (size_t)e * kCone, hinges + (size_t)e * kHinge);
    Rng r{rng[e]};
    v3 origin, dir;
    float* ray = rays8 + 8 * (size_t)e;
    if (drawPush(r, rows, e, origin, dir)) {
        ray[0] = origin.x; ray[1] = origin.y; ray[2] = origin.z; ray[3] = dir.x; ray[4] = dir.y; ray[5] = dir.z; ray[6] = 1000.f; ray[7] = 0.f;
        ranges2[2 * e] = (uint32_t)(e * kEntitiesPerEnv); ranges2[2 * e + 1] = (uint32_t)((e + 1) * kEntitiesPerEnv);
        atomicAdd(&counters[0], 1u);
    } else { ranges2[2 * e] = 0u; ranges2[2 * e + 1] = 0u; }   // an empty range: the slot costs the interaction kernel nothing
    rng[e] = r.state;
}

struct EnvArrays {   // the device twin of learning.cpp's Env: every field a step reads or writes (torsoVelocityTarget is the constant kTorsoVelocityTarget, totalReward is not observable)
    float* smoothed;          // [n][27]
    float* headTargetHeight;  // [n]
    Target* targets;          // [n][14]
    mi_cone_twist_constraint* cones; mi_hinge_constraint* hinges;
};

// state, reward, done flag; reset of the fallen in place (stepAll's last three phases).  pos / rot / lin / ang: the device pose cache, which
// the reset patches like resetEnvs patches the host's.
__global__ __launch_bounds__(256) void k_learn_state_reward(int n, float* pos, float* rot, float* lin, float* ang, const EnvTables* __restrict__ tables, EnvArrays env,
                                                            const float* __restrict__ initialStates, float* __restrict__ outStates, float* __restrict__ outRewards, int* __restrict__ outDone,
                                                            uint32_t* __restrict__ counters) {
    __shared__ float sPe[kEnvsPerBlock][kParts], sVe[kEnvsPerBlock][kParts], sRe[kEnvsPerBlock][kParts];
    __shared__ int sFell[kEnvsPerBlock];
    __shared__ EnvTables tb;
    for (uint32_t i = threadIdx.x; i < sizeof(EnvTables) / 4u; i += blockDim.x) reinterpret_cast<uint32_t*>(&tb)[i] = reinterpret_cast<const uint32_t*>(tables)[i];
    __syncthreads();
    const int le = (int)threadIdx.x / kLanesPerEnv, p = (int)threadIdx.x % kLanesPerEnv;
    const int e = (int)blockIdx.x * kEnvsPerBlock + le;
    const bool live = e < n;
    const PoseRows rows{pos, rot, lin, ang};
    if (live && p < kParts) {
        v3 pp[6], pv[6]; q4 localRot;
        partPoints(rows, tb, e, p, pp, pv, localRot);
        float pe, ve, re;
        partErrors(pp, pv, localRot, env.targets[(size_t)e * kParts + p], pe, ve, re);
        sPe[le][p] = pe; sVe[le][p] = ve; sRe[le][p] = re;
    }
    __syncthreads();
    if (live && p == 0) {
        float state[kStateFloats];
        const bool failure = stateOf(rows, tb.localCOG, e, env.smoothed + (size_t)e * kActionFloats, state);
        float reward = 0.f;
        if (!failure) {
            float positionError = 0.f, velocityError = 0.f, rotationError = 0.f;
            for (int k = 0; k < kParts; ++k) { positionError += sPe[le][k]; velocityError += sVe[le][k]; rotationError += sRe[le][k]; }   // the host's order: the sums decide the bits
            reward = rewardOfSums(positionError, velocityError, rotationError, entityLin(rows, entityOf(e, TORSO)), kTorsoVelocityTarget, env.headTargetHeight[e], entityPos(rows, entityOf(e, HEAD)).y);
        } else atomicAdd(&counters[1], 1u);
        for (int i = 0; i < kStateFloats; ++i) outStates[(size_t)e * kStateFloats + i] = state[i];
        outRewards[e] = reward;
        outDone[e] = failure ? 1 : 0;
        sFell[le] = failure ? 1 : 0;
    }
    __syncthreads();
    const bool reset = live && sFell[le] != 0;
    // resetEnvs: the pose cache of the reset parts = the initial pose, velocities zero ...
    if (reset && p < kParts) {
        const uint32_t ent = entityOf(e, p);
        const float* st = initialStates + ((size_t)e * kParts + p) * MI_BODY_STATE_FLOATS;
        for (int k = 0; k < 3; ++k) { pos[3 * ent + k] = st[k]; lin[3 * ent + k] = 0.f; ang[3 * ent + k] = 0.f; }
        for (int k = 0; k < 4; ++k) rot[4 * ent + k] = st[3 + k];
    }
    __syncthreads();   // (a part's target reads its parent's patched rotation)
    // ... resetEnvState: targets from the patched pose, smoothed action zero, head target height; applyActions(null): motors re-armed with the zero action
    if (reset && p < kParts) {
        Target t;
        partPoints(rows, tb, e, p, t.pos, t.vel, t.localRot);
        env.targets[(size_t)e * kParts + p] = t;
    }
    if (reset && p == kParts) {
        float sm[kActionFloats];
        for (int i = 0; i < kActionFloats; ++i) sm[i] = 0.f;
        smoothAction(sm, nullptr);
        for (int i = 0; i < kActionFloats; ++i) env.smoothed[(size_t)e * kActionFloats + i] = sm[i];
        env.headTargetHeight[e] = entityPos(rows, entityOf(e, HEAD)).y;
        armMotors(sm, env.cones + (size_t)e * kCone, env.hinges + (size_t)e * kHinge);
    }
}

template <class T> struct Dev {
    T* p = nullptr; size_t cap = 0;   // (no destructor: like the world itself the buffers die in release(), never at process exit after the runtime has gone)
    void free() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    hipError_t ensure(size_t n) { if (n <= cap) return hipSuccess; free(); hipError_t e = hipMalloc((void**)&p, n * sizeof(T)); if (e == hipSuccess) cap = n; return e; }
    hipError_t upload(const T* src, size_t n) { hipError_t e = ensure(n); return e != hipSuccess ? e : hipMemcpy(p, src, n * sizeof(T), hipMemcpyHostToDevice); }
};

struct DeviceBatch {
    bool live = false; int n = 0; hipStream_t stream = nullptr;
    Dev<float> smoothed, headTargetHeight, pos, rot, lin, ang, rays, initialStates, states, rewards;
    Dev<Target> targets; Dev<EnvTables> tables; Dev<uint64_t> rng;
    Dev<mi_cone_twist_constraint> cones; Dev<mi_hinge_constraint> hinges;
    Dev<uint32_t> coneIdx, hingeIdx, bodyIdx, ranges, counters;   // counters: pushes drawn, environments fallen — of the step under way
    Dev<int> done;
    uint32_t* hostCounters = nullptr;   // pinned: the one thing that comes back per step (two words, not per environment)
    void release() {
        live = false; n = 0; stream = nullptr;
        for (Dev<float>* d : {&smoothed, &headTargetHeight, &pos, &rot, &lin, &ang, &rays, &initialStates, &states, &rewards}) d->free();
        targets.free(); tables.free(); rng.free(); cones.free(); hinges.free();
        for (Dev<uint32_t>* d : {&coneIdx, &hingeIdx, &bodyIdx, &ranges, &counters}) d->free();
        done.free();
        if (hostCounters) (void)hipHostFree(hostCounters);
        hostCounters = nullptr;
    }
};
DeviceBatch d;

bool hipOk(hipError_t e, const char* what) {
    if (e == hipSuccess) return true;
    learn_device::setError(std::string(what) + ": " + hipGetErrorString(e));
    return false;
}
#define LEARN_HIP(expr) do { if (!hipOk((expr), #expr)) return MI_ERR_DEVICE; } while (0)
#define LEARN_PHYS(expr) do { if (learn_device::failed((expr), #expr)) return MI_ERR_DEVICE; } while (0)

// the host's freshly reset batch goes up: the device twin of every field the step reads or writes
int uploadBatch(const learn_device::HostBatch& h) {
    const size_t n = (size_t)h.n, ne = n * kEntitiesPerEnv;
    LEARN_HIP(hipSetDevice(h.device));
    void* st = nullptr;
    LEARN_PHYS(mi_world_get_stream(h.world, &st));
    d.stream = (hipStream_t)st; d.n = h.n;
    std::vector<float> smoothed(n * kActionFloats), head(n); std::vector<Target> targets(n * kParts); std::vector<uint64_t> rng(n);
    for (size_t e = 0; e < n; ++e) {
        std::memcpy(&smoothed[e * kActionFloats], h.envs[e].smoothed, sizeof(h.envs[e].smoothed));
        head[e] = h.envs[e].headTargetHeight; rng[e] = h.envs[e].rng.state;
        std::memcpy(&targets[e * kParts], h.envs[e].targets, sizeof(h.envs[e].targets));
    }
    LEARN_HIP(d.smoothed.upload(smoothed.data(), smoothed.size())); LEARN_HIP(d.headTargetHeight.upload(head.data(), n));
    LEARN_HIP(d.targets.upload(targets.data(), targets.size())); LEARN_HIP(d.rng.upload(rng.data(), n));
    LEARN_HIP(d.tables.upload(h.tables, 1));
    LEARN_HIP(d.cones.upload(h.cones, n * kCone)); LEARN_HIP(d.hinges.upload(h.hinges, n * kHinge));
    LEARN_HIP(d.initialStates.upload(h.initialStates, n * kParts * MI_BODY_STATE_FLOATS));
    LEARN_HIP(d.pos.upload(h.pos, 3 * ne)); LEARN_HIP(d.rot.upload(h.rot, 4 * ne)); LEARN_HIP(d.lin.upload(h.lin, 3 * ne)); LEARN_HIP(d.ang.upload(h.ang, 3 * ne));   // (the grounds' rows stay as they are: no step writes them)
    std::vector<uint32_t> idx(n * kCone);
    LEARN_PHYS(mi_constraints_to_device_indices(h.world, MI_CONSTRAINT_CONE_TWIST, (uint32_t)idx.size(), h.coneIds, idx.data()));
    LEARN_HIP(d.coneIdx.upload(idx.data(), idx.size()));
    idx.resize(n * kHinge);
    LEARN_PHYS(mi_constraints_to_device_indices(h.world, MI_CONSTRAINT_HINGE, (uint32_t)idx.size(), h.hingeIds, idx.data()));
    LEARN_HIP(d.hingeIdx.upload(idx.data(), idx.size()));
    std::vector<uint32_t> ents(n * kParts), bodies(n * kParts);
    for (size_t e = 0; e < n; ++e) for (int p = 0; p < kParts; ++p) ents[e * kParts + p] = entityOf((int)e, p);
    LEARN_PHYS(mi_world_entities_to_bodies(h.world, (uint32_t)ents.size(), ents.data(), bodies.data()));
    LEARN_HIP(d.bodyIdx.upload(bodies.data(), bodies.size()));
    LEARN_HIP(d.rays.ensure(8 * n)); LEARN_HIP(d.ranges.ensure(2 * n)); LEARN_HIP(d.counters.ensure(2));
    LEARN_HIP(d.states.ensure(n * kStateFloats)); LEARN_HIP(d.rewards.ensure(n)); LEARN_HIP(d.done.ensure(n));
    if (!d.hostCounters) LEARN_HIP(hipHostMalloc((void**)&d.hostCounters, 2 * sizeof(uint32_t)));
    d.live = true;
    return MI_OK;
}

}  // namespace

namespace learn_device {
void release() { d.release(); }
bool pushRng(const Env* envs, int n) {
    if (!d.live || n != d.n) return true;
    std::vector<uint64_t> rng((size_t)n);
    for (int e = 0; e < n; ++e) rng[(size_t)e] = envs[e].rng.state;
    return hipOk(hipMemcpy(d.rng.p, rng.data(), rng.size() * sizeof(uint64_t), hipMemcpyHostToDevice), "sending the RNG states");
}
bool pullRng(Env* envs, int n) {
    if (!d.live || n != d.n) return true;   // (nothing of this batch is up there)
    std::vector<uint64_t> rng((size_t)n);
    if (!hipOk(hipMemcpy(rng.data(), d.rng.p, rng.size() * sizeof(uint64_t), hipMemcpyDeviceToHost), "fetching the RNG states")) return false;
    for (int e = 0; e < n; ++e) envs[e].rng.state = rng[(size_t)e];
    return true;
}
}  // namespace learn_device

EXPORT int resetPhysicsBatchDevice(int numEnvs, float* outStatesDev) {
    if (numEnvs <= 0) { learn_device::setError("resetPhysicsBatchDevice: numEnvs must be positive"); return MI_ERR_INVALID_ARGUMENT; }
    if (!learn_device::hostReset(numEnvs)) return MI_ERR_DEVICE;   // (no device: world creation has failed, and said so)
    const learn_device::HostBatch h = learn_device::hostBatch();
    int rc = uploadBatch(h); if (rc != MI_OK) return rc;
    if (outStatesDev) {
        std::vector<float> states((size_t)numEnvs * kStateFloats);
        learn_device::hostStates(states.data());
        LEARN_HIP(hipMemcpy(outStatesDev, states.data(), states.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    learn_device::enterDeviceMode();
    return MI_OK;
}

EXPORT int updatePhysicsBatchDevice(const float* actionsDev, float* outStatesDev, float* outRewardsDev, int* outDoneDev) {
    const learn_device::HostBatch h = learn_device::hostBatch();
    if (!h.world || !h.deviceMode || !d.live) {
        learn_device::setError("the batch was not reset with resetPhysicsBatchDevice: call it first (updatePhysicsBatch steps a batch that resetPhysicsBatch / resetPhysics made)");
        return MI_ERR_INVALID_ARGUMENT;
    }
    if (!actionsDev) { learn_device::setError("updatePhysicsBatchDevice: actionsDev is null"); return MI_ERR_INVALID_ARGUMENT; }
    LEARN_HIP(hipSetDevice(h.device));
    const int n = d.n;
    const uint32_t un = (uint32_t)n;
    float* states = outStatesDev ? outStatesDev : d.states.p; float* rewards = outRewardsDev ? outRewardsDev : d.rewards.p; int* done = outDoneDev ? outDoneDev : d.done.p;
    const PoseRows rows{d.pos.p, d.rot.p, d.lin.p, d.ang.p};
    // actions -> motors; the random pushes
    LEARN_HIP(hipMemsetAsync(d.counters.p, 0, 2 * sizeof(uint32_t), d.stream));
    hipLaunchKernelGGL(k_learn_actions, dim3((un + 63u) / 64u), dim3(64), 0, d.stream, n, actionsDev, d.smoothed.p, d.cones.p, d.hinges.p, d.rng.p, rows, d.rays.p, d.ranges.p, d.counters.p);
    LEARN_HIP(hipGetLastError());
    LEARN_PHYS(mi_constraints_update_device_async(h.world, MI_CONSTRAINT_CONE_TWIST, un * kCone, d.coneIdx.p, d.cones.p, sizeof(mi_cone_twist_constraint)));
    LEARN_PHYS(mi_constraints_update_device_async(h.world, MI_CONSTRAINT_HINGE, un * kHinge, d.hingeIdx.p, d.hinges.p, sizeof(mi_hinge_constraint)));
    LEARN_PHYS(mi_world_test_interactions_device_async(h.world, un, d.rays.p, d.ranges.p));
    // physicsStep(scene, arena, timer = 0, settings{frameRate 60}, 1/60): one internal step (see stepAll)
    mi_step_settings settings; std::memset(&settings, 0, sizeof(settings));
    settings.fixed_frame_rate = 1; settings.frame_rate = 60; settings.max_physics_iterations_per_frame = 4; settings.num_rigid_solver_iterations = 30;
    LEARN_PHYS(mi_world_step(h.world, &settings, 1.f / 60.f));
    // the entity transforms and velocities after it, into the device pose cache; state, reward, done flag, in-place reset of the cache and the episode state
    LEARN_PHYS(mi_world_get_transforms_device_async(h.world, 0u, d.pos.p, d.rot.p, d.lin.p, d.ang.p));
    const EnvArrays env{d.smoothed.p, d.headTargetHeight.p, d.targets.p, d.cones.p, d.hinges.p};
    hipLaunchKernelGGL(k_learn_state_reward, dim3((un + kEnvsPerBlock - 1u) / kEnvsPerBlock), dim3(kEnvsPerBlock * kLanesPerEnv), 0, d.stream, n, d.pos.p, d.rot.p, d.lin.p, d.ang.p, d.tables.p, env,
                       d.initialStates.p, states, rewards, done, d.counters.p);
    LEARN_HIP(hipGetLastError());
    LEARN_HIP(hipMemcpyAsync(d.hostCounters, d.counters.p, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, d.stream));
    LEARN_HIP(hipStreamSynchronize(d.stream));
    learn_device::addPushes(d.hostCounters[0]);
    if (d.hostCounters[1]) {   // somebody fell: body states of the fallen (the done flags are the mask), motors re-armed.  (Only then: a body-state write voids what the step ran ahead.)
        LEARN_PHYS(mi_world_set_body_states_masked_device_async(h.world, un * kParts, d.bodyIdx.p, d.initialStates.p, reinterpret_cast<const uint32_t*>(done), kParts));
        LEARN_PHYS(mi_constraints_update_device_async(h.world, MI_CONSTRAINT_CONE_TWIST, un * kCone, d.coneIdx.p, d.cones.p, sizeof(mi_cone_twist_constraint)));
        LEARN_PHYS(mi_constraints_update_device_async(h.world, MI_CONSTRAINT_HINGE, un * kHinge, d.hingeIdx.p, d.hinges.p, sizeof(mi_hinge_constraint)));
        LEARN_HIP(hipStreamSynchronize(d.stream));
    }
    return MI_OK;
}

EXPORT void* getPhysicsStream(void) {
    const learn_device::HostBatch h = learn_device::hostBatch();
    void* st = nullptr;
    if (!h.world || mi_world_get_stream(h.world, &st) != MI_OK) return nullptr;
    return st;
}
