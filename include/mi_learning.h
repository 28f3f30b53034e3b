/*
 * mi_learning.h — the learning DLL's C ABI (libPhysics-Lib.so), SURVEY §8(b)(2) / §8(f).2.
 *
 * The first five functions are, name for name and signature for signature, the reference's only true C ABI:
 * the __declspec(dllexport) functions of src/learning/learned_locomotion.cpp:395-489 that learning/loco_env.py:8-47 binds
 * with ctypes (Physics-Lib.dll).  State = learned_locomotion::learning_state (66 floats), action = learning_action
 * (27 floats), src/learning/learned_locomotion.h:15-65.  The rest steps many such environments per call in ONE device world.
 * Implementation: d3d12renderer_amd/csrc/learning.cpp (host C++ over include/mi_physics.h) and, for the device-resident step,
 * d3d12renderer_amd/csrc/learning_device.hip (HIP kernels over the device-side calls of include/mi_physics.h).
 */
#ifndef MI_LEARNING_H
#define MI_LEARNING_H

#ifdef __cplusplus
extern "C" {
#endif

#ifndef MI_LEARNING_API
#define MI_LEARNING_API
#endif

/* learned_locomotion.cpp:395-396 */
MI_LEARNING_API int getPhysicsStateSize(void);
MI_LEARNING_API int getPhysicsActionSize(void);
/* learned_locomotion.cpp:398-427: state unbounded (-FLT_MAX / FLT_MAX); action bounds from the joint limits. */
MI_LEARNING_API void getPhysicsRanges(float* stateMin, float* stateMax, float* actionMin, float* actionMax);
/* learned_locomotion.cpp:429-450: ground slab + humanoid at hip height 1.25 m, episode state reset.  Unlike the reference it
 * also writes the initial state to outState (may be NULL). */
MI_LEARNING_API void resetPhysics(float* outState);
/* learned_locomotion.cpp:452-489: smooth + apply the action (position motors, 200 Nm), a random push with probability 0.02,
 * one physicsStep at 60 Hz, state, reward; returns 1 when the ragdoll has fallen (head below 1 m; reward 0 then). */
MI_LEARNING_API int updatePhysics(float* action, float* outState, float* outReward);

/* ---- batched environments: numEnvs ragdolls, each on its own ground slab, in one world on one GPU ---- */
/* (Re)creates the environments, writes [numEnvs][stateSize] initial states (may be NULL); 0 on success. */
MI_LEARNING_API int resetPhysicsBatch(int numEnvs, float* outStates);
/* actions [numEnvs][actionSize] -> states [numEnvs][stateSize], rewards [numEnvs], done [numEnvs]; an environment whose
 * ragdoll fell is reset in place after its terminal state was written; 0 on success. */
MI_LEARNING_API int updatePhysicsBatch(const float* actions, float* outStates, float* outRewards, int* outDone);
MI_LEARNING_API int getPhysicsNumEnvs(void);
MI_LEARNING_API void setPhysicsSeed(unsigned long long seed);   /* push RNG (the reference seeds with time(0)); takes effect on the next step, on either path */
MI_LEARNING_API void setPhysicsDevice(int device);              /* HIP device of the next (re)created world */
MI_LEARNING_API const char* getPhysicsError(void);              /* message of the last failure */
MI_LEARNING_API void shutdownPhysics(void);
/* Random pushes applied since the environments were last (re)created; the host path and the device path both count. */
MI_LEARNING_API unsigned long long getPhysicsPushCount(void);

/* ---- the same batch stepped without a host copy of any per-environment data: actions in from a device buffer, states, rewards and
 * done flags out to device buffers (e.g. torch tensors' data_ptr() on the world's GPU; float32 / int32, contiguous).  Semantics are
 * updatePhysicsBatch's, step for step: states and done flags are the same bits, rewards differ by the device maths library's acos
 * and exp (measured: at most 4.8e-7; the tests allow 4e-5, derived from 4 ulp of acos over the 14 parts).
 * Which path steps the batch is fixed by the reset call: after resetPhysicsBatchDevice only updatePhysicsBatchDevice does, after
 * resetPhysicsBatch / resetPhysics only updatePhysicsBatch / updatePhysics; the wrong one returns MI_ERR_INVALID_ARGUMENT (-1) and
 * getPhysicsError() names the reset to use.  Either reset keeps the world when numEnvs is unchanged, and the per-environment push
 * generators carry over from one path to the other as they carry over resets. ---- */
/* (Re)creates the environments, writes the initial states to out_states_dev ([numEnvs][stateSize], may be NULL); 0 on success.
 * Without a HIP device it fails like every other call: there is no CPU fallback. */
MI_LEARNING_API int resetPhysicsBatchDevice(int numEnvs, float* outStatesDev);
/* One step of every environment.  The call returns after the world's stream is idle: the outputs are complete on return.
 * actionsDev must be complete when the call is made: the caller either synchronises the stream that produces it, or produces it
 * on getPhysicsStream().  outStatesDev / outRewardsDev / outDoneDev may be NULL. */
MI_LEARNING_API int updatePhysicsBatchDevice(const float* actionsDev, float* outStatesDev, float* outRewardsDev, int* outDoneDev);
/* The world's hipStream_t (NULL before the first reset): everything the device path enqueues runs on it. */
MI_LEARNING_API void* getPhysicsStream(void);

#ifdef __cplusplus
}
#endif
#endif
