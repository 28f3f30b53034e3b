// learning_device.hpp — what the two translation units of libPhysics-Lib.so know of each other.  learning.cpp owns the world, the
// host's copy of the environments and the choice of path; learning_device.hip owns the device twin of that state and the kernels of
// resetPhysicsBatchDevice / updatePhysicsBatchDevice.  (Not part of a build of learning.cpp over another physics backend.)
#ifndef MI_LEARNING_DEVICE_HPP
#define MI_LEARNING_DEVICE_HPP
#include <string>

#include "../../include/mi_physics.h"
#include "learning_shared.hpp"

namespace learn_device {

// the host's batch as the device path sees it (pointers into learning.cpp's vectors: valid until the next call into that unit)
struct HostBatch {
    mi_world* world; int n, device; bool deviceMode;
    learn::Env* envs;
    mi_cone_twist_constraint* cones; mi_hinge_constraint* hinges;   // [env][slot]
    const uint32_t *coneIds, *hingeIds;
    const float* initialStates;                                      // [env][part][13]
    const float *pos, *rot, *lin, *ang;                              // the host's pose cache, per entity
    const learn::EnvTables* tables;
};

// ---- learning.cpp
HostBatch hostBatch();
bool hostReset(int numEnvs);              // ensureBatch + every environment reset on the host (RNG states fetched first if the device held them): the host's copy IS the initial state
void hostStates(float* out);              // [n][66] from the host's copy
void setError(const std::string& what);
bool failed(int rc, const char* what);    // a physics-library status: records the message of a failure
void enterDeviceMode();
void addPushes(unsigned long long n);

// ---- learning_device.hip
void release();                           // the world goes away
bool pullRng(learn::Env* envs, int n);    // the per-environment RNG states, device -> host
bool pushRng(const learn::Env* envs, int n);   // ... and host -> device (setPhysicsSeed while the device path steps the batch)

}  // namespace learn_device
#endif
