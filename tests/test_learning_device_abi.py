"""The device-resident learning step without a GPU: its C ABI is declared and exported, it refuses to run without a device (no CPU
fallback), and the build of learning.cpp ALONE over the oracle backend — what every learning parity test stands on — still works."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
DEVICE_ABI = ("resetPhysicsBatchDevice", "updatePhysicsBatchDevice", "getPhysicsStream", "getPhysicsPushCount")
DEVICE_PRIMITIVES = ("mi_world_get_transforms_device_async", "mi_constraints_to_device_indices", "mi_constraints_update_device_async",
                     "mi_world_test_interactions_device_async", "mi_world_set_body_states_masked_device_async")


def test_learning_header_declares_and_library_exports_the_device_abi(mi_lib):
    from d3d12renderer_amd import learning
    names = re.findall(r"MI_LEARNING_API\s+[\w\s\*]+?\b(\w+)\s*\(", (ROOT / "include" / "mi_learning.h").read_text())
    lib = C.CDLL(str(learning.LIB_PATH))
    for n in DEVICE_ABI:
        assert n in names, f"{n} is not declared in mi_learning.h"
        assert hasattr(lib, n), f"libPhysics-Lib.so does not export {n}"


def test_physics_header_declares_and_library_exports_the_device_primitives(mi_lib):
    names = re.findall(r"MI_API\s+[\w\s\*]+?\b(mi_\w+)\s*\(", (ROOT / "include" / "mi_physics.h").read_text())
    L = mi_lib.library()
    for n in DEVICE_PRIMITIVES:
        assert n in names, f"{n} is not declared in mi_physics.h"
        assert hasattr(L.lib, n), f"libmi_physics.so does not export {n}"


def test_no_cpu_fallback_for_the_device_reset(mi_lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    from d3d12renderer_amd.learning import PhysicsDLL
    d = PhysicsDLL()
    assert d.has_device_path
    rc = d._physics.resetPhysicsBatchDevice(4, None)
    assert rc != 0
    assert "no HIP device" in d.error(), d.error()
    # ... and nothing is left half made: the step refuses too, and says which reset it wants
    assert d._physics.updatePhysicsBatchDevice(None, None, None, None) != 0
    assert "resetPhysicsBatchDevice" in d.error()
    assert d.stream() == 0


def test_learning_source_alone_still_builds_over_the_oracle_and_steps(oracle_mod):
    from d3d12renderer_amd.learning import PhysicsDLL
    d = PhysicsDLL(oracle_mod.build_learning())
    assert not d.has_device_path                      # the device path is a unit of its own; this build has none
    d.shutdown(); d.seed(3)
    s0 = d.reset_batch(2)
    assert s0.shape == (2, 66) and np.isfinite(s0).all()
    assert d.push_count() == 0
    for _ in range(3):
        s, r, dn = d.step_batch(np.zeros((2, 27), np.float32))
    assert np.isfinite(s).all() and (r > 0).all() and not dn.any()
    d.shutdown()


def test_new_learning_sources_do_not_read_the_environment():
    csrc = ROOT / "d3d12renderer_amd" / "csrc"
    for n in ("learning_device.hip", "learning_device.hpp", "learning_shared.hpp"):
        assert "getenv" not in (csrc / n).read_text(), n
