"""The device-resident learning step (resetPhysicsBatchDevice / updatePhysicsBatchDevice) and the four device-side calls of the physics
library it stands on, on the GPU.  Device buffers are torch tensors.  The yardstick of the environments is the one of
tests/test_learning.py: the environment code of learning.cpp over the oracle backend.

Rewards are the one output that may differ from that yardstick, by the two maths libraries' acos and exp; the bound is derived in
`REWARD_ATOL` below.  Measured on an MI355X: the largest |reward difference| over every comparison in this file is 4.8e-7 (4 ulp of
a reward near 3); each comparison prints its own maximum, and a failure carries it in the assertion message."""
import numpy as np
import pytest

from d3d12renderer_amd import capi, scenes
from d3d12renderer_amd.learning import PhysicsDLL

pytestmark = pytest.mark.gpu

# Positions, velocities, the error sums and `fall` are bit-equal; each of the four reward terms is exp(x <= 0) <= 1, and two
# implementations correct to 2 ulp differ by <= 2 ulp(1) = 2.4e-7 there.  rotationError adds 14 x 2 acos(.), acos <= pi: 4 ulp(pi) = 9.5e-7
# between the two acosf gives <= 2.7e-5 in the sum, <= 1.9e-5 in the exponent (x 10 / 14) and in rlocal.  ~2e-5 in total, doubled for
# the rounding of the sum.
REWARD_ATOL = 4e-5


@pytest.fixture(scope="module")
def torch_mod(mi_lib):
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def envs(mi_lib, oracle_mod):
    g = PhysicsDLL(); o = PhysicsDLL(oracle_mod.build_learning())
    _, _, amin, amax = g.ranges()
    g.shutdown()
    yield g, o, amin, amax
    g.shutdown(); o.shutdown()


def _actions(rng, amin, amax, n):
    a = (rng.uniform(-1, 1, (n, 27)) * 0.5 * (amax - amin) * 0.3).astype(np.float32)
    return (a * (1.0 + 3.0 * (np.arange(n) % 3 == 0))[:, None]).astype(np.float32)


def _compare_with_oracle(torch, g, o, amin, amax, n, steps, seed):
    """Device path against learning.cpp over the oracle; returns (resets, largest reward difference)."""
    for d in (g, o):
        d.shutdown(); d.seed(seed)
    s0 = g.reset_batch_device(n)
    assert s0.cpu().numpy().tobytes() == o.reset_batch(n).tobytes(), "initial states"
    rng = np.random.default_rng(2)
    resets, worst = 0, 0.0
    for i in range(steps):
        a = _actions(rng, amin, amax, n)
        sg, rg, dg = g.step_batch_device(torch.from_numpy(a).cuda())
        so, ro, do = o.step_batch(a)
        sg, rg, dg = sg.cpu().numpy(), rg.cpu().numpy(), dg.cpu().numpy()
        assert sg.tobytes() == so.tobytes(), f"n={n} step {i}: states differ in environments {np.unique(np.nonzero(sg.view(np.uint32) != so.view(np.uint32))[0])}"
        assert (dg == do).all(), f"n={n} step {i}: done flags"
        assert (rg[dg] == 0).all() and (ro[do] == 0).all(), f"n={n} step {i}: a fallen environment's reward is not 0"
        diff = float(np.abs(rg.astype(np.float64) - ro.astype(np.float64)).max())
        worst = max(worst, diff)
        assert diff <= REWARD_ATOL, f"n={n} step {i}: max |reward difference| {diff:.3e} > {REWARD_ATOL}"
        resets += int(dg.sum())
    assert g.push_count() == o.push_count(), f"pushes: device {g.push_count()} oracle {o.push_count()}"
    print(f"n={n} steps={steps} seed={seed}: resets {resets}, pushes {g.push_count()}, max |reward difference| {worst:.3e}")
    return resets, worst


def test_device_path_equals_the_environment_over_the_oracle(torch_mod, envs):
    g, o, amin, amax = envs
    resets, worst = _compare_with_oracle(torch_mod, g, o, amin, amax, 24, 120, 33)
    assert resets > 0, "no environment fell: the in-place reset was not exercised"
    assert g.push_count() > 0, "no push was drawn"
    assert worst <= REWARD_ATOL, f"max |reward difference| {worst:.3e}"


@pytest.mark.parametrize("n", [1, 5, 70])   # fewer environments than a wave holds; not a multiple of the 4 per wave; several workgroups with a ragged tail
def test_partial_waves_and_blocks(torch_mod, envs, n):
    g, o, amin, amax = envs
    _compare_with_oracle(torch_mod, g, o, amin, amax, n, 40, 21)


def _device_run(torch, g, amin, amax, n, steps, seed):
    g.shutdown(); g.seed(seed)
    out = [g.reset_batch_device(n).cpu().numpy()]
    rng = np.random.default_rng(11)
    for _ in range(steps):
        s, r, d = g.step_batch_device(torch.from_numpy(_actions(rng, amin, amax, n)).cuda())
        out.append(np.concatenate([s.cpu().numpy(), r.cpu().numpy()[:, None], d.cpu().numpy()[:, None].astype(np.float32)], axis=1))
    return out


def test_device_path_is_deterministic(torch_mod, envs):
    g, _, amin, amax = envs
    a, b, c = (_device_run(torch_mod, g, amin, amax, 16, 80, s) for s in (5, 5, 6))
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    assert any(x.tobytes() != y.tobytes() for x, y in zip(a, c))   # another seed: other pushes


def test_modes_and_rng_carry_over(torch_mod, envs):
    torch = torch_mod
    g, _, amin, amax = envs
    n = 8
    zeros = np.zeros((n, 27), np.float32)
    g.shutdown(); g.seed(9)
    g.reset_batch_device(n)
    with pytest.raises(RuntimeError) as e:
        g.step_batch(zeros)
    assert "updatePhysicsBatchDevice" in str(e.value) and "(-1)" in str(e.value)
    g.step_batch_device(torch.from_numpy(zeros).cuda())          # the right call still works
    g.reset_batch(n)
    with pytest.raises(RuntimeError) as e:
        g.step_batch_device(torch.from_numpy(zeros).cuda())
    assert "resetPhysicsBatchDevice" in str(e.value) and "(-1)" in str(e.value)
    g.step_batch(zeros)
    g.shutdown()
    g.reset_batch_device(n); g.step_batch_device(torch.from_numpy(zeros).cuda())   # after a shutdown either mode works again
    g.shutdown()
    g.reset_batch(n); g.step_batch(zeros)

    # the per-environment generators carry over from the device path to the host path as they carry over resets: 30 steps on either path, a host
    # reset, 30 host steps — the same bytes whichever path ran the first 30 (rewards included: the host computes them in the second half)
    def second_half(first_on_device):
        g.shutdown(); g.seed(17)
        rng = np.random.default_rng(4)
        if first_on_device:
            g.reset_batch_device(n)
        else:
            g.reset_batch(n)
        for _ in range(30):
            a = _actions(rng, amin, amax, n)
            if first_on_device:
                g.step_batch_device(torch.from_numpy(a).cuda())
            else:
                g.step_batch(a)
        out = [g.reset_batch(n)]
        for _ in range(30):
            s, r, d = g.step_batch(_actions(rng, amin, amax, n))
            out.append(np.concatenate([s, r[:, None], d[:, None].astype(np.float32)], axis=1))
        return out, g.push_count()
    (host, host_pushes), (mixed, mixed_pushes) = second_half(False), second_half(True)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(host, mixed))
    assert host_pushes == mixed_pushes > 0
    g.shutdown()


# ---- the four device-side calls, on small worlds built through capi ----------------------------------------------------------
SETTINGS = capi.StepSettings(1, 60, 4, 30)
NBOX = 40


def _boxes_world(mi):
    """40 dynamic boxes (entities 0..39) over one static slab (entity 40)."""
    e = scenes.make_entities(NBOX)
    e["position"] = scenes._lattice(5, 2, 4, 1.5, 0.9, 1, 0.0)
    e["rotation"] = scenes.random_unit_quaternions(3, 20, NBOX)
    c = scenes.make_colliders(NBOX, capi.AABB, restitution=0.1, friction=0.5)
    c["shape"][:, 0:3] = -0.4; c["shape"][:, 3:6] = 0.4
    ge, gc = scenes._ground(30.0)
    sc = scenes.Scene("boxes_over_slab", np.concatenate([e, ge]), np.arange(NBOX + 1, dtype=np.uint32), np.concatenate([c, gc]), 30)
    return sc.populate(mi.create_world(0))


def _chain_world(mi):
    """8 capsules in a row (entities 0..7) joined by 7 hinges about z, over a slab; returns (world, hinge ids)."""
    n = 8
    e = scenes.make_entities(n)
    e["position"][:, 0] = np.arange(n); e["position"][:, 1] = 2.0
    c = scenes.make_colliders(n, capi.CAPSULE, restitution=0.1, friction=0.5)
    c["shape"][:, 0:7] = (-0.3, 0, 0, 0.3, 0, 0, 0.15)
    ge, gc = scenes._ground(30.0)
    sc = scenes.Scene("hinged_chain", np.concatenate([e, ge]), np.arange(n + 1, dtype=np.uint32), np.concatenate([c, gc]), 30)
    w = sc.populate(mi.create_world(0))
    ids = [w.add_constraint_from_global(capi.CONSTRAINT_HINGE, i, i + 1, (i + 0.5, 2.0, 0.0), (0.0, 0.0, 1.0), -1.5, 1.5) for i in range(n - 1)]
    return w, np.asarray(ids, np.uint32)


def _states(w, n):
    return w.get_body_states(np.arange(n, dtype=np.uint32))


def _same_after_steps(a, b, n, steps=10):
    """The host-side bookkeeping of a device call (step-ahead, pose epoch, host staleness): both worlds go on identically."""
    for i in range(steps):
        a.step(SETTINGS, 1.0 / 60.0); b.step(SETTINGS, 1.0 / 60.0)
        assert _states(a, n).tobytes() == _states(b, n).tobytes(), f"step {i} after the call"
    assert a.transforms()[0].tobytes() == b.transforms()[0].tobytes() and a.velocities()[0].tobytes() == b.velocities()[0].tobytes()


def _dev(torch, array, dtype=None):
    """A numpy array as a torch tensor on the GPU (uint32 travels as int32: the bytes are what counts)."""
    a = np.ascontiguousarray(array)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    elif a.dtype.fields is not None:
        a = a.view(np.uint8)
    t = torch.from_numpy(a).cuda()
    torch.cuda.synchronize()
    return t


def test_transforms_device_rows_equal_the_host_calls(torch_mod, mi_lib):
    torch = torch_mod
    a, b = _boxes_world(mi_lib), _boxes_world(mi_lib)
    for w in (a, b):
        w.step(SETTINGS, 1.0 / 90.0); w.step(SETTINGS, 1.0 / 90.0)   # the second call steps and leaves an interpolation factor of 1 / 3
    n = NBOX + 1
    sentinel = 777.0
    pos, lin, ang = (torch.full((n, 3), sentinel, device="cuda") for _ in range(3))
    rot = torch.full((n, 4), sentinel, device="cuda"); ppos = torch.full((n, 3), sentinel, device="cuda"); prot = torch.full((n, 4), sentinel, device="cuda")
    torch.cuda.synchronize()
    b.get_transforms_device_async(pos.data_ptr(), rot.data_ptr(), lin.data_ptr(), ang.data_ptr())
    b.get_transforms_device_async(ppos.data_ptr(), prot.data_ptr(), physics=True)
    torch.cuda.synchronize()
    hp, hr = a.transforms(); hl, ha = a.velocities(); hpp, hpr = a.physics_transforms()
    assert hp[:NBOX].tobytes() != hpp[:NBOX].tobytes()               # the interpolation is really pending
    for name, dev, host in (("positions", pos, hp), ("rotations", rot, hr), ("linear", lin, hl), ("angular", ang, ha), ("physics positions", ppos, hpp), ("physics rotations", prot, hpr)):
        d = dev.cpu().numpy()
        assert d[:NBOX].tobytes() == host[:NBOX].tobytes(), name
        assert (d[NBOX] == sentinel).all(), f"{name}: the static entity's row was written"
    # the world the device call was made on answers its own host calls like the other one (nothing of the pose stream was disturbed)
    for x, y in zip(b.transforms() + b.velocities() + b.physics_transforms(), (hp, hr, hl, ha, hpp, hpr)):
        assert x.tobytes() == y.tobytes()
    # velocities alone, positions alone
    lin2 = torch.full((n, 3), sentinel, device="cuda"); pos2 = torch.full((n, 3), sentinel, device="cuda"); torch.cuda.synchronize()
    b.get_transforms_device_async(linear_ptr=lin2.data_ptr()); b.get_transforms_device_async(positions_ptr=pos2.data_ptr()); torch.cuda.synchronize()
    assert lin2.cpu().numpy()[:NBOX].tobytes() == hl[:NBOX].tobytes() and pos2.cpu().numpy()[:NBOX].tobytes() == hp[:NBOX].tobytes()
    _same_after_steps(a, b, NBOX)
    # before anything has stepped (the host holds the transforms): still the host call's rows
    c = _boxes_world(mi_lib)
    pos3 = torch.full((n, 3), sentinel, device="cuda"); rot3 = torch.full((n, 4), sentinel, device="cuda"); torch.cuda.synchronize()
    c.get_transforms_device_async(pos3.data_ptr(), rot3.data_ptr()); torch.cuda.synchronize()
    cp, cr = c.transforms()
    assert pos3.cpu().numpy()[:NBOX].tobytes() == cp[:NBOX].tobytes() and rot3.cpu().numpy()[:NBOX].tobytes() == cr[:NBOX].tobytes()
    for w in (a, b, c):
        w.close()


def test_constraint_pods_written_on_the_device(torch_mod, mi_lib):
    torch = torch_mod
    (a, ids), (b, ids_b) = _chain_world(mi_lib), _chain_world(mi_lib)
    assert (ids == ids_b).all()
    H = capi.CONSTRAINT_HINGE
    pods = np.concatenate([a.get_constraint(H, i) for i in ids])
    pods["motor_type"] = 1; pods["max_motor_torque"] = 50.0
    pods["motor_velocity_or_target_angle"] = 0.3 * (np.arange(len(ids)) + 1) * (-1.0) ** np.arange(len(ids))
    a.update_constraints(H, ids, pods)
    idx = b.constraints_to_device_indices(H, ids)
    d_idx, d_pods = _dev(torch, idx), _dev(torch, pods)
    b.update_constraints_device_async(H, len(ids), d_idx.data_ptr(), d_pods.data_ptr())
    for i in range(5):
        a.step(SETTINGS, 1.0 / 60.0); b.step(SETTINGS, 1.0 / 60.0)
        assert _states(a, 8).tobytes() == _states(b, 8).tobytes(), f"step {i}"
    assert np.abs(_states(a, 8)[:, 10:13]).max() > 1e-3              # the motors do something
    for k, i in enumerate(ids):
        assert b.get_constraint(H, i).tobytes() == pods[k:k + 1].tobytes(), f"constraint {i}: the host copy does not hold the device-written POD"
    # a device update, then a HOST update of one constraint: the re-upload of the whole array must carry what the device wrote into the others
    pods2 = pods.copy(); pods2["motor_velocity_or_target_angle"] *= -0.5
    a.update_constraints(H, ids, pods2)
    d_pods2 = _dev(torch, pods2)
    b.update_constraints_device_async(H, len(ids), d_idx.data_ptr(), d_pods2.data_ptr())
    one = pods2[3:4].copy(); one["motor_velocity_or_target_angle"] = 0.7
    a.update_constraint(H, ids[3], one); b.update_constraint(H, ids[3], one)
    for i in range(5):
        a.step(SETTINGS, 1.0 / 60.0); b.step(SETTINGS, 1.0 / 60.0)
        assert _states(a, 8).tobytes() == _states(b, 8).tobytes(), f"step {i} after the host update"
    assert b.get_constraint(H, ids[5]).tobytes() == pods2[5:6].tobytes() and b.get_constraint(H, ids[3]).tobytes() == one.tobytes()
    assert a.save_checkpoint() == b.save_checkpoint()
    # ... and a checkpoint taken right after a device update holds it
    b.update_constraints_device_async(H, len(ids), d_idx.data_ptr(), d_pods.data_ptr()); a.update_constraints(H, ids, pods)
    assert a.save_checkpoint() == b.save_checkpoint()
    _same_after_steps(a, b, 8)
    a.close(); b.close()


def test_interactions_from_device_rays(torch_mod, mi_lib):
    torch = torch_mod
    a, b = _boxes_world(mi_lib), _boxes_world(mi_lib)
    for w in (a, b):
        w.step(SETTINGS, 1.0 / 60.0)
    p = a.physics_transforms()[0]
    hit, idle = 4, 5                                                    # two boxes of the upper layer (the lattice is x-major, then y, then z: nothing above them)
    origins = np.array([p[hit] + (0.1, 5.0, 0.05), (1000.0, 5.0, 0.0), p[idle] + (0.0, 5.0, 0.0)], np.float32)   # a hit, a miss, a ray at another box with an empty range
    dirs = np.array([(0, -1, 0), (0, 1, 0), (0, -1, 0)], np.float32)
    strengths = np.array([500.0, 500.0, 500.0], np.float32)
    ranges = np.array([(0, NBOX + 1), (0, NBOX + 1), (3, 3)], np.uint32)
    a.test_interactions(origins, dirs, strengths, ranges)
    rays = np.zeros((3, 8), np.float32); rays[:, 0:3] = origins; rays[:, 3:6] = dirs; rays[:, 6] = strengths
    d_rays, d_ranges = _dev(torch, rays), _dev(torch, ranges)
    b.test_interactions_device_async(3, d_rays.data_ptr(), d_ranges.data_ptr())
    before = _states(a, NBOX)
    a.step(SETTINGS, 1.0 / 60.0); b.step(SETTINGS, 1.0 / 60.0)
    sa, sb = _states(a, NBOX), _states(b, NBOX)
    assert sa.tobytes() == sb.tobytes()
    assert np.abs(sa[hit, 7:10] - before[hit, 7:10]).max() > 0.5 and np.abs(sa[idle, 7:10] - before[idle, 7:10]).max() < 0.5   # one box was pushed, the one behind the empty range was not
    # no ranges = the whole scene
    a.test_interactions(origins[:1], dirs[:1], strengths[:1]); b.test_interactions_device_async(1, d_rays.data_ptr())
    _same_after_steps(a, b, NBOX)
    a.close(); b.close()


def test_masked_body_states(torch_mod, mi_lib):
    torch = torch_mod
    a, b = _boxes_world(mi_lib), _boxes_world(mi_lib)
    for w in (a, b):
        w.step(SETTINGS, 1.0 / 60.0); w.step(SETTINGS, 1.0 / 60.0)
    before = _states(b, NBOX)
    ents = np.arange(6, dtype=np.uint32)
    new = before[:6].copy(); new[:, 1] += 1.0; new[:, 3:7] = (0, 0, 0, 1); new[:, 7:10] = (0.1, 0.2, 0.3); new[:, 10:13] = 0.0
    mask = np.array([1, 0, 1], np.uint32)
    d_ids, d_new, d_mask = _dev(torch, b.entities_to_bodies(ents)), _dev(torch, new), _dev(torch, mask)
    b.set_body_states_masked_device_async(6, d_ids.data_ptr(), d_new.data_ptr(), d_mask.data_ptr(), 2)
    a.set_body_states(ents[[0, 1, 4, 5]], new[[0, 1, 4, 5]])        # the host twin: the same rows, chosen on the host
    after = _states(b, NBOX)
    assert after[[2, 3]].tobytes() == before[[2, 3]].tobytes() and after[6:].tobytes() == before[6:].tobytes()   # group 1 and everybody else: untouched
    assert after[[0, 1, 4, 5]].tobytes() == new[[0, 1, 4, 5]].tobytes()
    assert after.tobytes() == _states(a, NBOX).tobytes()
    _same_after_steps(a, b, NBOX)
    a.close(); b.close()
