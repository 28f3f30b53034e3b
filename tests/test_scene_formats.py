"""Scene import / export in the reference's YAML schema (src/scene/serialization_yaml.cpp:74-233, 364-524) and the
checkpoint of the solver-relevant state."""
import numpy as np
import pytest

from d3d12renderer_amd import capi, scene_yaml, scenes

REFERENCE_STYLE = """
Scene: My scene
Camera: {Position: [0, 5, 10], Rotation: [0, 0, 0, 1], Near plane: 0.1}
Entities:
  - Tag: Platform
    Transform: {Position: [0, -0.5, 0], Rotation: [0, 0, 0, 1], Scale: [1, 1, 1]}
    Mesh: {Handle: 1234, Flags: 0}
    Colliders:
      - {Type: AABB, Min corner: [-10, -0.5, -10], Max corner: [10, 0.5, 10], Restitution: 0.1, Friction: 1, Density: 4}
  - Tag: Ball
    Transform: {Position: [0.1, 3, 0], Rotation: [0, 0, 0, 1], Scale: [1, 1, 1]}
    Dynamic: true
    Rigid body: {Local COG: [0, 0, 0], Inv mass: 0.25, Inv inertia: [1, 0, 0, 0, 1, 0, 0, 0, 1], Gravity factor: 1, Linear damping: 0.4, Angular damping: 0.4}
    Colliders:
      - {Type: Sphere, Center: [0, 0, 0], Radius: 0.5, Restitution: 0.3, Friction: 0.6, Density: 2}
  - Tag: Crate
    Transform: {Position: [0.3, 1, 0.2], Rotation: [0, 0.38268343, 0, 0.92387953], Scale: [1, 1, 1]}
    Dynamic: true
    Rigid body: {Local COG: [0, 0, 0], Inv mass: 1, Inv inertia: [1, 0, 0, 0, 1, 0, 0, 0, 1], Gravity factor: 0.5, Linear damping: 0.1, Angular damping: 0.2}
    Colliders:
      - {Type: OBB, Center: [0, 0, 0], Radius: [0.5, 0.4, 0.3], Rotation: [0, 0, 0, 1], Restitution: 0.1, Friction: 0.5, Density: 1}
      - {Type: Capsule, Position A: [0, 0.4, 0], Position B: [0, 0.9, 0], Radius: 0.2, Restitution: 0.1, Friction: 0.5, Density: 1}
  - Tag: Mover
    Transform: {Position: [4, 1, 0], Rotation: [0, 0, 0, 1], Scale: [1, 1, 1]}
    Rigid body: {Local COG: [0, 0, 0], Inv mass: 0, Inv inertia: [0, 0, 0, 0, 0, 0, 0, 0, 0], Gravity factor: 1, Linear damping: 0.4, Angular damping: 0.4}
    Colliders:
      - {Type: AABB, Min corner: [-1, -1, -1], Max corner: [1, 1, 1], Restitution: 0.1, Friction: 0.5, Density: 1}
  - Tag: Wind
    Transform: {Position: [0, 0, 0], Rotation: [0, 0, 0, 1], Scale: [1, 1, 1]}
    Force field: {Force: [1.5, 0, 0]}
  - Tag: Lamp
    Position: {Position: [0, 8, 0]}
    Point light: {Color: [1, 1, 1], Intensity: 10, Radius: 20}
"""


def test_load_reference_style_scene_and_simulate(oracle_mod):
    sc = scene_yaml.load_scene(REFERENCE_STYLE)
    assert sc.tags == ["Platform", "Ball", "Crate", "Mover", "Wind", "Lamp"]
    k = sc.entities["kind"]
    assert list(k) == [capi.ENTITY_STATIC, capi.ENTITY_DYNAMIC, capi.ENTITY_DYNAMIC, capi.ENTITY_KINEMATIC, capi.ENTITY_FORCE_FIELD, capi.ENTITY_STATIC]
    assert len(sc.colliders) == 5 and list(sc.collider_entities) == [0, 1, 2, 2, 3]
    assert np.allclose(sc.entities["gravity_factor"][2], 0.5) and sc.forces == [(4, (1.5, 0, 0))]
    assert np.allclose(sc.colliders["shape"][2, :10], (0, 0, 0, 1, 0, 0, 0, 0.5, 0.4, 0.3))     # OBB: rotation, centre, radius
    w = sc.populate(oracle_mod.create_world(oracle_mod.ORDER_REFERENCE))
    im, _, _ = w.mass_properties()
    assert np.isclose(1 / im[1], 2 * 4 / 3 * np.pi * 0.5 ** 3, rtol=1e-5)                       # recomputed from the collider, not "Inv mass: 0.25"
    assert im[3] == 0                                                                          # kinematic
    w.step_fixed(sc.settings(), sc.dt, 240)
    p, _ = w.physics_transforms()
    assert abs(p[1, 1] - 0.5) < 0.05 and p[1, 0] > 0.15          # the ball rests on the platform, blown along +x by the global field
    assert np.allclose(p[3], (4, 1, 0)) and np.allclose(p[5], (0, 8, 0))


def test_yaml_round_trip_is_exact(oracle_mod):
    sc = scenes.mixed_stack(5, 3, 5)
    w = sc.populate(oracle_mod.create_world(oracle_mod.ORDER_CANONICAL))
    text = scene_yaml.dump_scene(sc, w)
    back = scene_yaml.load_scene(text, solver_iterations=sc.solver_iterations)
    assert back.entities.tobytes() == sc.entities.tobytes() and back.colliders.tobytes() == sc.colliders.tobytes()
    assert np.array_equal(back.collider_entities, sc.collider_entities)
    a = sc.populate(oracle_mod.create_world(oracle_mod.ORDER_CANONICAL)); b = back.populate(oracle_mod.create_world(oracle_mod.ORDER_CANONICAL))
    a.step_fixed(sc.settings(), sc.dt, 60); b.step_fixed(back.settings(), back.dt, 60)
    assert a.physics_transforms()[0].tobytes() == b.physics_transforms()[0].tobytes()
    # like the reference, saving walks an entity's collider list newest first, so a multi-collider entity comes back reversed
    multi = scene_yaml.load_scene(scene_yaml.dump_scene(scene_yaml.load_scene(REFERENCE_STYLE)))
    assert [int(t) for t in multi.colliders["type"][multi.collider_entities == 2]] == [capi.CAPSULE, capi.OBB]
    # what the format cannot hold is refused, not dropped silently
    with pytest.raises(ValueError):
        scene_yaml.dump_scene(scenes.ragdolls(1, 1))          # constraints
    with pytest.raises(ValueError):
        scene_yaml.dump_scene(scenes.shape_zoo(2, 2, 2))      # cylinders / hulls
    with pytest.raises(ValueError):
        scene_yaml.load_scene("Camera: {Near plane: 0.1}\nSun: {Intensity: 50}\n")


@pytest.mark.gpu
def test_gpu_yaml_scene_matches_oracle(mi_lib, oracle_mod):
    sc = scene_yaml.load_scene(REFERENCE_STYLE)
    g = sc.populate(mi_lib.create_world(0)); o = sc.populate(oracle_mod.create_world(oracle_mod.ORDER_CANONICAL))
    for i in range(200):
        g.step_fixed(sc.settings(), sc.dt, 1); o.step_fixed(sc.settings(), sc.dt, 1)
        assert g.counts() == o.counts(), f"step {i}"
    assert g.physics_transforms()[0].tobytes() == o.physics_transforms()[0].tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("make,events", [(lambda: scenes.zones(), True), (lambda: scenes.ragdolls(3, 3), False), (lambda: scenes.terrain_field(6, 2, 6), False),
                                         (lambda: scenes.joint_zoo(copies=1), False)])   # every joint type in the POD section
def test_gpu_checkpoint_resume_is_bit_identical(mi_lib, oracle_mod, make, events):
    """Save after 70 steps, load into a FRESH world built from the same scene, continue: poses, velocities, counts and events
    equal the uninterrupted run (and the oracle) bit for bit — colour history, SAP axis, trigger overlaps, accumulators, motor
    PODs and the step accumulator all travel in the blob."""
    sc = make()
    s = sc.settings()
    def build(world):
        w = sc.populate(world)
        w.create_cloth(2.0, 1.5, 10, 8, 3.0)      # a cloth rides along: its particle state is part of the checkpoint
        return w
    a = build(mi_lib.create_world(0)); o = build(oracle_mod.create_world(oracle_mod.ORDER_CANONICAL))
    if events:
        a.enable_events(); o.enable_events()
    nh = 6 * 9
    def drive(w, it):
        if sc.constraints and it % 5 == 0:       # ragdolls: keep editing the hinge motors
            pods = np.concatenate([w.get_constraint(capi.CONSTRAINT_HINGE, i) for i in range(nh)])
            pods["motor_type"] = 1; pods["max_motor_torque"] = 150.0; pods["motor_velocity_or_target_angle"] = 0.4 * np.sin(0.1 * it)
            w.update_constraints(capi.CONSTRAINT_HINGE, np.arange(nh), pods)
        w.step(s, 1.0 / 90.0)                     # physicsStep with a frame time that is not a multiple of the fixed step
    for it in range(70):
        drive(a, it); drive(o, it)
        if events:
            assert a.poll_events().tobytes() == o.poll_events().tobytes()
    a.set_cloth_properties(0, 4.0, 0.7, 0.5, 0.9); o.set_cloth_properties(0, 4.0, 0.7, 0.5, 0.9)
    blob = a.save_checkpoint()
    joint_types = [c[0] for c in sc.constraints] + [c[0] for c in sc.global_constraints]
    if joint_types:
        # the POD section's place and order: after the header (68 bytes), entities (28 each), bodies (104), history (12) and trigger overlaps (8);
        # the six types in CONSTRAINT_DTYPES order, each in pool order = creation order (nothing was deleted)
        import struct
        _, _, ne, nb, _, nhist, ntrig, _ = struct.unpack_from("<8I", blob, 0)
        at = 68 + 28 * ne + 104 * nb + 12 * nhist + 8 * ntrig
        pods = b"".join(a.get_constraint(t, i).tobytes() for t in range(len(capi.CONSTRAINT_DTYPES)) for i in range(joint_types.count(t)))
        assert len(pods) == sum(capi.CONSTRAINT_DTYPES[t].itemsize for t in joint_types) > 0
        assert blob[at:at + len(pods)] == pods, "constraint PODs are not where / in the order the checkpoint format has them"
    b = build(mi_lib.create_world(0))
    if events:
        b.enable_events()
    b.load_checkpoint(blob)
    assert b.transforms()[0].tobytes() == a.transforms()[0].tobytes()
    for it in range(70, 140):
        drive(a, it); drive(b, it); drive(o, it)
        assert a.counts() == b.counts() == o.counts(), f"step {it}"
        if events:
            ea = a.poll_events()
            assert ea.tobytes() == b.poll_events().tobytes() == o.poll_events().tobytes()
    for x, y, z in zip(a.transforms() + a.velocities() + a.cloth_state(0, 80), b.transforms() + b.velocities() + b.cloth_state(0, 80),
                       o.transforms() + o.velocities() + o.cloth_state(0, 80)):
        assert x.tobytes() == y.tobytes() == z.tobytes()
    with pytest.raises(mi_lib.PhysicsError):
        scenes.obb_pile(3, 2, 3).populate(mi_lib.create_world(0)).load_checkpoint(blob)     # other scene
    with pytest.raises(mi_lib.PhysicsError):
        b.load_checkpoint(blob[:-8])                                                         # truncated


@pytest.mark.gpu
def test_gpu_rejected_checkpoint_leaves_the_world_untouched(mi_lib, oracle_mod):
    """mi_world_load_checkpoint validates the blob against its own header and the scene BEFORE it allocates or overwrites anything:
    truncated, oversized and corrupt-header blobs (history / overlap counts in the billions) are refused with an error status, and
    the world that refused them continues bit-identically to one that never saw them.  A checkpoint taken while a topology edit is
    pending keeps the colour history, like the live world does."""
    import struct
    sc = scenes.obb_pile(8, 4, 8, spacing=1.0)
    s = sc.settings()
    a = sc.populate(mi_lib.create_world(0)); b = sc.populate(mi_lib.create_world(0)); o = sc.populate(oracle_mod.create_world(oracle_mod.ORDER_CANONICAL))
    for w in (a, b, o):
        w.step_fixed(s, sc.dt, 60)
    blob = a.save_checkpoint()
    words = list(struct.unpack_from("<8I", blob, 0))        # magic, version, numEntities, numBodies, numColliders, numHistory, numTriggerOverlaps, sapAxis
    bad = [blob[:-1], blob + b"\0", blob[: len(blob) // 2], b"", blob[:16]]
    for idx, val in ((5, 0xFFFFFFF0), (5, 0x7FFFFFFF), (6, 0xFFFFFFFF), (5, words[5] + 1), (2, words[2] + 1)):
        w2 = list(words); w2[idx] = val
        bad.append(struct.pack("<8I", *w2) + blob[32:])
    for k, x in enumerate(bad):
        with pytest.raises(mi_lib.PhysicsError):
            a.load_checkpoint(x)
    for i in range(40):
        for w in (a, b, o):
            w.step_fixed(s, sc.dt, 1)
        assert a.counts() == b.counts() == o.counts(), f"step {i}"
    assert a.physics_transforms()[0].tobytes() == b.physics_transforms()[0].tobytes() == o.physics_transforms()[0].tobytes()
    # save with a pending topology edit (a force applied through the host path marks nothing dirty; adding a collider does)
    e = scenes.make_entities(1); e["position"][0] = (0.0, 30.0, 0.0)
    c = scenes.make_colliders(1, capi.SPHERE); c["shape"][0, :4] = (0, 0, 0, 0.4)
    for w in (a, o):
        first = w.create_entities(e); w.add_colliders([first], c)
    blob2 = a.save_checkpoint()
    words2 = struct.unpack_from("<8I", blob2, 0)
    assert words2[5] > 0, "colour history dropped from a checkpoint taken with a pending topology edit"
    for i in range(30):
        a.step_fixed(s, sc.dt, 1); o.step_fixed(s, sc.dt, 1)
        assert a.counts() == o.counts(), f"after edit, step {i}"
    assert a.physics_transforms()[0].tobytes() == o.physics_transforms()[0].tobytes()


# ------------------------------------------------------------------------------------------------ binary entity stream
def _same_entity_record(a, b, tag):
    assert set(a) == set(b), f"{tag}: components {sorted(a)} vs {sorted(b)}"
    for k in a:
        if k == "tag":
            continue                                  # names are free text
        if k == "colliders":
            assert len(a[k]) == len(b[k]), tag
            for f in a[k].dtype.names:
                if f in ("object_type", "object_index"):
                    continue                          # "only used internally" (physics.h:103-105): uninitialised in the stored colliders
                for x, y in zip(a[k], b[k]):
                    if f == "shape":                  # bytes of the union beyond the collider type's own fields are indeterminate in the reference
                        n = {0: 4, 1: 7, 2: 7, 3: 6, 4: 10, 5: 7}[int(x["type"])]
                        assert x[f][:n].tobytes() == y[f][:n].tobytes(), f"{tag}: collider shape"
                    elif f == "hull_geometry":
                        assert int(x["type"]) != capi.HULL or x[f] == y[f], f"{tag}: hull geometry index"
                    else:
                        assert x[f] == y[f], f"{tag}: collider {f}"
        elif k == "constraints":
            assert len(a[k]) == len(b[k]), tag
            for (ta, ea, eb, pa), (tb_, fa, fb, pb) in zip(a[k], b[k]):
                assert (ta, ea, eb) == (tb_, fa, fb) and pa.tobytes() == pb.tobytes(), f"{tag}: constraint"
        elif isinstance(a[k], bool):
            assert a[k] == b[k]
        else:
            assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), f"{tag}: {k}"


@pytest.mark.skipif(not __import__("oracle").reference_available(), reason="needs oracle/_ref")
@pytest.mark.parametrize("make", [lambda: scenes.shape_zoo(), lambda: scenes.ragdolls(2, 2), lambda: scenes.zones(localized=False), lambda: scenes.vehicles(1, 1),
                                  lambda: scenes.joint_zoo()], ids=["zoo", "ragdolls", "zones", "vehicles", "joint_zoo"])
def test_binary_entity_stream_equals_reference_struct_images(oracle_mod, make):
    """d3d12renderer_amd/scene_binary.py against streams written with the REFERENCE's own struct definitions (oracle/_ref: the component
    list and order of serialization_binary.cpp:105-133, `stream.write(component)` of the compiled reference structs): same length,
    same presence flags, every field of every component image identical — mid-simulation, so velocities, mass properties and
    motor PODs are non-trivial."""
    from d3d12renderer_amd import scene_binary
    sc = make()
    r = sc.populate(oracle_mod.create_reference_world()); o = sc.populate(oracle_mod.create_world(oracle_mod.ORDER_REFERENCE))
    s = sc.settings()
    r.step_fixed(s, sc.dt, 25); o.step_fixed(s, sc.dt, 25)
    for e in range(len(sc.entities)):
        native = r.serialize_entity_native(e)
        mine = scene_binary.serialize_entity(sc, o, e)
        assert len(native) == len(mine), f"entity {e}: stream length"
        _same_entity_record(scene_binary.parse_entity(native), scene_binary.parse_entity(mine), f"{sc.name} entity {e}")
    with pytest.raises(ValueError):
        scene_binary.parse_entity(mine[:-3])
    with pytest.raises(ValueError):
        scene_binary.parse_entity(mine + b"\0")


def test_binary_entity_stream_round_trip(oracle_mod):
    """Entities written out of a running world and read back into a fresh one continue bit-identically (contacts-only scene; the
    stream carries transforms, velocities, damping, colliders and materials; mass properties are recomputed from the colliders like
    deserializeFromMemoryStream<physics_reference_component> does by adding the colliders again)."""
    from d3d12renderer_amd import scene_binary
    sc = scenes.mixed_stack(5, 3, 5)
    a = sc.populate(oracle_mod.create_world(oracle_mod.ORDER_CANONICAL))
    a.step_fixed(sc.settings(), sc.dt, 40)
    blobs = [scene_binary.serialize_entity(sc, a, e) for e in range(len(sc.entities))]
    back = scene_binary.load_entities(blobs, solver_iterations=sc.solver_iterations)
    assert back.colliders.tobytes() == sc.colliders.tobytes() and np.array_equal(back.collider_entities, sc.collider_entities)
    b = back.populate(oracle_mod.create_world(oracle_mod.ORDER_CANONICAL))
    fresh = sc.populate(oracle_mod.create_world(oracle_mod.ORDER_CANONICAL))     # reference run: same state, no colour history either
    fresh.set_body_states(np.arange(sc.num_bodies, dtype=np.uint32), a.get_body_states(np.arange(sc.num_bodies, dtype=np.uint32)))
    b.step_fixed(back.settings(), back.dt, 30); fresh.step_fixed(sc.settings(), sc.dt, 30)
    assert b.physics_transforms()[0].tobytes() == fresh.physics_transforms()[0].tobytes()
    # constraints survive as a multiset (the stream has no global creation order)
    rg = scenes.ragdolls(1, 2)
    w = rg.populate(oracle_mod.create_world(oracle_mod.ORDER_CANONICAL))
    back = scene_binary.load_entities([scene_binary.serialize_entity(rg, w, e) for e in range(len(rg.entities))])
    key = lambda c: (int(c[0]), int(c[1]), int(c[2]), np.asarray(c[3]).tobytes())
    assert sorted(map(key, back.constraints)) == sorted(key((t, ea, eb, w.get_constraint(t, i))) for t, i, ea, eb in scene_binary._constraint_list(rg))


@pytest.mark.gpu
def test_gpu_binary_entity_stream_matches_oracle(mi_lib, oracle_mod):
    from d3d12renderer_amd import scene_binary
    for sc in (scenes.shape_zoo(), scenes.ragdolls(2, 2)):
        g = sc.populate(mi_lib.create_world(0)); o = sc.populate(oracle_mod.create_world(oracle_mod.ORDER_CANONICAL))
        g.step_fixed(sc.settings(), sc.dt, 40); o.step_fixed(sc.settings(), sc.dt, 40)
        for e in range(len(sc.entities)):
            assert scene_binary.serialize_entity(sc, g, e) == scene_binary.serialize_entity(sc, o, e), f"{sc.name} entity {e}"
