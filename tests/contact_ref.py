"""The yardstick of the contact-manifold scene query (include/mi_physics.h, mi_world_volume_contacts), none of which needs a GPU.

A rigid body of a volume's shape, placed at the volume's pose in an oracle world next to the scene, gets from ONE step of the reference's
narrow phase exactly the manifolds the query reports: same (A, B), same bits.  The one difference is the orientation of a pair of EQUAL
world types: the query makes the volume A; the step makes A whichever AABB starts earlier on the step's sweep axis (on a tie the larger
world index; pairKey in csrc/kernels_broad.hpp).  Equal-type pairs whose A is the scene collider are "reversed": no comparison uses them.

Also here: the volume sets of the GPU tests (those of overlap_ref plus probes placed on the scene's hulls and on the corner of its ground,
for the type pairs random volumes hardly ever give)."""
from dataclasses import replace

import numpy as np

import overlap_ref as R
from d3d12renderer_amd import capi, scenes

INCLUDE = 3            # rigid bodies and statics: what a step's narrow phase sees
HULL_PROBE_OFFSETS = ((-0.25, -0.2, -0.15), (-0.1, -0.3, -0.2))   # negative on every axis: the probe's AABB starts first whatever the sweep axis


def probes(sc, positions, rotations):
    """What random volumes hardly ever give.  Per hull collider of the scene: two hull volumes of the same geometry and rotation a fraction
    of its size (0.6) away, and a true AABB about it (hull-hull, AABB-hull).  Per static world AABB of the scene (the ground): AABB volumes
    over its minimum corner, reaching 0.1 .. 1.0 into it, which therefore start first on every axis (AABB-AABB with the volume as A)."""
    out = []
    for ci in range(len(sc.colliders)):
        c = sc.colliders[ci]
        ent = int(sc.collider_entities[ci])
        pos = np.asarray(positions[ent], np.float64)
        if int(c["type"]) == R.HULL:
            for off in HULL_PROBE_OFFSETS:
                out.append(capi.make_volume(R.HULL, c["shape"][:7], position=pos + off, rotation=rotations[ent], hull_geometry=int(c["hull_geometry"])))
            out.append(capi.box_volume(pos + HULL_PROBE_OFFSETS[0], (0.3, 0.25, 0.35)))
        elif int(c["type"]) == R.AABB and int(sc.entities["kind"][ent]) == capi.ENTITY_STATIC and tuple(float(x) for x in rotations[ent]) == (0.0, 0.0, 0.0, 1.0):
            corner = pos + np.asarray(c["shape"][:3], np.float64)
            for i in range(10):
                d = 0.1 * (i + 1)
                out.append(capi.box_volume(corner + (d - 1.0) / 2, ((d + 1.0) / 2,) * 3))
    return np.concatenate(out) if out else np.zeros(0, capi.query_volume_dtype)


def contact_volume_set(name, settled, sc, positions, rotations, per_type=32):
    """The volumes of one (scene, state): overlap_ref's random set and the probes at the given entity poses."""
    return np.concatenate([R.volume_set(name, settled, per_type=per_type), probes(sc, positions, rotations)])


def start_poses(sc):
    return sc.entities["position"].copy(), sc.entities["rotation"].copy()


def oracle_manifolds(oracle_mod, sc, vols, body_states=None):
    """One step of an oracle world holding the scene plus one DYNAMIC entity per volume.  Returns (expected, reversed_pairs, info):
    expected[(volume, scene world collider)] = dict(entity, object_type, volume_is_b, normal (3 f32), points ((n, 4) f32: xyz, depth)) for
    every non-reversed volume-versus-scene manifold; reversed_pairs = the (volume, collider) pairs of equal world type whose A is the scene
    collider (with or without a manifold); info = per-type-pair counts and the reversed manifolds."""
    count = len(vols); n_ent = len(sc.entities); nc_s = len(sc.colliders)
    ve = scenes.make_entities(count, capi.ENTITY_DYNAMIC)
    ve["position"] = vols["position"]; ve["rotation"] = vols["rotation"]
    vc = scenes.make_colliders(count, capi.SPHERE)
    vc["type"] = vols["type"]; vc["shape"] = vols["shape"]; vc["hull_geometry"] = vols["hull_geometry"]
    big = replace(sc, entities=np.concatenate([sc.entities, ve]),
                  collider_entities=np.concatenate([sc.collider_entities, np.arange(n_ent, n_ent + count, dtype=np.uint32)]).astype(np.uint32),
                  colliders=np.concatenate([sc.colliders, vc]))
    w = big.populate(oracle_mod.create_world(oracle_mod.ORDER_REFERENCE))
    if body_states is not None:
        w.set_body_states(*body_states)
    positions, rotations = w.physics_transforms()
    w.step_fixed(sc.settings(), sc.dt, 1)
    contacts = w.contacts(); boxes = w.aabbs(); axis = int(w.counts()["sorting_axis"])
    w.close()
    # the volumes were created last: volume v is world collider count - 1 - v, scene world collider k is world collider count + k
    shapes = R.scene_world_shapes(sc, positions[:n_ent], rotations[:n_ent])
    ktype = np.array([s[2][0] for s in shapes]); vtype = np.array([R.volume_world_shape(v)[0] for v in vols])
    assert len(boxes) == count + nc_s

    def scene_is_a(v, k):   # equal world types: A = the earlier start on the sweep axis, on a tie the larger world index (the scene collider)
        return boxes[count + k, axis] <= boxes[count - 1 - v, axis]

    groups = {}
    for c in contacts:
        groups.setdefault((int(c["collider_a"]), int(c["collider_b"])), []).append(c)
    expected = {}; reversed_manifolds = []; per_pair = {}
    for (a, b), cs in groups.items():
        if a < count and b < count:
            continue   # volume versus volume
        if a >= count and b >= count:
            continue   # the scene's own
        vol_is_a = a < count
        v = count - 1 - (a if vol_is_a else b); k = (b if vol_is_a else a) - count
        tv, tk = int(vtype[v]), int(ktype[k])
        if tv != tk:
            assert vol_is_a == (tv < tk), f"pair ({a}, {b}): A is not the smaller world type ({tv}, {tk})"
        else:
            assert vol_is_a == (not scene_is_a(v, k)), f"pair ({a}, {b}) of type {tv}: the sweep rule gives the other orientation"
            if not vol_is_a:
                reversed_manifolds.append((v, k))
                continue
        assert 1 <= len(cs) <= 4 and all(np.array_equal(c["normal"], cs[0]["normal"]) for c in cs)
        ent, obj, _ = shapes[k]
        expected[(v, k)] = dict(entity=ent, object_type=obj, volume_is_b=not vol_is_a, normal=np.array(cs[0]["normal"], np.float32),
                                points=np.array([[*c["point"], c["penetration_depth"]] for c in cs], np.float32))
        key = (min(tv, tk), max(tv, tk))
        per_pair[key] = per_pair.get(key, 0) + 1
    reversed_pairs = {(v, k) for v in range(count) for k in np.flatnonzero(ktype == vtype[v]) if scene_is_a(v, int(k))}
    equal_manifolds = sum(n for (ta, tb), n in per_pair.items() if ta == tb) + len(reversed_manifolds)
    info = dict(per_pair=per_pair, reversed_manifolds=len(reversed_manifolds), equal_type_manifolds=equal_manifolds, axis=axis)
    return expected, reversed_pairs, info


def records_by_pair(offsets, recs):
    return {(int(r["volume"]), int(r["collider"])): r for r in recs}


def compare_with_oracle(offsets, recs, expected, reversed_pairs):
    """The set of non-reversed records equals the oracle's, and every compared record holds the oracle's bits.  Returns the differences."""
    got = {key: r for key, r in records_by_pair(offsets, recs).items() if key not in reversed_pairs}
    problems = []
    missing = sorted(set(expected) - set(got)); extra = sorted(set(got) - set(expected))
    if missing:
        problems.append(f"{len(missing)} manifolds of the oracle are not reported (volume, collider): {missing[:8]}")
    if extra:
        problems.append(f"{len(extra)} records without a manifold of the oracle (volume, collider): {extra[:8]}")
    for key in sorted(set(expected) & set(got)):
        e, r = expected[key], got[key]
        n = int(r["count_flags"]) & 7
        want_points = np.zeros((4, 4), np.float32); want_points[:len(e["points"])] = e["points"]
        same = (n == len(e["points"]) and int(r["count_flags"]) == (n | (256 if e["volume_is_b"] else 0)) and int(r["entity"]) == e["entity"]
                and int(r["object_type"]) == e["object_type"] and r["normal"].tobytes() == e["normal"].tobytes() and r["points"].tobytes() == want_points.tobytes())
        if not same:
            problems.append(f"{key}: got flags {int(r['count_flags']):#x} entity {int(r['entity'])} normal {r['normal']} points {r['points'][:max(n, 1)]}; "
                            f"oracle B={e['volume_is_b']} entity {e['entity']} normal {e['normal']} points {e['points']}")
    return problems


def sunk_sphere_case():
    """The facade program's single pair: a static box with its top at y = 0 and a sphere volume of radius 0.5 sunk 0.1 into it."""
    e = scenes.make_entities(1, capi.ENTITY_STATIC)
    c = scenes.make_colliders(1, capi.AABB); c["shape"][0, :6] = (-2, -1, -2, 2, 0, 2)
    sc = scenes.Scene("sunk_sphere", e, np.zeros(1, np.uint32), c, 10)
    return sc, capi.sphere_volume((0.25, 0.4, -0.5), 0.5)
