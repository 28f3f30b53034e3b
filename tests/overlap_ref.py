"""Yardsticks of the volume-overlap scene query (include/mi_physics.h, mi_world_overlap), none of which needs a GPU.

  * world shapes of a scene's colliders and of query volumes in float64 (the reference's promotion of a rotated AABB to an OBB included)
    and a SIGNED GAP for the closed-form pairs: negative = the shapes overlap, positive = they are apart by that distance (sphere vs
    sphere / capsule / AABB / OBB, capsule vs capsule: distance minus radii; AABB vs AABB: the largest slab gap);
  * the volume sets the GPU tests use, and the same sets shrunk / grown about every volume's centre;
  * the reference's own answer through its trigger path: an oracle world holding the scene plus one trigger entity per volume takes one
    step with events enabled; its TRIGGER_ENTER events are the overlaps at the step's starting poses."""
import numpy as np

from d3d12renderer_amd import capi, scenes

SPHERE, CAPSULE, CYLINDER, AABB, OBB, HULL = range(6)
OBJ_RIGID, OBJ_STATIC, OBJ_FORCE_FIELD, OBJ_TRIGGER = 0, 1, 2, 3
FLAG_OF_OBJ = {OBJ_RIGID: 1, OBJ_STATIC: 2, OBJ_TRIGGER: 8, OBJ_FORCE_FIELD: 16}
OBJ_OF_KIND = {capi.ENTITY_DYNAMIC: OBJ_RIGID, capi.ENTITY_KINEMATIC: OBJ_RIGID, capi.ENTITY_STATIC: OBJ_STATIC,
               capi.ENTITY_TRIGGER: OBJ_TRIGGER, capi.ENTITY_FORCE_FIELD: OBJ_FORCE_FIELD}
CLOSED_FORM = {(SPHERE, SPHERE), (SPHERE, CAPSULE), (SPHERE, AABB), (SPHERE, OBB), (CAPSULE, CAPSULE), (AABB, AABB)}


def qmat(q):
    """Rotation matrix of the quaternion (x, y, z, w)."""
    x, y, z, w = (float(v) for v in q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def world_shape(ctype, shape, position, rotation):
    """(world type, parameters) of a collider with local shape words `shape` on an entity at (position, rotation), as the step's first
    kernel places it: sphere (c, r); capsule / cylinder (a, b, r); AABB (mn, mx); OBB (c, half, R); hull (p, R)."""
    s = np.asarray(shape, np.float64); p = np.asarray(position, np.float64)
    identity = tuple(float(v) for v in rotation) == (0.0, 0.0, 0.0, 1.0)
    R = qmat(rotation)
    if ctype == SPHERE:
        return SPHERE, (p + R @ s[:3], s[3])
    if ctype in (CAPSULE, CYLINDER):
        return ctype, (p + R @ s[:3], p + R @ s[3:6], s[6])
    if ctype == AABB:
        if identity:
            return AABB, (s[:3] + p, s[3:6] + p)
        return OBB, (p + R @ ((s[:3] + s[3:6]) / 2), (s[3:6] - s[:3]) / 2, R)
    if ctype == OBB:
        return OBB, (p + R @ s[4:7], s[7:10], R @ qmat(s[:4]))
    return HULL, (p + R @ s[4:7], R @ qmat(s[:4]))


def _seg_point(a, b, p):
    ab = b - a
    aa = ab @ ab
    t = np.clip((p - a) @ ab / aa, 0, 1) if aa > 0 else 0.0
    return np.linalg.norm(p - (a + t * ab))


def _seg_seg(p1, q1, p2, q2):
    """Distance between two segments (Ericson, Real-Time Collision Detection 5.1.9)."""
    d1, d2, r = q1 - p1, q2 - p2, p1 - p2
    a, e, f = d1 @ d1, d2 @ d2, d2 @ r
    if a <= 1e-30 and e <= 1e-30:
        return np.linalg.norm(r)
    if a <= 1e-30:
        s, t = 0.0, np.clip(f / e, 0, 1)
    else:
        c = d1 @ r
        if e <= 1e-30:
            t, s = 0.0, np.clip(-c / a, 0, 1)
        else:
            b = d1 @ d2
            den = a * e - b * b
            s = np.clip((b * f - c * e) / den, 0, 1) if den > 1e-30 else 0.0
            t = (b * s + f) / e
            if t < 0:
                t, s = 0.0, np.clip(-c / a, 0, 1)
            elif t > 1:
                t, s = 1.0, np.clip((b - c) / a, 0, 1)
    return np.linalg.norm((p1 + s * d1) - (p2 + t * d2))


def _box_point(mn, mx, p):
    return np.linalg.norm(p - np.clip(p, mn, mx))


def signed_gap(a, b):
    """The signed gap of two world shapes (type, parameters), or None when the pair has no closed form here."""
    (ta, pa), (tb, pb) = a, b
    if ta > tb:
        (ta, pa), (tb, pb) = (tb, pb), (ta, pa)
    if (ta, tb) not in CLOSED_FORM:
        return None
    if ta == SPHERE:
        c, r = pa
        if tb == SPHERE:
            return np.linalg.norm(c - pb[0]) - r - pb[1]
        if tb == CAPSULE:
            return _seg_point(pb[0], pb[1], c) - r - pb[2]
        if tb == AABB:
            return _box_point(pb[0], pb[1], c) - r
        cc, half, R = pb
        return _box_point(-half, half, R.T @ (c - cc)) - r
    if ta == CAPSULE:
        return _seg_seg(pa[0], pa[1], pb[0], pb[1]) - pa[2] - pb[2]
    return float(np.max(np.maximum(pa[0] - pb[1], pb[0] - pa[1])))


def scene_world_shapes(sc, positions, rotations):
    """Per WORLD collider index (reverse creation order): (entity, object type, world shape)."""
    out = []
    nc = len(sc.colliders)
    for k in range(nc):
        ci = nc - 1 - k
        ent = int(sc.collider_entities[ci]); c = sc.colliders[ci]
        out.append((ent, OBJ_OF_KIND[int(sc.entities["kind"][ent])], world_shape(int(c["type"]), c["shape"], positions[ent], rotations[ent])))
    return out


def volume_world_shape(v):
    return world_shape(int(v["type"]), v["shape"], v["position"], v["rotation"])


# ---- the volume sets
def volume_hull():
    """The hull geometry the volume sets use (geometry 0 of shape_zoo; added to scenes without one)."""
    return scenes.convex_hull_mesh(5)


def make_volumes(seed, per_type, lo, hi, size_lo=0.15, size_hi=4.0, hull_geometry=0):
    """per_type volumes of each of the six types, random poses in the box [lo, hi], sizes log-uniform in [size_lo, size_hi] (from a
    fraction of a collider to several lattice spacings); every second AABB keeps the identity rotation (a true AABB, the others become
    OBBs); hull volumes have the size of the geometry."""
    rng = np.random.default_rng(seed)
    vols = np.zeros(6 * per_type, dtype=capi.query_volume_dtype)
    for i in range(len(vols)):
        t = i % 6
        s = float(np.exp(rng.uniform(np.log(size_lo), np.log(size_hi))))
        q = rng.normal(size=4); q /= np.linalg.norm(q)
        lq = rng.normal(size=4); lq /= np.linalg.norm(lq)
        off = rng.uniform(-0.2, 0.2, 3) * s
        v = vols[i]
        v["type"] = t
        v["position"] = rng.uniform(lo, hi)
        v["rotation"] = q
        if t == SPHERE:
            v["shape"][:4] = (*off, s)
        elif t in (CAPSULE, CYLINDER):
            v["shape"][:7] = (off[0], off[1] - s, off[2], off[0], off[1] + s, off[2], 0.5 * s)
        elif t == AABB:
            h = rng.uniform(0.4, 1.0, 3) * s
            v["shape"][:6] = (*(off - h), *(off + h))
            if (i // 6) % 2 == 0:
                v["rotation"] = (0, 0, 0, 1)
        elif t == OBB:
            v["shape"][:10] = (*lq, *off, *(rng.uniform(0.4, 1.0, 3) * s))
        else:
            v["shape"][:7] = (*lq, *rng.uniform(-0.2, 0.2, 3))
            v["hull_geometry"] = hull_geometry
    return vols


def scale_volumes(vols, factor, scaled_hull_geometry):
    """Every volume scaled by `factor` about its own centre: radius, half-extents, the segment about its midpoint; hull volumes switch to
    `scaled_hull_geometry` (the same vertices times factor)."""
    out = vols.copy()
    for v in out:
        t = int(v["type"]); s = v["shape"].astype(np.float64)
        if t == SPHERE:
            s[3] *= factor
        elif t in (CAPSULE, CYLINDER):
            mid = (s[:3] + s[3:6]) / 2
            s[:3] = mid + (s[:3] - mid) * factor; s[3:6] = mid + (s[3:6] - mid) * factor; s[6] *= factor
        elif t == AABB:
            mid = (s[:3] + s[3:6]) / 2; h = (s[3:6] - s[:3]) / 2 * factor
            s[:3] = mid - h; s[3:6] = mid + h
        elif t == OBB:
            s[7:10] *= factor
        else:
            v["hull_geometry"] = scaled_hull_geometry
        v["shape"] = s
    return out


SCENE_BOXES = {   # where the volumes go: (initial poses, settled poses)
    "shape_zoo": (((-4.5, 0.5, -4.5), (4.5, 6.3, 4.5)), ((-5.5, 0.0, -5.5), (5.5, 2.0, 5.5))),
    # (after 300 steps the wind zone has pushed the zones bodies along +x and -z: they lie on the ground over about x 0..11, z -7..2)
    "zones": (((-4.0, 0.3, -4.0), (4.0, 5.8, 4.0)), ((0.0, 0.0, -7.0), (11.0, 0.8, 2.0))),
}


def query_scene(name):
    """The scene of that name with the volume sets' hull geometry as geometry 0."""
    sc = getattr(scenes, name)()
    if not sc.hulls:
        sc.hulls = [volume_hull()]
    return sc


def volume_set(name, settled, per_type=16):
    lo, hi = SCENE_BOXES[name][1 if settled else 0]
    return make_volumes({"shape_zoo": 101, "zones": 202}[name] + (1 if settled else 0), per_type, lo, hi)


# ---- the reference's trigger path
def oracle_trigger_overlaps(oracle_mod, sc, vols, factor, body_states=None):
    """Per volume the set of rigid-body entities the reference reports as overlapping the volume scaled by `factor`: a fresh oracle world
    with the scene (bodies at `body_states` = (entities, 13 floats each) when given), one trigger entity per volume, one step."""
    from dataclasses import replace
    verts, tris = sc.hulls[0]
    hulls = list(sc.hulls) + [((verts.astype(np.float64) * factor).astype(np.float32), tris)]
    scaled = scale_volumes(vols, factor, len(hulls) - 1)
    n_ent = len(sc.entities)
    te = scenes.make_entities(len(vols), capi.ENTITY_TRIGGER)
    te["position"] = scaled["position"]; te["rotation"] = scaled["rotation"]
    tc = scenes.make_colliders(len(vols), capi.SPHERE)
    tc["type"] = scaled["type"]; tc["shape"] = scaled["shape"]; tc["hull_geometry"] = scaled["hull_geometry"]
    big = replace(sc, entities=np.concatenate([sc.entities, te]),
                  collider_entities=np.concatenate([sc.collider_entities, np.arange(n_ent, n_ent + len(vols), dtype=np.uint32)]).astype(np.uint32),
                  colliders=np.concatenate([sc.colliders, tc]), hulls=hulls)
    w = big.populate(oracle_mod.create_world(oracle_mod.ORDER_REFERENCE))
    if body_states is not None:
        w.set_body_states(*body_states)
    w.enable_events(True)
    w.step_fixed(sc.settings(), sc.dt, 1)
    sets = [set() for _ in vols]
    rigid = (sc.entities["kind"] == capi.ENTITY_DYNAMIC) | (sc.entities["kind"] == capi.ENTITY_KINEMATIC)
    for e in w.poll_events():
        if e["type"] != capi.EVENT_TRIGGER_ENTER:
            continue
        a, b = int(e["entity_a"]), int(e["entity_b"])
        trig, other = (a, b) if a >= n_ent else (b, a)
        if trig >= n_ent and other < n_ent and rigid[other]:
            sets[trig - n_ent].add(other)
    w.close()
    return sets


def oracle_sandwich(oracle_mod, sc, vols, body_states=None, rel=1e-3):
    """(shrunk, grown) entity sets per volume and the inputs' quality: (shrunk is a subset of grown, share of volumes with both sets
    non-empty, ambiguous share |grown \\ shrunk| / |grown|)."""
    shrunk = oracle_trigger_overlaps(oracle_mod, sc, vols, 1.0 - rel, body_states)
    grown = oracle_trigger_overlaps(oracle_mod, sc, vols, 1.0 + rel, body_states)
    subset = all(s <= g for s, g in zip(shrunk, grown))
    both = sum(1 for s, g in zip(shrunk, grown) if s and g) / max(len(vols), 1)
    n_grown = sum(len(g) for g in grown)
    ambiguous = sum(len(g - s) for s, g in zip(shrunk, grown)) / max(n_grown, 1)
    return shrunk, grown, (subset, both, ambiguous)


def entity_sets(offsets, hits, count):
    return [set(int(e) for e in hits["entity"][offsets[v]:offsets[v + 1]]) for v in range(count)]
