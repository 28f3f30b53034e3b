"""Float64 yardstick of the shape-cast scene query (include/mi_physics.h, mi_world_sweep); numpy only, no GPU.

  * convex shapes as a CORE plus a radius margin: spheres and capsules are a point / a segment plus their radius, cylinders are the disc
    support of the whole shape, boxes their corners, hulls their vertices (world shapes come from overlap_ref.world_shape);
  * the DISTANCE between two cores by GJK, whose closest point of a simplex of at most 4 vertices is found by solving every sub-simplex
    (the affine minimiser of each, kept when its weights are non-negative; the nearest of those wins);
  * the TIME OF IMPACT of a volume moved along a displacement by conservative advancement: t += gap / -(d.n) with n the unit direction
    from the collider to the volume at the current t; a miss when d.n >= 0 or t > 1; a hit once the gap is <= 1e-10; with a slack, the
    cast of the shapes grown or shrunk by it;
  * the CLOSEST APPROACH of a volume's path to a collider: the gap of the collider and the convex shape the moving volume covers;
  * a cast against a scene: the candidates are culled by the swept bounds (the slab entry time of the displacement into the collider's
    AABB grown by the volume's half-extents, a lower bound of the time of impact) before the pair loop runs;
  * the cast set the tests use.

Nothing here restates the GPU code: that one clips a ray against support planes of the Minkowski difference in float32."""
import itertools

import numpy as np

import overlap_ref as R

GAP_EPS = 1e-10


# ---- shapes: ("pts", vertices[n, 3], margin), ("cyl", a, b, radius) or ("swept", shape, d): everything the shape covers while it moves by d
def convex(world_shape, hull_vertices=None):
    """The core-plus-margin form of an overlap_ref world shape (type, parameters); hull_vertices = the geometry's local vertices."""
    t, p = world_shape
    if t == R.SPHERE:
        return ("pts", np.asarray(p[0], np.float64).reshape(1, 3), float(p[1]))
    if t == R.CAPSULE:
        return ("pts", np.stack([p[0], p[1]]).astype(np.float64), float(p[2]))
    if t == R.CYLINDER:
        return ("cyl", np.asarray(p[0], np.float64), np.asarray(p[1], np.float64), float(p[2]))
    if t == R.AABB:
        mn, mx = p
        return ("pts", np.array([[(mn, mx)[i][0], (mn, mx)[j][1], (mn, mx)[k][2]] for i, j, k in itertools.product((0, 1), repeat=3)], np.float64), 0.0)
    if t == R.OBB:
        c, half, rot = p
        signs = np.array(list(itertools.product((-1.0, 1.0), repeat=3)))
        return ("pts", c + (signs * half) @ rot.T, 0.0)
    pos, rot = p
    return ("pts", pos + np.asarray(hull_vertices, np.float64) @ rot.T, 0.0)


def moved(shape, offset):
    offset = np.asarray(offset, np.float64)
    if shape[0] == "pts":
        return ("pts", shape[1] + offset, shape[2])
    if shape[0] == "swept":
        return ("swept", moved(shape[1], offset), shape[2])
    return ("cyl", shape[1] + offset, shape[2] + offset, shape[3])


def margin(shape):
    return shape[2] if shape[0] == "pts" else margin(shape[1]) if shape[0] == "swept" else 0.0


def bounds(shape):
    """World AABB of the whole shape (margin included)."""
    if shape[0] == "pts":
        return shape[1].min(axis=0) - shape[2], shape[1].max(axis=0) + shape[2]
    if shape[0] == "swept":
        mn, mx = bounds(shape[1])
        return np.minimum(mn, mn + shape[2]), np.maximum(mx, mx + shape[2])
    a, b, r = shape[1:]
    u = b - a
    n = np.linalg.norm(u)
    e = r * np.sqrt(np.maximum(0.0, 1.0 - (u / n) ** 2)) if n > 0 else np.full(3, r)
    return np.minimum(a, b) - e, np.maximum(a, b) + e


def support(shape, direction):
    """The core's support point along `direction`."""
    if shape[0] == "pts":
        return shape[1][int(np.argmax(shape[1] @ direction))]
    if shape[0] == "swept":
        p = support(shape[1], direction)
        return p + shape[2] if direction @ shape[2] > 0 else p
    a, b, r = shape[1:]
    far = a if direction @ a > direction @ b else b
    u = b - a
    n = np.linalg.norm(u)
    perp = direction - (direction @ u) / (n * n) * u if n > 0 else direction
    if n > 0:
        perp = perp - (perp @ u) / (n * n) * u   # (once more: under a direction nearly along the axis the short remainder keeps rounding error along the axis, which the scaling to the radius blows up: the rim point would leave the cap's plane)
    ln = np.linalg.norm(perp)
    return far + (r / ln) * perp if ln > 1e-14 * max(np.linalg.norm(direction), 1e-300) else far


# ---- GJK distance between two cores
def _closest_on_simplex(ys):
    """Closest point of conv(ys) to the origin by solving every sub-simplex: (point, indices kept, their weights)."""
    best = None
    n = len(ys)
    for k in range(1, n + 1):
        for idx in itertools.combinations(range(n), k):
            y = ys[list(idx)]
            if k == 1:
                w = np.ones(1)
            else:
                e = y[1:] - y[0]
                s, _, rank, sv = np.linalg.lstsq(e.T, -y[0], rcond=None)   # (on the edges themselves, not their Gram matrix: half the digits lost)
                if rank < k - 1 or sv[-1] <= 1e-7 * sv[0]:
                    continue   # a (nearly) degenerate sub-simplex: its faces are solved on their own
                w = np.concatenate([[1.0 - s.sum()], s])
                if (w < 0).any():
                    continue
            p = w @ y
            if k == 4:
                p = np.zeros(3)   # (the affine hull of a proper tetrahedron is the whole space: the origin is inside)
            d2 = p @ p
            if best is None or d2 < best[0]:
                kept = [i for i in range(k) if w[i] > 0] or [0]
                best = (d2, p, [idx[i] for i in kept], w[kept])
    return best[1], best[2], best[3]


def core_distance(a, b, max_iterations=64):
    """(distance, unit direction from b to a, closest point on b's core) of the two CORES; distance 0 (direction 0) when they intersect."""
    pb = support(b, np.array([-1.0, 0.0, 0.0]))
    v = support(a, np.array([1.0, 0.0, 0.0])) - pb
    ys = v.reshape(1, 3); bs = pb.reshape(1, 3)
    for _ in range(max_iterations):
        vv = v @ v
        if vv <= 1e-28:
            return 0.0, np.zeros(3), pb
        sa, sb = support(a, -v), support(b, v)
        y = sa - sb
        if vv - v @ y <= 1e-14 * vv or any(np.array_equal(y, q) for q in ys):   # no support point closer than v: v is the closest vector
            break
        ys = np.vstack([ys, y]); bs = np.vstack([bs, sb])
        p, keep, w = _closest_on_simplex(ys)
        if len(keep) == 4 or p @ p <= 1e-28:
            return 0.0, np.zeros(3), pb
        ys, bs = ys[keep], bs[keep]
        pb = w @ bs   # the witness on b: the same weights on b's support points
        v = p
    dist = float(np.linalg.norm(v))
    return dist, v / dist, pb


def gap(a, b):
    """Signed-at-zero gap of two shapes: core distance minus both margins (negative only as far as the margins reach; 0 when the cores meet
    and there is no margin).  For a certain overlap test use gap < 0."""
    return core_distance(a, b)[0] - margin(a) - margin(b)


def point_gap(point, shape):
    """Distance of a point from a shape's surface (outside: positive) — the gap of a zero-radius sphere at `point`."""
    return gap(("pts", np.asarray(point, np.float64).reshape(1, 3), 0.0), shape)


def closest_approach(vol, col, d):
    """The smallest gap between `col` and `vol` anywhere on its way along d, t in [0, 1]: the gap of the collider and everything the moving
    volume covers (a convex shape again), so one distance query and no search over t.  0 or below (as far as the margins reach): a hit."""
    return gap(("swept", vol, np.asarray(d, np.float64)), col)


def time_of_impact(vol, col, d, max_steps=256, slack=0.0, plain=None):
    """Conservative advancement of `vol` along d against `col`: None on a miss, else (t, unit normal from col to vol, point on col,
    initial overlap).  t in [0, 1].  slack is added to the sum of the margins: the cast of shapes grown (slack > 0) or shrunk (slack < 0) by
    that much between them.  Where the margins cannot be shrunk that far (boxes, hulls and cylinders have none; the core distance does
    not measure a depth), the shrunk cast is the plain one required to travel on past its touch until it is -slack deep along the
    touch's normal: exact while the touching features stay the same (flat contacts), an upper bound of the depth elsewhere.  plain = the
    result of the plain cast (slack 0) where the caller has it, not to compute it again."""
    d = np.asarray(d, np.float64)
    rr = margin(vol) + margin(col) + slack
    if rr < 0:
        hit = plain if plain is not None else time_of_impact(vol, col, d, max_steps)
        if hit is None or hit[3]:
            return hit
        t = hit[0] + rr / (d @ hit[1])   # (d.n < 0 at a hit)
        return (t, *hit[1:]) if t <= 1 else None
    t = 0.0
    last = np.zeros(3)
    for step in range(max_steps):
        dist, n, pb = core_distance(moved(vol, t * d), col)
        g = dist - rr
        if g <= GAP_EPS:
            if step == 0:
                return 0.0, np.zeros(3), None, True
            if dist <= 1e-7:
                n = last   # cores this close (shapes without a margin) no longer resolve their direction: the last approach's, from a healthy distance
            return t, n, pb + margin(col) * n, False
        last = n
        dn = d @ n
        if dn >= 0:
            return None
        t += g / -dn
        if t > 1:
            return None
    raise RuntimeError("conservative advancement did not converge")


# ---- casts against a scene
def slab_entry(mn, mx, half, origin, d):
    """Entry time in [0, 1] of the segment origin + t d into the box [mn - half, mx + half], or None: a lower bound of the time of impact
    of a volume with these half-extents about `origin`."""
    lo, hi = mn - half - origin, mx + half - origin
    t0, t1 = 0.0, 1.0
    for i in range(3):
        if d[i] == 0:
            if lo[i] > 0 or hi[i] < 0:
                return None
        else:
            a, b = lo[i] / d[i], hi[i] / d[i]
            t0, t1 = max(t0, min(a, b)), min(t1, max(a, b))
    return t0 if t0 <= t1 else None


def cast(vol, d, colliders, lead=None):
    """The first hit of `vol` moved along d among `colliders` (a list of shapes; None entries are skipped): (index, t, normal, point,
    initial) or None.  lead = a list to receive (t, index) of every collider whose time of impact was computed (all those that could
    come within the cull of the winner)."""
    d = np.asarray(d, np.float64)
    vmn, vmx = bounds(vol)
    origin, half = (vmn + vmx) / 2, (vmx - vmn) / 2
    cands = []
    for k, c in enumerate(colliders):
        if c is None:
            continue
        cmn, cmx = bounds(c)
        e = slab_entry(cmn, cmx, half + 1e-9, origin, d)
        if e is not None:
            cands.append((e, k))
    cands.sort()
    best = None
    slack = 0.05 / max(np.linalg.norm(d), 1e-300)   # runner-ups are evaluated up to this far behind the winner
    for e, k in cands:
        if best is not None and e > best[1] + (slack if lead is not None else 0.0):
            break
        hit = time_of_impact(vol, colliders[k], d)
        if hit is None:
            continue
        if lead is not None:
            lead.append((hit[0], k))
        if best is None or (hit[0], k) < (best[1], best[0]):
            best = (k, *hit)
    return best


# ---- the scene and the cast set of the tests
def scene_convex(sc, positions, rotations):
    """Per world collider index: (entity, object type, convex shape) of a scene at the given entity poses."""
    out = []
    nc = len(sc.colliders)
    for k, (ent, obj, ws) in enumerate(R.scene_world_shapes(sc, positions, rotations)):
        c = sc.colliders[nc - 1 - k]
        hv = sc.hulls[int(c["hull_geometry"])][0] if int(c["type"]) == R.HULL else None
        out.append((ent, obj, convex(ws, hv)))
    return out


def volume_convex(v, hulls):
    hv = hulls[int(v["hull_geometry"])][0] if int(v["type"]) == R.HULL else None
    return convex(R.volume_world_shape(v), hv)


def cast_set(seed, per_type=8):
    """Volumes of all six types started on a half-sphere of radius 10 about (0, 3.4, 0) — outside every collider of shape_zoo — and cast
    through the scene box: (volumes, displacements float32 [n, 3])."""
    lo, hi = R.SCENE_BOXES["shape_zoo"][0]
    vols = R.make_volumes(seed, per_type, lo, hi, 0.15, 1.0)
    rng = np.random.default_rng(seed + 1000)
    n = len(vols)
    u = rng.normal(size=(n, 3)); u /= np.linalg.norm(u, axis=1, keepdims=True); u[:, 1] = np.abs(u[:, 1])
    start = np.array([0.0, 3.4, 0.0]) + 10.0 * u
    target = rng.uniform(lo, hi, (n, 3))
    vols["position"] = start.astype(np.float32)
    disp = (1.3 * (target - vols["position"].astype(np.float64))).astype(np.float32)
    return vols, disp


def initial_entity_poses(sc):
    return sc.entities["position"].astype(np.float64), sc.entities["rotation"]


_CAST_SET_CACHE = {}


def cast_set_reference(seed):
    """The cast set of `seed` against shape_zoo at its initial poses, computed once per process: a dict with the scene, its colliders as
    (entity, object type, convex shape), the volumes and displacements, the volumes' convex shapes, per cast the reference's hit
    (collider, t, normal, point, initial) or None, and per cast the lead of the winner over the runner-up in travelled distance (inf
    without a runner-up within reach)."""
    if seed not in _CAST_SET_CACHE:
        sc = R.query_scene("shape_zoo")
        cols = scene_convex(sc, *initial_entity_poses(sc))
        shapes = [c[2] for c in cols]
        vols, disp = cast_set(seed)
        convs, hits, leads = [], [], []
        for v, d in zip(vols, disp):
            vc = volume_convex(v, sc.hulls)
            found = []
            hit = cast(vc, d, shapes, found)
            found.sort()
            convs.append(vc); hits.append(hit)
            leads.append((found[1][0] - found[0][0]) * float(np.linalg.norm(d.astype(np.float64))) if len(found) > 1 else np.inf)
        _CAST_SET_CACHE[seed] = dict(scene=sc, colliders=cols, volumes=vols, displacements=disp, convex=convs, hits=hits, leads=leads)
    return _CAST_SET_CACHE[seed]
