"""Distance scene queries on the GPU (mi_world_distance, mi_world_distance_device_async, mi_debug_distance_exhaustive), one record per
volume and always through both kernels: a closed-form table, the pair-level matrix of tests/distance_matrix.py against the float64 reference
of tests/sweep_ref.py, the accelerated kernel against the exhaustive one byte for byte on scenes built to exercise the shell walk, a float64
brute force over a scene, the filters and invalid input, the device variant, and that queries change nothing a step computes while following
every step, body-state write and checkpoint load."""
import numpy as np
import pytest

import distance_matrix as D
import overlap_ref as R
import query_helpers as Q
import sweep_matrix as M
import sweep_ref as S

pytestmark = pytest.mark.gpu

RIGID, STATIC, TERRAIN, TRIGGERS, FIELDS, ALL = 1, 2, 4, 8, 16, 31
MISS = 0xFFFFFFFF
OVERLAP, UNCONVERGED = 1, 2
INF = np.float32(np.inf)
# THE BOUNDS (distance_matrix.BOUNDS, per unit of scale = max(1, the largest |coordinate| of the pair)): 4 x the largest value measured on the
# MI355X against the float64 reference, rounded up to one digit; the factor covers compilers and seeds, not the algorithm.  The largest of
# |distance - reference|, both points' distances from their shapes, ||point_volume - point_collider| - distance| and
# |point_volume - point_collider - distance x normal| per family, per unit of scale, as test_matrix_family prints them:
#   generic 6.76e-7 -> 3e-6, aligned 1.23e-6 -> 5e-6, near 1.04e-6 -> 5e-6, far (coordinates of 1e2 and 1e3) 1.75e-6 -> 7e-6,
#   size_ratio (1e-2 against 20 to 200 units) 6.07e-6 -> 3e-5, separation (gaps of 10 to 1e3 sizes) 9.77e-7 -> 4e-6, cut 1.32e-6 -> 6e-6.
# In every family the figure is the distance's: the pair test stops once its upper and lower bound are within 2e-6 x the coordinates, and the
# points stay within 1.1e-7 scale of their shapes.  No case of the matrix ends unconverged.  The brute force over the built scene measured
# 1.40e-6 (SCENE_BOUND: 4 x that); the closed-form table is held to the generic bound at its largest coordinate, 25.
SCENE_BOUND = 6e-6
TABLE_BOUND = 25 * D.BOUNDS["generic"]


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


def _bytes_equal(a, b, what):
    if a.tobytes() != b.tobytes():
        bad = [i for i in range(len(a)) if a[i].tobytes() != b[i].tobytes()]
        raise AssertionError(f"{what}: {len(bad)} of {len(a)} records differ; first {bad[:4]}: {a[bad[:2]]} vs {b[bad[:2]]}")


def _both(w, vols, max_d=None, include=ALL, ranges=None, what=""):
    """The accelerated records, equal byte for byte to the exhaustive ones, in the shape every record has."""
    a = w.distance(vols, max_d, include, ranges)
    _bytes_equal(a, w.debug_distance_exhaustive(vols, max_d, include, ranges), what)
    assert np.array_equal(a["volume"], np.arange(len(vols), dtype=np.uint32)) and (a["pad"] == 0).all(), what
    miss = a["entity"] == MISS
    assert (a["collider"][miss] == MISS).all() and np.isposinf(a["distance"][miss]).all() and (a["object_type"][miss] == 0).all() and (a["flags"][miss] == 0).all(), what
    assert (a["point_collider"][miss] == 0).all() and (a["point_volume"][miss] == 0).all() and (a["normal"][miss] == 0).all(), what
    hit = a[~miss]
    assert (hit["distance"] >= 0).all() and np.isfinite(hit["distance"]).all(), what
    if max_d is not None:
        assert (hit["distance"] <= np.broadcast_to(np.asarray(max_d, np.float32), (len(a),))[~miss]).all(), what
    over = (hit["flags"] & OVERLAP) != 0
    assert ((hit["distance"] == 0) == over).all() and (hit["normal"][over] == 0).all(), what
    assert (hit["point_collider"][over] == np.asarray(vols)["position"][~miss][over]).all() and (hit["point_volume"][over] == np.asarray(vols)["position"][~miss][over]).all(), what
    return a


def _measures(rec, vconv, cconv):
    """Of a hit that is no overlap: both points off their shapes, ||pv - pc| - distance|, |pv - pc - distance n|, ||n| - 1|."""
    pc, pv, n, d = rec["point_collider"].astype(np.float64), rec["point_volume"].astype(np.float64), rec["normal"].astype(np.float64), float(rec["distance"])
    return (abs(S.point_gap(pc, cconv)), abs(S.point_gap(pv, vconv)), abs(np.linalg.norm(pv - pc) - d), float(np.linalg.norm(pv - pc - d * n)), abs(np.linalg.norm(n) - 1))


# ---- 1. closed forms
def _table_world(mi_lib):
    from d3d12renderer_amd import capi, scenes
    e = scenes.make_entities(6, capi.ENTITY_STATIC)
    e["position"] = [(0, 0, 0), (10, 0, 0), (0, 0, 10), (0, 0, 20), (20, 0, 0), (0, 0, -10)]
    e["rotation"][5] = scenes.q_axis_angle((0, 1, 0), np.pi / 6)
    c = scenes.make_colliders(6, capi.SPHERE)
    c["shape"][0, :4] = (0, 0, 0, 0.5)
    c["type"][1] = capi.AABB; c["shape"][1, :6] = (-1, -1, -1, 1, 1, 1)
    c["type"][2] = capi.CAPSULE; c["shape"][2, :7] = (0, -1, 0, 0, 1, 0, 0.3)
    c["type"][3] = capi.CYLINDER; c["shape"][3, :7] = (0, -1, 0, 0, 1, 0, 0.4)
    c["type"][4] = capi.HULL; c["shape"][4, :7] = (0, 0, 0, 1, 0, 0, 0); c["hull_geometry"][4] = 0
    c["type"][5] = capi.AABB; c["shape"][5, :6] = (-1, -0.5, -0.7, 1, 0.5, 0.7)   # (under the entity's rotation: an OBB)
    sc = scenes.Scene("distance_table", e, np.arange(6, dtype=np.uint32), c, 10, hulls=[R.volume_hull()])
    return sc, Q.world(mi_lib, sc)


def test_closed_form_table(mi_lib):
    from d3d12renderer_amd import capi, scenes
    sc, w = _table_world(mi_lib)
    lowest = float(sc.hulls[0][0][:, 1].min())
    u = R.qmat(sc.entities["rotation"][5])[:, 0]   # the rotated box's own x axis
    r2 = np.sqrt(0.5)
    cases = [   # (volume, entity range, distance, point on the collider, point on the volume, normal); None = not unique
        (capi.sphere_volume((-3, 0, 0), 0.25), 0, 2.25, (-0.5, 0, 0), (-2.75, 0, 0), (-1, 0, 0)),                                          # sphere - sphere
        (capi.sphere_volume((1.2, 1.6, 0), 0.25), 0, 1.25, (0.3, 0.4, 0), (1.05, 1.4, 0), (0.6, 0.8, 0)),
        (capi.sphere_volume((13, 0.1, 0.2), 0.25), 1, 1.75, (11, 0.1, 0.2), (12.75, 0.1, 0.2), (1, 0, 0)),                                 # sphere - box face
        (capi.sphere_volume((12, 2, 0.2), 0.25), 1, np.sqrt(2) - 0.25, (11, 1, 0.2), (12 - 0.25 * r2, 2 - 0.25 * r2, 0.2), (r2, r2, 0)),   # ... edge
        (capi.sphere_volume((12, 2, 2), 0.25), 1, np.sqrt(3) - 0.25, (11, 1, 1), None, np.ones(3) / np.sqrt(3)),                           # ... corner
        (capi.sphere_volume((13, 0.1, 0.2), 0.0), 1, 2.0, (11, 0.1, 0.2), (13, 0.1, 0.2), (1, 0, 0)),                                      # a point
        (capi.capsule_volume((-1, 2, 10), (1, 2, 10), 0.2), 2, 1.0 - 0.5, (0, 1.3, 10), (0, 1.8, 10), (0, 1, 0)),                          # capsule across the end of a capsule
        (capi.capsule_volume((-1, 0.5, 12), (1, 0.5, 12), 0.2), 2, 2.0 - 0.5, (0, 0.5, 10.3), (0, 0.5, 11.8), (0, 0, 1)),                  # skew capsules: axes x and y, 2 apart in z
        (capi.box_volume((13, 0.2, 0.1), (0.5, 0.5, 0.5)), 1, 1.5, None, None, (1, 0, 0)),                                                 # box - box, faces
        (capi.box_volume((13, 3.5, 0.1), (0.5, 0.5, 0.5)), 1, 2.5, None, None, (0.6, 0.8, 0)),                                             # ... edges (1.5 and 2.0 apart)
        (capi.box_volume((10, 3, 0), (0.5, 0.5, 0.5), rotation=scenes.q_axis_angle((0, 0, 1), np.pi / 4)), 1, 2 - r2, None, None, (0, 1, 0)),   # a turned box, edge towards the face
        (capi.cylinder_volume((13, -0.5, 0), (13, 0.5, 0), 0.3), 1, 1.7, (11, None, 0), (12.7, None, 0), (1, 0, 0)),                       # cylinder side - box face
        (capi.cylinder_volume((10, 3, 0), (10, 4, 0), 0.3), 1, 2.0, None, None, (0, 1, 0)),                                                # cylinder cap - box top
        (capi.sphere_volume((2, 0.5, 20), 0.25), 3, 2 - 0.4 - 0.25, (0.4, 0.5, 20), (1.75, 0.5, 20), (1, 0, 0)),                           # sphere - cylinder side
        (capi.sphere_volume((0.1, 3, 20), 0.25), 3, 2 - 0.25, (0.1, 1, 20), (0.1, 2.75, 20), (0, 1, 0)),                                   # sphere - cylinder cap
        (capi.box_volume((20, -5, 0), (3, 0.5, 3)), 4, lowest + 4.5, None, None, (0, -1, 0)),                                             # box under the hull: its lowest vertex
        (capi.hull_volume(0, position=(10, 6, 0)), 1, 5 + lowest, None, None, (0, 1, 0)),                                                  # hull over the box
        (capi.sphere_volume(np.array((0, 0, -10)) - 3 * u, 0.25), 5, 1.75, np.array((0, 0, -10)) - u, np.array((0, 0, -10)) - 2.75 * u, -u),   # sphere - rotated box, along its axis
        (capi.sphere_volume((-1.2, 0, 0), 1.0), 0, 0.0, None, None, None),                                                                 # overlapping
    ]
    vols = np.concatenate([c[0] for c in cases])
    ranges = np.array([(c[1], c[1] + 1) for c in cases], np.uint32)
    got = _both(w, vols, None, ALL, ranges, "table")
    worst = [0.0, 0.0, 0.0]
    for i, (_, ent, dist, pc, pv, n) in enumerate(cases):
        rec = got[i]
        assert rec["entity"] == ent and rec["object_type"] == 1, (i, rec)
        if dist == 0.0:
            assert rec["flags"] == OVERLAP and rec["distance"] == 0, (i, rec)
            continue
        assert rec["flags"] == 0, (i, rec)
        # the distance within the bound e; a direction t off the true one lengthens the distance by dist t^2 / 2 to second order, so e admits
        # t = sqrt(2 e / dist) (exact features give far less; a cylinder's side is that ill-conditioned); a point of a convex shape within e of the
        # smallest distance lies within sqrt(2 dist e + e^2) of the closest one
        e = TABLE_BOUND
        err_d, err_n = abs(float(rec["distance"]) - dist), float(np.linalg.norm(rec["normal"].astype(np.float64) - n))
        err_p = max([abs(float(h) - x) for have, want in ((rec["point_collider"], pc), (rec["point_volume"], pv)) if want is not None for h, x in zip(have, want) if x is not None] + [0.0])
        worst = [max(a, b) for a, b in zip(worst, (err_d, err_n, err_p))]
        assert err_d <= e and err_n <= np.sqrt(2 * e / dist) and err_p <= np.sqrt(2 * dist * e + e * e) + e, (i, rec, err_d, err_n, err_p)
        assert abs(np.linalg.norm(rec["normal"].astype(np.float64)) - 1) <= 1e-5, (i, rec)
    # the whole scene at once: the nearest of the six
    whole = _both(w, vols, None, ALL, None, "table, whole scene")
    assert (whole["distance"] <= got["distance"]).all() and (whole["entity"][:2] == 0).all()
    print(f"closed-form table: largest error of the distance {worst[0]:.2e}, of the normal {worst[1]:.2e}, of the points {worst[2]:.2e}")
    w.close()


# ---- 2. the pair-level matrix
# UNCONVERGED is allowed only for the cases listed here by name (family, volume type, collider type, tag), each with the largest distance error per
# unit of scale it is held to instead of the family's bound (4 x its measured figure, rounded up to one digit).
KNOWN_UNCONVERGED = {}


def _matrix_queries(mi_lib, cases, what):
    """One world per family, one static entity with one collider per case; query i sees entity i alone.  The batch is made odd (never a multiple
    of the volumes per workgroup) by a repeat of the first query."""
    w = Q.world(mi_lib, D.scene_of(cases, what))
    pick = list(range(len(cases))) + ([0] if len(cases) % 2 == 0 else [])
    vols = np.concatenate([cases[i]["volume"] for i in pick])
    max_d = np.array([INF if cases[i]["max_distance"] is None else cases[i]["max_distance"] for i in pick], np.float32)
    ranges = np.array([(i, i + 1) for i in pick], np.uint32)
    got = _both(w, vols, max_d, ALL, ranges, what)
    w.close()
    return vols, got


@pytest.mark.parametrize("name", D.FAMILIES)
def test_matrix_family(mi_lib, name):
    """All 36 (volume type, collider type) pairs of one family against the float64 reference, no case left out: the decision (hit, miss by the
    largest distance, overlap) in every case; the distance within the family's bound x scale; both points on their shapes; their distance the
    reported one; the normal unit and along them; the points themselves where they are unique (a sphere on either side: the closest point of a
    convex shape to a point is unique, and a point of that shape within e of the smallest distance d lies within sqrt(2 d e + e^2) of it);
    the flags as the family says.  Every failure of the family is reported, after the worst values."""
    cases = D.family(name)
    assert set((c["vt"], c["ct"]) for c in cases) == set(D.PAIRS)
    vols, got = _matrix_queries(mi_lib, cases, f"matrix {name}")
    bad, worst = [], {}
    for i, c in enumerate(cases):
        rec, who = got[i], f"{name}[{i}] {D.TYPES[c['vt']]} -> {D.TYPES[c['ct']]} {c['tag']} (scale {c['scale']:.3g})"
        bound = D.BOUNDS[name] * c["scale"]
        if c["expect"] == "miss":
            if rec["entity"] != MISS:
                bad.append(f"{who}: reports distance {rec['distance']:.7g} above the largest distance {c['max_distance']:.7g} (reference {c['ref']:.7g})")
            continue
        if rec["entity"] != i or rec["object_type"] != 1:
            bad.append(f"{who}: entity {rec['entity']}, object type {rec['object_type']} (reference distance {c['ref']:.7g})")
            continue
        if c["expect"] == "overlap":
            if rec["flags"] != OVERLAP or rec["distance"] != 0:
                bad.append(f"{who}: {-c['placed']:.3e} deep but flags {rec['flags']}, distance {rec['distance']:.3e}")
            continue
        known = KNOWN_UNCONVERGED.get((name, c["vt"], c["ct"], c["tag"]))
        if int(rec["flags"]) & ~(UNCONVERGED if known is not None else 0):
            bad.append(f"{who}: flags {rec['flags']} (distance {rec['distance']:.7g}, the reference {c['ref']:.7g})")
            continue
        err = float(rec["distance"]) - c["ref"]
        m = _measures(rec, c["vconv"], c["cconv"])
        row = worst.setdefault(c["vt"], [0.0] * 6)
        if known is None:
            row[0] = max(row[0], abs(err) / c["scale"])
        else:
            print(f"{who}: known unconverged case, flags {rec['flags']}, distance {err:.3e} = {err / c['scale']:.3e} scale above the reference's (allowed {known:.0e} scale)")
        for j in range(4):
            row[1 + j] = max(row[1 + j], m[j] / c["scale"])
        if abs(err) > (bound if known is None else known * c["scale"]) or (known is not None and err < -bound):
            bad.append(f"{who}: distance {rec['distance']:.7g}, the reference {c['ref']:.7g}: off by {err:.3e} > {bound:.3e}")
        for j, label in enumerate(("point_collider lies off the collider by", "point_volume lies off the volume by", "|point_volume - point_collider| differs from the distance by",
                                   "point_volume - point_collider differs from distance x normal by")):
            if m[j] > bound:
                bad.append(f"{who}: {label} {m[j]:.3e} > {bound:.3e}")
        if m[4] > 1e-5:
            bad.append(f"{who}: |normal| - 1 = {m[4]:.2e}")
        if R.SPHERE in (c["vt"], c["ct"]):
            e = 2.0 * bound
            d_centre = c["ref"] + (S.margin(c["vconv"]) if c["vt"] == R.SPHERE else S.margin(c["cconv"]))
            tol = np.sqrt(2.0 * d_centre * e + e * e) + e
            off = max(float(np.linalg.norm(rec["point_collider"] - c["ref_point_collider"])), float(np.linalg.norm(rec["point_volume"] - c["ref_point_volume"])))
            row[5] = max(row[5], off / tol)
            if off > tol:
                bad.append(f"{who}: the points lie {off:.3e} > {tol:.3e} from the reference's")
    for vt, row in sorted(worst.items()):
        print(f"{name}, {D.TYPES[vt]} volumes, per unit of scale: |distance - reference| {row[0]:.2e}, point off the collider {row[1]:.2e}, point off the volume {row[2]:.2e}, "
              f"||pv - pc| - distance| {row[3]:.2e}, |pv - pc - distance n| {row[4]:.2e}; unique points / their tolerance {row[5]:.2f}")
    if worst:
        print(f"{name}: the largest measure per unit of scale {max(max(r[:5]) for r in worst.values()):.2e} (bound {D.BOUNDS[name]:.0e})")
    assert not bad, f"{len(bad)} of {len(cases)} cases fail:\n" + "\n".join(bad)


# ---- 3. scenes: accelerated == exhaustive, byte for byte
def _zoo_volumes(rng):
    lo, hi = (-7.0, -1.0, -7.0), (7.0, 8.0, 7.0)
    vols, n_bad = Q.edge_volumes(rng, lo, hi, True, (4, 2, 2), 2, 1)   # (x 6 types each)
    return vols, n_bad


def test_zoo_accelerated_equals_exhaustive(mi_lib):
    rng = np.random.default_rng(31)
    sc = R.query_scene("shape_zoo")
    w = Q.world(mi_lib, sc)
    vols, n_bad = _zoo_volumes(rng)
    for steps in (0, 60):
        if steps:
            w.step_fixed(sc.settings(), sc.dt, steps)
        got = _both(w, vols, None, ALL, None, f"shape_zoo after {steps} steps")
        assert (got["entity"][-n_bad:] == MISS).all() and (got["entity"][:-n_bad] != MISS).all()
        assert ((got["flags"] & OVERLAP) != 0).any() and (got["distance"] > 0).any()
        for max_d in (0.0, 0.5, 4.0):
            cut = _both(w, vols[:-1], max_d, ALL, None, f"shape_zoo after {steps} steps, largest distance {max_d}")
            keep = got["distance"][:-1] <= max_d
            assert (cut["entity"] != MISS).tolist() == keep.tolist() and cut[keep].tobytes() == got[:-1][keep].tobytes()
    w.close()


_BUILT = {}


def built_scene():
    """About 300 static colliders on a ground box (the large list): a cluster of all six types in a box of 6 about (3, 1.5, 3), a row of 80 small spheres
    along x (more than 64 entries in one x-row span), a far cluster about (20, 1, 20) (the cells between the clusters are empty: more than four
    rings), twins at equal distances from (-12, 2, 0) and three overlapping spheres about (-12, 2, 10)."""
    if "scene" in _BUILT:
        return _BUILT["scene"]
    from d3d12renderer_amd import capi, scenes
    rng = np.random.default_rng(404)
    pos, rot, typ, words, hull = [], [], [], [], []

    def add(p, q, t, s, h=0):
        pos.append(p); rot.append(q); typ.append(t); hull.append(h)
        row = np.zeros(12); row[:len(s)] = s; words.append(row)

    def random_shape(centre, size):
        q = M._rand_q(rng); t = int(rng.integers(6))
        if t == R.SPHERE:
            add(centre, M.I4, capi.SPHERE, (0, 0, 0, size))
        elif t in (R.CAPSULE, R.CYLINDER):
            add(centre, q, capi.CAPSULE if t == R.CAPSULE else capi.CYLINDER, (0, -size, 0, 0, size, 0, 0.5 * size))
        elif t == R.HULL:
            add(centre, q, capi.HULL, (0, 0, 0, 1, 0, 0, 0), 0)
        else:
            h = size * rng.uniform(0.5, 1.0, 3)
            add(centre, q if t == R.OBB else M.I4, capi.AABB, (*-h, *h))
    for _ in range(200):
        random_shape(rng.uniform((0, 0.3, 0), (6, 3, 6)), rng.uniform(0.1, 0.3))
    for i in range(80):
        add((0.05 * i, 0.5, 8.0), M.I4, capi.SPHERE, (0, 0, 0, 0.05))
    for _ in range(20):
        random_shape(rng.uniform((19, 0.3, 19), (21, 2, 21)), rng.uniform(0.1, 0.3))
    twins = len(pos)
    add((-12, 2, -1.5), M.I4, capi.SPHERE, (0, 0, 0, 0.25)); add((-12, 2, 1.5), M.I4, capi.SPHERE, (0, 0, 0, 0.25))
    add((-14, 2, 0), M.I4, capi.AABB, (-0.2, -0.2, -0.2, 0.2, 0.2, 0.2)); add((-14, 2, 0), M.I4, capi.AABB, (-0.2, -0.2, -0.2, 0.2, 0.2, 0.2))   # two colliders in one place
    triple = len(pos)
    for dx in (-0.2, 0.0, 0.2):
        add((-12 + dx, 2, 10), M.I4, capi.SPHERE, (0, 0, 0, 0.3))
    add((0, -0.5, 0), M.I4, capi.AABB, (-30, -0.5, -30, 30, 0.5, 30))   # the ground
    n = len(pos)
    e = scenes.make_entities(n, capi.ENTITY_STATIC)
    e["position"] = np.array(pos, np.float32); e["rotation"] = np.array(rot, np.float32)
    c = scenes.make_colliders(n, capi.SPHERE)
    c["type"] = typ; c["shape"][:, :12] = np.array(words, np.float32); c["hull_geometry"] = hull
    sc = scenes.Scene("distance_built", e, np.arange(n, dtype=np.uint32), c, 10, hulls=list(M.hulls()))
    _BUILT["scene"] = (sc, twins, triple)
    return _BUILT["scene"]


def _collider_of(cols, entity):
    return min(k for k, c in enumerate(cols) if c[0] == entity)


def test_built_scene_accelerated_equals_exhaustive(mi_lib):
    from d3d12renderer_amd import capi
    sc, twins, triple = built_scene()
    assert 290 <= len(sc.colliders) <= 330
    w = Q.world(mi_lib, sc)
    cols = S.scene_convex(sc, *S.initial_entity_poses(sc))
    rng = np.random.default_rng(32)
    sets = [R.make_volumes(1, 3, (0, 0.3, 0), (6, 3, 6), 0.1, 0.6),                 # inside the grid, among the cluster
            R.make_volumes(2, 2, (8, 0.3, 8), (17, 3, 17), 0.1, 0.6),               # inside the grid, in the empty region between the clusters
            R.make_volumes(3, 2, (-15, 0, -3), (22, 4, 22), 0.5, 3.0),              # anywhere, larger: on the grid's border too
            R.make_volumes(4, 2, (40, 5, 40), (60, 30, 60), 0.3, 2.0),              # outside the grid
            R.make_volumes(5, 2, (990, -20, -1010), (1010, 20, -990), 0.3, 2.0)]    # 1e3 away
    big = [capi.sphere_volume((5, 3, 5), 25.0), capi.box_volume((10, 2, 10), (22, 5, 22)), capi.box_volume((0, 0, 0), (18, 18, 18), rotation=(0.1, 0.2, 0.3, 0.9)),
           capi.capsule_volume((-20, 4, -20), (25, 4, 25), 6.0), capi.cylinder_volume((3, 12, 3), (3, 40, 3), 12.0), capi.box_volume((70, 2, 3), (30, 1, 1))]   # more than 512 cells; the last ends beside the grid
    special = [capi.sphere_volume((-12, 2, 0), 0.1), capi.box_volume((-12, 2, 0), (0.1, 0.1, 0.1)), capi.sphere_volume((-14, 5, 0), 0.2),     # between the twins; above the two in one place
               capi.sphere_volume((-12, 2, 10), 0.2), capi.box_volume((-12, 2.1, 10), (0.3, 0.1, 0.1)),                                       # over the three overlapping spheres
               capi.sphere_volume((2.0, 0.5, 9.0), 0.1), capi.capsule_volume((0, 0.5, 8.4), (4, 0.5, 8.4), 0.05)]                              # beside the row of 80
    vols = np.concatenate(sets + big + special)
    n_big, n_special = len(big), len(special)
    first_special = len(vols) - n_special
    got = _both(w, vols, None, ALL, None, "built scene")
    assert (got["entity"] != MISS).all()
    # twins: the lower world collider index of the two at equal distance
    tw = [_collider_of(cols, twins + j) for j in range(4)]
    for i in (first_special, first_special + 1):
        assert got["collider"][i] == min(tw[0], tw[1]) and got["flags"][i] == 0, (i, got[i], tw)
    assert got["collider"][first_special] in tw[:2] and abs(float(got["distance"][first_special]) - (1.5 - 0.35)) <= 1e-5
    assert got["collider"][first_special + 2] == min(tw[2], tw[3]) and abs(float(got["distance"][first_special + 2]) - 2.6) <= 1e-5, got[first_special + 2]
    # three overlapping colliders: the lowest index, with the flag
    tr = [_collider_of(cols, triple + j) for j in range(3)]
    for i in (first_special + 3, first_special + 4):
        assert got["collider"][i] == min(tr) and got["flags"][i] == OVERLAP, (i, got[i], tr)
    # the ground (the large list) and the row of 80 are found
    ground = len(sc.entities) - 1
    assert (got["entity"] == ground).any()
    # the ground left out: the volumes between the clusters walk the empty cells; the far ones start on the grid's border
    no_ground = np.tile(np.array([(0, ground)], np.uint32), (len(vols), 1))
    free = _both(w, vols, None, ALL, no_ground, "built scene without the ground")
    far = slice(sum(len(x) for x in sets[:4]), sum(len(x) for x in sets))
    assert (free["entity"] != MISS).all() and (free["entity"] != ground).all() and (free["distance"][far] > 500).all()
    assert 200 <= free["entity"][first_special + 5] < 280 and 200 <= free["entity"][first_special + 6] < 280, free[first_special + 5:]
    # largest distances: 0, about a cell, many cells, per volume mixed with +inf
    for max_d in (0.0, 0.4, 6.0, np.where(np.arange(len(vols)) % 3 == 0, INF, rng.uniform(0.0, 8.0, len(vols))).astype(np.float32)):
        cut = _both(w, vols, max_d, ALL, no_ground, "built scene, largest distances")
        keep = free["distance"] <= np.broadcast_to(np.asarray(max_d, np.float32), (len(vols),))
        assert (cut["entity"] != MISS).tolist() == keep.tolist() and cut[keep].tobytes() == free[keep].tobytes()
    assert n_big == 6
    w.close()


# ---- 4. against the float64 brute force
def test_built_scene_matches_the_brute_force(mi_lib):
    sc, _, _ = built_scene()
    w = Q.world(mi_lib, sc)
    cols = S.scene_convex(sc, *S.initial_entity_poses(sc))
    boxes = [S.bounds(c[2]) for c in cols]
    cand = np.concatenate([R.make_volumes(11, 6, (-1, 0.3, -1), (8, 4, 10), 0.1, 0.8), R.make_volumes(12, 5, (8, 0.5, 8), (24, 6, 24), 0.2, 1.5),
                           R.make_volumes(13, 3, (-16, 1, -4), (-8, 6, 14), 0.1, 0.5)])
    picked, refs = [], []
    for j, v in enumerate(cand):   # the reference, culled by the gaps of the world AABBs (lower bounds of the gaps): the colliders in that order until the bound passes the best
        vc = S.volume_convex(v, sc.hulls)
        vmn, vmx = S.bounds(vc)
        lower = [float(np.linalg.norm(np.maximum(0.0, np.maximum(mn - vmx, vmn - mx)))) for mn, mx in boxes]
        gaps = {}
        best = np.inf
        for k in np.argsort(lower):
            if lower[k] > best + 0.01:
                break
            gaps[int(k)] = S.gap(vc, cols[k][2])
            best = min(best, gaps[int(k)])
        if best > 0.05 and len(picked) < 48:   # (clear of everything: overlaps are the matrix's and the scene test's)
            picked.append(j); refs.append((vc, gaps, best))
    assert len(picked) == 48
    vols = cand[picked]
    got = _both(w, vols, None, ALL, None, "brute force")
    worst = 0.0
    for i, (rec, (vc, gaps, best)) in enumerate(zip(got, refs)):
        k = int(rec["collider"])
        scale = max(1.0, max(np.abs(b).max() for s in (vc, cols[k][2]) for b in S.bounds(s)))
        bound = SCENE_BOUND * scale
        assert rec["entity"] == cols[k][0] and rec["object_type"] == cols[k][1] and rec["flags"] == 0, (i, rec)
        assert k in gaps and gaps[k] <= best + 2.0 * bound, (i, rec, best, gaps.get(k))
        worst = max(worst, abs(float(rec["distance"]) - gaps[k]) / scale)
        assert abs(float(rec["distance"]) - gaps[k]) <= bound, (i, rec, gaps[k])
        m = _measures(rec, vc, cols[k][2])
        assert max(m[:4]) <= bound and m[4] <= 1e-5, (i, rec, m)
    print(f"brute force: 48 volumes, largest |distance - reference| per unit of scale {worst:.2e}")
    w.close()


# ---- 5. filters and invalid input
def test_filters_and_invalid_input(mi_lib):
    from d3d12renderer_amd import capi, scenes
    sc = R.query_scene("zones")
    w = Q.world(mi_lib, sc)
    rng = np.random.default_rng(33)
    vols = R.make_volumes(21, 4, (-6, 0.5, -6), (6, 7, 6), 0.15, 1.0)
    n = len(vols)
    everything = _both(w, vols, None, ALL, None, "zones")
    seen = set()
    for include in (RIGID, STATIC, TRIGGERS, FIELDS, TERRAIN, 0, RIGID | TRIGGERS):
        m = _both(w, vols, None, include, None, f"zones include {include}")
        flags = np.array([RIGID, STATIC, FIELDS, TRIGGERS])[m["object_type"]]   # (object types 0 to 3: rigid body, static, force field, trigger)
        assert ((flags & include) != 0)[m["entity"] != MISS].all(), include
        seen |= set(int(t) for t in m["object_type"][m["entity"] != MISS])
        if include in (0, TERRAIN):   # nothing selected; the terrain is accepted and ignored
            assert (m["entity"] == MISS).all()
        else:
            assert (m["entity"] != MISS).all(), include
        assert (m["distance"] >= everything["distance"]).all()
    assert seen == {0, 1, 2, 3}
    # entity ranges: empty, one entity, all
    n_ent = len(sc.entities)
    one = rng.integers(0, n_ent, n).astype(np.uint32)
    assert (_both(w, vols, None, ALL, np.stack([one, one], axis=1), "empty ranges")["entity"] == MISS).all()
    single = _both(w, vols, None, ALL, np.stack([one, one + 1], axis=1), "one entity")
    assert (single["entity"] == one).all() and (single["distance"] >= everything["distance"]).all()
    _bytes_equal(_both(w, vols, None, ALL, np.tile(np.array([(0, MISS)], np.uint32), (n, 1)), "all entities"), everything, "the full range")
    # largest distances that are no distances; every kind of invalid volume
    odd = np.array([np.nan, -1.0, -0.0, -np.inf] * (n // 4), np.float32)
    m = _both(w, vols, odd, ALL, None, "NaN and negative largest distances")
    zero = np.arange(n) % 4 == 2   # (-0 is 0: valid)
    assert (m["entity"][~zero] == MISS).all() and (m[zero]["entity"] != MISS).tolist() == (everything["distance"][zero] == 0).tolist()
    edge, n_bad = Q.edge_volumes(rng, (-6, -1, -6), (6, 7, 6), True, (1, 1, 1), 1, 1)
    m = _both(w, edge, None, ALL, None, "invalid volumes")
    assert (m["entity"][-n_bad:] == MISS).all() and (m["entity"][:-n_bad] != MISS).all()
    assert len(w.distance(np.zeros(0, capi.query_volume_dtype))) == 0 and len(w.debug_distance_exhaustive(np.zeros(0, capi.query_volume_dtype), np.zeros(0, np.float32))) == 0
    w.close()
    # a world with a heightmap: the terrain bit changes nothing
    sc = scenes.terrain_field()
    w = Q.world(mi_lib, sc, 10)
    vols = np.concatenate([capi.sphere_volume(p, 0.3) for p in rng.uniform((-15, 0, -15), (15, 8, 15), (21, 3))])
    _bytes_equal(_both(w, vols, None, ALL, None, "terrain_field with the terrain bit"), _both(w, vols, None, ALL & ~TERRAIN, None, "terrain_field without"), "the terrain bit")
    assert (_both(w, vols, None, TERRAIN, None, "terrain alone")["entity"] == MISS).all()
    w.close()
    # an empty world
    w = mi_lib.create_world(0)
    assert (_both(w, vols, None, ALL, None, "empty world")["entity"] == MISS).all()
    w.close()


def test_errors(mi_lib):
    import ctypes as C
    from d3d12renderer_amd import capi, scenes, sharding
    sc = scenes.shape_zoo(2, 1, 2)
    w = Q.world(mi_lib, sc)
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    u = C.c_uint32
    vol = capi.sphere_volume((0, 5, 0), 0.2); d = np.array([100.0], np.float32); out = np.zeros(1, capi.distance_hit_dtype)
    for name in ("world_distance", "debug_distance_exhaustive"):
        f = w.L.fn(name)
        assert f(None, u(1), p(vol), p(d), u(ALL), None, p(out)) == -1
        assert f(w.h, u(1), None, p(d), u(ALL), None, p(out)) == -1
        assert f(w.h, u(1), p(vol), p(d), u(ALL), None, None) == -1
        assert f(w.h, u(0), None, None, u(ALL), None, None) == 0
        assert f(w.h, u(1), p(vol), None, u(ALL), None, p(out)) == 0 and out["entity"][0] != MISS
    dv = w.L.fn("world_distance_device_async")
    assert dv(w.h, u(1), None, None, u(ALL), None, None) == -1 and dv(None, u(0), None, None, u(ALL), None, None) == -1
    assert dv(w.h, u(0), None, None, u(ALL), None, None) == 0
    w.close()
    w = Q.world(mi_lib, sc)
    w.shard_enable(sharding._desc_for(sharding.tile_grid(sc, 1), 0))
    for name in ("world_distance", "debug_distance_exhaustive"):
        assert w.L.fn(name)(w.h, u(1), p(vol), p(d), u(ALL), None, p(out)) == -6
    w.close()


# ---- 6. device variant
def test_device_variant_equals_host_variant(mi_lib):
    import torch
    sc = R.query_scene("shape_zoo")
    vols = R.make_volumes(41, 7, (-5, 0.5, -5), (5, 9, 5), 0.15, 1.0)
    w = Q.world(mi_lib, sc, 5)
    n = len(vols)
    rng = np.random.default_rng(5)
    max_d = rng.uniform(0.0, 3.0, n).astype(np.float32); max_d[::5] = np.inf
    vols_d = torch.tensor(np.frombuffer(vols.tobytes(), np.uint8).copy(), device="cuda")
    max_dev = torch.tensor(max_d, device="cuda")
    out_d = torch.zeros(n * 64, dtype=torch.uint8, device="cuda")
    lo_e = rng.integers(0, len(sc.entities), n).astype(np.uint32)
    ranges = np.stack([lo_e, lo_e + 80], axis=1).astype(np.uint32)
    ranges_d = torch.tensor(ranges.view(np.int32), device="cuda")
    torch.cuda.synchronize()
    previous = None
    for _ in range(2):
        w.step_fixed(sc.settings(), sc.dt, 1)
        w.distance_device_async(n, vols_d.data_ptr(), out_d.data_ptr(), include=ALL)   # right behind the step, only enqueued on the world's stream
        host = w.distance(vols, None, ALL)                                              # (synchronises that stream)
        dev = out_d.cpu().numpy().tobytes()
        assert dev == host.tobytes()
        assert previous is None or dev != previous
        previous = dev
        w.distance_device_async(n, vols_d.data_ptr(), out_d.data_ptr(), max_distances_ptr=max_dev.data_ptr(), include=ALL)
        host = w.distance(vols, max_d, ALL)
        assert out_d.cpu().numpy().tobytes() == host.tobytes() and (host["entity"] == MISS).any() and (host["entity"] != MISS).any()
        w.distance_device_async(n, vols_d.data_ptr(), out_d.data_ptr(), max_distances_ptr=max_dev.data_ptr(), include=RIGID, ranges_ptr=ranges_d.data_ptr())
        host = w.distance(vols, max_d, RIGID, ranges)
        assert out_d.cpu().numpy().tobytes() == host.tobytes()
        w.step_fixed(sc.settings(), sc.dt, 20)
    w.close()


# ---- 7. read-only, and the cache
def test_queries_change_nothing_and_follow_the_poses(mi_lib):
    from d3d12renderer_amd import capi
    sc = R.query_scene("shape_zoo")
    vols = R.make_volumes(51, 4, (-5, 0.5, -5), (5, 9, 5), 0.15, 1.0)
    a = Q.world(mi_lib, sc); b = Q.world(mi_lib, sc)
    s = sc.settings()
    ents = Q.bodies(sc)
    previous = None
    for i in range(30):
        a.step_fixed(s, sc.dt, 1); b.step_fixed(s, sc.dt, 1)
        if i % 5 == 0:
            got = _both(b, vols, None, ALL, None, f"step {i}")
            assert previous is None or got.tobytes() != previous   # the queries see the moved poses
            previous = got.tobytes()
        else:
            b.distance(vols, 2.0, ALL)
    assert a.get_body_states(ents).tobytes() == b.get_body_states(ents).tobytes()
    assert a.debug_step_ahead_stats() == b.debug_step_ahead_stats()
    a.close()
    # a body-state write and a checkpoint load are seen
    probe = capi.sphere_volume((40.0, 3.0, -35.0), 0.3)
    before = _both(b, probe, None, RIGID, None, "before the write")
    blob = b.save_checkpoint()
    body = int(ents[3])
    st = b.get_body_states([body]); st[0, :3] = (40.0, 4.5, -35.0); b.set_body_states([body], st)   # far from the grid the last query built
    after = _both(b, probe, None, RIGID, None, "after the write")
    assert after["entity"][0] == body and after["distance"][0] < 2.0 and before["entity"][0] != MISS and before["distance"][0] > 20.0
    b.load_checkpoint(blob)
    _bytes_equal(_both(b, probe, None, RIGID, None, "after the checkpoint load"), before, "the checkpoint's poses")
    b.close()
