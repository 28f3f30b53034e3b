"""Shape-cast scene queries on the GPU (mi_world_sweep, mi_world_sweep_device_async, mi_debug_sweep_exhaustive): a closed-form table, the
float64 yardstick of tests/sweep_ref.py on its cast set, the ray cast (zero-radius spheres; the Minkowski identity), the accelerated
kernel against the exhaustive one byte for byte, the filters, initial overlaps, the device variant, that casts change nothing a step
computes while following every step, and the pair-level matrix of tests/sweep_matrix.py (every volume type against every collider type)."""
import numpy as np
import pytest

import overlap_ref as R
import query_helpers as Q
import sweep_matrix as M
import sweep_ref as S

pytestmark = pytest.mark.gpu

RIGID, STATIC, TRIGGERS, ALL = 1, 2, 8, 31
MISS = 0xFFFFFFFF
INITIAL_OVERLAP, UNCONVERGED = 1, 2
# The bound on |t_gpu - t_ref| * |d|, on the distance of `point` from the collider and on the normal's separation, in world units: 4 x the
# largest value measured on the GPU against the float64 reference in cases 1-2 (6.24e-5: |dt| * |d| of a cylinder cast in the cast set; the
# closed-form table 1.04e-5; points stay within 6e-7; case 3 compares with the float32 ray cast, 1.70e-4 between the two), rounded up to one digit.  The factor covers compiler versions and seeds, not the algorithm.
# The pair-level matrix (case 9) measures PER UNIT OF SCALE (scale = max(1, the largest |coordinate| of the cast)); the largest of |dt| |d|, the point's
# distance and the separation's shortfall per family: generic 1.90e-6, aligned 1.61e-6, grazing 4.87e-6 (all under this BOUND x scale, scale up to 7);
# far (coordinates of 1e2 and 1e3) 1.23e-5, size ratio (1e-2 against 20 to 200 units) 1.66e-6 (KNOWN_UNCONVERGED apart; the 1e-2 volumes on the trimmed
# 200-unit boxes within 4.4e-7), displacement length (1e-3 to 1e4) 1.99e-6: their bounds in sweep_matrix.BOUNDS are 4 x these, rounded up to one digit.
# Points stay within 1e-7 scale of the collider in every family.
BOUND = 3e-4


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


def _bytes_equal(a, b, what):
    if a.tobytes() != b.tobytes():
        bad = [i for i in range(len(a)) if a[i].tobytes() != b[i].tobytes()]
        raise AssertionError(f"{what}: {len(bad)} of {len(a)} records differ; first {bad[:4]}: {a[bad[:2]]} vs {b[bad[:2]]}")


def _accel_equals_exhaustive(w, vols, disp, include, ranges=None, what=""):
    a = w.sweep(vols, disp, include, ranges)
    _bytes_equal(a, w.debug_sweep_exhaustive(vols, disp, include, ranges), what)
    assert np.array_equal(a["volume"], np.arange(len(vols), dtype=np.uint32)), what
    miss = a["entity"] == MISS
    assert (a["collider"][miss] == MISS).all() and np.isinf(a["t"][miss]).all() and (a["object_type"][miss] == 0).all() and (a["flags"][miss] == 0).all(), what
    assert (a["point"][miss] == 0).all() and (a["normal"][miss] == 0).all(), what
    assert ((a["t"][~miss] >= 0) & (a["t"][~miss] <= 1)).all(), what
    return a


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
    sc = scenes.Scene("sweep_table", e, np.arange(6, dtype=np.uint32), c, 10, hulls=[R.volume_hull()])
    return sc, Q.world(mi_lib, sc)


def test_closed_form_table(mi_lib):
    from d3d12renderer_amd import capi, scenes
    sc, w = _table_world(mi_lib)
    lowest = float(sc.hulls[0][0][:, 1].min())
    h2, h3 = 0.5 * np.sqrt(2.0), 0.5 * np.sqrt(3.0)
    # the rotation that takes the cube's diagonal (1, 1, 1) / sqrt(3) onto +x: about (0, 1, -1) / sqrt(2) by acos(1 / sqrt(3))
    vertex_first = scenes.q_axis_angle(_unit((0, 1, -1)), np.arccos(1 / np.sqrt(3)))
    u = R.qmat(sc.entities["rotation"][5])[:, 0]   # the rotated box's own x axis
    off = np.sqrt(0.75 ** 2 - 0.3 ** 2)
    cases = [   # (volume, displacement, entity hit or None, t, normal or None)
        (capi.sphere_volume((-5, 0, 0), 0.25), (8, 0, 0), 0, 4.25 / 8, (-1, 0, 0)),                                    # sphere -> sphere
        (capi.sphere_volume((-5, 0.3, 0), 0.25), (8, 0, 0), 0, (5 - off) / 8, _unit((-off, 0.3, 0))),
        (capi.sphere_volume((-5, 0, 0), 0.0), (8, 0, 0), 0, 4.5 / 8, (-1, 0, 0)),                                       # a ray
        (capi.capsule_volume((5, 0, 0), (6, 0, 0), 0.2), (5, 0, 0), 1, 2.8 / 5, (-1, 0, 0)),                             # capsule end-on -> box face
        (capi.capsule_volume((5, -0.5, 0), (5, 0.5, 0), 0.2), (5, 0, 0), 1, 3.8 / 5, (-1, 0, 0)),                        # capsule side -> box face
        (capi.box_volume((5, 0.2, 0.1), (0.5, 0.5, 0.5)), (6, 0, 0), 1, 3.5 / 6, (-1, 0, 0)),                            # box -> box along an axis: gap / |d|
        (capi.box_volume((10, 5, 0), (0.5, 0.5, 0.5)), (0, -6, 0), 1, 3.5 / 6, (0, 1, 0)),
        (capi.cylinder_volume((5, -0.5, 0), (5, 0.5, 0), 0.3), (5, 0, 0), 1, 3.7 / 5, (-1, 0, 0)),                       # cylinder side -> box face
        (capi.cylinder_volume((10, 3, 0), (10, 4, 0), 0.3), (0, -4, 0), 1, 2.0 / 4, (0, 1, 0)),                          # cylinder cap -> box top
        (capi.box_volume((5, 0, 0), (0.5, 0.5, 0.5), rotation=scenes.q_axis_angle((0, 0, 1), np.pi / 4)), (6, 0, 0), 1, (4 - h2) / 6, (-1, 0, 0)),   # turned 45 degrees: edge first
        (capi.box_volume((5, 0, 0), (0.5, 0.5, 0.5), rotation=vertex_first), (6, 0, 0), 1, (4 - h3) / 6, (-1, 0, 0)),    # vertex first into the face
        (capi.hull_volume(0, position=(10, 6, 0)), (0, -8, 0), 1, (5 + lowest) / 8, (0, 1, 0)),                          # hull -> box: its lowest vertex
        (capi.box_volume((20, -5, 0), (3, 0.5, 3)), (0, 8, 0), 4, (lowest + 4.5) / 8, (0, -1, 0)),                       # box -> hull from below
        (capi.sphere_volume((-5, 0.5, 10), 0.25), (8, 0, 0), 2, 4.45 / 8, (-1, 0, 0)),                                   # sphere -> capsule side
        (capi.sphere_volume((0, 5, 10), 0.25), (0, -6, 0), 2, 3.45 / 6, (0, 1, 0)),                                      # sphere -> capsule end
        (capi.sphere_volume((-5, 0.5, 20), 0.25), (8, 0, 0), 3, 4.35 / 8, (-1, 0, 0)),                                   # sphere -> cylinder side
        (capi.sphere_volume((0.1, 5, 20), 0.25), (0, -6, 0), 3, 3.75 / 6, (0, 1, 0)),                                    # sphere -> cylinder cap
        (capi.sphere_volume(np.array((0, 0, -10)) - 5 * u, 0.25), 8 * u, 5, 3.75 / 8, -u),                               # sphere -> rotated box, along its axis
        (capi.sphere_volume((-5, 0, 0), 0.25), (4.249, 0, 0), None, None, None),                                         # stops just short
        (capi.sphere_volume((-5, 0, 0), 0.25), (4.251, 0, 0), 0, 4.25 / 4.251, (-1, 0, 0)),                              # just reaches
        (capi.sphere_volume((-5, 0, 0), 0.25), (-8, 0, 0), None, None, None),                                            # moves away
        (capi.sphere_volume((-1.5, 0, 0), 1.0), (1, 0, 0), 0, 0.0, None),                                                # starts touching
    ]
    vols = np.concatenate([c[0] for c in cases]); disp = np.array([c[1] for c in cases], np.float32)
    got = _accel_equals_exhaustive(w, vols, disp, ALL, what="table")
    worst_t = worst_n = 0.0
    for i, (_, d, ent, t, n) in enumerate(cases):
        rec = got[i]
        if ent is None:
            assert rec["entity"] == MISS, (i, rec)
            continue
        assert rec["entity"] == ent and rec["object_type"] == 1 and not rec["flags"] & UNCONVERGED, (i, rec)
        dt = abs(float(rec["t"]) - t) * np.linalg.norm(d)
        worst_t = max(worst_t, dt)
        assert dt <= BOUND, (i, rec, t)
        if n is not None:
            assert not rec["flags"] & INITIAL_OVERLAP, (i, rec)
            dn = float(np.linalg.norm(rec["normal"].astype(np.float64) - n))
            worst_n = max(worst_n, dn)
            assert dn <= BOUND and abs(np.linalg.norm(rec["normal"].astype(np.float64)) - 1) <= 1e-5, (i, rec, n)
        elif rec["flags"] & INITIAL_OVERLAP:
            assert rec["t"] == 0 and np.allclose(rec["normal"], -_unit(d), atol=1e-6) and (rec["point"] == vols["position"][i]).all(), (i, rec)   # (the pose position, not the shape's centre)
    print(f"closed-form table: largest |dt| * |d| {worst_t:.2e}, largest normal error {worst_n:.2e}")
    w.close()


# ---- 2. against the float64 reference
@pytest.mark.parametrize("seed", [909, 911])
def test_cast_set_matches_the_reference(mi_lib, seed):
    ref = S.cast_set_reference(seed)
    sc, vols, disp = ref["scene"], ref["volumes"], ref["displacements"]
    w = Q.world(mi_lib, sc)
    got = _accel_equals_exhaustive(w, vols, disp, ALL, what=f"cast set {seed}")
    shapes = [c[2] for c in ref["colliders"]]
    worst = {}
    for i, (rec, hit) in enumerate(zip(got, ref["hits"])):
        d = disp[i].astype(np.float64)
        assert not rec["flags"] & UNCONVERGED, (i, rec)
        assert (rec["entity"] == MISS) == (hit is None), (i, rec, hit)
        if hit is None:
            continue
        k, t, n_ref, p_ref, initial = hit
        assert rec["collider"] == k and rec["entity"] == ref["colliders"][k][0] and rec["object_type"] == ref["colliders"][k][1] and rec["flags"] == 0, (i, rec, hit)
        n = rec["normal"].astype(np.float64)
        dt = abs(float(rec["t"]) - t) * np.linalg.norm(d)
        dp = abs(S.point_gap(rec["point"], shapes[k]))
        separated = S.gap(S.moved(ref["convex"][i], float(rec["t"]) * d + 0.05 * n), shapes[k])
        m = worst.setdefault(int(vols["type"][i]), [0.0, 0.0, 0.0, 0.0])
        m[0] = max(m[0], dt); m[1] = max(m[1], dp); m[2] = max(m[2], 0.05 - separated); m[3] = max(m[3], float(np.linalg.norm(n - n_ref)))
        assert dt <= BOUND, (i, rec, t)
        assert dp <= BOUND, (i, rec, dp)
        assert abs(np.linalg.norm(n) - 1) <= 1e-5 and n @ d < 0, (i, rec)
        assert separated >= 0.05 - BOUND, (i, rec, separated)
    for vt, m in sorted(worst.items()):
        print(f"seed {seed} volume type {vt}: largest |dt| * |d| {m[0]:.2e}, point off the collider {m[1]:.2e}, separation short by {m[2]:.2e}, normal vs reference {m[3]:.2e}")
    w.close()


# ---- 3. against the ray cast
def test_zero_radius_spheres_are_rays(mi_lib):
    from d3d12renderer_amd import capi
    worst = 0.0
    for seed in (909, 911):
        ref = S.cast_set_reference(seed)
        sc, disp = ref["scene"], ref["displacements"]
        origins = ref["volumes"]["position"]
        w = Q.world(mi_lib, sc)
        vols = np.concatenate([capi.sphere_volume(o, 0.0) for o in origins])
        got = _accel_equals_exhaustive(w, vols, disp, ALL, what="rays")
        rays = w.raycast(origins, disp, max_t=1.0, include=ALL)
        assert (got["entity"] != MISS).sum() >= 0.5 * len(vols)
        for i in range(len(vols)):
            assert got["collider"][i] == rays["collider"][i] and got["entity"][i] == rays["entity"][i], (i, got[i], rays[i])
            if got["entity"][i] != MISS:
                dt = abs(float(got["t"][i]) - float(rays["t"][i])) * float(np.linalg.norm(disp[i]))
                worst = max(worst, dt)
                assert dt <= BOUND and not got["flags"][i], (i, got[i], rays[i])
        w.close()
    print(f"zero-radius spheres vs rays: largest |dt| * |d| {worst:.2e}")


def _round_world(mi_lib, grow):
    """Static spheres and capsules in a box about the origin, radii `grow` larger than the base set's."""
    from d3d12renderer_amd import capi, scenes
    rng = np.random.default_rng(55)
    n = 48
    e = scenes.make_entities(n, capi.ENTITY_STATIC)
    e["position"] = rng.uniform(-4, 4, (n, 3))
    e["rotation"] = scenes.random_unit_quaternions(3, 7, n)
    c = scenes.make_colliders(n, capi.SPHERE)
    for i in range(n):
        if i % 2:
            c["type"][i] = capi.CAPSULE; c["shape"][i, :7] = (0, -0.5, 0, 0, 0.5, 0, rng.uniform(0.1, 0.4) + grow)
        else:
            c["shape"][i, :4] = (0, 0, 0, rng.uniform(0.1, 0.5) + grow)
    sc = scenes.Scene("sweep_round", e, np.arange(n, dtype=np.uint32), c, 10)
    return Q.world(mi_lib, sc)


def test_minkowski_identity_with_the_ray_cast(mi_lib):
    """A sphere of radius 0.3 swept through spheres and capsules = a ray through the same shapes with radii 0.3 larger."""
    from d3d12renderer_amd import capi
    rng = np.random.default_rng(56)
    n = 64
    start = 12.0 * np.array([_unit(v) for v in rng.normal(size=(n, 3))])
    disp = (1.2 * (rng.uniform(-3, 3, (n, 3)) - start)).astype(np.float32)
    start = start.astype(np.float32)
    w, grown = _round_world(mi_lib, 0.0), _round_world(mi_lib, 0.3)
    got = _accel_equals_exhaustive(w, np.concatenate([capi.sphere_volume(o, 0.3) for o in start]), disp, ALL, what="round world")
    rays = grown.raycast(start, disp, max_t=1.0, include=ALL)
    assert (got["entity"] != MISS).sum() >= n // 2
    worst = 0.0
    for i in range(n):
        assert got["collider"][i] == rays["collider"][i], (i, got[i], rays[i])
        if got["entity"][i] != MISS:
            dt = abs(float(got["t"][i]) - float(rays["t"][i])) * float(np.linalg.norm(disp[i]))
            worst = max(worst, dt)
            assert dt <= BOUND and not got["flags"][i], (i, got[i], rays[i])
            assert np.linalg.norm(got["normal"][i] - rays["normal"][i]) <= 1e-3, (i, got[i], rays[i])   # (the same outward normal, up to where on the surface each t lands)
    print(f"Minkowski identity: largest |dt| * |d| {worst:.2e}")
    w.close(); grown.close()


# ---- 4. accelerated equals exhaustive
def _edge_casts(rng, lo, hi, hull_ok):
    """67 casts and more: inside the grid, starting or ending outside it, wholly outside, over more cells than the walk takes (the stride
    over all colliders), zero and non-finite displacements, every invalid volume.  Returns (volumes, displacements)."""
    lo = np.asarray(lo, float); hi = np.asarray(hi, float); span = hi - lo
    vols, n_bad = Q.edge_volumes(rng, lo, hi, hull_ok, (6, 2, 1), 4, 2)   # (x 6 types each)
    n = len(vols)
    disp = rng.normal(size=(n, 3)) * rng.uniform(0.1, 0.4, (n, 1)) * span.max()
    disp[0:6] = rng.normal(size=(6, 3)) * 3.0 * span.max()      # ends far outside; the swept box covers the whole grid: more than kOvMaxCells cells
    disp[6:10] = 0.0                                            # zero displacement
    disp[10] = (np.nan, 0, 0); disp[11] = (0, np.inf, 0); disp[12] = (3e38, 3e38, 3e38)   # non-finite; and a finite one near the largest float (valid: only the bytes are compared)
    disp[13:16] = (0.0, -1.0, 0.0) * np.array([[2.0], [6.0], [40.0]])   # straight down, onto whatever lies below (the ground box of the large list)
    return vols, disp.astype(np.float32), n_bad


def test_accelerated_equals_exhaustive(mi_lib):
    rng = np.random.default_rng(21)
    # shape_zoo, settled a little; count = 67: not a multiple of the casts per workgroup
    sc = R.query_scene("shape_zoo")
    w = Q.world(mi_lib, sc, 30)
    vols, disp, n_bad = _edge_casts(rng, (-7, -1, -7), (7, 8, 7), True)
    assert len(vols) >= 67
    for count in (67, len(vols)):
        sel = np.r_[0:count - n_bad, len(vols) - n_bad:len(vols)] if count < len(vols) else np.arange(len(vols))
        got = _accel_equals_exhaustive(w, vols[sel], disp[sel], ALL, what=f"shape_zoo {count}")
        assert len(got) == count and (got["entity"][-n_bad:] == MISS).all(), "an invalid volume hit something"
        assert (got["entity"][10:12] == MISS).all(), "a non-finite displacement hit something"
        assert (got["entity"] == MISS).any() and (got["entity"] != MISS).sum() > count // 4
    ground = len(sc.entities) - 1
    assert (got["entity"] == ground).any(), "no cast reached the ground box (the large list)"
    zero = got[6:10]
    assert ((zero["entity"] == MISS) | ((zero["flags"] & INITIAL_OVERLAP) != 0)).all()
    w.close()
    # zones: every object type, include = 31 and entity ranges
    sc = R.query_scene("zones")
    w = Q.world(mi_lib, sc, 30)
    vols, disp, n_bad = _edge_casts(rng, (-6, -1, -6), (6, 7, 6), True)
    vols, disp = vols[:67], disp[:67]
    got = _accel_equals_exhaustive(w, vols, disp, ALL, what="zones")
    assert {0, 1}.issubset(set(int(t) for t in got["object_type"][got["entity"] != MISS]))
    n_ent = len(sc.entities)
    lo_e = rng.integers(0, n_ent, len(vols)).astype(np.uint32)
    ranges = np.stack([lo_e, np.minimum(lo_e + rng.integers(1, n_ent // 2, len(vols)), n_ent)], axis=1).astype(np.uint32)
    ranges[::5] = (0, 0xFFFFFFFF)
    rg = _accel_equals_exhaustive(w, vols, disp, ALL, ranges, what="zones ranges")
    hit = rg["entity"] != MISS
    assert hit.any() and ((rg["entity"][hit] >= ranges[hit, 0]) & (rg["entity"][hit] < ranges[hit, 1])).all()
    for include in (0, 1, 2, 4, 8, 16, 9, 30):
        m = _accel_equals_exhaustive(w, vols, disp, include, what=f"zones include {include}")
        flags = np.array([1, 2, 16, 8])[m["object_type"][m["entity"] != MISS]]
        assert ((flags & include) != 0).all(), include
        if include in (0, 4):   # nothing selected; the terrain is accepted and ignored
            assert (m["entity"] == MISS).all()
    w.close()
    # the dense cluster: many entries per cell, long rows
    from d3d12renderer_amd import capi
    sc = Q.dense_cluster()
    w = Q.world(mi_lib, sc)
    n = 67
    start = rng.uniform((-2, 0, -2), (3, 2.5, 3), (n, 3))
    vols = np.concatenate([capi.sphere_volume(p, 0.05) if i % 3 == 0 else capi.box_volume(p, (0.04, 0.08, 0.06)) if i % 3 == 1 else capi.capsule_volume(p, p + (0, 0.1, 0), 0.03)
                           for i, p in enumerate(start)])
    disp = (rng.uniform((0, 0.5, 0), (1, 1.5, 1), (n, 3)) - start).astype(np.float32) * 1.5
    disp[:4] = (30.0, 0.0, 0.0)   # across the ring of bodies: the whole grid
    got = _accel_equals_exhaustive(w, vols, disp, ALL, what="dense cluster")
    assert (got["entity"] != MISS).sum() > n // 2
    w.close()


# ---- 5. filters
def test_filters(mi_lib):
    from d3d12renderer_amd import capi
    sc = R.query_scene("zones")
    w = Q.world(mi_lib, sc)
    kinds = sc.entities["kind"]
    # straight down through the trigger volumes from above the lattice
    rng = np.random.default_rng(3)
    n = 96
    start = np.stack([rng.uniform(-3.5, 3.5, n), np.full(n, 9.0), rng.uniform(-3.5, 3.5, n)], axis=1)
    vols = np.concatenate([capi.sphere_volume(p, 0.1) for p in start])
    disp = np.tile(np.array([0.0, -12.0, 0.0], np.float32), (n, 1))
    with_triggers, without = RIGID | STATIC | TRIGGERS, RIGID | STATIC   # (the force fields stay out: two of them enclose the triggers)
    everything = _accel_equals_exhaustive(w, vols, disp, with_triggers, what="filters with triggers")
    solid = _accel_equals_exhaustive(w, vols, disp, without, what="filters without triggers")
    only = _accel_equals_exhaustive(w, vols, disp, TRIGGERS, what="filters triggers only")
    assert (everything["entity"] != MISS).all()   # (the ground is below everything)
    assert (solid["object_type"] != 3).all() and (only["object_type"][only["entity"] != MISS] == 3).all()
    first_is_trigger = everything["object_type"] == 3
    assert first_is_trigger.sum() >= 3, "no cast meets a trigger first"
    for i in np.flatnonzero(first_is_trigger):
        assert kinds[everything["entity"][i]] == capi.ENTITY_TRIGGER and only[i].tobytes() == everything[i].tobytes()
        assert solid["t"][i] >= everything["t"][i] and solid["entity"][i] != everything["entity"][i]   # the body (or ground) behind it
    for i in np.flatnonzero(~first_is_trigger):
        assert solid[i].tobytes() == everything[i].tobytes()
    # an entity range that excludes the winner yields the runner-up: the better of the casts over the entities below and above it
    win = solid["entity"]
    below = w.sweep(vols, disp, without, np.stack([np.zeros(n, np.uint32), win], axis=1).astype(np.uint32))
    above = w.sweep(vols, disp, without, np.stack([win + 1, np.full(n, 0xFFFFFFFF, np.uint32)], axis=1).astype(np.uint32))
    assert (below["entity"] != win).all() and (above["entity"] != win).all()
    runner_t = np.minimum(below["t"], above["t"])
    assert (runner_t >= solid["t"]).all() and np.isfinite(runner_t).sum() > n // 4   # (a cast that went down to the ground has nothing behind it)
    # ... and is the reference's answer without that entity's colliders (a few casts)
    cols = S.scene_convex(sc, *S.initial_entity_poses(sc))
    for i in np.flatnonzero(np.isfinite(runner_t))[:8]:
        shapes = [c[2] if c[0] != win[i] and c[1] != 3 and c[1] != 2 else None for c in cols]
        hit = S.cast(S.volume_convex(vols[i], sc.hulls), disp[i], shapes)
        best = below[i] if below["t"][i] <= above["t"][i] else above[i]
        assert hit is not None and hit[0] == best["collider"] and abs(hit[1] - float(best["t"])) * 12.0 <= BOUND, (i, hit, best)
    w.close()


# ---- 6. initial overlap
def test_initial_overlap(mi_lib):
    from d3d12renderer_amd import capi
    sc = R.query_scene("shape_zoo")
    w = Q.world(mi_lib, sc)
    shapes = R.scene_world_shapes(sc, *S.initial_entity_poses(sc))
    rng = np.random.default_rng(8)
    vols, disp, expect = [], [], []
    for k, (ent, obj, ws) in enumerate(shapes):   # spheres sunk into colliders with a closed-form gap: sphere, capsule, box
        if ws[0] not in (R.SPHERE, R.CAPSULE, R.OBB) or len(vols) >= 40:
            continue
        centre = ws[1][0] if ws[0] != R.CAPSULE else (ws[1][0] + ws[1][1]) / 2
        p = (centre + rng.uniform(-0.1, 0.1, 3)).astype(np.float32)
        v = capi.make_volume(capi.SPHERE, [0, 0, 0, 0.2], position=p)
        gaps = [R.signed_gap(R.volume_world_shape(v[0]), s[2]) for s in shapes]
        if not gaps[k] < -0.05:
            continue
        vols.append(v); disp.append(rng.normal(size=3) * 2.0)
        expect.append(min(j for j, g in enumerate(gaps) if g is not None and g < -0.05))
    assert len(vols) >= 20
    vols = np.concatenate(vols); disp = np.array(disp, np.float32)
    got = _accel_equals_exhaustive(w, vols, disp, ALL, what="initial overlap")
    for i, rec in enumerate(got):
        assert rec["t"] == 0 and rec["flags"] == INITIAL_OVERLAP and rec["collider"] <= expect[i], (i, rec, expect[i])   # (the lowest index among all it overlaps)
        assert np.allclose(rec["normal"], -_unit(disp[i]), atol=1e-6) and (rec["point"] == vols["position"][i]).all(), (i, rec)
    # a zero displacement: the overlap still shows (normal 0), and a volume more than 0.05 clear of everything misses
    still = _accel_equals_exhaustive(w, vols, np.zeros_like(disp), ALL, what="zero displacement, overlapping")
    assert (still["t"] == 0).all() and (still["flags"] == INITIAL_OVERLAP).all() and (still["normal"] == 0).all() and (still["collider"] == got["collider"]).all()
    clear = np.concatenate([capi.sphere_volume(p, 0.2) for p in rng.uniform((-4, 9, -4), (4, 12, 4), (8, 3))])
    for v in clear:
        assert all(g is None or g > 0.05 for g in (R.signed_gap(R.volume_world_shape(v), s[2]) for s in shapes))
    assert (_accel_equals_exhaustive(w, clear, np.zeros((8, 3), np.float32), ALL, what="zero displacement, clear")["entity"] == MISS).all()
    w.close()


# ---- 7. device variant
def test_device_variant_equals_host_variant(mi_lib):
    import torch
    ref = S.cast_set_reference(909)
    sc, vols, disp = ref["scene"], ref["volumes"], ref["displacements"]
    w = Q.world(mi_lib, sc, 5)
    n = len(vols)
    vols_d = torch.tensor(np.frombuffer(vols.tobytes(), np.uint8).copy(), device="cuda")
    disp4 = np.zeros((n, 4), np.float32); disp4[:, :3] = disp; disp4[:, 3] = np.nan   # (w is ignored)
    disp_d = torch.tensor(disp4, device="cuda")
    out_d = torch.zeros(n * 48, dtype=torch.uint8, device="cuda")
    rng = np.random.default_rng(4)
    lo_e = rng.integers(0, len(sc.entities), n).astype(np.uint32)
    ranges = np.stack([lo_e, lo_e + 80], axis=1).astype(np.uint32)
    ranges_d = torch.tensor(ranges.view(np.int32), device="cuda")
    torch.cuda.synchronize()
    previous = None
    for _ in range(2):
        w.step_fixed(sc.settings(), sc.dt, 1)
        w.sweep_device_async(n, vols_d.data_ptr(), disp_d.data_ptr(), out_d.data_ptr(), include=ALL)   # right behind the step, only enqueued
        host = w.sweep(vols, disp, ALL)                                                                  # (synchronises that stream)
        dev = out_d.cpu().numpy().tobytes()
        assert dev == host.tobytes()
        assert previous is None or dev != previous
        previous = dev
        w.sweep_device_async(n, vols_d.data_ptr(), disp_d.data_ptr(), out_d.data_ptr(), include=RIGID, ranges_ptr=ranges_d.data_ptr())
        host = w.sweep(vols, disp, RIGID, ranges)
        assert out_d.cpu().numpy().tobytes() == host.tobytes()
        w.step_fixed(sc.settings(), sc.dt, 20)
    w.close()


# ---- 8. read-only, and the cache
def test_casts_change_nothing_and_follow_the_steps(mi_lib):
    ref = S.cast_set_reference(911)
    sc, vols, disp = ref["scene"], ref["volumes"], ref["displacements"]
    a = Q.world(mi_lib, sc); b = Q.world(mi_lib, sc)
    s = sc.settings()
    ents = Q.bodies(sc)
    previous = None
    for i in range(40):
        a.step_fixed(s, sc.dt, 1); b.step_fixed(s, sc.dt, 1)
        if i % 4 == 0:
            got = _accel_equals_exhaustive(b, vols, disp, ALL, what=f"step {i}")
            assert previous is None or got.tobytes() != previous   # the casts see the moved poses
            previous = got.tobytes()
        else:
            b.sweep(vols, disp, ALL)
    assert a.get_body_states(ents).tobytes() == b.get_body_states(ents).tobytes()
    assert a.debug_step_ahead_stats() == b.debug_step_ahead_stats()
    a.close(); b.close()


# ---- 9. the pair-level matrix: every volume type against every collider type, one collider at a time (tests/sweep_matrix.py)
def _matrix_casts(mi_lib, cases, what):
    """One world per family, one static entity with one collider per case; cast i is aimed at entity i alone.  The batch is made odd (never
    a multiple of the casts per workgroup) by a repeat of the first cast."""
    w = Q.world(mi_lib, M.scene_of(cases, what))
    pick = list(range(len(cases))) + ([0] if len(cases) % 2 == 0 else [])
    vols = np.concatenate([cases[i]["volume"] for i in pick]); disp = np.stack([cases[i]["disp"] for i in pick])
    ranges = np.array([(i, i + 1) for i in pick], np.uint32)
    got = _accel_equals_exhaustive(w, vols, disp, ALL, ranges, what=what)
    assert got[len(cases):].tobytes()[:44] == got[:1].tobytes()[:44] or len(pick) == len(cases)   # (the repeat: the same record but for its cast index)
    return w, vols, disp, ranges, got


def _who(name, i, c):
    return f"{name}[{i}] {M.TYPES[c['vt']]} -> {M.TYPES[c['ct']]} {c['tag']} (scale {c['scale']:.3g})"


# The one place of the matrix where the pair test ends unconverged, and not avoidably so in float32: a box of 1e-2 on the curved side of a
# cylinder of radius 15 and length 50 (size_ratio, tiny0 and tiny1).  The search stalls on a thin triangle of points of the side that lie
# about 0.5 apart: 2.5e-3 (tiny1: 42 tolerances; t |d| 3.4e-3 = 1.13e-4 scale before the reference's) and 5.1e-4 (tiny0: 8 tolerances, t |d|
# 9.9e-4 = 3.28e-5 scale before it; within the 16 tolerances at which a stalled search counts as converged, so without the flag) short of the touch.
# These may carry the flag and do not set the family's bound.  The documented contract is
# asserted for them: the reference hits too, t does not pass the reference's time by more than the family's bound, and it lies before it by no
# more than the value here (per unit of scale: 4 x the measured figure, rounded up to one digit); point, normal and separation as for every case.
KNOWN_UNCONVERGED = {("size_ratio", R.AABB, R.CYLINDER, "tiny0"): 2e-4, ("size_ratio", R.AABB, R.CYLINDER, "tiny1"): 5e-4}


def _check_against_reference(name, cases, got):
    """Every record against the reference's hit of its case, all measures per unit of the case's scale; returns the failures and prints the
    worst values per volume type: |dt| |d|, how far t |d| lies past the reference's, the point off the collider, the separation short of
    0.05 scale after backing off along the normal, and for round pairs |n - n_ref| x the smaller radius."""
    bad, worst = [], {}
    for i, c in enumerate(cases):
        rec, hit, who = got[i], c["ref"], _who(name, i, c)
        bound = M.BOUNDS[name] * c["scale"]
        if (rec["entity"] == MISS) != (hit is None):
            bad.append(f"{who}: decision: GPU {'misses' if rec['entity'] == MISS else 'hits at t = %.6g, flags %d' % (rec['t'], rec['flags'])}, "
                       f"the reference {'misses' if hit is None else 'hits at t = %.6g' % hit[0]}")
            continue
        if hit is None:
            continue
        if rec["entity"] != i or rec["object_type"] != 1:
            bad.append(f"{who}: entity {rec['entity']}, object type {rec['object_type']}")
        early = KNOWN_UNCONVERGED.get((name, c["vt"], c["ct"], c["tag"]))
        if int(rec["flags"]) & ~(UNCONVERGED if early is not None else 0):
            bad.append(f"{who}: flags {rec['flags']} (t = {rec['t']:.6g}, the reference {hit[0]:.6g})")
        t, n_ref = hit[0], hit[1]
        length = float(np.linalg.norm(c["d"]))
        n = rec["normal"].astype(np.float64)
        past = (float(rec["t"]) - t) * length
        m = worst.setdefault(c["vt"], [0.0] * 5)
        m[1] = max(m[1], past / c["scale"])
        if early is None:
            m[0] = max(m[0], abs(past) / c["scale"])
        else:
            print(f"{who}: known unconverged case, flags {rec['flags']}, t |d| {-past:.3e} = {-past / c['scale']:.3e} scale before the reference's (allowed {early:.0e} scale)")
        if past > bound:
            bad.append(f"{who}: t passes the reference's time of impact by {past:.3e} > {bound:.3e}")
        elif -past > (bound if early is None else early * c["scale"]):
            bad.append(f"{who}: |dt| |d| = {abs(past):.3e} > {bound if early is None else early * c['scale']:.3e}")
        if rec["flags"] & INITIAL_OVERLAP:
            continue
        dp = abs(S.point_gap(rec["point"], c["cconv"]))
        short = 0.05 * c["scale"] - S.gap(S.moved(c["vconv"], float(rec["t"]) * c["d"] + 0.05 * c["scale"] * n), c["cconv"])
        m[2] = max(m[2], dp / c["scale"]); m[3] = max(m[3], short / c["scale"])
        if dp > bound:
            bad.append(f"{who}: the point lies {dp:.3e} > {bound:.3e} off the collider")
        if abs(np.linalg.norm(n) - 1) > 1e-5 or n @ c["d"] > 0:
            bad.append(f"{who}: normal {n}, |n| - 1 = {np.linalg.norm(n) - 1:.2e}, n.d = {n @ c['d']:.3e}")
        if short > bound:
            bad.append(f"{who}: backed off by 0.05 scale along the normal the volume is {short:.3e} > {bound:.3e} short of 0.05 scale clear")
        if c["vt"] <= R.CAPSULE and c["ct"] <= R.CAPSULE and min(S.margin(c["vconv"]), S.margin(c["cconv"])) > 0:   # round pairs: the normal is exact
            radius = min(S.margin(c["vconv"]), S.margin(c["cconv"]))
            dn = float(np.linalg.norm(n - n_ref)) * radius
            m[4] = max(m[4], dn / c["scale"])
            if dn > bound:
                bad.append(f"{who}: |n - n_ref| = {dn / radius:.3e} > {bound:.3e} / the smaller radius {radius:.3g}")
    for vt, m in sorted(worst.items()):
        print(f"{name}, {M.TYPES[vt]} volumes, per unit of scale: largest |dt| |d| {m[0]:.2e}, t |d| past the reference {m[1]:.2e}, point off the collider {m[2]:.2e}, "
              f"separation short by {m[3]:.2e}, round normals x radius {m[4]:.2e}")
    if worst:
        print(f"{name}: the largest measure per unit of scale {max(max(m) for m in worst.values()):.2e} (bound {M.BOUNDS[name]:.0e})")
    return bad


assert M.UNIT_BOUND == BOUND


@pytest.mark.parametrize("name", M.BASE_FAMILIES + M.DERIVED_FAMILIES)
def test_matrix_family(mi_lib, name):
    """All 36 (volume type, collider type) pairs of one family against the float64 reference: the decision in every case (the CPU filter has
    removed the ambiguous ones; none is left out here), t within the family's bound x scale and never past the reference's by more, the point
    on the collider, the normal unit, against the motion and separating, the flags 0 (no unconverged hit in the matrix but KNOWN_UNCONVERGED); the derived
    families as tests/sweep_matrix.py states them.  Every failure of the family is reported, after the worst values."""
    cases = M.kept(name)
    assert set((c["vt"], c["ct"]) for c in cases) == set(M.PAIRS) or name == "zero_radius"
    w, vols, disp, ranges, got = _matrix_casts(mi_lib, cases, f"matrix {name}")
    bad = []
    if name in M.BASE_FAMILIES:
        bad = _check_against_reference(name, cases, got)
    elif name == "zero_radius":
        bad = _check_against_reference(name, cases, got)
        rays = w.raycast(vols["position"], disp, max_t=1.0, include=ALL, entity_ranges=ranges)
        worst = 0.0
        for i, c in enumerate(cases):
            if rays["entity"][i] != got["entity"][i]:
                bad.append(f"{_who(name, i, c)}: the ray cast reports entity {rays['entity'][i]}, the sweep {got['entity'][i]}")
            elif got["entity"][i] != MISS:
                dt = abs(float(got["t"][i]) - float(rays["t"][i])) * float(np.linalg.norm(c["d"]))
                worst = max(worst, dt / c["scale"])
                if dt > M.BOUNDS[name] * c["scale"]:
                    bad.append(f"{_who(name, i, c)}: |t - t of the ray cast| |d| = {dt:.3e}")
        print(f"{name}: largest |dt| |d| against the ray cast per unit of scale {worst:.2e}")
    else:
        worst = 0.0
        for i, c in enumerate(cases):
            rec, who, bound = got[i], _who(name, i, c), M.BOUNDS[name] * c["scale"]
            length = float(np.linalg.norm(c["d"]))
            if c["expect"] is None:
                if rec["entity"] != MISS:
                    bad.append(f"{who}: ends delta short of the touch but hits at t = {rec['t']:.6g}, flags {rec['flags']}")
                continue
            if rec["entity"] != i:
                bad.append(f"{who}: a miss; expected t = {c['expect']:.6g}")
                continue
            if name.endswith("starts_just_inside"):
                if not (rec["t"] == 0 and rec["flags"] == INITIAL_OVERLAP and np.allclose(rec["normal"], -_unit(c["d"]), atol=1e-6) and (rec["point"] == vols["position"][i]).all()):
                    bad.append(f"{who}: starts delta = {M.delta(c['base']):.3e} past the touch: t = {rec['t']:.6g}, flags {rec['flags']}, normal {rec['normal']}, point {rec['point']}")
                continue
            dt = (float(rec["t"]) - c["expect"]) * length
            worst = max(worst, abs(dt) / c["scale"])
            if rec["flags"] != 0 or abs(dt) > bound:
                bad.append(f"{who}: t |d| = {float(rec['t']) * length:.6e}, expected {c['expect'] * length:.6e} within {bound:.3e}; flags {rec['flags']}")
        print(f"{name}: {len(cases)} cases, largest |dt| |d| per unit of scale {worst:.2e}")
    w.close()
    assert not bad, f"{len(bad)} of {len(cases)} cases fail:\n" + "\n".join(bad)


# ---- 10. errors
def test_errors(mi_lib):
    import ctypes as C
    from d3d12renderer_amd import capi, scenes, sharding
    sc = scenes.shape_zoo(2, 1, 2)
    w = Q.world(mi_lib, sc)
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    u = C.c_uint32
    vol = capi.sphere_volume((0, 5, 0), 0.2); d = np.array([0, -10, 0], np.float32); out = np.zeros(1, capi.sweep_hit_dtype)
    for name in ("world_sweep", "debug_sweep_exhaustive"):
        f = w.L.fn(name)
        assert f(None, u(1), p(vol), p(d), u(ALL), None, p(out)) == -1
        assert f(w.h, u(1), None, p(d), u(ALL), None, p(out)) == -1
        assert f(w.h, u(1), p(vol), None, u(ALL), None, p(out)) == -1
        assert f(w.h, u(1), p(vol), p(d), u(ALL), None, None) == -1
        assert f(w.h, u(0), None, None, u(ALL), None, None) == 0
        assert f(w.h, u(1), p(vol), p(d), u(ALL), None, p(out)) == 0 and out["entity"][0] != MISS
    dv = w.L.fn("world_sweep_device_async")
    assert dv(w.h, u(1), None, None, u(ALL), None, None) == -1 and dv(None, u(0), None, None, u(ALL), None, None) == -1
    assert dv(w.h, u(0), None, None, u(ALL), None, None) == 0
    assert len(w.sweep(np.zeros(0, capi.query_volume_dtype), np.zeros((0, 3), np.float32))) == 0
    w.close()
    w = Q.world(mi_lib, sc)
    w.shard_enable(sharding._desc_for(sharding.tile_grid(sc, 1), 0))
    for name in ("world_sweep", "debug_sweep_exhaustive"):
        assert w.L.fn(name)(w.h, u(1), p(vol), p(d), u(ALL), None, p(out)) == -6
    w.close()
