"""Shape casts against the heightmap terrain on the GPU (mi_world_sweep, mi_world_sweep_device_async, mi_debug_sweep_exhaustive with
the terrain flag in the include mask): closed forms on a flat and a tilted map, the float64 yardstick of tests/sweep_terrain_ref.py on its comparison set, the
accelerated walk against the exhaustive kernel where the walk can go wrong, the composition with the colliders, the filters, the ray cast, the
device variant, heightmap edits, and that casts change nothing a step computes.  Every case also runs the exhaustive kernel and requires the
same bytes.

The bound (sweep_terrain_ref.BOUND = 6e-6, per unit of scale = max(1, the largest |coordinate| of the cast)) is 4 x the largest value measured on
the MI355X, rounded up to one digit.  Measured, per unit of scale:
  * the comparison set (48 casts on the rolling map, scales up to 32.2; every hit / miss decision equal, none left out, no record unconverged): the
    largest |t - t_ref| * |d| is 1.44e-6 (a cylinder; sphere 1.3e-8, capsule 8.4e-9, AABB 4.0e-8, OBB 1.0e-8, hull 1.5e-8), the point lies within
    3.1e-8 of the terrain, the separation of 0.05 along the normal is short by at most 1.2e-8; the normals lie within 2.2e-6 of the reference's
    (the cylinder: 4.8e-4, a rim on a slope);
  * the closed forms on the flat and the tilted map (scale 16): |t - t_closed| * |d| up to 4.3e-7; the normal of a sphere on the tilted plane up
    to 8.7e-3 off the plane's (see _normal_bound: up to 2 sqrt(tol / r) by construction);
  * zero-radius spheres against mi_world_raycast: 6.7e-8.
The collider sweeps' bound is 3e-4 (tests/test_gpu_sweep.py): the terrain needs a fiftieth of it."""
import numpy as np
import pytest

import overlap_ref as R
import query_helpers as Q
import sweep_ref as S
import sweep_terrain_ref as ST

pytestmark = pytest.mark.gpu

RIGID, STATIC, TERRAIN_BIT, ALL = 1, 2, 4, 31
MISS, TERRAIN = 0xFFFFFFFF, 0xFFFFFFFE
INITIAL_OVERLAP, UNCONVERGED = 1, 2
BOUND = ST.BOUND


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


def _normal_bound(radius):
    """How far the normal of a round volume may lie off a flat surface's: the pair test ends within its distance tolerance (2e-6 x the largest
    coordinate, 16 on the one-chunk maps) of touching, at a core-to-triangle distance of at most r + tol while the core is still r - tol above the
    plane, so the touch may be found up to sqrt((r + tol)^2 - (r - tol)^2) = 2 sqrt(r tol) beside the foot point (on a coplanar neighbour of the
    triangle under it): an angle of 2 sqrt(tol / r).  Boxes (no radius) touch flat on flat with the last support plane's normal, a direction the search
    resolves to its stall limit of 16 tolerances per unit of length: 16 x 2e-6."""
    return 16 * 2e-6 if radius is None else 2.0 * np.sqrt(2e-6 * 16.0 / radius)


def _bytes_equal(a, b, what):
    if a.tobytes() != b.tobytes():
        bad = [i for i in range(len(a)) if a[i].tobytes() != b[i].tobytes()]
        raise AssertionError(f"{what}: {len(bad)} of {len(a)} records differ; first {bad[:4]}: {a[bad[:2]]} vs {b[bad[:2]]}")


def _cast(w, vols, disp, include=TERRAIN_BIT, ranges=None, what=""):
    """The accelerated records, which are the exhaustive kernel's byte for byte and well-formed."""
    a = w.sweep(vols, disp, include, ranges)
    _bytes_equal(a, w.debug_sweep_exhaustive(vols, disp, include, ranges), what)
    assert np.array_equal(a["volume"], np.arange(len(a), dtype=np.uint32)), what
    miss = a["entity"] == MISS
    assert (a["collider"][miss] == MISS).all() and np.isinf(a["t"][miss]).all() and (a["object_type"][miss] == 0).all() and (a["flags"][miss] == 0).all(), what
    assert (a["point"][miss] == 0).all() and (a["normal"][miss] == 0).all(), what
    assert ((a["t"][~miss] >= 0) & (a["t"][~miss] <= 1)).all(), what
    ter = a["entity"] == TERRAIN
    assert (a["collider"][ter] == TERRAIN).all() and (a["object_type"][ter] == 1).all() and ((a["collider"] == TERRAIN) == ter).all(), what
    return a


# ---- 1. closed forms
def test_closed_forms_on_the_flat_and_the_tilted_map(mi_lib):
    from d3d12renderer_amd import capi
    H = ST.FLAT_Y
    w = Q.world(mi_lib, ST.scene("flat"))
    box = lambda c: capi.box_volume(c, (0.4, 0.3, 0.5))   # noqa: E731
    radii = [0.5, None, None, 0.4, 0.4, 0.5, None, 0.4, 0.5, 0.5]
    cases = [   # (volume, displacement, t or None for a miss, normal)
        (capi.sphere_volume((3.3, 5.0, 4.7), 0.5), (0.3, -4.0, 0.2), (4.5 - H) / 4, (0, 1, 0)),
        (box((6.1, 4.0, 9.2)), (0.0, -3.0, 0.0), (3.7 - H) / 3, (0, 1, 0)),
        (box((6.1, 4.0, 9.2)), (0.7, -3.0, -0.4), (3.7 - H) / 3, (0, 1, 0)),
        (capi.capsule_volume((8.0, 4.0, 8.0), (8.0, 5.0, 8.0), 0.4), (0.0, -3.0, 0.5), (3.6 - H) / 3, (0, 1, 0)),
        (capi.capsule_volume((7.5, 4.5, 8.0), (8.5, 4.5, 8.0), 0.4), (0.2, -3.0, 0.0), (4.1 - H) / 3, (0, 1, 0)),
        (capi.sphere_volume((3.3, -1.0, 4.7), 0.5), (0.3, 4.0, 0.2), (H + 0.5) / 4, (0, -1, 0)),          # wholly below, moving up: a hit from below
        (box((6.1, 0.0, 9.2)), (0.1, 3.0, 0.0), (H - 0.3) / 3, (0, -1, 0)),
        (capi.capsule_volume((8.0, -1.0, 8.0), (8.0, 0.0, 8.0), 0.4), (0.0, 3.0, 0.5), (H - 0.4) / 3, (0, -1, 0)),
        (capi.sphere_volume((3.3, 5.0, 4.7), 0.5), (0, -(4.5 - H) + 1e-3, 0), None, None),                  # stops just short
        (capi.sphere_volume((3.3, 5.0, 4.7), 0.5), (0, -(4.5 - H) - 1e-3, 0), (4.5 - H) / (4.5 - H + 1e-3), (0, 1, 0)),   # just reaches
        (capi.sphere_volume((3.3, 5.0, 4.7), 0.5), (0, 2, 0), None, None),                                  # moves away
        (capi.sphere_volume((3.3, 5.0, 4.7), 0.5), (3, 0, 1), None, None),                                  # level above
        (capi.sphere_volume((3.3, -1.0, 4.7), 0.5), (0, -1, 0), None, None),                                # wholly below, moving down
        (capi.sphere_volume((-3.0, 5.0, 4.7), 0.5), (0, -8, 0), None, None),                                # beside the map
    ]
    vols = np.concatenate([c[0] for c in cases]); disp = np.array([c[1] for c in cases], np.float32)
    got = _cast(w, vols, disp, what="flat map")
    assert (w.sweep(vols, disp, RIGID | STATIC)["entity"] == MISS).all()
    worst = worst_n = worst_flat = 0.0
    for i, (_, d, t, n) in enumerate(cases):
        rec = got[i]
        if t is None:
            assert rec["entity"] == MISS, (i, rec)
            continue
        assert rec["entity"] == TERRAIN and rec["collider"] == TERRAIN and rec["object_type"] == 1 and rec["flags"] == 0, (i, rec)
        dt = abs(float(rec["t"]) - t) * np.linalg.norm(d)
        worst = max(worst, dt / 16.0)
        assert dt <= BOUND * 16.0, (i, rec, t)
        dn = float(np.linalg.norm(rec["normal"].astype(np.float64) - n))
        worst_n = max(worst_n, dn); worst_flat = max(worst_flat, dn if radii[i] is None else 0.0)
        assert dn <= _normal_bound(radii[i]) and abs(np.linalg.norm(rec["normal"].astype(np.float64)) - 1) <= 1e-5 and abs(float(rec["point"][1]) - H) <= BOUND * 16.0, (i, rec)
    # resting in the plane: an initial overlap, whatever the direction
    rest = capi.sphere_volume((3.3, H + 0.2, 4.7), 0.5)
    for d in ((0, -1, 0), (1, 0.5, 0)):
        rec = _cast(w, rest, np.array([d], np.float32), what="resting")[0]
        assert rec["entity"] == TERRAIN and rec["t"] == 0 and rec["flags"] == INITIAL_OVERLAP and (rec["point"] == rest["position"][0]).all(), rec
        assert np.allclose(rec["normal"], -_unit(d), atol=1e-6), rec
    w.close()
    # the tilted plane y = slope * x: t = (n.c - r) / -(n.d)
    w = Q.world(mi_lib, ST.scene("tilted"))
    n = ST.TILT_NORMAL
    rng = np.random.default_rng(5)
    c = np.stack([rng.uniform(4, 12, 8), rng.uniform(6, 8, 8), rng.uniform(4, 12, 8)], axis=1).astype(np.float32)
    r = rng.uniform(0.1, 0.8, 8).astype(np.float32)
    disp = np.stack([rng.uniform(-1, 1, 8), np.full(8, -7.0), rng.uniform(-1, 1, 8)], axis=1).astype(np.float32)
    got = _cast(w, np.concatenate([capi.sphere_volume(ci, ri) for ci, ri in zip(c, r)]), disp, what="tilted map")
    for i, rec in enumerate(got):
        want = (n @ c[i].astype(np.float64) - float(r[i])) / -(n @ disp[i].astype(np.float64))
        dt = abs(float(rec["t"]) - want) * np.linalg.norm(disp[i])
        worst = max(worst, dt / 16.0)
        assert rec["entity"] == TERRAIN and rec["flags"] == 0 and dt <= BOUND * 16.0, (i, rec, want)
        dn = float(np.linalg.norm(rec["normal"].astype(np.float64) - n))
        worst_n = max(worst_n, dn)
        assert dn <= _normal_bound(float(r[i])) and abs(n @ rec["point"].astype(np.float64)) <= BOUND * 16.0, (i, rec, dn)
    print(f"closed forms: largest |dt| * |d| per unit of scale (16) {worst:.2e}, largest normal error {worst_n:.2e} (boxes {worst_flat:.2e})")
    w.close()


# ---- 2. against the float64 reference
def test_comparison_set_matches_the_reference(mi_lib):
    ref = ST.comparison_reference()
    vols, disp = ref["volumes"], ref["displacements"]
    w = Q.world(mi_lib, ref["scene"])
    got = _cast(w, vols, disp, what="comparison set")
    worst, bad = {}, []
    for i, (rec, hit) in enumerate(zip(got, ref["hits"])):
        d = disp[i].astype(np.float64); scale = ref["scales"][i]; bound = BOUND * scale
        assert not rec["flags"] & UNCONVERGED, (i, rec)
        assert (rec["entity"] == MISS) == (hit is None), (i, rec, hit)
        if hit is None:
            continue
        assert rec["entity"] == TERRAIN and rec["flags"] == 0, (i, rec)
        n = rec["normal"].astype(np.float64)
        dt = abs(float(rec["t"]) - hit[0]) * np.linalg.norm(d)
        dp = abs(ST.point_gap("rolling", rec["point"]))
        short = 0.05 - ST.separation("rolling", ref["convex"][i], float(rec["t"]) * d + 0.05 * n, n)
        m = worst.setdefault(int(vols["type"][i]), [0.0, 0.0, 0.0, 0.0])
        m[0] = max(m[0], dt / scale); m[1] = max(m[1], dp / scale); m[2] = max(m[2], short / scale); m[3] = max(m[3], float(np.linalg.norm(n - hit[1])))
        if dt > bound or dp > bound or short > bound or abs(np.linalg.norm(n) - 1) > 1e-5 or n @ d > 0:
            bad.append((i, rec, hit, dt, dp, short))
    for vt, m in sorted(worst.items()):
        print(f"volume type {vt}, per unit of scale: largest |dt| * |d| {m[0]:.2e}, point off the terrain {m[1]:.2e}, separation short by {m[2]:.2e}; normal vs reference {m[3]:.2e}")
    print(f"comparison set: the largest measure per unit of scale {max(max(m[:3]) for m in worst.values()):.2e} (bound {BOUND:.0e})")
    w.close()
    assert not bad, bad


# ---- 3. accelerated equals exhaustive where the walk can go wrong
def _walk_casts():
    """The rolling map: x, z in [-32, 32], cells of 0.25, blocks of 2, the chunk seams at x = 0 and z = 0, the hole x in [0, 32], z in [-32, 0], the
    hills between y = 0.48 and 3.12.  Returns (volumes, displacements, indices that must miss)."""
    from d3d12renderer_amd import capi
    sph = capi.sphere_volume
    cases = [
        (sph((-1.0, 4.0, 5.0), 0.3), (2.0, -3.8, 0.0)), (sph((5.0, 4.0, 1.0), 0.3), (0.5, -3.0, -1.5)),                  # across a chunk seam (x = 0; z = 0 into the hole's row)
        (capi.box_volume((-0.2, 3.5, 0.1), (0.5, 0.2, 0.5)), (0.3, -3.4, -0.3)),                                          # the corner where the four chunks meet
        (sph((3.5, 4.0, 5.0), 0.2), (1.0, -3.8, 0.0)), (sph((-6.1, 4.0, 9.9), 0.2), (0.3, -3.8, 0.3)),                   # across a block border (x = 4; x = -6, z = 10)
        (sph((4.25, 4.0, 3.0), 0.1), (0.0, -3.8, 6.0)), (sph((4.0, 2.5, 3.125), 0.0), (-9.0, -1.0, 0.0)),                # along a cell edge (x = 4.25; z = 3.125)
        (sph((0.0, 4.0, 3.0), 0.1), (0.0, -3.8, 6.0)), (sph((-12.0, 3.0, 0.0), 0.0), (9.0, -2.0, 0.0)),                  # along a chunk edge (x = 0; z = 0)
        (sph((-3.0, 2.6, -10.0), 0.3), (10.0, -1.5, 0.0)), (sph((10.0, 5.0, -10.0), 0.5), (0.0, -8.0, 0.0)),             # over the hole's rim into it; down the hole
        (sph((10.0, 1.5, -2.0), 0.3), (0.0, 0.0, 6.0)), (sph((3.0, 2.0, -20.0), 0.3), (-8.0, 0.0, 0.0)),                 # out of the hole into the hills (+z; -x)
        (sph((-36.0, 3.0, 5.0), 0.4), (8.0, -2.9, 0.0)), (sph((-30.0, 4.0, 5.0), 0.4), (-6.0, -12.0, 0.0)),               # from outside inwards; from inside outwards
        (sph((-40.0, 3.0, 5.0), 0.4), (0.0, -6.0, 0.0)), (sph((5.0, 3.0, 40.0), 0.4), (3.0, -6.0, 1.0)),                 # wholly outside
        (sph((5.1, 6.0, 7.3), 0.3), (0.0, -6.0, 0.0)), (capi.capsule_volume((-9.0, 6.0, -9.0), (-9.0, 7.0, -9.0), 0.4), (0.0, -7.0, 0.0)),   # vertical
        (sph((-20.0, 2.2, 10.0), 0.2), (15.0, 0.0, 0.0)), (sph((-5.0, 2.2, 10.0), 0.2), (-15.0, 0.0, 0.0)),              # along +x, -x
        (sph((-10.0, 2.2, 3.0), 0.2), (0.0, 0.0, 15.0)), (sph((-10.0, 2.2, 18.0), 0.2), (0.0, 0.0, -15.0)),              # along +z, -z
        (capi.capsule_volume((-31.0, 3.3, -31.0), (-31.0, 3.8, -31.0), 0.3), (62.0, -1.8, 62.0)),                         # the diagonal of the map: 32 block rows
        (sph((-31.0, 7.0, -31.0), 0.3), (62.0, 0.0, 62.0)), (sph((31.0, 3.4, 31.0), 0.3), (-62.0, -1.5, -60.0)),         # ... above every hill; ... backwards
        (capi.box_volume((8.0, 5.0, 8.0), (3.0, 0.2, 3.0)), (1.0, -4.5, 0.5)), (sph((-15.0, 6.0, 15.0), 2.5), (2.0, -5.0, 0.0)),   # wider than a block
        (sph((6.0, 2.0, 6.0), 1.6), (0.0, 0.0, 0.0)), (sph((6.0, 9.0, 6.0), 0.5), (0.0, 0.0, 0.0)),                      # zero displacement: touching, clear
        (sph((6.0, 6.0, 6.0), 0.5), (np.nan, -1.0, 0.0)), (sph((6.0, 6.0, 6.0), 0.5), (0.0, -np.inf, 0.0)),              # non-finite displacement
        (sph((6.0, 6.0, 6.0), -1.0), (0.0, -8.0, 0.0)), (capi.hull_volume(99, position=(6, 6, 6)), (0.0, -8.0, 0.0)),    # invalid volume
    ]
    # down the hole, wholly outside (2), above every hill, zero displacement and clear, non-finite (2), invalid (2)
    must_miss = [10, 15, 16, 24, 29, 30, 31, 32, 33]
    assert len(cases) == 34
    rng = np.random.default_rng(12)
    more = R.make_volumes(13, 6, (-30, 3.5, -30), (30, 6.0, 30), 0.15, 1.5)[:67 - len(cases)]
    vols = np.concatenate([c[0] for c in cases] + [more])
    disp = np.concatenate([np.array([c[1] for c in cases], np.float64), rng.uniform((-8, -8, -8), (8, -3, 8), (len(more), 3))]).astype(np.float32)
    return vols, disp, must_miss


def _cannot_miss(vols, disp, must_miss):
    """The casts that are no must_miss and cannot miss, by raycast_terrain_matrix.Map.height alone: the terrain is a continuous surface over solid
    cells, so a cast hits when a point of the volume passes from above the surface to below it on a stretch of its way that lies over
    solid cells throughout (400 samples; whatever the way does before or after, over the hole or outside the map), or when the volume touches the
    terrain at the pose it ends in (then it touched it at some t <= 1) or starts in."""
    import raycast_terrain_matrix as RT
    m = RT.the_map("rolling")
    hulls = ST.scene("rolling").hulls
    out = []
    for i in range(len(vols)):
        d = disp[i].astype(np.float64)
        if i in must_miss or not np.isfinite(d).all():
            continue
        conv = S.volume_convex(vols[i], hulls)
        mn, mx = S.bounds(conv)
        # points of the volume itself: the centre of its bounds (volumes are symmetric about it or contain it: hull 0 does) and its cores' lowest corners
        points = [(mn + mx) / 2] + [S.support(conv, np.array(u, np.float64)) for u in ((-1, -1, -1), (-1, -1, 1), (1, -1, -1), (1, -1, 1))]
        crossed = False
        for start in points:
            above = False
            for s in np.linspace(0.0, 1.0, 401):
                p = start + s * d
                over = m.x0 <= p[0] <= m.x0 + m.size and m.z0 <= p[2] <= m.z0 + m.size
                h = m.height(p[0], p[2]) if over else np.nan
                if not np.isfinite(h):
                    above = False                       # (off the solid cells: the stretch ends)
                elif p[1] > h:
                    above = True
                elif above and p[1] < h:
                    crossed = True
                    break
            if crossed:
                break
        if crossed or ST.min_gap("rolling", S.moved(conv, d), 1e-3) <= 0 or ST.min_gap("rolling", conv, 1e-3) <= 0:
            out.append(i)
    return out


def test_accelerated_equals_exhaustive_on_the_rolling_map(mi_lib):
    w = Q.world(mi_lib, ST.scene("rolling"))
    vols, disp, must_miss = _walk_casts()
    assert len(vols) == 67   # (a partial last workgroup)
    got = _cast(w, vols, disp, what="walk")
    assert (got["entity"][must_miss] == MISS).all(), got[must_miss]
    hit = got["entity"] == TERRAIN
    assert hit.sum() >= 20 and (hit | (got["entity"] == MISS)).all(), hit.sum()
    # what cannot miss, computed from the map; the casts the earlier version of this test listed by hand are among them
    required = _cannot_miss(vols, disp, must_miss)
    print("walk casts that cannot miss:", required)
    assert set(required) >= {0, 2, 3, 4, 5, 7, 13, 14, 17, 18, 26, 27, 28}, required
    assert hit[required].all(), np.flatnonzero(~hit)
    print("walk casts that hit:", np.flatnonzero(hit).tolist())
    assert got["flags"][28] == INITIAL_OVERLAP and (got["normal"][28] == 0).all() and got["t"][28] == 0
    assert (got["normal"][hit & (got["flags"] == 0)] * disp[hit & (got["flags"] == 0)]).sum(axis=1).max() <= 0
    one = _cast(w, vols[:1], disp[:1], what="one cast")
    assert one.tobytes() == got[:1].tobytes()
    w.close()


# ---- 4. composition with the colliders
def test_composition_with_the_colliders(mi_lib):
    from d3d12renderer_amd import scenes
    sc = scenes.terrain_field()
    sc.hulls = list(sc.hulls) or [R.volume_hull()]
    w = Q.world(mi_lib, sc, 30)
    rng = np.random.default_rng(17)
    vols = R.make_volumes(18, 32, (-9, 6, -9), (9, 9, 9), 0.1, 0.5)
    disp = rng.uniform((-3, -12, -3), (3, -9, 3), (len(vols), 3)).astype(np.float32)
    both = _cast(w, vols, disp, 7, what="include 7")
    cols = _cast(w, vols, disp, 3, what="include 3")
    ter = _cast(w, vols, disp, 4, what="include 4")
    assert (cols["entity"] != TERRAIN).all() and ((ter["entity"] == TERRAIN) | (ter["entity"] == MISS)).all()
    took_terrain = 0
    for i in range(len(vols)):
        want = ter[i] if ter["t"][i] < cols["t"][i] else cols[i]   # (a miss has t = inf; a collider wins a tie)
        assert both[i].tobytes() == want.tobytes(), (i, both[i], cols[i], ter[i])
        took_terrain += int(both["entity"][i] == TERRAIN)
    assert 1 <= took_terrain <= len(vols) - 1, took_terrain   # both occur
    w.close()


# ---- 5. filters
def test_filters(mi_lib):
    ref = ST.comparison_reference()
    vols, disp = ref["volumes"], ref["displacements"]
    n = len(vols)
    w = Q.world(mi_lib, ref["scene"])
    base = _cast(w, vols, disp, 4, what="include 4")
    assert (base["entity"] == TERRAIN).sum() >= n // 3
    for include in (7, 31):
        assert _cast(w, vols, disp, include, what=f"include {include}").tobytes() == base.tobytes()
    for include in (0, 3):
        assert (_cast(w, vols, disp, include, what=f"include {include}")["entity"] == MISS).all()
    whole = np.tile(np.array([0, 0xFFFFFFFF], np.uint32), (n, 1))
    below = np.tile(np.array([0, TERRAIN], np.uint32), (n, 1))
    only = np.tile(np.array([TERRAIN, 0xFFFFFFFF], np.uint32), (n, 1))
    mixed = np.where((np.arange(n) % 2 == 0)[:, None], whole, below).astype(np.uint32)
    assert _cast(w, vols, disp, 7, whole, what="whole range").tobytes() == base.tobytes()
    assert _cast(w, vols, disp, 7, only, what="the terrain alone").tobytes() == base.tobytes()
    assert (_cast(w, vols, disp, 7, below, what="range below the terrain")["entity"] == MISS).all()
    m = _cast(w, vols, disp, 7, mixed, what="mixed ranges")
    assert m[::2].tobytes() == base[::2].tobytes() and (m["entity"][1::2] == MISS).all()
    w.close()
    # a world without a heightmap: the bit changes nothing
    sc = R.query_scene("shape_zoo")
    w = Q.world(mi_lib, sc)
    cs = S.cast_set_reference(909)
    with_bit = _cast(w, cs["volumes"], cs["displacements"], 7, what="no heightmap, include 7")
    assert with_bit.tobytes() == _cast(w, cs["volumes"], cs["displacements"], 3, what="no heightmap, include 3").tobytes()
    assert (with_bit["entity"] != MISS).any() and (_cast(w, cs["volumes"], cs["displacements"], 4, what="no heightmap, include 4")["entity"] == MISS).all()
    w.close()


# ---- 6. the ray cast
def test_zero_radius_spheres_are_rays(mi_lib):
    from d3d12renderer_amd import capi
    ref = ST.comparison_reference()
    disp, origins = ref["displacements"], ref["volumes"]["position"]
    w = Q.world(mi_lib, ref["scene"])
    vols = np.concatenate([capi.sphere_volume(o, 0.0) for o in origins])
    got = _cast(w, vols, disp, 4, what="rays")
    rays = w.raycast(origins, disp, max_t=1.0, include=4)
    assert (got["entity"] == TERRAIN).sum() >= len(vols) // 3
    worst = 0.0
    for i in range(len(vols)):
        assert got["entity"][i] == rays["entity"][i] and got["collider"][i] == rays["collider"][i], (i, got[i], rays[i])
        if got["entity"][i] != MISS:
            dt = abs(float(got["t"][i]) - float(rays["t"][i])) * float(np.linalg.norm(disp[i])) / ref["scales"][i]
            worst = max(worst, dt)
            assert dt <= BOUND and not got["flags"][i], (i, got[i], rays[i])
    print(f"zero-radius spheres vs rays: largest |dt| * |d| per unit of scale {worst:.2e}")
    w.close()


# ---- 7. device variant
def test_device_variant_equals_host_variant(mi_lib):
    import torch
    ref = ST.comparison_reference()
    vols, disp = ref["volumes"], ref["displacements"]
    w = Q.world(mi_lib, ref["scene"])
    n = len(vols)
    vols_d = torch.tensor(np.frombuffer(vols.tobytes(), np.uint8).copy(), device="cuda")
    disp4 = np.zeros((n, 4), np.float32); disp4[:, :3] = disp; disp4[:, 3] = np.nan   # (w is ignored)
    disp_d = torch.tensor(disp4, device="cuda")
    out_d = torch.zeros(n * 48, dtype=torch.uint8, device="cuda")
    ranges = np.where((np.arange(n) % 3 == 0)[:, None], np.array([0, TERRAIN], np.uint32), np.array([5, 0xFFFFFFFF], np.uint32)).astype(np.uint32)
    ranges_d = torch.tensor(ranges.view(np.int32), device="cuda")
    torch.cuda.synchronize()
    w.sweep_device_async(n, vols_d.data_ptr(), disp_d.data_ptr(), out_d.data_ptr(), include=7)
    host = w.sweep(vols, disp, 7)   # (synchronises that stream)
    assert out_d.cpu().numpy().tobytes() == host.tobytes() and (host["entity"] == TERRAIN).any()
    w.sweep_device_async(n, vols_d.data_ptr(), disp_d.data_ptr(), out_d.data_ptr(), include=4, ranges_ptr=ranges_d.data_ptr())
    host = w.sweep(vols, disp, 4, ranges)
    assert out_d.cpu().numpy().tobytes() == host.tobytes() and (host["entity"][::3] == MISS).all() and (host["entity"] == TERRAIN).any()
    w.close()


# ---- 8. heightmap edits
def test_a_heightmap_edit_is_seen_by_the_next_cast(mi_lib):
    from d3d12renderer_amd import capi
    sc = ST.scene("rolling")
    hm = sc.heightmap
    w = Q.world(mi_lib, sc)
    vols = np.concatenate([capi.sphere_volume((-10.3, 9.0, 12.1), 0.4), capi.box_volume((7.7, 9.0, 9.4), (0.3, 0.2, 0.5))])
    disp = np.array([[0, -9, 0], [0, -9, 0]], np.float32)   # (straight down: raised by 1, the same column of terrain is met 1 earlier)
    before = _cast(w, vols, disp, what="before the edit")
    w.update_heightmap(np.asarray(hm["min_corner"], np.float32) + np.array([0, 1, 0], np.float32), hm["amplitude"])
    after = _cast(w, vols, disp, what="after the edit")
    assert (before["entity"] == TERRAIN).all() and (after["entity"] == TERRAIN).all()
    travelled = (before["t"].astype(np.float64) - after["t"]) * 9.0   # (the casts go 9 down)
    assert np.abs(travelled - 1.0).max() <= BOUND * 32, travelled
    assert np.abs(after["point"][:, 1].astype(np.float64) - before["point"][:, 1] - 1.0).max() <= BOUND * 32
    w.close()


# ---- 9. steps
def test_casts_change_nothing_a_step_computes(mi_lib):
    from d3d12renderer_amd import scenes
    sc = scenes.terrain_field()
    sc.hulls = list(sc.hulls) or [R.volume_hull()]
    a = Q.world(mi_lib, sc); b = Q.world(mi_lib, sc)
    s = sc.settings()
    ents = Q.bodies(sc)
    rng = np.random.default_rng(19)
    vols = R.make_volumes(20, 4, (-9, 6, -9), (9, 9, 9), 0.1, 0.5)
    disp = rng.uniform((-3, -12, -3), (3, -9, 3), (len(vols), 3)).astype(np.float32)
    previous = None
    for i in range(24):
        a.step_fixed(s, sc.dt, 1); b.step_fixed(s, sc.dt, 1)
        if i % 8 == 0:
            got = _cast(b, vols, disp, 7, what=f"step {i}")
            assert previous is None or got.tobytes() != previous   # the casts see the moved bodies
            previous = got.tobytes()
        else:
            b.sweep(vols, disp, 7)
    assert a.get_body_states(ents).tobytes() == b.get_body_states(ents).tobytes()
    a.close(); b.close()
