"""Terrain distance scene queries on the GPU (mi_world_terrain_distance, mi_world_terrain_distance_device_async,
mi_debug_terrain_distance_exhaustive), one record per volume and always through both kernels, byte for byte: closed forms on the flat and the
tilted map, the comparison set against the float64 reference of tests/terrain_distance_ref.py, the places where the ring walk can go wrong on the
wide map, merging with mi_world_distance on a scene with bodies, the device variant on torch tensors, and consistency with the shape cast, with
heightmap edits and with the step.

MEASURED on the MI355X against the float64 reference, per unit of scale = max(1, the largest |coordinate| of the volume's bounds grown by its
distance), on the comparison set (48 volumes, scales up to 46; every decision equal, none left out, no record unconverged).  Per volume type:
|distance - reference|, point_collider off the terrain, point_volume off the volume, ||pv - pc| - distance|, |pv - pc - distance n|:
  sphere   2.85e-8  1.32e-8  2.09e-8  2.84e-8  2.96e-8
  capsule  4.42e-8  3.56e-8  6.88e-8  2.44e-8  4.62e-8
  cylinder 1.41e-6  3.12e-8  4.32e-8  9.82e-9  3.72e-8
  AABB     3.21e-8  1.68e-8  3.23e-8  6.35e-9  2.32e-8
  OBB      1.77e-8  1.15e-8  6.48e-8  1.27e-8  3.52e-8
  hull     4.65e-8  7.27e-9  7.34e-8  1.27e-8  3.66e-8
The largest is the cylinder's distance, 1.41e-6 (the pair test stops within 2e-6 x the coordinates; a cylinder's curved side is the one support
that is not a vertex).  The closed forms of item 1 are met to 1.21e-8.  BOUND = 6e-6: 4 x 1.41e-6 = 5.64e-6, rounded up to one digit; it is also the
terrain casts' bound.  A sweep along -normal x (distance + 0.05) meets the terrain at t x length within 2.32e-6 of the distance (held to the sum
of the two bounds, 1.2e-5)."""
import numpy as np
import pytest

import overlap_ref as R
import query_helpers as Q
import sweep_ref as S
import sweep_terrain_ref as ST
import terrain_distance_ref as TD

pytestmark = pytest.mark.gpu

TERRAIN, MISS = TD.TERRAIN, TD.MISS
OVERLAP, UNCONVERGED = 1, 2
INF = np.float32(np.inf)
BOUND = TD.BOUND
TYPES = ("sphere", "capsule", "cylinder", "AABB", "OBB", "hull")


def _bytes_equal(a, b, what):
    if a.tobytes() != b.tobytes():
        bad = [i for i in range(len(a)) if a[i].tobytes() != b[i].tobytes()]
        raise AssertionError(f"{what}: {len(bad)} of {len(a)} records differ; first {bad[:4]}: {a[bad[:2]]} vs {b[bad[:2]]}")


def _both(w, vols, max_d=None, merge_into=None, what=""):
    """The accelerated records, equal byte for byte to the exhaustive ones; without merging, in the shape every record has."""
    a = w.terrain_distance(vols, max_d, merge_into)
    _bytes_equal(a, w.debug_terrain_distance_exhaustive(vols, max_d, merge_into), what)
    if merge_into is not None:
        return a
    assert np.array_equal(a["volume"], np.arange(len(a), dtype=np.uint32)) and (a["pad"] == 0).all(), what
    miss = a["entity"] == MISS
    assert (a["collider"][miss] == MISS).all() and np.isposinf(a["distance"][miss]).all() and (a["object_type"][miss] == 0).all() and (a["flags"][miss] == 0).all(), what
    assert (a["point_collider"][miss] == 0).all() and (a["point_volume"][miss] == 0).all() and (a["normal"][miss] == 0).all(), what
    hit = a[~miss]
    assert (hit["entity"] == TERRAIN).all() and (hit["collider"] == TERRAIN).all() and (hit["object_type"] == 1).all(), what
    assert (hit["distance"] >= 0).all() and np.isfinite(hit["distance"]).all(), what
    if max_d is not None:
        assert (hit["distance"] <= np.broadcast_to(np.asarray(max_d, np.float32), (len(a),))[~miss]).all(), what
    over = (hit["flags"] & OVERLAP) != 0
    pos = np.asarray(vols)["position"][~miss][over]
    assert ((hit["distance"] == 0) == over).all() and (hit["normal"][over] == 0).all(), what
    assert (hit["point_collider"][over] == pos).all() and (hit["point_volume"][over] == pos).all(), what
    return a


def _measures(rec, vconv, map_name):
    """Of a hit that is no overlap: point_collider off the terrain, point_volume off the volume, ||pv - pc| - distance|, |pv - pc - distance n|, ||n| - 1|."""
    pc, pv, n, d = rec["point_collider"].astype(np.float64), rec["point_volume"].astype(np.float64), rec["normal"].astype(np.float64), float(rec["distance"])
    return (abs(ST.point_gap(map_name, pc)), abs(S.point_gap(pv, vconv)), abs(np.linalg.norm(pv - pc) - d), float(np.linalg.norm(pv - pc - d * n)), abs(np.linalg.norm(n) - 1))


# ---- 1. closed forms
def test_closed_forms_on_the_flat_and_the_tilted_map(mi_lib):
    from d3d12renderer_amd import capi
    Y = ST.FLAT_Y
    w = Q.world(mi_lib, ST.scene("flat"))
    # (volume, height of its position, reach below / above the position, half-extent of the footprint about (x, z) in which point_collider may lie)
    shapes = lambda x, y, z: [(capi.sphere_volume((x, y, z), 0.5), 0.5, 0.0),                                                       # noqa: E731
                              (capi.box_volume((x, y, z), (0.4, 0.3, 0.6)), 0.3, 0.6),
                              (capi.capsule_volume((x, y - 0.5, z), (x, y + 0.5, z), 0.25), 0.75, 0.0),                             # upright
                              (capi.capsule_volume((x - 0.7, y, z), (x + 0.7, y, z), 0.25), 0.25, 0.7)]                             # lying
    cases = []
    for k, (x, z) in enumerate([(5.3, 6.1), (11.77, 2.45)]):
        for y, sign in ((Y + 2.0 + 0.37 * k, 1.0), (Y - 1.5 - 0.21 * k, -1.0)):      # above the plane, below it
            for vol, reach, foot in shapes(x, y, z):
                cases.append((vol, sign * (y - Y) - reach, (0.0, sign, 0.0), (x, z), foot))
    for y, r in ((Y + 1.0, 0.5), (Y - 2.0, 0.25), (Y, 0.3)):                          # beside the map at x = -3: the rim's edge x = 0
        cases.append((capi.sphere_volume((-3.0, y, 8.03), r), np.hypot(3.0, y - Y) - r, np.array((-3.0, y - Y, 0.0)) / np.hypot(3.0, y - Y), None, None))
    vols = np.concatenate([c[0] for c in cases])
    got = _both(w, vols, None, what="flat")
    worst = 0.0
    for i, (_, dist, n, at, foot) in enumerate(cases):
        rec = got[i]
        scale = TD.scale_of(S.volume_convex(vols[i], [R.volume_hull()]), dist)
        e = BOUND * scale
        assert rec["entity"] == TERRAIN and rec["flags"] == 0, (i, rec)
        err = abs(float(rec["distance"]) - dist)
        worst = max(worst, err / scale)
        assert err <= e, (i, rec, dist)
        # (a direction t off the true one lengthens the distance by dist t^2 / 2: e admits t = sqrt(2 e / dist))
        assert np.linalg.norm(rec["normal"].astype(np.float64) - n) <= np.sqrt(2 * e / dist) + 1e-6, (i, rec, n)
        pc, pv = rec["point_collider"].astype(np.float64), rec["point_volume"].astype(np.float64)
        assert np.linalg.norm(pv - pc - float(rec["distance"]) * rec["normal"].astype(np.float64)) <= e, (i, rec)
        if at is not None:   # point_collider in the plane, under the volume
            slack = np.sqrt(2 * dist * e + e * e) + e
            assert abs(pc[1] - Y) <= e and abs(pc[0] - at[0]) <= foot + slack and abs(pc[2] - at[1]) <= foot + slack, (i, rec)
        else:
            assert abs(pc[0]) <= e and abs(pc[1] - Y) <= e, (i, rec)
    # resting in the plane: the overlap record
    rest = np.concatenate([v for v, reach, _ in shapes(7.0, Y + 0.1, 9.0)] + [capi.sphere_volume((3.0, Y - 0.2, 3.0), 0.5)])
    got = _both(w, rest, None, what="resting in the plane")
    assert (got["flags"] == OVERLAP).all() and (got["distance"] == 0).all() and (got["entity"] == TERRAIN).all()
    # a largest distance just short and just enough
    vol, dist = cases[0][0], cases[0][1]
    d = 16 * BOUND * 8.0
    got = _both(w, np.concatenate([vol, vol, vol, vol]), np.array([dist - d, dist + d, 0.0, np.inf], np.float32), what="largest distances")
    assert got["entity"].tolist() == [MISS, TERRAIN, MISS, TERRAIN]
    assert got[1].tobytes()[:44] == got[3].tobytes()[:44] and got[1].tobytes()[48:] == got[3].tobytes()[48:]   # (all but the query's index)
    w.close()
    # spheres over and under the tilted plane y = TILT_SLOPE x: n . c - r
    w = Q.world(mi_lib, ST.scene("tilted"))
    n = ST.TILT_NORMAL
    centres = [(4.2, 3.0, 5.5), (9.9, 4.1, 12.3), (6.6, -1.0, 3.3), (12.0, 0.2, 8.0)]
    vols = np.concatenate([capi.sphere_volume(c, 0.35) for c in centres])
    got = _both(w, vols, None, what="tilted")
    for i, c in enumerate(centres):
        signed = float(n @ np.asarray(c))
        dist = abs(signed) - 0.35
        scale = TD.scale_of(S.volume_convex(vols[i], [R.volume_hull()]), dist)
        e = BOUND * scale
        err = abs(float(got["distance"][i]) - dist)
        worst = max(worst, err / scale)
        assert got["entity"][i] == TERRAIN and got["flags"][i] == 0 and err <= e, (i, got[i], dist)
        assert np.linalg.norm(got["normal"][i].astype(np.float64) - np.sign(signed) * n) <= np.sqrt(2 * e / dist) + 1e-6, (i, got[i])
    print(f"closed forms: largest |distance - closed form| per unit of scale {worst:.2e}")
    w.close()


# ---- 2. the comparison set
def test_comparison_set_matches_the_reference(mi_lib):
    c = TD.comparison_reference()
    w = Q.world(mi_lib, c["scene"])
    got = _both(w, c["volumes"], c["max_distances"], what="comparison set")
    bad, worst = [], {}
    for i, rec in enumerate(got):
        who = f"[{i}] {TYPES[i % 6]} {c['groups'][i]} (scale {c['scales'][i]:.3g}, reference {c['ref'][i]:.7g})"
        bound = BOUND * c["scales"][i]
        if c["expect"][i] == "miss":
            if rec["entity"] != MISS:
                bad.append(f"{who}: reports distance {rec['distance']:.7g} above the largest distance {c['max_distances'][i]:.7g}")
            continue
        if rec["entity"] != TERRAIN:
            bad.append(f"{who}: a miss")
            continue
        if c["expect"][i] == "overlap":
            if rec["flags"] != OVERLAP or rec["distance"] != 0:
                bad.append(f"{who}: cuts the surface but flags {rec['flags']}, distance {rec['distance']:.3e}")
            continue
        if rec["flags"] != 0:
            bad.append(f"{who}: flags {rec['flags']} (distance {rec['distance']:.7g})")
            continue
        m = (abs(float(rec["distance"]) - c["ref"][i]),) + _measures(rec, c["convex"][i], TD.MAP)
        row = worst.setdefault(i % 6, [0.0] * 5)
        for j in range(5):
            row[j] = max(row[j], m[j] / c["scales"][i])
        for j, label in enumerate(("the distance differs from the reference by", "point_collider lies off the terrain by", "point_volume lies off the volume by",
                                   "|point_volume - point_collider| differs from the distance by", "point_volume - point_collider differs from distance x normal by")):
            if m[j] > bound:
                bad.append(f"{who}: {label} {m[j]:.3e} > {bound:.3e}")
        if m[5] > 1e-5:
            bad.append(f"{who}: |normal| - 1 = {m[5]:.2e}")
        if c["groups"][i] == "below" and not rec["normal"][1] < 0:
            bad.append(f"{who}: below the surface but the normal {rec['normal']} does not point down")
    for t, row in sorted(worst.items()):
        print(f"{TYPES[t]} volumes, per unit of scale: |distance - reference| {row[0]:.2e}, point off the terrain {row[1]:.2e}, point off the volume {row[2]:.2e}, "
              f"||pv - pc| - distance| {row[3]:.2e}, |pv - pc - distance n| {row[4]:.2e}")
    if worst:
        print(f"comparison set: the largest measure per unit of scale {max(max(r) for r in worst.values()):.2e} (bound {BOUND:.0e})")
    assert not bad, f"{len(bad)} of {len(got)} volumes fail:\n" + "\n".join(bad)
    w.close()


# ---- 3. where the walk can go wrong: accelerated against exhaustive on the wide map
def test_the_walk_on_the_wide_map(mi_lib):
    """5 x 5 chunks of 8 m, cells of 1 / 16 m, x and z in [-20, 20]; only the middle row and the middle column have heights: a floor at 0.37 with bumps
    of 3 x 3 vertices up to 11 and 22 at the ends of the centre lines."""
    from d3d12renderer_amd import capi
    w = Q.world(mi_lib, ST.scene("wide"))
    floor = ST.WIDE_FLOOR * 24.0 / 65535.0
    near = ST.WIDE_NEAR * 24.0 / 65535.0
    bump_x = -20.0 + 17 * ST.WIDE_CELL          # the middle vertex of the near bump on the row's centre line
    vols = np.concatenate([
        capi.sphere_volume((12.0, 3.0, 12.0), 0.4), capi.box_volume((-12.3, 1.0, 11.6), (0.5, 0.2, 0.3)),                        # over a quadrant of holes, 16 blocks from the heights
        capi.sphere_volume((bump_x + 0.6, 6.0, 0.0), 0.2), capi.box_volume((bump_x - 0.55, 0.6 * near, 0.3), (0.1, 0.1, 0.1)),   # at mid height beside a bump: its flank, not the floor
        capi.sphere_volume((4.0, 1.0, 0.21), 0.3), capi.capsule_volume((-4.0, 1.2, -3.0), (-4.0, 1.2, 3.0), 0.2),                 # on a chunk seam (x = +-4), nearest triangle across it
        capi.sphere_volume((4.0 + 0.01, 2.0, 4.0 + 0.01), 0.5),                                                                    # over the corner where the hole quadrant begins
        capi.capsule_volume((-18.75, 2.0, 0.5), (18.75, 2.0, 0.5), 0.3), capi.box_volume((0.0, 1.5, 0.0), (0.2, 0.2, 18.75)),       # 600 cells long, along the row and the column
        capi.capsule_volume((-18.75, 9.0, 0.02), (18.75, 30.0, 0.02), 0.3),                                                       # 600 cells long and sloping: the near bump
        capi.sphere_volume((-23.0, 1.0, 0.3), 0.5), capi.sphere_volume((22.5, 4.0, -1.0), 0.5), capi.sphere_volume((0.7, 1.0, -24.0), 0.5),   # outside each of the four rims
        capi.box_volume((-1.1, 2.0, 21.5), (0.3, 0.3, 0.3)), capi.sphere_volume((23.0, 2.0, 22.0), 0.5), capi.sphere_volume((-26.0, -3.0, -27.0), 1.0),   # ... and beyond a corner (of holes)
        capi.hull_volume(0, position=(1.0, 5.0, -2.0)), capi.cylinder_volume((0.0, 3.0, 10.0), (0.5, 4.0, 10.0), 0.4)])
    cell = ST.WIDE_CELL
    free = _both(w, vols, None, what="wide map")
    assert (free["entity"] == TERRAIN).all()
    assert 7.5 < free["distance"][0] < 8.5                                    # the rim of the heights, 8 m off
    assert free["distance"][2] < 0.6 and free["distance"][3] < 1.0          # the bump's flank, not the floor 5 and 6 below
    assert floor < 0.4 and near > 10.0
    for max_d in (0.0, cell, 16 * cell, np.where(np.arange(len(vols)) % 2 == 0, INF, 1.0).astype(np.float32)):
        cut = _both(w, vols, max_d, what=f"wide map, largest distance {max_d}")
        keep = free["distance"] <= np.broadcast_to(np.asarray(max_d, np.float32), (len(vols),))
        assert (cut["entity"] != MISS).tolist() == keep.tolist() and cut[keep].tobytes() == free[keep].tobytes()
    w.close()


# ---- 4. merging
def _marked(records):
    m = records.copy()
    m["pad"] = 9
    return m


def test_merging_with_the_colliders(mi_lib):
    from d3d12renderer_amd import scenes
    sc = scenes.terrain_field()
    sc.hulls = list(sc.hulls) or [R.volume_hull()]
    w = Q.world(mi_lib, sc, 30)
    rng = np.random.default_rng(23)
    good = R.make_volumes(24, 8, (-9, 0.5, -9), (9, 8, 9), 0.1, 0.5)
    edge, n_bad = Q.edge_volumes(rng, (-9, 0, -9), (9, 8, 9), True, (1, 1, 1), 1, 1)
    vols = np.concatenate([good, edge])
    n = len(vols)
    took = kept = 0
    for max_d in (None, 1.0, np.where(np.arange(n) % 3 == 0, INF, rng.uniform(0.0, 3.0, n)).astype(np.float32)):
        cols = w.distance(vols, max_d, 31)
        ter = _both(w, vols, max_d, what="terrain alone")
        assert (cols["entity"] != TERRAIN).all() and (ter["entity"][-n_bad:] == MISS).all() and (cols["entity"][-n_bad:] == MISS).all()
        marked = cols.copy()
        marked["pad"] = 0x5EED5EED                                  # (what the terrain does not replace keeps its bytes)
        marked[-n_bad:] = np.frombuffer(bytes([0xAB]) * (64 * n_bad), marked.dtype)   # invalid volumes: whatever is there stays there
        merged = _both(w, vols, max_d, merge_into=marked, what="merged")
        for i in range(n):
            wins = i < n - n_bad and ter["distance"][i] < cols["distance"][i]   # (a miss has distance +inf; a collider wins a tie)
            want = ter[i] if wins else marked[i]
            assert merged[i].tobytes() == want.tobytes(), (i, merged[i], cols[i], ter[i])
            took += int(wins); kept += int(not wins and i < n - n_bad and cols["entity"][i] != MISS)
    assert took >= 3 and kept >= 3, (took, kept)   # both occur
    # a tie: the terrain's own record as the one to merge into stays (strictly nearer only)
    free = _marked(_both(w, vols, None, what="terrain alone, unbounded"))
    assert _both(w, vols, None, merge_into=free, what="a tie").tobytes() == free.tobytes() and (free["entity"] == TERRAIN).any()
    w.close()
    # a world without a heightmap: misses, and nothing written when merging
    sc = R.query_scene("shape_zoo")
    w = Q.world(mi_lib, sc)
    assert (_both(w, vols, None, what="no heightmap")["entity"] == MISS).all()
    cols = w.distance(vols, None, 31)
    cols["pad"] = 7
    assert _both(w, vols, None, merge_into=cols, what="no heightmap, merged").tobytes() == cols.tobytes() and (cols["entity"] != MISS).any()
    w.close()


def test_errors(mi_lib):
    import ctypes as C
    from d3d12renderer_amd import capi, sharding
    sc = ST.scene("flat")
    w = Q.world(mi_lib, sc)
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    u = C.c_uint32
    vol = capi.sphere_volume((5, 5, 5), 0.2); d = np.array([100.0], np.float32); out = np.zeros(1, capi.distance_hit_dtype)
    for name in ("world_terrain_distance", "debug_terrain_distance_exhaustive"):
        f = w.L.fn(name)
        assert f(None, u(1), p(vol), p(d), u(0), p(out)) == -1
        assert f(w.h, u(1), None, p(d), u(0), p(out)) == -1
        assert f(w.h, u(1), p(vol), p(d), u(0), None) == -1
        assert f(w.h, u(0), None, None, u(0), None) == 0
        assert f(w.h, u(1), p(vol), None, u(0), p(out)) == 0 and out["entity"][0] == TERRAIN
    dv = w.L.fn("world_terrain_distance_device_async")
    assert dv(w.h, u(1), None, None, u(0), None) == -1 and dv(None, u(0), None, None, u(0), None) == -1
    assert dv(w.h, u(0), None, None, u(0), None) == 0
    assert len(w.terrain_distance(np.zeros(0, capi.query_volume_dtype))) == 0
    # NaN and negative largest distances are misses; -0 is 0
    odd = _both(w, np.concatenate([vol] * 4), np.array([np.nan, -1.0, -0.0, -np.inf], np.float32), what="largest distances that are none")
    assert (odd["entity"] == MISS).all()
    w.close()
    from d3d12renderer_amd import scenes
    sc = scenes.terrain_field()
    w = Q.world(mi_lib, sc)
    w.shard_enable(sharding._desc_for(sharding.tile_grid(sc, 1), 0))
    for name in ("world_terrain_distance", "debug_terrain_distance_exhaustive"):
        assert w.L.fn(name)(w.h, u(1), p(vol), p(d), u(0), p(out)) == -6
    w.close()


# ---- 5. device variant
def test_device_variant_equals_host_variant(mi_lib):
    import torch
    from d3d12renderer_amd import scenes
    sc = scenes.terrain_field()
    sc.hulls = list(sc.hulls) or [R.volume_hull()]
    w = Q.world(mi_lib, sc, 30)
    vols = R.make_volumes(25, 7, (-9, 0.5, -9), (9, 8, 9), 0.1, 0.5)
    n = len(vols)
    rng = np.random.default_rng(26)
    max_d = rng.uniform(0.0, 3.0, n).astype(np.float32); max_d[::5] = np.inf
    vols_d = torch.tensor(np.frombuffer(vols.tobytes(), np.uint8).copy(), device="cuda")
    max_dev = torch.tensor(max_d, device="cuda")
    out_d = torch.full(((n + 1) * 64,), 0xCD, dtype=torch.uint8, device="cuda")   # one record more than asked for: it keeps its bytes
    torch.cuda.synchronize()
    guard = bytes([0xCD]) * 64
    for m_ptr, m in ((0, None), (max_dev.data_ptr(), max_d)):
        w.terrain_distance_device_async(n, vols_d.data_ptr(), out_d.data_ptr(), max_distances_ptr=m_ptr)   # only enqueued on the world's stream
        host = w.terrain_distance(vols, m)                                                                # (synchronises that stream)
        dev = out_d.cpu().numpy().tobytes()
        assert dev[:n * 64] == host.tobytes() and dev[n * 64:] == guard and (host["entity"] == TERRAIN).any()
        # the two-call pattern: the nearest of anything, no host work in between
        w.distance_device_async(n, vols_d.data_ptr(), out_d.data_ptr(), max_distances_ptr=m_ptr, include=31)
        w.terrain_distance_device_async(n, vols_d.data_ptr(), out_d.data_ptr(), max_distances_ptr=m_ptr, merge=1)
        host = w.terrain_distance(vols, m, merge_into=w.distance(vols, m, 31))
        dev = out_d.cpu().numpy().tobytes()
        assert dev[:n * 64] == host.tobytes() and dev[n * 64:] == guard
        assert (host["entity"] == TERRAIN).any() and ((host["entity"] != TERRAIN) & (host["entity"] != MISS)).any()
    w.close()


# ---- 6. consistency
def test_a_sweep_along_the_normal_meets_the_terrain_at_the_distance(mi_lib):
    c = TD.comparison_reference()
    w = Q.world(mi_lib, c["scene"])
    got = _both(w, c["volumes"], None, what="comparison set, unbounded")
    pick = [i for i in range(len(got)) if got["flags"][i] == 0 and got["entity"][i] == TERRAIN]
    assert len(pick) >= 40
    length = got["distance"][pick].astype(np.float64) + 0.05
    disp = (-got["normal"][pick].astype(np.float64) * length[:, None]).astype(np.float32)
    hits = w.sweep(c["volumes"][pick], disp, 4)
    worst = 0.0
    for k, i in enumerate(pick):
        travelled = float(hits["t"][k]) * float(np.linalg.norm(disp[k].astype(np.float64)))
        err = abs(travelled - float(got["distance"][i])) / c["scales"][i]
        worst = max(worst, err)
        assert hits["entity"][k] == TERRAIN and hits["flags"][k] == 0 and err <= ST.BOUND + BOUND, (i, got[i], hits[k], travelled)
    print(f"sweeps along -normal: largest |t x length - distance| per unit of scale {worst:.2e}")
    w.close()


def test_a_heightmap_edit_is_seen_by_the_next_query(mi_lib):
    from d3d12renderer_amd import capi
    sc = ST.scene("flat")
    hm = sc.heightmap
    w = Q.world(mi_lib, sc)
    vols = np.concatenate([capi.sphere_volume((10.3, 6.0, 12.1), 0.4), capi.box_volume((7.7, 7.0, 9.4), (0.3, 0.2, 0.5))])
    before = _both(w, vols, None, what="before the edit")
    w.update_heightmap(np.asarray(hm["min_corner"], np.float32) + np.array([0, 1, 0], np.float32), hm["amplitude"])
    after = _both(w, vols, None, what="after the edit")
    assert (before["entity"] == TERRAIN).all() and (after["entity"] == TERRAIN).all()
    assert np.abs(before["distance"].astype(np.float64) - after["distance"] - 1.0).max() <= BOUND * 16
    assert np.abs(after["point_collider"][:, 1].astype(np.float64) - before["point_collider"][:, 1] - 1.0).max() <= BOUND * 16
    w.close()


def test_queries_change_nothing_a_step_computes(mi_lib):
    from d3d12renderer_amd import scenes
    sc = scenes.terrain_field()
    sc.hulls = list(sc.hulls) or [R.volume_hull()]
    a = Q.world(mi_lib, sc); b = Q.world(mi_lib, sc)
    s = sc.settings()
    ents = Q.bodies(sc)
    vols = R.make_volumes(27, 4, (-9, 0.5, -9), (9, 8, 9), 0.1, 0.5)
    previous = None
    for i in range(24):
        a.step_fixed(s, sc.dt, 1); b.step_fixed(s, sc.dt, 1)
        if i % 8 == 0:
            got = _both(b, vols, None, merge_into=b.distance(vols, None, 31), what=f"step {i}")
            assert previous is None or got.tobytes() != previous   # the merged records see the moved bodies
            previous = got.tobytes()
        else:
            b.terrain_distance(vols, 2.0)
    assert a.get_body_states(ents).tobytes() == b.get_body_states(ents).tobytes()
    a.close(); b.close()
