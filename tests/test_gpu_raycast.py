"""Ray-cast scene queries on the GPU (mi_world_raycast, mi_world_raycast_device_async, mi_debug_raycast_exhaustive): against the numpy
reference (tests/raycast_ref.py), the accelerated grid against the exhaustive scan byte for byte, the terrain, the existing poke, the
cache's invalidation, the device variant, and that queries change nothing a step computes."""
import ctypes as C

import numpy as np
import pytest

import query_helpers as Q
from raycast_ref import SceneRef

pytestmark = pytest.mark.gpu

ALL = 31


def _ref(w, sc):
    p, r = w.physics_transforms()
    return SceneRef(sc, p, r)


def _random_rays(rng, n, lo, hi):
    o = rng.uniform(lo, hi, (n, 3)).astype(np.float32)
    d = rng.normal(size=(n, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    return o, d


def _edge_rays(rng, n, lo, hi):
    """Rays starting outside the grid, axis-parallel ones (zero direction components), misses, max_t cut-offs."""
    o, d = _random_rays(rng, n, lo, hi)
    far = np.asarray(hi, np.float32) * 3.0
    o[: n // 8] = far * np.sign(rng.normal(size=(n // 8, 3))).astype(np.float32)          # outside, aimed back at the scene
    d[: n // 8] = -o[: n // 8] / np.linalg.norm(o[: n // 8], axis=1, keepdims=True)
    axes = np.eye(3, dtype=np.float32)
    k = slice(n // 8, n // 4)
    d[k] = axes[rng.integers(0, 3, n // 4 - n // 8)] * np.where(rng.random((n // 4 - n // 8, 1)) < 0.5, -1, 1).astype(np.float32)
    d[n // 4: n // 4 + 16] = (0.0, -1.0, 0.0)                                             # down: through the ground (a large collider)
    d[n // 4 + 16: n // 4 + 32] = (0.0, 1.0, 0.0)
    o[n // 4 + 16: n // 4 + 32, 1] = np.float32(hi[1] * 4)                              # up, from above everything: misses
    max_t = rng.uniform(0.1, 20.0, n).astype(np.float32)
    max_t[::3] = np.inf
    return o, d, max_t


def _same_bytes(a, b):
    assert a.dtype == b.dtype and len(a) == len(b)
    if a.tobytes() != b.tobytes():
        bad = [i for i in range(len(a)) if a[i].tobytes() != b[i].tobytes()]
        raise AssertionError(f"{len(bad)} of {len(a)} hits differ; first {bad[:4]}: {a[bad[:2]]} vs {b[bad[:2]]}")


def _compare_to_ref(hits, ref, o, d, what, budget=0.002):
    """Entity / collider / t / point / normal against the numpy reference; rays whose two nearest candidates lie within 1e-5 of each other
    (relative) are not compared, and a few decisions at a test's own tolerance (grazing rays, edges) may go either way."""
    o = o.astype(np.float64); d = d.astype(np.float64)
    close = ref["margin"] < 1e-5
    same = (hits["collider"].astype(np.uint64) == ref["collider"]) & (hits["entity"].astype(np.uint64) == ref["entity"])
    wrong = ~same & ~close
    assert wrong.sum() <= max(2, budget * len(o)), f"{what}: {wrong.sum()} rays hit something else; first {np.nonzero(wrong)[0][:5]}"
    m = same & ~close & (hits["entity"] != 0xFFFFFFFF)
    if not m.any():
        return
    t = hits["t"][m].astype(np.float64)
    tbad = ~np.isclose(t, ref["t"][m], rtol=1e-5, atol=1e-5)   # (a grazing ray's t is ill-conditioned in float32: sqrt of a near-zero discriminant)
    assert tbad.sum() <= max(2, budget * len(o)), f"{what}: {tbad.sum()} t differ: {t[tbad][:4]} vs {ref['t'][m][tbad][:4]}, colliders {hits['collider'][m][tbad][:4]}"
    assert np.allclose(hits["point"][m], o[m] + t[:, None] * d[m], rtol=1e-5, atol=1e-4), what
    n = hits["normal"][m].astype(np.float64)
    assert np.allclose(np.linalg.norm(n, axis=1), 1.0, atol=1e-5), what
    nbad = ~np.all(np.abs(n - ref["normal"][m]) <= 1e-4, axis=1) & ~tbad
    assert nbad.sum() <= max(2, budget * len(o)), f"{what}: {nbad.sum()} normals differ: {n[nbad][:3]} vs {ref['normal'][m][nbad][:3]}, colliders {hits['collider'][m][nbad][:3]}"
    assert np.array_equal(hits["object_type"][m], ref["object_type"][m]), what


def test_zoo_matches_numpy_reference(mi_lib):
    from d3d12renderer_amd import scenes
    sc = scenes.shape_zoo()
    w = Q.world(mi_lib, sc, 30)
    ref = _ref(w, sc)
    rng = np.random.default_rng(11)
    o, d = _random_rays(rng, 4096, (-7, -1, -7), (7, 8, 7))
    for include in (1, 2, 3, 7, ALL):
        hits = w.raycast(o, d, include=include)
        _compare_to_ref(hits, ref.raycast(o, d, include=include), o, d, f"include {include}")
    assert (w.raycast(o, d, include=0)["entity"] == 0xFFFFFFFF).all()


def test_directions_of_any_length(mi_lib):
    """t is in the direction's units for every shape (the sphere tests included): scaled rays hit what the unit rays hit, at t / scale,
    match the numpy reference, and the grid still equals the exhaustive scan."""
    from d3d12renderer_amd import scenes
    sc = scenes.shape_zoo()
    w = Q.world(mi_lib, sc, 30)
    ref = _ref(w, sc)
    rng = np.random.default_rng(12)
    o, d = _random_rays(rng, 2048, (-7, -1, -7), (7, 8, 7))
    unit = w.raycast(o, d, include=ALL)
    for scale in (0.5, 3.0):
        ds = (d * np.float32(scale)).astype(np.float32)
        hits = w.raycast(o, ds, include=ALL)
        _compare_to_ref(hits, ref.raycast(o, ds, include=ALL), o, ds, f"scale {scale}")
        same = hits["entity"] == unit["entity"]
        assert (~same).sum() <= 4, f"scale {scale}: {(~same).sum()} rays hit something else than the unit ray"
        m = same & (unit["entity"] != 0xFFFFFFFF)
        assert (~np.isclose(hits["t"][m] * scale, unit["t"][m], rtol=1e-5, atol=1e-5)).sum() <= 4, scale
        eo, ed, emt = _edge_rays(rng, 2048, (-7, -1, -7), (7, 8, 7))
        _check_accel_equals_exhaustive(w, eo, (ed * np.float32(scale)).astype(np.float32), emt, include=ALL)
    w.close()


def _check_accel_equals_exhaustive(w, o, d, max_t, ranges=None, include=7):
    a = w.raycast(o, d, max_t=max_t, include=include, entity_ranges=ranges)
    b = w.debug_raycast_exhaustive(o, d, max_t=max_t, include=include, entity_ranges=ranges)
    _same_bytes(a, b)
    return a


def test_accelerated_equals_exhaustive(mi_lib):
    from d3d12renderer_amd import scenes
    rng = np.random.default_rng(5)
    cases = [(scenes.shape_zoo(), 30, (-7, -1, -7), (7, 8, 7)),
             (scenes.obb_pile(128, 4, 128), 60, (-100, -1, -100), (100, 8, 100)),
             (scenes.terrain_field(), 30, (-18, -1, -18), (18, 10, 18))]
    for sc, steps, lo, hi in cases:
        w = Q.world(mi_lib, sc, steps)
        o, d, max_t = _edge_rays(rng, 4096, lo, hi)
        h = _check_accel_equals_exhaustive(w, o, d, max_t)
        assert (h["entity"] == 0xFFFFFFFF).any() and (h["entity"] != 0xFFFFFFFF).any(), sc.name
        _check_accel_equals_exhaustive(w, o, d, None, include=ALL)
        n_ent = len(sc.entities)
        lo_e = rng.integers(0, n_ent, len(o)).astype(np.uint32)
        ranges = np.stack([lo_e, np.minimum(lo_e + rng.integers(1, 64, len(o)), n_ent)], axis=1).astype(np.uint32)
        ranges[::5] = (0, 0xFFFFFFFF)
        h = _check_accel_equals_exhaustive(w, o, d, max_t, ranges=ranges)
        ok = (h["entity"] == 0xFFFFFFFF) | (h["entity"] == 0xFFFFFFFE) | ((h["entity"] >= ranges[:, 0]) & (h["entity"] < ranges[:, 1]))
        assert ok.all(), sc.name
        w.close()


def _terrain_scene(holes=()):
    from d3d12renderer_amd import scenes
    sc = scenes.terrain_field(4, 1, 4, with_unsupported=False)
    sc.heightmap = scenes.rolling_heightmap(holes=holes)
    return sc


def test_terrain(mi_lib):
    sc = _terrain_scene(holes=((1, 1),))
    w = Q.world(mi_lib, sc)
    hm = sc.heightmap
    s = hm["chunk_size"] / 128.0
    corner = np.asarray(hm["min_corner"], np.float64)
    rng = np.random.default_rng(3)
    # vertical rays over grid vertices and along cell edges (chunk (1, 1) is a hole)
    gx = rng.integers(0, 128, 300); gz = rng.integers(0, 128, 300)
    frac = np.where(rng.random(300) < 0.5, 0.0, rng.random(300))
    x = corner[0] + gx * s + np.where(np.arange(300) % 2 == 0, frac * s, 0.0)
    z = corner[2] + gz * s + np.where(np.arange(300) % 2 == 1, frac * s, 0.0)
    o = np.stack([x, np.full(300, 20.0), z], axis=1).astype(np.float32)
    d = np.tile(np.float32([0, -1, 0]), (300, 1))
    hits = w.raycast(o, d, include=4)
    amp = hm["amplitude"]
    assert (hits["entity"] == 0xFFFFFFFE).all()
    for i in range(300):
        y = float(o[i, 1]) - float(hits["t"][i])
        assert abs(y - w.heightmap_height(float(o[i, 0]), float(o[i, 2]))) <= 1e-4 * amp, i
        assert hits["normal"][i][1] > 0
    # oblique rays against the triangle reference
    o, d = _random_rays(rng, 256, (-15, 7, -15), (15, 9, 15))
    d[:, 1] = -np.abs(d[:, 1]) - 0.2
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    length = np.float32(30.0)
    hits = w.raycast(o, d, max_t=length, include=4)
    ref = SceneRef(sc, *w.physics_transforms()).raycast(o, d, max_t=np.full(256, length), include=4)
    _compare_to_ref(hits, ref, o, d, "terrain")
    # holes: nothing under chunk (1, 1)
    cx = corner[0] + hm["chunk_size"] * 1.5; cz = corner[2] + hm["chunk_size"] * 1.5
    hole = w.raycast(np.float32([[cx, 20.0, cz]]), np.float32([[0, -1, 0]]), include=4)
    assert hole["entity"][0] == 0xFFFFFFFF
    _same_bytes(w.raycast(o, d, max_t=length, include=4), w.debug_raycast_exhaustive(o, d, max_t=length, include=4))


def test_rigid_hits_are_what_the_poke_pushes(mi_lib):
    """mi_world_test_interactions pushes the entity mi_world_raycast reports (rigid bodies only): two identical worlds, one poked."""
    from d3d12renderer_amd import scenes
    sc = scenes.shape_zoo(3, 2, 3)
    rng = np.random.default_rng(8)
    pos = sc.entities["position"][:18]
    for i in range(6):
        target = pos[rng.integers(0, 18)] + rng.uniform(-0.2, 0.2, 3)
        o = (target + np.float32([rng.uniform(-2, 2), 6.0, rng.uniform(-2, 2)])).astype(np.float32)
        d = (target - o) / np.linalg.norm(target - o)
        a = Q.world(mi_lib, sc); b = Q.world(mi_lib, sc)
        hit = a.raycast(o[None], d[None].astype(np.float32), include=1)[0]
        b.test_interactions(o[None], d[None].astype(np.float32))
        a.step_fixed(sc.settings(), sc.dt, 1); b.step_fixed(sc.settings(), sc.dt, 1)
        (la, _), (lb, _) = a.velocities(), b.velocities()
        changed = np.nonzero(np.any(la != lb, axis=1))[0]
        if hit["entity"] == 0xFFFFFFFF:
            assert len(changed) == 0
        else:
            assert int(hit["entity"]) in changed.tolist() and int(np.argmax(np.linalg.norm(la - lb, axis=1))) == int(hit["entity"])
        a.close(); b.close()


def test_cache_follows_every_change(mi_lib):
    from d3d12renderer_amd import capi, scenes
    import torch
    sc = scenes.shape_zoo(3, 2, 3)
    w = Q.world(mi_lib, sc, 5)
    rng = np.random.default_rng(2)
    o, d, max_t = _edge_rays(rng, 1024, (-4, -1, -4), (4, 6, 4))

    def check(what):
        h = _check_accel_equals_exhaustive(w, o, d, max_t, include=ALL)
        return h

    def down_at(p):
        return np.float32([[p[0], p[1] + 5.0, p[2]]]), np.float32([[0, -1, 0]])

    check("start")
    w.step_fixed(sc.settings(), sc.dt, 1); check("step")
    # host body-state write: entity 3 teleported far from the grid the last query built
    st = w.get_body_states([3]); st[0, :3] = (40.0, 3.0, -35.0); w.set_body_states([3], st)
    h = w.raycast(*down_at((40.0, 3.0, -35.0)), include=ALL)
    assert h["entity"][0] == 3; check("set_body_states")
    # device write, enqueued on the world's stream
    body = w.entities_to_bodies([4])
    st = w.get_body_states([4]); st[0, :3] = (-30.0, 2.0, 33.0)
    ids = torch.tensor(body.astype(np.int32), device="cuda"); sd = torch.tensor(st, device="cuda")
    torch.cuda.synchronize()
    w.set_body_states_device_async(1, ids.data_ptr(), sd.data_ptr())
    h = w.raycast(*down_at((-30.0, 2.0, 33.0)), include=ALL)
    assert h["entity"][0] == 4; check("set_body_states_device_async")
    # checkpoint: back to this state after steps and queries
    blob = w.save_checkpoint()
    before = w.raycast(o, d, max_t=max_t, include=ALL)
    w.step_fixed(sc.settings(), sc.dt, 10); check("steps")
    w.load_checkpoint(blob)
    _same_bytes(w.raycast(o, d, max_t=max_t, include=ALL), before); check("load_checkpoint")
    # topology: destroy an entity, add a collider
    w.destroy_entity(3)
    h = w.raycast(*down_at((40.0, 3.0, -35.0)), include=ALL)
    assert h["entity"][0] == len(sc.entities) - 1 and abs(h["t"][0] - 8.0) < 1e-4; check("destroy")   # through to the ground
    e = w.create_entities(scenes.make_entities(1, capi.ENTITY_STATIC))
    c = scenes.make_colliders(1, capi.SPHERE); c["shape"][0, :4] = (25.0, 4.0, 25.0, 1.0)
    w.add_colliders([e], c)
    h = w.raycast(*down_at((25.0, 4.0, 25.0)), include=ALL)
    assert h["entity"][0] == e and abs(h["t"][0] - 4.0) < 1e-5 and h["object_type"][0] == 1; check("collider add")
    w.close()
    # the heightmap
    sc = _terrain_scene()
    w = Q.world(mi_lib, sc)
    p = np.float32([[1.3, 30.0, -2.1]]); dn = np.float32([[0, -1, 0]])
    y0 = 30.0 - float(w.raycast(p, dn, include=4)["t"][0])
    w.update_heightmap(np.asarray(sc.heightmap["min_corner"]) + np.float32([0, 3.0, 0]), sc.heightmap["amplitude"])
    y1 = 30.0 - float(w.raycast(p, dn, include=4)["t"][0])
    assert abs(y1 - y0 - 3.0) < 1e-4 and abs(y1 - w.heightmap_height(1.3, -2.1)) < 1e-3
    w.close()


def test_device_variant_equals_host_variant(mi_lib):
    from d3d12renderer_amd import capi, scenes
    import torch
    sc = scenes.shape_zoo()
    w = Q.world(mi_lib, sc, 10)
    rng = np.random.default_rng(4)
    o, d, max_t = _edge_rays(rng, 2048, (-7, -1, -7), (7, 8, 7))
    rays = np.zeros((len(o), 8), np.float32); rays[:, :3] = o; rays[:, 3:6] = d; rays[:, 6] = max_t
    rays_d = torch.tensor(rays, device="cuda")
    out_d = torch.zeros(len(o) * capi.ray_hit_dtype.itemsize, dtype=torch.uint8, device="cuda")
    lo_e = rng.integers(0, len(sc.entities), len(o)).astype(np.uint32)
    ranges = np.stack([lo_e, lo_e + 40], axis=1).astype(np.uint32)
    ranges_d = torch.tensor(ranges.view(np.int32), device="cuda")
    torch.cuda.synchronize()
    previous = None
    for _ in range(2):
        w.step_fixed(sc.settings(), sc.dt, 1)
        w.raycast_device_async(len(o), rays_d.data_ptr(), out_d.data_ptr(), include=ALL)   # right behind the step, on the world's stream
        host = w.raycast(o, d, max_t=max_t, include=ALL)                                 # (synchronises that stream)
        dev = out_d.cpu().numpy().view(capi.ray_hit_dtype)
        _same_bytes(dev, host)
        if previous is not None:
            assert dev.tobytes() != previous
        previous = dev.tobytes()
        w.raycast_device_async(len(o), rays_d.data_ptr(), out_d.data_ptr(), include=7, ranges_ptr=ranges_d.data_ptr())
        host = w.raycast(o, d, max_t=max_t, include=7, entity_ranges=ranges)
        _same_bytes(out_d.cpu().numpy().view(capi.ray_hit_dtype), host)
    w.close()


def test_queries_change_nothing(mi_lib):
    from d3d12renderer_amd import scenes
    sc = scenes.shape_zoo()
    a = Q.world(mi_lib, sc); b = Q.world(mi_lib, sc)
    rng = np.random.default_rng(6)
    o, d = _random_rays(rng, 512, (-7, -1, -7), (7, 8, 7))
    s = sc.settings()
    ents = np.nonzero(sc.entities["kind"] != 2)[0]
    for _ in range(100):
        a.step_fixed(s, sc.dt, 1); b.step_fixed(s, sc.dt, 1)
        b.raycast(o, d)
    assert a.get_body_states(ents).tobytes() == b.get_body_states(ents).tobytes()
    assert a.debug_step_ahead_stats() == b.debug_step_ahead_stats()
    a.close(); b.close()


def test_errors(mi_lib):
    from d3d12renderer_amd import capi, scenes, sharding
    sc = scenes.shape_zoo(2, 1, 2)
    w = Q.world(mi_lib, sc)
    assert len(w.raycast(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32))) == 0
    f = w.L.fn("world_raycast")
    out = np.zeros(1, capi.ray_hit_dtype); v = np.zeros(3, np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    assert f(w.h, C.c_uint32(1), None, p(v), None, C.c_uint32(7), None, p(out)) == -1
    assert f(w.h, C.c_uint32(1), p(v), p(v), None, C.c_uint32(7), None, None) == -1
    assert w.L.fn("world_raycast_device_async")(w.h, C.c_uint32(1), None, C.c_uint32(7), None, None) == -1
    assert w.L.fn("debug_raycast_exhaustive")(w.h, C.c_uint32(1), None, p(v), None, C.c_uint32(7), None, p(out)) == -1
    assert f(w.h, C.c_uint32(0), None, None, None, C.c_uint32(7), None, None) == 0
    h = w.raycast(np.float32([[0, 5, 0], [0, 5, 0], [0, 5, 0]]), np.float32([[0, 0, 0], [np.nan, -1, 0], [0, -1, 0]]))
    assert h["entity"][0] == 0xFFFFFFFF and h["entity"][1] == 0xFFFFFFFF and h["entity"][2] != 0xFFFFFFFF   # zero / NaN direction: a miss
    w.close()
    w = Q.world(mi_lib, sc)
    w.shard_enable(sharding._desc_for(sharding.tile_grid(sc, 1), 0))
    assert f(w.h, C.c_uint32(1), p(v), p(v), None, C.c_uint32(7), None, p(out)) == -6
    w.close()


# ---- the matrix: every collider type at its hard rays, one collider at a time, against the exact float64 reference (tests/raycast_matrix.py)
import raycast_exact as X   # noqa: E402
import raycast_matrix as M   # noqa: E402

MISS = 0xFFFFFFFF


def _who(name, i, c):
    return f"{name}[{i}] {M.KINDS[c['kind']]} {c['tag']} (scale {c['scale']:.3g}, |d| {np.linalg.norm(c['d']):.3g})"


def _is_miss_record(rec):
    return (rec["entity"] == MISS and rec["collider"] == MISS and np.isposinf(rec["t"]) and not rec["point"].any() and not rec["normal"].any()
            and rec["object_type"] == 0)


# The one place of the matrix with a figure of its own: a capsule / cylinder whose axis lies 1e-3 rad off -y, hit on its side.  The cylinder
# test turns the ray into the cylinder's frame by rotateFromTo(axis, +y), and next to that function's half-turn branch s = sqrt(2 (1 + d)) is
# taken of 1 + d = 5e-7, a float32 difference good to one part in ten: the frame is off by about 1e-4 rad, the side by that times the ray's
# lever.  Measured per unit of scale: capsule 8.2e-5, cylinder 6.8e-5 (their end rays and the axes 1e-2 rad off -y stay within the family's
# bound).  It is the reference's arithmetic (rayVsCollider), kept for unit rays.  Held to 4 x their own figure; they do not set the family's bound.
KNOWN_ILL_CONDITIONED = {("axes", 1, "-y+1e-3_side"): 4e-4, ("axes", 2, "-y+1e-3_side"): 3e-4}


def _check_matrix(name, cases, ranges, got):
    """Every record against the exact reference's answer of its case, all measures per unit of the case's scale; returns the failures and
    prints the worst values per collider type: |dt| |d|, the point off o + t d, the point off the collider's surface, the separation short of
    0.05 scale after backing off along the normal (one admissible normal only), and |n - the nearest admissible normal| (x the radius of a
    round shape)."""
    bad, worst = [], {}
    nc = int(ranges[-1, 1])
    for i, c in enumerate(cases):
        rec, ref, who = got[i], c["ref"], _who(name, i, c)
        own = KNOWN_ILL_CONDITIONED.get((name, c["kind"], c["tag"]))
        bound, length = (M.BOUNDS[name] if own is None else own) * c["scale"], float(np.linalg.norm(c["d"]))
        expect = c.get("expect") if name == "inside" else None
        want_hit = expect != "miss" if name == "inside" else c["win"] is not None
        if (rec["entity"] == MISS) == want_hit:
            bad.append(f"{who}: decision: GPU {'misses' if rec['entity'] == MISS else 'hits at t = %.6g' % rec['t']}, expected "
                       f"{'a miss' if not want_hit else 'a hit at t = %.6g' % (ref['t_exit'] if expect == 'exit' else ref['t'])}")
            continue
        if not want_hit:
            if not _is_miss_record(rec):
                bad.append(f"{who}: a miss record that is not all-miss: {rec}")
            continue
        ent = int(ranges[i, 0]) + c["win"]
        if rec["entity"] != ent or rec["collider"] != nc - 1 - ent or rec["object_type"] != 1:
            bad.append(f"{who}: entity {rec['entity']} (expected {ent}), collider {rec['collider']} (expected {nc - 1 - ent}), object type {rec['object_type']}")
            continue
        shape = c["cols"][c["win"]]["shape"]
        t, p, n = float(rec["t"]), rec["point"].astype(np.float64), rec["normal"].astype(np.float64)
        if abs(np.linalg.norm(n) - 1) > 1e-5:
            bad.append(f"{who}: |n| - 1 = {np.linalg.norm(n) - 1:.2e}")
        if expect == "t0":
            if t != 0 or not np.allclose(n, -c["d"] / length, atol=1e-6) or not (rec["point"] == c["o32"]).all():
                bad.append(f"{who}: the origin is inside: expected t = 0, the origin and -normalize(d); got t = {t:.6g}, point {p}, normal {n}")
            continue
        t_ref, normals = (ref["t_exit"], c["exit_normals"]) if expect == "exit" else (ref["t"], c["normals"])
        m = worst.setdefault(c["kind"], [0.0] * 5)
        dt = abs(t - t_ref) * length
        dp = float(np.linalg.norm(p - (c["o"] + t * c["d"])))
        ds = abs(X.sdf(shape, p))
        rho = float(shape[1][-1]) if shape[0] in (X.SPHERE, X.CAPSULE, X.CYLINDER) else 1.0
        dn = min(float(np.linalg.norm(n - a)) for a in normals) * rho
        short = 0.0
        if len(normals) == 1 and expect is None:
            short = 0.05 * c["scale"] - X.sdf(shape, p + 0.05 * c["scale"] * n)
        if own is not None:
            print(f"{who}: known ill-conditioned case, the largest measure per unit of scale {max(dt, dp, ds, short, dn) / c['scale']:.2e} (allowed {own:.0e})")
        for k, v in enumerate((dt, dp, ds, short, dn) if own is None else ()):
            m[k] = max(m[k], v / c["scale"])
        if dt > bound:
            bad.append(f"{who}: |t - t_ref| |d| = {dt:.3e} > {bound:.3e} (t = {t:.8g}, the reference {t_ref:.8g})")
        if dp > bound or ds > bound:
            bad.append(f"{who}: the point lies {dp:.3e} off o + t d and {ds:.3e} off the collider's surface (bound {bound:.3e})")
        if short > bound or dn > bound:
            bad.append(f"{who}: normal {n}: {dn:.3e} off the nearest of {len(normals)} admissible normals, separation short by {short:.3e} (bound {bound:.3e})")
        if (n @ c["d"] > 0) != (expect == "exit"):
            bad.append(f"{who}: normal {n} . d = {n @ c['d']:.3e}")
    for kind, m in sorted(worst.items()):
        print(f"{name}, {M.KINDS[kind]}, per unit of scale: largest |dt| |d| {m[0]:.2e}, point off o + t d {m[1]:.2e}, point off the surface {m[2]:.2e}, "
              f"separation short by {m[3]:.2e}, normal off the admissible ones {m[4]:.2e}")
    if worst:
        print(f"{name}: the largest measure per unit of scale {max(max(m) for m in worst.values()):.2e} (bound {M.BOUNDS[name]:.0e})")
    return bad


@pytest.mark.parametrize("name", M.FAMILIES)
def test_matrix_family(mi_lib, name):
    """One family of tests/raycast_matrix.py in one world, ray i aimed at the entities of case i alone, through the grid and through the
    exhaustive scan (the same bytes).  Every kept case, without a budget: the exact reference's decision, entity, collider and object type; t,
    point and normal within the family's bound x scale (_check_matrix); dot(normal, d) <= 0 but for the documented answers of the `inside`
    family (t = 0 with -normalize(d); a hull's far side); a miss record all-miss.  Every failure of the family is reported, after the worst
    values."""
    cases = M.kept(name)
    sc, ranges = M.scene_of(cases, f"raycast matrix {name}")
    w = Q.world(mi_lib, sc)
    pick = list(range(len(cases))) + ([0] if len(cases) % 2 == 0 else [])   # (an odd batch)
    o, d = np.stack([cases[i]["o32"] for i in pick]), np.stack([cases[i]["d32"] for i in pick])
    max_t = np.array([cases[i]["max_t32"] for i in pick], np.float32)
    got = _check_accel_equals_exhaustive(w, o, d, max_t, ranges=ranges[pick], include=ALL)
    w.close()
    bad = _check_matrix(name, cases, ranges, got)
    assert not bad, f"{len(bad)} of {len(cases)} cases fail:\n" + "\n".join(bad)
