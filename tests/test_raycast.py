"""Ray-cast scene queries without a GPU: the ABI (header, exports, record size) and the numpy reference the GPU tests compare against."""
import re
from pathlib import Path

import numpy as np

from raycast_ref import (AABB, OBB, SPHERE, CAPSULE, CYLINDER, HULL, collider_t_and_normal, ray_terrain, terrain_triangles)

ROOT = Path(__file__).resolve().parent.parent
QUERY_SYMBOLS = ("mi_world_raycast", "mi_world_raycast_device_async", "mi_debug_raycast_exhaustive")


def test_header_declares_and_library_exports_the_query_api(mi_lib):
    text = (ROOT / "include" / "mi_physics.h").read_text()
    declared = set(re.findall(r"MI_API\s+[\w\s\*]+?\b(mi_\w+)\s*\(", text))
    for name in QUERY_SYMBOLS:
        assert name in declared, name
    L = mi_lib.library()
    missing = [n for n in QUERY_SYMBOLS if not hasattr(L.lib, n)]
    assert not missing, missing
    from d3d12renderer_amd import capi
    assert capi.ray_hit_dtype.itemsize == 40
    assert capi.QUERY_DEFAULT == capi.QUERY_RIGID_BODIES | capi.QUERY_STATIC | capi.QUERY_TERRAIN == 7
    assert "} mi_ray_hit;" in text and re.search(r"_QUERY_DEFAULT = 7\b", text)


def _one(ctype, shape, o, d, hull=None):
    t, n = collider_t_and_normal(ctype, np.asarray(shape, np.float64), hull, np.asarray([o], np.float64), np.asarray([d], np.float64))
    n = n[0] / np.linalg.norm(n[0]) if np.isfinite(t[0]) else None
    return t[0], n


def test_sphere():
    t, n = _one(SPHERE, [1, 0, 0, 0.5], (-3, 0, 0), (1, 0, 0))
    assert np.isclose(t, 3.5) and np.allclose(n, (-1, 0, 0))
    t, n = _one(SPHERE, [0, 0, 0, 1], (-3, 0.6, 0), (1, 0, 0))
    assert np.isclose(t, 3 - np.sqrt(1 - 0.36)) and np.allclose(n, (-np.sqrt(0.64), 0.6, 0))
    assert np.isinf(_one(SPHERE, [0, 0, 0, 1], (-3, 2, 0), (1, 0, 0))[0])          # passes by
    assert np.isinf(_one(SPHERE, [0, 0, 0, 1], (3, 0, 0), (1, 0, 0))[0])           # behind
    assert _one(SPHERE, [0, 0, 0, 1], (0.2, 0, 0), (1, 0, 0))[0] == 0.0            # inside: t = 0
    # any direction length: t in the direction's units
    assert np.isinf(_one(SPHERE, [10, 0, 0, 1], (0, 5, 0), (10, 0, 0))[0])           # passes 4 units clear
    t, n = _one(SPHERE, [10, 0, 0, 1], (0, 0, 0), (2, 0, 0))
    assert np.isclose(t, 4.5) and np.allclose(n, (-1, 0, 0))
    t, n = _one(CAPSULE, [0, -1, 0, 0, 1, 0, 0.5], (0, 5, 0), (0, -0.25, 0))          # an end sphere, quarter-length direction
    assert np.isclose(t, 14.0) and np.allclose(n, (0, 1, 0))


def test_capsule_and_cylinder():
    cap = [0, -1, 0, 0, 1, 0, 0.5]
    t, n = _one(CAPSULE, cap, (-3, 0.3, 0), (1, 0, 0))                              # side: normal from the segment
    assert np.isclose(t, 2.5) and np.allclose(n, (-1, 0, 0))
    t, n = _one(CAPSULE, cap, (0, 5, 0), (0, -1, 0))                                # end sphere
    assert np.isclose(t, 3.5) and np.allclose(n, (0, 1, 0))
    t, n = _one(CYLINDER, cap, (-3, 0.3, 0), (1, 0, 0))
    assert np.isclose(t, 2.5) and np.allclose(n, (-1, 0, 0))
    t, n = _one(CYLINDER, cap, (0.2, 5, 0.1), (0, -1, 0))                           # top cap
    assert np.isclose(t, 4.0) and np.allclose(n, (0, 1, 0))
    t, n = _one(CYLINDER, cap, (0.2, -5, 0.1), (0, 1, 0))                           # bottom cap
    assert np.isclose(t, 4.0) and np.allclose(n, (0, -1, 0))
    assert np.isinf(_one(CYLINDER, cap, (0.2, 5, 0.1), (0, 1, 0))[0])              # away from it: the cap behind is no hit


def test_boxes():
    t, n = _one(AABB, [-1, -2, -3, 1, 2, 3], (-5, 0.5, 0.5), (1, 0, 0))
    assert np.isclose(t, 4) and np.allclose(n, (-1, 0, 0))
    t, n = _one(AABB, [-1, -2, -3, 1, 2, 3], (0.5, 9, 0.5), (0, -1, 0))          # axis-parallel: other slabs infinite
    assert np.isclose(t, 7) and np.allclose(n, (0, 1, 0))
    assert np.isinf(_one(AABB, [-1, -2, -3, 1, 2, 3], (0, 0, 0), (1, 0, 0))[0])   # from inside: no hit
    s = 0.5 ** 0.5
    obb = [0, 0, s, s, 1, 0, 0, 1, 2, 3]                                          # 90 degrees about z, centre (1, 0, 0)
    t, n = _one(OBB, obb, (1, 10, 0), (0, -1, 0))                                 # the rotated box's x half-extent 1 lies along y
    assert np.isclose(t, 9) and np.allclose(n, (0, 1, 0), atol=1e-6)


def test_hull_triangle_normal():
    v = np.array([[-1, -1, -1], [1, -1, -1], [1, 1, -1], [-1, 1, -1], [-1, -1, 1], [1, -1, 1], [1, 1, 1], [-1, 1, 1]], np.float64)
    tris = np.array([[0, 2, 1], [0, 3, 2], [4, 5, 6], [4, 6, 7], [0, 1, 5], [0, 5, 4], [2, 3, 7], [2, 7, 6], [1, 2, 6], [1, 6, 5], [0, 4, 7], [0, 7, 3]])
    t, n = _one(HULL, [0, 0, 0, 1, 0, 0, 0], (0.2, 0.3, 5), (0, 0, -1), hull=(v, tris))
    assert np.isclose(t, 4) and np.allclose(n, (0, 0, 1))
    t, n = _one(HULL, [0, 0, 0, 1, 2, 0, 0], (-5, 0.1, 0.2), (1, 0, 0), hull=(v, tris))   # hull at x = 2
    assert np.isclose(t, 6) and np.allclose(n, (-1, 0, 0))


def test_terrain_triangles():
    h = np.zeros((129, 129), np.uint16)
    h[:, 64:] = 65535                                                             # a step along x
    hm = dict(chunk_size=128.0, amplitude=2.0, min_corner=np.zeros(3, np.float32), chunks={(0, 0): h})
    tris = terrain_triangles(hm)
    assert len(tris[0]) == 2 * 128 * 128
    o = np.array([[10.5, 5, 10.25], [100.0, 5, 100.0], [64.0, 5, 3.0]]); d = np.array([[0, -1, 0], [0, -1, 0], [0, -1, 0]], np.float64)
    t, n = ray_terrain(o, d, tris, np.full(3, 100.0))
    assert np.allclose(t, [5, 3, 3]) and np.allclose(n[:2], [[0, 1, 0], [0, 1, 0]])   # flat parts; on the step's top edge x = 64
    t, n = ray_terrain(np.array([[63.5, 5, 3.0]]), np.array([[0, -1.0, 0]]), tris, np.full(1, 100.0))
    assert np.isclose(t[0], 4.0)                                                  # halfway up the ramp cell (63, z)
    assert n[0][0] < 0 and n[0][1] > 0                                            # facing -x and up


# ---- the exact reference (tests/raycast_exact.py) and the matrix (tests/raycast_matrix.py), from the reference alone
import pytest   # noqa: E402

import raycast_exact as X   # noqa: E402
import raycast_matrix as M   # noqa: E402
from raycast_ref import qconj, qrot   # noqa: E402

I = (0, 0, 0, 1)
CUBE = (np.array([[-1, -1, -1], [1, -1, -1], [1, 1, -1], [-1, 1, -1], [-1, -1, 1], [1, -1, 1], [1, 1, 1], [-1, 1, 1]], np.float64),
        np.array([[0, 2, 1], [0, 3, 2], [4, 5, 6], [4, 6, 7], [0, 1, 5], [0, 5, 4], [2, 3, 7], [2, 7, 6], [1, 2, 6], [1, 6, 5], [0, 4, 7], [0, 7, 3]]))


def _exact(ctype, words, o, d, max_t=np.inf, pos=(0, 0, 0), rot=I, hull=None):
    shape = X.shape_of(ctype, np.asarray(words, np.float64), pos, rot, hull)
    return shape, X.cast(shape, np.asarray(o, np.float64), np.asarray(d, np.float64), max_t)


def test_exact_reference_equals_the_closed_forms():
    """The hand values of the tests above and a few more, to 1e-12: entry, normal, inside, max_t, exit, signed distance, closest approach."""
    near = lambda a, b: np.allclose(a, b, rtol=0, atol=1e-12)   # noqa: E731
    cap = [0, -1, 0, 0, 1, 0, 0.5]
    s, h = _exact(SPHERE, [0, 0, 0, 1], (-3, 0.6, 0), (1, 0, 0))
    assert near(h["t"], 3 - 0.8) and near(h["normal"], (-0.8, 0.6, 0)) and not h["inside"] and near(h["t_exit"], 3.8)
    assert near(X.closest_approach(s, (-3, 0.6, 0), (1, 0, 0))[0], -0.4) and near(X.closest_approach(s, (-3, 0.6, 0), (1, 0, 0), 1.0)[0], np.hypot(2, 0.6) - 1)
    assert _exact(SPHERE, [0, 0, 0, 1], (-3, 2, 0), (1, 0, 0))[1]["t"] is None and _exact(SPHERE, [0, 0, 0, 1], (3, 0, 0), (1, 0, 0))[1]["t"] is None
    assert near(X.closest_approach(s, (-3, 2, 0), (0.01, 0, 0))[0], 1.0)
    h = _exact(SPHERE, [0, 0, 0, 1], (0.2, 0, 0), (1, 0, 0))[1]
    assert h["t"] == 0 and h["inside"] and near(h["t_exit"], 0.8)
    assert near(_exact(SPHERE, [10, 0, 0, 1], (0, 0, 0), (2, 0, 0))[1]["t"], 4.5) and _exact(SPHERE, [10, 0, 0, 1], (0, 0, 0), (2, 0, 0), 4.4)[1]["t"] is None
    for d in (1e-3, 1.0, 1e4):   # the issue's ray through the middle of a thin capsule / cylinder, at any length
        for ctype in (CAPSULE, CYLINDER):
            h = _exact(ctype, [0, -1, 0, 0, 1, 0, 0.1], (-3, 0.3, 0), (d, 0, 0))[1]
            assert near(h["t"] * d, 2.9) and near(h["normal"], (-1, 0, 0))
    h = _exact(CAPSULE, cap, (0, 5, 0), (0, -0.25, 0))[1]
    assert near(h["t"], 14.0) and near(h["normal"], (0, 1, 0))
    s, h = _exact(CYLINDER, cap, (0.2, 5, 0.1), (0, -1, 0))
    assert near(h["t"], 4.0) and near(h["normal"], (0, 1, 0)) and near(h["t_exit"], 6.0)
    assert near(X.sdf(s, (0.2, 5, 0.1)), 4.0) and near(X.sdf(s, (0, 0.5, 0)), -0.5) and near(X.sdf(s, (0.8, 1.4, 0)), 0.5) and near(X.sdf(s, (0.3, 0, 0)), -0.2)
    h = _exact(CYLINDER, cap, (0.2, -5, 0.1), (0, 1, 0))[1]
    assert near(h["t"], 4.0) and near(h["normal"], (0, -1, 0))
    assert _exact(CYLINDER, cap, (0.2, 5, 0.1), (0, 1, 0))[1]["t"] is None and _exact(CYLINDER, cap, (0.6, 5, 0), (0, -1, 0))[1]["t"] is None
    h = _exact(CYLINDER, cap, (-3, 2.25, 0), (1, -0.5, 0))[1]   # onto the rim: side and cap are entered together
    assert near(h["t"], 2.5) and len(h["entries"]) == 2 and near(sorted(t for t, _ in h["entries"]), (2.5, 2.5))
    s, h = _exact(AABB, [-1, -2, -3, 1, 2, 3], (-5, 0.5, 0.5), (1, 0, 0))
    assert near(h["t"], 4) and near(h["normal"], (-1, 0, 0)) and near(X.sdf(s, (-5, 0.5, 0.5)), 4) and near(X.sdf(s, (0, 0, 0)), -1) and near(X.sdf(s, (2, 3, 4)), np.sqrt(3))
    assert _exact(AABB, [-1, -2, -3, 1, 2, 3], (0, 0, 0), (1, 0, 0))[1]["inside"] and _exact(AABB, [-1, -2, -3, 1, 2, 3], (0.5, 9, 3.5), (0, -1, 0))[1]["t"] is None
    r = 0.5 ** 0.5
    h = _exact(OBB, [0, 0, r, r, 1, 0, 0, 1, 2, 3], (1, 10, 0), (0, -1, 0))[1]
    assert near(h["t"], 9) and near(h["normal"], (0, 1, 0))
    s, h = _exact(HULL, [0, 0, 0, 1, 2, 0, 0], (-5, 0.1, 0.2), (1, 0, 0), hull=CUBE)
    assert near(h["t"], 6) and near(h["normal"], (-1, 0, 0)) and near(h["t_exit"], 8) and near(X.sdf(s, (-5, 0.1, 0.2)), 6) and near(X.sdf(s, (2.5, 0, 0)), -0.5)
    assert near(X.sdf(s, (4, 2, 2)), np.sqrt(3)) and near(X.sdf(s, (4, 2, 0.3)), np.sqrt(2))
    h = _exact(HULL, [0, 0, 0, 1, 0, 0, 0], (3, 3, 0.25), (-1, -1, 0), hull=CUBE)[1]   # onto the edge x = y = 1, where two triangles' planes meet
    assert near(h["t"], 2) and sum(abs(t - 2) < 1e-12 for t, _ in h["entries"]) == 4
    h = _exact(HULL, [0, 0, 0, 1, 0, 0, 0], (0.2, 0.3, 0.1), (0, 0, -2), hull=CUBE)[1]
    assert h["inside"] and h["t"] == 0 and near(h["t_exit"], 0.55)


def _mirror(case):
    """The kernel's arithmetic in float64 (raycast_ref.collider_t_and_normal) on a case's first collider: (t, world normal)."""
    c = case["cols"][0]
    q = c["rot"].astype(np.float64)
    t, n = collider_t_and_normal(c["ctype"], c["words"], M.SM.hulls()[c["hull"]], qrot(qconj(q), case["o"] - c["pos"])[None], qrot(qconj(q), case["d"])[None])
    ok = np.isfinite(t[0]) and t[0] <= case["max_t"]
    return (t[0], qrot(q, n[0]) / np.linalg.norm(n[0])) if ok else (None, None)


@pytest.mark.parametrize("name", M.FAMILIES)
def test_ray_matrix_family_is_a_valid_yardstick(name):
    """What the GPU comparison of a family relies on, from the exact reference alone: per collider type the robustness filter keeps at least 3
    of every 4 generated cases and at least two hits, in generic, grazing and limits at least one miss too (ordering, whose rows hold several
    collider types: over the whole family), and each family holds what it is meant to."""
    cases = M.family(name)
    table = M.counts(cases)
    kept = [c for c in cases if c["kept"]]
    print(f"{name}: {len(cases)} cases, {len(kept)} kept, scale up to {max(c['scale'] for c in cases):.3g}, delta {min(M.delta(c) for c in cases):.2e} .. {max(M.delta(c) for c in cases):.2e}")
    print("  " + "  ".join(f"{M.KINDS[k]} {m[1]}/{m[0]} ({m[2]} hit, {m[3]} miss)" for k, m in table.items()))
    rows = [[sum(m[i] for m in table.values()) for i in range(4)]] if name == "ordering" else [m for k, m in table.items() if name != "axes" or k in (1, 2)]
    assert all(m[0] >= 3 for m in rows)
    assert all(4 * m[1] >= 3 * m[0] and m[2] >= 2 for m in rows), table
    if name in ("generic", "grazing", "limits"):
        assert all(m[3] >= 1 for m in rows), table
    # (1e-6 below: a rounded quaternion is of unit length to 6e-8 only, and overlap_ref.qmat and raycast_ref.qrot turn a vector differently by that much)
    if name == "generic":   # the exact reference and the kernel's arithmetic in float64 agree where no epsilon of the kernel's is near
        for c in kept:
            t, n = _mirror(c)
            assert (t is None) == (c["win"] is None), c["tag"]
            if t is not None:
                assert abs(t - c["ref"]["t"]) <= 1e-6 and np.linalg.norm(n - c["ref"]["normal"]) <= 1e-6, (c["tag"], M.KINDS[c["kind"]], t, c["ref"]["t"], n, c["ref"]["normal"])
    if name == "grazing":
        for c in kept:
            k = int(c["tag"].split("_k")[1].rstrip("hitms"))
            assert (c["win"] is None) == c["tag"].endswith("miss") and abs(abs(c["approach"]) - k * M.delta(c)) <= 0.02 * k * M.delta(c), (c["tag"], c["approach"], M.delta(c))
    if name == "features":
        assert all(c["win"] is not None for c in cases if "outside" not in c["tag"] and "above" not in c["tag"] and c["tag"] != "axis+y")
        assert sum(len(c["normals"]) > 1 for c in kept) >= 12   # edges, corners, rims, vertices: several admissible normals
        assert sum(np.count_nonzero(c["d32"]) == 1 for c in kept) >= 28
    if name == "direction_length":
        for kind in range(7):
            group = [c for c in kept if c["kind"] == kind and c["win"] is not None]
            lengths = sorted(float(np.linalg.norm(c["d"])) for c in group)
            assert len(group) == len(M.LENGTHS) and np.allclose(lengths, M.LENGTHS, rtol=1e-6)
            assert np.ptp([c["ref"]["t"] * np.linalg.norm(c["d"]) for c in group]) <= 1e-5
    if name == "far":
        assert min(c["scale"] for c in cases) >= 90 and max(c["scale"] for c in cases) >= 900
    if name == "size_ratio":
        assert max(c["scale"] for c in kept) >= 100 and any(c["tag"].startswith("tiny") and c["win"] is not None for c in kept)
    if name == "limits":
        assert len(kept) == len(cases)
        assert any(c["tag"].endswith("d1000_near") for c in kept) and any(c["tag"].endswith("d0.001_short") for c in kept)
        for c in kept:
            want, L = c["expect"], np.linalg.norm(c["d"])
            assert (want is None) == (c["win"] is None) and (want is None or abs(c["ref"]["t"] - want) * L <= 0.25 * M.delta(c)), (c["tag"], want, c["ref"]["t"])
    if name == "inside":   # the documented answers are what the kernel's arithmetic gives
        assert len(kept) == len(cases) and all(c["ref"]["inside"] for c in cases)
        for c in cases:
            t, n = _mirror(c)
            if c["expect"] == "miss":
                assert t is None, c["tag"]
            elif c["expect"] == "t0":
                assert t == 0.0, (c["tag"], t)
            else:
                assert abs(t - c["ref"]["t_exit"]) * np.linalg.norm(c["d"]) <= 1e-6 and n @ c["d"] > 0 and min(np.linalg.norm(n - e) for e in c["exit_normals"]) <= 1e-6, c["tag"]
    if name == "ordering":
        assert sorted(len(c["cols"]) for c in kept) == [2, 2, 2, 2, 2, 3, 3, 3, 3] and any(c["win"] > 0 for c in kept)
        assert [c["win"] for c in kept if c.get("identical")] == [2]
