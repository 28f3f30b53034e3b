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
