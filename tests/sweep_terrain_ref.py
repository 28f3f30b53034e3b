"""Float64 yardstick of shape casts against the heightmap terrain (include/mi_physics.h, mi_world_sweep with the terrain flag of the include mask); numpy only, no GPU.

The terrain is what the ray cast hits: the collision triangles of raycast_ref.terrain_triangles, each one a convex shape ("pts", vertices[3, 3], 0.0)
of tests/sweep_ref.py — a two-sided surface without volume.  A cast culls the triangles by its swept bounds and hands the rest to sweep_ref.cast.
Neighbouring triangles share edges and vertices: the winner and the runner-up tie to 1e-16, so nothing here (and no test) says WHICH triangle won.

Also here: the maps of the tests (flat, tilted, the coarse rolling map with a hole) and the comparison set of the GPU test with what makes it a
valid yardstick (tests/test_sweep_terrain.py asserts it)."""
import numpy as np

import overlap_ref as R
import raycast_ref
import sweep_ref as S
import terrain_contact_ref as T
from d3d12renderer_amd import capi, scenes

TERRAIN = 0xFFFFFFFE   # capi.RAY_TERRAIN
# The bound of the GPU comparison per unit of scale (scale = max(1, the largest |coordinate| of the cast)): 4 x the largest value measured on the
# MI355X (1.44e-6; tests/test_gpu_sweep_terrain.py states the figures), rounded up to one digit.  The comparison set keeps every decision 16 of
# these clear of flipping.
BOUND = 6e-6
SEED = 4


def flat_map():
    """One chunk of 16 m at the origin, every height 32768 of amplitude 4: the plane y = FLAT_Y."""
    return T.flat_heightmap()


FLAT_Y = 32768 * 4.0 / 65535.0


def tilted_map():
    """One chunk of 16 m at the origin, height 500 * x counts of amplitude 4: exactly the plane y = TILT_SLOPE * x."""
    hm = T.flat_heightmap()
    hm["chunks"] = {(0, 0): np.tile((500 * np.arange(129)).astype(np.uint16), (129, 1))}
    return hm


TILT_SLOPE = 500 * 4.0 / 65535.0 / 0.125
TILT_NORMAL = np.array([-TILT_SLOPE, 1.0, 0.0]) / np.hypot(TILT_SLOPE, 1.0)


def rolling_map():
    """2 x 2 chunks of 32 m (cells of 0.25 m: the yardstick stays quick), amplitude 6, chunk (1, 0) a hole; x and z in [-32, 32]."""
    return scenes.rolling_heightmap(2, 32.0, 6.0, holes=((1, 0),))


MAPS = {"flat": flat_map, "tilted": tilted_map, "rolling": rolling_map}
_TRIANGLES = {}


def triangles(name):
    """(vertices [M, 3, 3], lower bounds [M, 3], upper bounds [M, 3]) of a map of MAPS, computed once per process."""
    if name not in _TRIANGLES:
        a, b, c = raycast_ref.terrain_triangles(MAPS[name]())
        v = np.stack([a, b, c], axis=1)
        v.setflags(write=False)
        _TRIANGLES[name] = (v, v.min(axis=1), v.max(axis=1))
    return _TRIANGLES[name]


def culled(name, vol, d, grow=1e-6):
    """The triangles whose AABB meets the swept bounds of `vol` moved along d (grown by `grow`), as sweep_ref shapes."""
    v, lo, hi = triangles(name)
    mn, mx = S.bounds(("swept", vol, np.asarray(d, np.float64)))
    keep = np.flatnonzero(((hi >= mn - grow) & (lo <= mx + grow)).all(axis=1))
    return [("pts", v[k], 0.0) for k in keep]


def cast(name, vol, d):
    """The first touch of `vol` moved along d with the terrain of map `name`: (t, unit normal from the terrain to the volume, point, initial overlap) or None."""
    hit = S.cast(vol, d, culled(name, vol, d))
    return None if hit is None else hit[1:]


def min_gap(name, shape, reach, axis=None):
    """The smallest sweep_ref.gap between `shape` and the triangles of map `name`, among those within `reach` of it (inf: none there).  A triangle is
    left out without a distance query once a lower bound of its gap — the distance of the two AABBs, and along `axis` (a unit vector, optional) the gap
    of the two projections — reaches the smallest gap found so far: the result is the minimum over all of them."""
    v, lo, hi = triangles(name)
    mn, mx = S.bounds(shape)
    lb = np.linalg.norm(np.maximum(np.maximum(lo - mx, mn - hi), 0.0), axis=1)
    if axis is not None:
        axis = np.asarray(axis, np.float64)
        lb = np.maximum(lb, S.support(shape, -axis) @ axis - S.margin(shape) - (v @ axis).max(axis=1))
    best = np.inf
    for k in np.argsort(lb, kind="stable"):
        if lb[k] > reach or lb[k] >= best:
            break
        best = min(best, S.gap(shape, ("pts", v[k], 0.0)))
    return best


def closest_approach(name, vol, d, reach):
    """The smallest gap between the moving volume and the terrain (sweep_ref.closest_approach over the triangles within `reach` of its swept bounds)."""
    return min_gap(name, ("swept", vol, np.asarray(d, np.float64)), reach)


def scale_of(vol, d):
    mn, mx = S.bounds(("swept", vol, np.asarray(d, np.float64)))
    return max(1.0, float(np.abs(np.concatenate([mn, mx])).max()))


def scene(name):
    """A world of the map alone, with the hull geometry the hull volumes use."""
    return scenes.Scene("sweep_terrain_" + name, scenes.make_entities(0), np.zeros(0, np.uint32), scenes.make_colliders(0, capi.SPHERE), 10,
                        hulls=[R.volume_hull()], heightmap=MAPS[name]())


def comparison_casts(seed=SEED):
    """48 casts on the rolling map, eight per volume type (cast i has type i % 6, group i // 6): groups 0-3 come down from above the hills to a point
    below them, group 4 starts below the surface and moves up (a hit from below), group 5 passes level above the hills, group 6 comes down but
    stops short, group 7 goes down through the hole.  (volumes, displacements float32 [48, 3])."""
    vols = R.make_volumes(seed, 8, (-1, -1, -1), (1, 1, 1), 0.15, 1.0)
    rng = np.random.default_rng(seed + 2000)
    n = len(vols)
    disp = np.zeros((n, 3))
    for i in range(n):
        g = i // 6
        x, z = rng.uniform(-27, 27, 2)
        if g <= 3:
            start = (x, rng.uniform(5.5, 8.0), z); d = (rng.uniform(-4, 4), -2.0 - start[1], rng.uniform(-4, 4))
        elif g == 4:
            start = (x, -4.0, z); d = (rng.uniform(-2, 2), 11.0, rng.uniform(-2, 2))
        elif g == 5:
            start = (x, 8.0, z); d = (rng.uniform(-10, 10), 0.0, rng.uniform(-10, 10))
        elif g == 6:
            start = (x, 8.5, z); d = (rng.uniform(-3, 3), -2.5, rng.uniform(-3, 3))
        else:
            start = (rng.uniform(5, 27), 7.0, rng.uniform(-27, -5)); d = (rng.uniform(-0.5, 0.5), -14.0, rng.uniform(-0.5, 0.5))
        vols["position"][i] = start
        disp[i] = d
    return vols, disp.astype(np.float32)


_COMPARISON = {}


def comparison_reference(seed=SEED):
    """The comparison set against the rolling map, computed once per process and left unchanged: the scene, the volumes and displacements, the
    volumes' convex shapes, per cast the hit (t, normal, point, initial) or None, its scale, and its `clearance`: how far the decision is from
    flipping — for a miss the closest approach to the terrain, for a hit the smaller of the gap at the start (travel x -d.n to the touch) and the
    depth the volume would reach along the touch's normal by the end of the displacement."""
    if seed not in _COMPARISON:
        sc = scene("rolling")
        vols, disp = comparison_casts(seed)
        convs, hits, scales, clear = [], [], [], []
        for v, d in zip(vols, disp):
            vc = S.volume_convex(v, sc.hulls)
            d64 = d.astype(np.float64)
            hit = cast("rolling", vc, d64)
            sca = scale_of(vc, d64)
            if hit is None:
                c = closest_approach("rolling", vc, d64, 32 * BOUND * sca)
            elif hit[3]:
                c = 0.0
            else:
                along = -(d64 @ hit[1])
                c = min(hit[0], 1.0 - hit[0]) * along
            convs.append(vc); hits.append(hit); scales.append(sca); clear.append(c)
        _COMPARISON[seed] = dict(scene=sc, volumes=vols, displacements=disp, convex=convs, hits=hits, scales=scales, clearance=clear)
    return _COMPARISON[seed]


def point_gap(name, point, reach=0.5):
    """Distance of a point from the terrain of map `name` (the nearest triangle within `reach`)."""
    return min_gap(name, ("pts", np.asarray(point, np.float64).reshape(1, 3), 0.0), reach)


def separation(name, vol, offset, normal, reach=0.5):
    """The gap between `vol` moved by `offset` and the terrain; `normal`: the unit direction the volume was backed off along (prunes the search)."""
    return min_gap(name, S.moved(vol, offset), reach, normal)
