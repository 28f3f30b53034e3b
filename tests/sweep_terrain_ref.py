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


WIDE_CELL = 8.0 / 128.0
WIDE_FLOOR, WIDE_NEAR, WIDE_FAR = 1000, 30000, 60000   # height counts of amplitude 24: the floor, the lower bump at the near end, the higher at the far end
WIDE_BUMPS = ((16, WIDE_NEAR), (622, WIDE_FAR))         # (first vertex of the 3 x 3 raised vertices along the long axis, counts)


def wide_map():
    """5 x 5 chunks of 8 m (cells of 1 / 16 m, 640 a side; x and z in [-20, 20]) of which only the middle row (z in [-4, 4]) and the middle
    column (x in [-4, 4]) have heights: the constant WIDE_FLOOR but for two bumps of 3 x 3 vertices each, on the row's centre line at cells 16 and
    622 along x and on the column's at the same cells along z.  A volume more than 512 cells long lying along the row or the column and coming
    down onto the bump at the far end puts its only touch behind the first 64 blocks of its footprint."""
    chunks = {(x, z): np.full((129, 129), WIDE_FLOOR, np.uint16) for x in range(5) for z in range(5) if x == 2 or z == 2}
    for at, counts in WIDE_BUMPS:
        for along_x in (True, False):
            for k in range(at, at + 3):
                for j in range(319, 322):
                    gx, gz = (k, j) if along_x else (j, k)
                    for (cx, cz), h in chunks.items():    # (a vertex on a chunk's edge row belongs to both chunks)
                        if 0 <= gx - 128 * cx <= 128 and 0 <= gz - 128 * cz <= 128:
                            h[gz - 128 * cz, gx - 128 * cx] = counts
    return dict(chunks_per_dim=5, chunk_size=8.0, restitution=0.05, friction=0.8, min_corner=np.array([-20.0, 0.0, -20.0], np.float32), amplitude=24.0,
                chunks=chunks)


MAPS = {"flat": flat_map, "tilted": tilted_map, "rolling": rolling_map}
_TRIANGLES = {}


def map_of(name):
    """The heightmap of a map of MAPS, of raycast_terrain_matrix.MAPS (offset, floor) or the wide map."""
    if name in MAPS:
        return MAPS[name]()
    if name == "wide":
        return wide_map()
    import raycast_terrain_matrix
    return raycast_terrain_matrix.MAPS[name]()


def triangles(name):
    """(vertices [M, 3, 3], lower bounds [M, 3], upper bounds [M, 3]) of a map of MAPS, computed once per process."""
    if name not in _TRIANGLES:
        a, b, c = raycast_ref.terrain_triangles(map_of(name))
        v = np.stack([a, b, c], axis=1)
        v.setflags(write=False)
        _TRIANGLES[name] = (v, v.min(axis=1), v.max(axis=1))
    return _TRIANGLES[name]


def _culled(name, vol, d, grow=1e-6):
    """(indices, entry times) of the triangles whose AABB meets the swept bounds of `vol` moved along d (grown by `grow`) and, of those, the ones
    whose AABB grown by the volume's half-extents the displacement from the volume's centre passes through (sweep_ref.slab_entry on all of them at
    once, `grow` wider: a cast from 1e4 away keeps the triangles along its way, not every one under its swept bounds)."""
    v, lo, hi = triangles(name)
    mn, mx = S.bounds(("swept", vol, d))
    keep = np.flatnonzero(((hi >= mn - grow) & (lo <= mx + grow)).all(axis=1))
    vmn, vmx = S.bounds(vol)
    origin, half = (vmn + vmx) / 2, (vmx - vmn) / 2 + grow
    a, b = lo[keep] - half - origin, hi[keep] + half - origin
    t0, t1, ok = np.zeros(len(keep)), np.ones(len(keep)), np.ones(len(keep), bool)
    for i in range(3):
        if d[i] == 0:
            ok &= (a[:, i] <= 0) & (b[:, i] >= 0)
        else:
            ta, tb = a[:, i] / d[i], b[:, i] / d[i]
            t0, t1 = np.maximum(t0, np.minimum(ta, tb)), np.minimum(t1, np.maximum(ta, tb))
    # (the slab's own rounding: a time is off by a few ulps of its size, which `slack` covers)
    slack = 1e-12 * (1.0 + np.maximum(np.abs(t0), np.abs(t1)))
    ok &= t0 <= t1 + slack
    return keep[ok], t0[ok]


def culled(name, vol, d, grow=1e-6):
    """The triangles of _culled as sweep_ref shapes."""
    v = triangles(name)[0]
    return [("pts", v[k], 0.0) for k in _culled(name, vol, np.asarray(d, np.float64), grow)[0]]


def _directions(count=96):
    """Unit vectors spread over the sphere (a Fibonacci lattice) and the six axes."""
    k = np.arange(count) + 0.5
    y, phi = 1.0 - 2.0 * k / count, np.pi * (1.0 + 5.0 ** 0.5) * k
    r = np.sqrt(1.0 - y * y)
    return np.concatenate([np.stack([r * np.cos(phi), y, r * np.sin(phi)], axis=1), np.eye(3), -np.eye(3)])


_DIRECTIONS = _directions()


def cast(name, vol, d):
    """The first touch of `vol` moved along d with the terrain of map `name`: (t, unit normal from the terrain to the volume, point, initial overlap)
    or None.  The smallest sweep_ref.time_of_impact over the culled triangles, taken in the order of a lower bound of each one's time and ended
    once that bound lies behind the best time found.  The bound: along a unit direction a the volume and the triangle are g_a apart at the start
    (the volume's lowest projection less the triangle's highest) and close at the rate -a . d, so they cannot touch before g_a / -(a . d), and never
    when they are apart and do not close; the largest of that over _DIRECTIONS, -d, the normals of the touches found so far and the slab's entry
    time (the box of a wide round or tilted volume reaches a thousand triangles long before the volume does)."""
    d = np.asarray(d, np.float64)
    keep, lb = _culled(name, vol, d)
    if not len(keep):
        return None
    v = triangles(name)[0][keep]
    if len(keep) <= 300:     # few candidates: sweep_ref.cast's own order (by the slab's entry time)
        hit = S.cast(vol, d, [("pts", t, 0.0) for t in v])
        return None if hit is None else hit[1:]
    length = np.linalg.norm(d)

    def bounded(lb, a):
        gap = -(S.support(vol, -a) @ -a + S.margin(vol)) - (v @ a).max(axis=1)
        rate = -(a @ d)
        return np.maximum(lb, (gap - 1e-9) / rate) if rate > 0 else np.where(gap > 1e-9, np.inf, lb)
    for a in (_DIRECTIONS if length == 0 else np.concatenate([_DIRECTIONS, [-d / length]])):
        lb = bounded(lb, a)
    best = None
    left = np.ones(len(keep), bool)
    while left.any():
        k = int(np.argmin(np.where(left, lb, np.inf)))
        if lb[k] > 1.0 or (best is not None and lb[k] > best[0]):
            break
        left[k] = False
        hit = S.time_of_impact(vol, ("pts", v[k], 0.0), d)
        if hit is not None and (best is None or hit[0] < best[0]):
            best = hit
            if not hit[3] and np.any(hit[1] != 0):
                lb = bounded(lb, hit[1])      # (the touch's own normal: a slab's face, which no direction of the fixed set equals)
    return best


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
    near = np.flatnonzero(lb <= reach)
    if len(near) > 500:     # (a wide round volume: its box is near a thousand triangles that its flank is far from; the same bound along _DIRECTIONS)
        for a in _DIRECTIONS:
            lb[near] = np.maximum(lb[near], S.support(shape, -a) @ a - S.margin(shape) - (v[near] @ a).max(axis=1))
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
                        hulls=[R.volume_hull()], heightmap=map_of(name))


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
