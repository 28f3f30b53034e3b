"""Float64 yardstick of the terrain distance queries (include/mi_physics.h, mi_world_terrain_distance); numpy only, no GPU.

The reference distance of a volume is sweep_terrain_ref.min_gap(map, sweep_ref.volume_convex(volume, hulls), reach): the smallest gap to the
collision triangles of raycast_ref.terrain_triangles, two-sided surfaces without volume.  Neighbouring triangles share edges and vertices, so
nothing here (and no test) says WHICH triangle is the nearest.

Also here: the comparison set of the GPU test, built from the reference's own answers (a volume is lowered by its measured gap, not by an assumed
height of the map), with what makes it a valid yardstick (tests/test_terrain_distance.py asserts it)."""
from pathlib import Path

import numpy as np

import overlap_ref as R
import sweep_ref as S
import sweep_terrain_ref as ST
from d3d12renderer_amd import capi

TERRAIN = 0xFFFFFFFE   # capi.RAY_TERRAIN
MISS = 0xFFFFFFFF
# The bound of the GPU comparison per unit of scale (scale = max(1, the largest |coordinate| of the volume's bounds grown by its distance)): 4 x the
# largest value measured on the MI355X (1.41e-6, a cylinder's distance; tests/test_gpu_terrain_distance.py states the figures), rounded up to one digit.
BOUND = 6e-6
SEED = 7
MAP = "rolling"
GROUPS = ("above", "below", "cutting", "beside", "hole", "short", "beyond", "near")   # (six volumes each; "near" fills the 48: a second "above", centimetres off the surface)
# what the set keeps every decision clear of flipping by: a hit / miss by the largest distance, a gap that is no overlap, and how far an
# overlapping volume may move along y and still overlap
DECISION_MARGIN, GAP_MARGIN, OVERLAP_MARGIN = 1e-2, 1e-2, 1e-3


def distance(name, vconv, reach=np.inf):
    """The reference distance of a convex volume from the terrain of map `name`: 0 or below (as far as the margin reaches) = touching."""
    return ST.min_gap(name, vconv, reach)


def scale_of(vconv, dist):
    mn, mx = S.bounds(vconv)
    grow = dist if np.isfinite(dist) and dist > 0 else 0.0
    return max(1.0, float(np.abs(np.concatenate([mn - grow, mx + grow])).max()))


def _moved(v, dy):
    w = v.copy()
    w["position"][1] += dy
    return w


def comparison_volumes(seed=SEED):
    """48 volumes on the rolling map (2 x 2 chunks of 32 m, x and z in [-32, 32], heights in [0, 6], chunk (1, 0): x > 0, z < 0 a hole), volume i of
    type i % 6 and group GROUPS[i // 6]: above the hills; wholly below the surface; cutting the surface (near the origin: the overlap margin is the
    smallest, so the coordinates are); beside the map, up to a few metres outside; over and inside the hole, the nearest triangle on its rim; above with
    a largest distance 1e-2 short of the reference distance (a miss) and 1e-2 beyond it (a hit); near the surface, a few centimetres above it.
    (volumes, largest distances float32 [48], reference distances float64 [48] of the volumes as placed)."""
    hulls = [R.volume_hull()]
    vols = R.make_volumes(seed, 8, (-1, -1, -1), (1, 1, 1), 0.15, 1.0)
    rng = np.random.default_rng(seed + 3000)
    n = len(vols)
    max_d = np.full(n, np.inf, np.float32)
    ref = np.zeros(n)

    def gap_of(v):
        return distance(MAP, S.volume_convex(v, hulls))
    for i in range(n):
        g = GROUPS[i // 6]
        v = vols[i:i + 1]
        if g in ("above", "short", "beyond"):
            v["position"][0] = (rng.uniform(-27, 27), rng.uniform(7.6, 8.4), rng.uniform(-27, 27))
        elif g == "near":      # (not over the hole: its rim is not reached by going down)
            v["position"][0] = (rng.uniform(-27, -2), rng.uniform(7.6, 8.4), rng.uniform(-27, 27))
        elif g == "below":
            v["position"][0] = (rng.uniform(-27, 27), rng.uniform(-4.0, -2.0), rng.uniform(-27, 27))
        elif g == "cutting":
            v["position"][0] = (rng.uniform(-4, -1), 8.0, rng.uniform(-4, 4))
        elif g == "beside":
            out, along = 32.0 + rng.uniform(0.5, 3.0), rng.uniform(-25, 25)
            side = int(rng.integers(4))   # -x, +z, the corner (-x, +z), the corner (-x, -z): the rims that have heights
            x, z = ((-out, along), (-abs(along), out), (-out, out), (-out, -out))[side]
            v["position"][0] = (x, rng.uniform(0.0, 7.0), z)
        else:   # the hole: x in (0, 32), z in (-32, 0); 0.5 to 3 from one of its two inner rims
            off, along = rng.uniform(0.5, 3.0), rng.uniform(4, 28)
            x, z = (off, -along) if i % 2 else (along, -off)
            v["position"][0] = (x, rng.uniform(-1.0, 7.0), z)
        d = gap_of(v[0])
        if g == "cutting":     # down by the gap and a little more until it cuts: the gap is no larger than the clearance along y
            for _ in range(8):
                if d <= 0:
                    break
                v["position"][0][1] -= np.float32(d + 0.05)
                d = gap_of(v[0])
        elif g == "near":      # down by the gap less 5 cm: at least that far along y, so a few centimetres off the surface
            v["position"][0][1] -= np.float32(d - 0.05)
            d = gap_of(v[0])
        elif g == "short":     # (rounded away from the distance: the margin holds in float32)
            max_d[i] = np.nextafter(np.float32(d - DECISION_MARGIN), np.float32(-np.inf))
        elif g == "beyond":
            max_d[i] = np.nextafter(np.float32(d + DECISION_MARGIN), np.float32(np.inf))
        ref[i] = d
    return vols, max_d, ref


_COMPARISON = {}
GOLDEN = Path(__file__).resolve().parent / "golden" / "terrain_distance_set.npz"


def comparison_reference(seed=SEED, recompute=False):
    """The comparison set against the rolling map, once per process and left unchanged: the scene, the volumes, their largest distances, their
    convex shapes, the reference distance of each, what the record must be ("hit", "miss", "overlap") and the scale.  The volumes and their
    reference distances take a minute to compute (comparison_volumes), so they are kept in tests/golden/terrain_distance_set.npz (written by
    `python tests/terrain_distance_ref.py`); recompute = True computes them here, and tests/test_terrain_distance.py holds the file to that."""
    key = (seed, recompute)
    if key not in _COMPARISON:
        sc = ST.scene(MAP)
        if recompute:
            vols, max_d, ref = comparison_volumes(seed)
        else:
            with np.load(GOLDEN) as z:
                assert int(z["seed"]) == seed
                vols = np.frombuffer(z["volumes"].tobytes(), capi.query_volume_dtype).copy(); max_d = z["max_distances"].copy(); ref = z["ref"].copy()
        convs = [S.volume_convex(v, sc.hulls) for v in vols]
        expect = ["overlap" if d <= 0 else "hit" if d <= m else "miss" for d, m in zip(ref, max_d.astype(np.float64))]
        scales = [scale_of(c, d) for c, d in zip(convs, ref)]
        for a in (vols, max_d, ref):
            a.setflags(write=False)
        _COMPARISON[key] = dict(scene=sc, volumes=vols, max_distances=max_d, convex=convs, ref=ref, expect=expect, scales=scales,
                                groups=[GROUPS[i // 6] for i in range(len(vols))])
    return _COMPARISON[key]


def overlap_holds(c, i):
    """Volume i of the set (an overlapping one) still overlaps in the reference when moved by +-OVERLAP_MARGIN along y."""
    return all(distance(MAP, S.volume_convex(_moved(c["volumes"][i], dy), c["scene"].hulls), 1.0) <= 0 for dy in (-OVERLAP_MARGIN, OVERLAP_MARGIN))


if __name__ == "__main__":
    c = comparison_reference(recompute=True)
    np.savez(GOLDEN, seed=np.int64(SEED), volumes=np.frombuffer(c["volumes"].tobytes(), np.uint8), max_distances=c["max_distances"], ref=c["ref"])
    print(f"wrote {GOLDEN}: {len(c['volumes'])} volumes, {c['expect'].count('overlap')} overlapping, {c['expect'].count('miss')} misses")
