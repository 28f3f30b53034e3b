"""The yardstick of the terrain contact scene query (include/mi_physics.h, mi_world_terrain_contacts), none of which needs a GPU.

A rigid body of a volume's shape, placed at the volume's pose in an oracle world that holds the heightmap, gets from ONE step of the
reference's heightmapCollision exactly the contacts the query reports for that volume: same number, same order, same bits.  The oracle
(oracle/ora_heightmap.cpp, heightmapCollision) visits the world colliders in ascending index and appends a collider's contacts one after
the other in emission order (the triangle contacts in the order of trianglesInVolume's stack walk, then the lowest point), and
ora_world_get_contacts hands the list out in that order with collider_b = 0xFFFFFFFF for the terrain: a collider's terrain contacts are
consecutive and in emission order, so they are compared as they come.  The volumes are created last to first in world-collider terms:
volume v is world collider count - 1 - v.

Also here: the two maps and the volume sets of the tests, with the boundary cases the pipeline has (stash boundary 16 / 17 contacts, the
cap of 255, cell windows of 64 and 65 cells, chunk borders, a hole, outside the map, far above it, an invalid volume), and the cell
window of a volume computed as HmVolume::window (csrc/heightmap.hpp) computes it."""
from functools import lru_cache

import numpy as np

from d3d12renderer_amd import capi, scenes

F = np.float32
TERRAIN = 0xFFFFFFFF
SEED = 9
TYPES = (capi.SPHERE, capi.CAPSULE, capi.CYLINDER, capi.AABB, capi.OBB, capi.HULL)
TRIANGLE_TYPES = (capi.SPHERE, capi.CAPSULE, capi.AABB, capi.OBB)   # the others get the lowest-point contact only


def coarse_map():
    """2 x 2 chunks of 16 m (cells of 12.4 cm), amplitude 6, chunk (1, 0) a hole."""
    return scenes.rolling_heightmap(2, 16.0, 6.0, holes=((1, 0),))


def fine_map():
    """terrain_wide_colliders' map: 2 x 2 chunks of 8 m (cells of 6.2 cm), amplitude 3."""
    return scenes.terrain_wide_colliders().heightmap


MAPS = {"coarse": coarse_map, "fine": fine_map}


def terrain_scene(hm, entities=None, collider_entities=None, colliders=None):
    """A scene of the heightmap, the one hull geometry the hull volumes use, and the given entities (none: the query's world)."""
    e = scenes.make_entities(0) if entities is None else entities
    ce = np.zeros(0, np.uint32) if collider_entities is None else collider_entities
    c = scenes.make_colliders(0, capi.SPHERE) if colliders is None else colliders
    return scenes.Scene("terrain_query", e, ce, c, 10, hulls=[scenes.convex_hull_mesh(SEED)], heightmap=hm)


def volume_bodies(vols):
    """The volumes as dynamic entities with one collider each (an invalid volume: a small sphere far outside every map)."""
    vols = substitute_invalid(vols)
    n = len(vols)
    e = scenes.make_entities(n, capi.ENTITY_DYNAMIC)
    e["position"] = vols["position"]; e["rotation"] = vols["rotation"]
    c = scenes.make_colliders(n, capi.SPHERE)
    c["type"] = vols["type"]; c["shape"] = vols["shape"]; c["hull_geometry"] = vols["hull_geometry"]
    return e, np.arange(n, dtype=np.uint32), c


def is_invalid(vols):
    """The invalid volumes of the sets below: a negative radius (the only kind they use)."""
    return (vols["type"] == capi.SPHERE) & (vols["shape"][:, 3] < 0)


def substitute_invalid(vols):
    out = vols.copy()
    bad = is_invalid(out)
    out["shape"][bad, :4] = (0, 0, 0, 0.1); out["position"][bad] = (500.0, 500.0, 500.0)
    return out


# ---- the oracle
def oracle_terrain_contacts(oracle_mod, hm, vols):
    """One step of an oracle world (ORDER_REFERENCE) holding the heightmap and one dynamic entity per volume.  Returns (offsets, records,
    boxes): the expected result of the query in its own layout, and the world AABB of every volume ([count][6], what the step tested with)."""
    count = len(vols)
    sc = terrain_scene(hm, *volume_bodies(vols))
    w = sc.populate(oracle_mod.create_world(oracle_mod.ORDER_REFERENCE))
    w.step_fixed(sc.settings(), sc.dt, 1)
    contacts = w.contacts(); boxes = np.asarray(w.aabbs(), F).reshape(-1, 6)
    w.close()
    assert len(boxes) == count
    t = contacts[contacts["collider_b"] == TERRAIN]
    a = t["collider_a"].astype(np.int64)
    # consecutive per collider (a collider's group appears once), colliders ascending: the list order is the emission order
    assert len(a) == 0 or (np.diff(a) >= 0).all(), "the oracle's terrain contacts are not grouped by ascending collider"
    per_volume = np.bincount(count - 1 - a, minlength=count) if len(a) else np.zeros(count, np.int64)
    assert not per_volume[is_invalid(vols)].any()
    offsets = np.concatenate([[0], np.cumsum(per_volume)]).astype(np.uint32)
    recs = np.zeros(len(t), capi.terrain_contact_dtype)
    # collider ascending = volume descending: place every group at its volume's segment, keeping the order inside the group
    starts = offsets[:-1].astype(np.int64)
    pos = 0
    for col in np.unique(a):
        v = count - 1 - int(col); n = int(per_volume[v])
        g = t[pos:pos + n]; pos += n
        seg = recs[starts[v]:starts[v] + n]
        seg["point"] = g["point"]; seg["depth"] = g["penetration_depth"]; seg["normal"] = g["normal"]; seg["volume"] = v
    return offsets, recs, boxes[::-1].copy()


def differences(offsets, recs, want_offsets, want_recs, limit=8):
    """Compares in list order with no tolerance: the per-volume counts, then the bytes of every record."""
    problems = []
    if offsets.tobytes() != want_offsets.tobytes():
        got_n = np.diff(offsets.astype(np.int64)); want_n = np.diff(want_offsets.astype(np.int64))
        bad = np.flatnonzero(got_n != want_n)
        problems.append(f"{len(bad)} volumes with another number of contacts (volume, got, oracle): {[(int(v), int(got_n[v]), int(want_n[v])) for v in bad[:limit]]}")
        return problems
    if recs.tobytes() != want_recs.tobytes():
        bad = [i for i in range(len(recs)) if recs[i].tobytes() != want_recs[i].tobytes()]
        problems.append(f"{len(bad)} of {len(recs)} records differ; first {bad[:limit]}: got {recs[bad[:2]]}, oracle {want_recs[bad[:2]]}")
    return problems


# ---- the cell window, as HmVolume (csrc/heightmap.hpp) computes it: float32 throughout
def _u32(f):
    return int(np.int64(np.trunc(F(f)))) & 0xFFFFFFFF


def chunk_windows(hm, box):
    """[(chunk x, chunk z, cells)] of one world AABB (mn xyz, mx xyz) over the chunks its range touches (holes included; a window that is
    empty after clamping counts 0 cells)."""
    corner = np.asarray(hm["min_corner"], F); cpd = int(hm["chunks_per_dim"])
    inv = F(1.0) / F(hm["chunk_size"])
    box = np.asarray(box, F)
    vmin = box[:3] - corner; vmax = box[3:] + np.asarray((0, 10, 0), F) - corner
    vmin_x, vmin_z, vmax_x, vmax_z = F(vmin[0] * inv), F(vmin[2] * inv), F(vmax[0] * inv), F(vmax[2] * inv)
    lo_x, lo_z = max(int(vmin_x), 0), max(int(vmin_z), 0)
    hi_x, hi_z = min(max(int(vmax_x), 0), cpd - 1), min(max(int(vmax_z), 0), cpd - 1)
    out = []
    for z in range(lo_z, hi_z + 1):
        for x in range(lo_x, hi_x + 1):
            def span(mn, mx, c):
                rel_min = max(F(mn - F(c)), F(0)); rel_max = F(1) if mx > F(c + 1) else F(np.fmod(mx, F(1)))
                return _u32(rel_min * F(129)), min(_u32(rel_max * F(129)), 127)
            x0, x1 = span(vmin_x, vmax_x, x); z0, z1 = span(vmin_z, vmax_z, z)
            out.append((x, z, (x1 - x0 + 1) * (z1 - z0 + 1) if x0 <= x1 and z0 <= z1 else 0))
    return out


def largest_window(hm, box):
    return max([c for _, _, c in chunk_windows(hm, box)], default=0)


# ---- heights without a world: the bilinear surface of heightmap_collider_chunk::getHeightAt, good enough to PLACE volumes (float64)
def height_fn(hm):
    cpd = int(hm["chunks_per_dim"]); size = float(hm["chunk_size"]); corner = np.asarray(hm["min_corner"], np.float64); scale = float(hm["amplitude"]) / 65535.0

    def height(x, z):
        cx, cz = (x - corner[0]) / size, (z - corner[2]) / size
        if cx < 0 or cz < 0 or cx >= cpd or cz >= cpd or (int(cx), int(cz)) not in hm["chunks"]:
            return None
        h = hm["chunks"][(int(cx), int(cz))].astype(np.float64) * scale
        fx, fz = (cx % 1.0) * 128, (cz % 1.0) * 128
        ix, iz = int(fx), int(fz); rx, rz = fx - ix, fz - iz
        top = h[iz, ix] * (1 - rx) + h[iz, ix + 1] * rx; bottom = h[iz + 1, ix] * (1 - rx) + h[iz + 1, ix + 1] * rx
        return top * (1 - rz) + bottom * rz + corner[1]
    return height


# ---- the volume sets
def _shaped(ctype, s, position, rotation):
    """A volume of type `ctype` and size s about its own origin, at a pose."""
    if ctype == capi.SPHERE: shape = (0, 0, 0, s)
    elif ctype in (capi.CAPSULE, capi.CYLINDER): shape = (0, -s, 0, 0, s, 0, 0.5 * s)
    elif ctype == capi.AABB: shape = (-s, -0.6 * s, -0.8 * s, s, 0.6 * s, 0.8 * s)
    elif ctype == capi.OBB: shape = (0, 0, 0, 1, 0, 0, 0, s, 0.6 * s, 0.8 * s)
    else: return capi.hull_volume(0, position, rotation)
    return capi.make_volume(ctype, shape, position, rotation)


def random_volumes(hm, seed, per_type, sizes):
    """per_type volumes of every type at random places of the map (holes too), resting on or sunk into the surface by a fraction of their size,
    with random rotations (every second AABB stays axis-aligned; the others become OBBs in the world)."""
    rng = np.random.default_rng(seed)
    height = height_fn(hm)
    half = hm["chunks_per_dim"] * hm["chunk_size"] / 2
    cx, cz = float(hm["min_corner"][0]) + half, float(hm["min_corner"][2]) + half
    out = []
    for t in TYPES:
        for k in range(per_type):
            x, z = rng.uniform(-0.98 * half, 0.98 * half, 2) + (cx, cz)
            s = float(np.exp(rng.uniform(np.log(sizes[0]), np.log(sizes[1]))))
            q = rng.normal(size=4); q /= np.linalg.norm(q)
            if t == capi.AABB and k % 2 == 0:
                q = np.array((0, 0, 0, 1.0))
            h = height(x, z)
            y = (2.0 if h is None else h) + s * rng.uniform(0.1, 0.9)
            out.append(_shaped(t, 1.0 if t == capi.HULL else s, (x, y, z), q))
    return np.concatenate(out)


SIZES = {"coarse": (0.15, 0.9), "fine": (0.08, 0.5)}
WINDOW_BOX_AT = (1.3, 2.1)                                  # on the fine map; half extents found by scanning chunk_windows
WINDOW_BOXES = {64: (0.1, 0.444), 65: (0.122, 0.364)}       # cell windows of 8 x 8 and 5 x 13 cells: the plain / large-window boundary


def boundary_volumes(name, hm):
    """(volumes, {label: index into them}) — the cases a random set need not hold."""
    height = height_fn(hm)
    labelled = []

    def add(label, v):
        labelled.append((label, v))
    half = hm["chunks_per_dim"] * hm["chunk_size"] / 2
    q = 0.25 * half
    add("two chunks", capi.sphere_volume((0.0, height(-0.01, q) + 0.15, q), 0.3))                 # the border x = 0 between chunks (0, 1) and (1, 1)
    add("four chunks", capi.box_volume((0.0, height(-0.01, 0.01), 0.0), (0.25, 0.2, 0.2)))         # the map's centre (coarse map: one of the four is the hole)
    add("outside", capi.sphere_volume((3.0 * half, 2.0, 0.0), 0.5))
    add("above", capi.sphere_volume((q, height(q, q) + 12.0, q), 0.5))
    add("invalid", capi.sphere_volume((q, height(q, q), q), -1.0))
    if name == "coarse":
        add("hole", capi.sphere_volume((0.5 * half, 2.0, -0.5 * half), 0.5))
        add("hole box", capi.box_volume((0.5 * half, 1.5, -0.5 * half), (1.0, 1.0, 1.0)))
    else:
        add("cap", capi.box_volume((-0.5 * half, height(-0.5 * half, -0.5 * half), -0.5 * half), (1.5, 0.1, 1.5)))   # a flat 3 m box: thousands of triangles
        x, z = WINDOW_BOX_AT
        for cells, (hx, hz) in WINDOW_BOXES.items():
            add(f"window {cells}", capi.box_volume((x, height(x, z) + 0.05, z), (hx, 0.05, hz)))
    return np.concatenate([v for _, v in labelled]), {label: i for i, (label, _) in enumerate(labelled)}


@lru_cache(maxsize=None)
def volume_set(name):
    """(heightmap, volumes, labels): 40 random volumes of every type and the boundary cases of the map (labels: index of each case)."""
    hm = MAPS[name]()
    rnd = random_volumes(hm, 3, 40, SIZES[name])
    edge, labels = boundary_volumes(name, hm)
    vols = np.concatenate([rnd, edge])
    vols.setflags(write=False)
    return hm, vols, {k: len(rnd) + i for k, i in labels.items()}


_EXPECTED = {}


def expected(oracle_mod, name):
    """The oracle's (offsets, records, boxes) of volume_set(name): computed once, shared, read-only."""
    if name not in _EXPECTED:
        hm, vols, _ = volume_set(name)
        out = oracle_terrain_contacts(oracle_mod, hm, vols)
        for a in out:
            a.setflags(write=False)
        _EXPECTED[name] = out
    return _EXPECTED[name]


def flat_heightmap():
    """The facade program's terrain: one chunk of 16 m, every height 32768, amplitude 4, corner at the origin."""
    return dict(chunks_per_dim=1, chunk_size=16.0, restitution=0.05, friction=0.8, min_corner=np.zeros(3, np.float32), amplitude=4.0,
                chunks={(0, 0): np.full((129, 129), 32768, np.uint16)})


def sunk_sphere_case():
    """The facade program's volumes: a sphere of radius 0.5 above the plane and one sunk 0.1 into it."""
    return flat_heightmap(), np.concatenate([capi.sphere_volume((3.3, 2.6, 4.7), 0.5), capi.sphere_volume((3.3, 2.4, 4.7), 0.5)])
