"""The test matrix of the terrain contact pipeline (csrc/heightmap.hpp: k_hm_lowest, k_hm_contacts<WRITE, LARGE>, k_hm_write_stashed; its two users are the
step's terrain narrow phase and mi_world_terrain_contacts): the placements at which a cell window, a stash or a cap goes wrong.  numpy and the oracle, no GPU.
tests/test_terrain_contact_matrix.py holds the oracle to the reference's own heightmapCollision on every case and checks the matrix's coverage,
tests/test_gpu_terrain_contact_matrix.py runs it on the GPU, bit for bit against the oracle.  Built the way tests/contact_matrix.py and
tests/sweep_terrain_matrix.py are:

  * a CASE is one map (MAPS), one volume, a family and a tag; a volume is posed in float64 and rounded to float32 once (capi.make_volume);
  * the yardstick is terrain_contact_ref.oracle_terrain_contacts: the volumes as rigid bodies of an oracle world, one step in the reference's order;
  * the maps are generated here: the rolling, offset, floor, flat and tilted maps of the terrain ray and shape cast matrices, the coarse and fine
    maps of terrain_contact_ref, the wide 5 x 5 map, and new ones: `exact` (a power-of-two chunk size and corner: chunk seams and edges are exact
    in float32), `plateau` (every height 65 535 counts), `ripple` (amplitude 1e-3) and `many256` / `many257` (256 and 257 chunks per dimension of
    which only the four around the highest indices of each have heights; both share the corner and the chunk (255, 255)).

A cylinder or hull volume gets the lowest-point contact only (a stated deviation: the reference reads an uninitialised point there); `lowest_point`
is its float64 yardstick and BOUNDS what the oracle may differ from it."""
import numpy as np

import overlap_matrix as OM
import raycast_terrain_matrix as RT
import sweep_terrain_ref as ST
import terrain_contact_ref as T
from d3d12renderer_amd import capi, scenes

FAMILIES = ("features", "rim", "seam_exact", "windows", "maps", "many_chunks", "size", "height_range")
TYPES = T.TYPES
NAMES = {capi.SPHERE: "sphere", capi.CAPSULE: "capsule", capi.CYLINDER: "cylinder", capi.AABB: "AABB", capi.OBB: "OBB", capi.HULL: "hull"}
LOWEST_ONLY = (capi.CYLINDER, capi.HULL)
# The families whose text names the volume types they hold (the others hold all six; the one hull geometry of the worlds has one size)
FAMILY_TYPES = {"seam_exact": (capi.AABB, capi.SPHERE), "windows": (capi.AABB,), "many_chunks": T.TRIANGLE_TYPES,
                "size": (capi.SPHERE, capi.CAPSULE, capi.CYLINDER, capi.AABB, capi.OBB)}
MIN_WITH = MIN_WITHOUT = 3              # THE CAP, per (family, type the family applies to); 1 for the families of LOOSE
LOOSE = ("many_chunks", "size")
STASH, CAP = 16, 255                    # kHmStash, kHmMaxContacts (csrc/heightmap.hpp)
# The lowest-point contact of cylinders and hulls against float64 (lowest_point below), PER UNIT OF scale = max(1, the largest |coordinate| of the
# point): 4 x the largest error measured on the oracle, on the CPU, rounded up to one digit.  Measured over the 238 single-contact cylinder and
# hull cases of the matrix (tests/test_terrain_contact_matrix.py prints them): point 7.15e-8 (maps: the shallow cylinder on the tilted map),
# depth 6.85e-8 (features: the upright hull sunk 0.06 at the four-chunk corner of the rolling map); about one float32 rounding of a coordinate
# each.  The depth is compared with the float64 height over the oracle's own point.  The GPU gets no tolerance: it equals the oracle's bytes.
MEASURED = {"point": 7.15e-8, "depth": 6.85e-8}
BOUNDS = {"point": 3e-7, "depth": 3e-7}
HULL_SIZE = 0.6                         # scenes.convex_hull_mesh's radius: the `size` of the hull volume
F32 = np.float32


# ---- maps
def exact_map():
    """2 x 2 chunks of 16 m, corner (32, 0, -64): the edges x = 32, 64 and z = -64, -32 and the seams x = 48, z = -48 are float32 numbers, and so
    is every bound of a volume divided by the chunk size."""
    return scenes.rolling_heightmap(2, 16.0, 4.0, seed=5, min_corner=(32.0, 0.0, -64.0))


def plateau_map():
    hm = T.flat_heightmap()
    hm["chunks"] = {(0, 0): np.full((129, 129), 65535, np.uint16)}
    return hm


def ripple_map():
    return scenes.rolling_heightmap(1, 16.0, 1e-3, seed=6, min_corner=(0.0, 1.0, 0.0))


MANY_CORNER = (-4080.0, 0.0, -4080.0)   # 255 chunks of 16 m: chunk (255, 255) is [0, 16] x [0, 16]


def many_map(cpd):
    """cpd chunks of 16 m per dimension, heights in the four chunks (cpd - 2 .. cpd - 1)^2 only: cut from one 3 x 3 field over the chunks 254 .. 256,
    so the 256 and the 257 map hold the same chunk (255, 255) at the same place."""
    field = scenes.rolling_heightmap(3, 16.0, 5.0, seed=11)["chunks"]
    chunks = {(x, z): field[(x - 254, z - 254)] for x in (cpd - 2, cpd - 1) for z in (cpd - 2, cpd - 1)}
    return dict(chunks_per_dim=cpd, chunk_size=16.0, restitution=0.05, friction=0.8, min_corner=np.array(MANY_CORNER, F32), amplitude=5.0, chunks=chunks)


MAPS = dict(RT.MAPS, coarse=T.coarse_map, fine=T.fine_map, wide=ST.wide_map, exact=exact_map, plateau=plateau_map, ripple=ripple_map,
            many256=lambda: many_map(256), many257=lambda: many_map(257))
_MAPS = {}


def the_map(name):
    if name not in _MAPS:
        _MAPS[name] = MAPS[name]()
    return _MAPS[name]


def extent(hm):
    """(x0, z0, x1, z1, cell) of a map in float64."""
    c = np.asarray(hm["min_corner"], np.float64); side = hm["chunks_per_dim"] * float(hm["chunk_size"])
    return c[0], c[2], c[0] + side, c[2] + side, float(hm["chunk_size"]) / 128.0


def near_height(hm, x, z):
    """The bilinear surface's height at the point of solid ground nearest to (x, z): the point clamped into the map and, on the rim of a chunk
    without heights, taken a step into a neighbour that has them.  Over the inside of such a chunk: 2 above the corner."""
    x0, z0, x1, z1, cell = extent(hm)
    e = 1e-6 * cell
    x, z = min(max(x, x0 + e), x1 - e), min(max(z, z0 + e), z1 - e)
    height = T.height_fn(hm)
    for dx, dz in ((0, 0), (-e, 0), (e, 0), (0, -e), (0, e), (-e, -e), (-e, e), (e, -e), (e, e)):
        h = height(x + 2 * dx, z + 2 * dz)
        if h is not None:
            return h
    return float(hm["min_corner"][1]) + 2.0


def top_height(hm, x, z, reach):
    """The highest near_height over the square of half side `reach` about (x, z), sampled at a third of a cell."""
    cell = extent(hm)[4]
    n = int(np.ceil(2 * reach / (cell / 3.0))) + 1
    n = min(n, 41)
    return max(near_height(hm, x + a, z + b) for a in np.linspace(-reach, reach, n) for b in np.linspace(-reach, reach, n))


# ---- the float64 side: support points of a volume record
def _rotate(q, v):
    u, w = q[:3], q[3]
    return v + 2.0 * np.cross(u, np.cross(u, v) + w * v)


_HULL = None


def hull_vertices():
    global _HULL
    if _HULL is None:
        _HULL = scenes.convex_hull_mesh(T.SEED)[0].astype(np.float64)
    return _HULL


def support64(v, d):
    """(support point of the volume record v along the unit vector d in float64, whether it is the only one).  A cylinder whose axis lies along d has
    a whole cap of them: the cap's centre stands for it."""
    t = int(v["type"]); s = v["shape"].astype(np.float64); p = v["position"].astype(np.float64); q = v["rotation"].astype(np.float64)
    d = np.asarray(d, np.float64)
    world = lambda a: _rotate(q, np.asarray(a, np.float64)) + p   # noqa: E731
    if t == capi.SPHERE:
        return world(s[:3]) + s[3] * d, True
    if t in (capi.CAPSULE, capi.CYLINDER):
        a, b = world(s[0:3]), world(s[3:6])
        far = a if a @ d > b @ d else b
        if t == capi.CAPSULE:
            return far + s[6] * d, True
        n = a - b
        side = np.cross(np.cross(n, d), n)
        ln = np.linalg.norm(side)
        # (the reference's cylinder support normalises `side` with noz, which gives 0 below a length of 1e-4: for an axis along d, and for any
        # cylinder whose squared length times the sine of its angle to d is less: a cylinder shorter than 1 cm has its lowest point at its axis' end)
        if ln < 1e-4 or ln <= 1e-5 * (n @ n):
            return far, False
        return far + s[6] * side / ln, True
    if t == capi.HULL:
        pts = np.array([world(x) for x in hull_vertices()])
    else:
        signs = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], np.float64)
        if t == capi.AABB:
            c, h = (s[0:3] + s[3:6]) / 2, (s[3:6] - s[0:3]) / 2
            pts = np.array([world(c + k * h) for k in signs])
        else:
            lq = s[0:4]
            pts = np.array([world(s[4:7] + _rotate(lq, k * s[7:10])) for k in signs])
    along = pts @ d
    k = int(np.argmax(along))
    return pts[k], bool(np.sum(along >= along[k] - 1e-6) == 1)


def bounds64(v):
    """(lower, upper) bounds of the volume record in float64."""
    return np.array([support64(v, -np.eye(3)[k])[0][k] for k in range(3)]), np.array([support64(v, np.eye(3)[k])[0][k] for k in range(3)])


def lowest_point(hm, v):
    """The float64 yardstick of the lowest-point contact: (the support point along -y, whether it is unique)."""
    return support64(v, (0.0, -1.0, 0.0))


def height64(hm, x, z):
    """The bilinear surface at the float64 place (x, z), or None off the map and over a chunk without heights."""
    return T.height_fn(hm)(float(x), float(z))


# ---- volumes and cases
I4 = np.array((0.0, 0.0, 0.0, 1.0))
YAW45 = scenes.q_axis_angle((0, 1, 0), np.pi / 4)


def _rng(*key):
    return np.random.default_rng(list(key))


def _rand_q(rng):
    q = rng.normal(size=4)
    return q / np.linalg.norm(q)


def vertex_down():
    if OM._VERTEX_DOWN is None:
        OM._feature_shapes(OM.R.SPHERE, True)
    return OM._VERTEX_DOWN


def size_of(t, s):
    return HULL_SIZE if t == capi.HULL else s


def shaped(t, s, position, q=I4, capsule_axis=None):
    """terrain_contact_ref._shaped; capsule_axis: a capsule or cylinder whose segment lies along that unit vector in its own frame, not along y."""
    if capsule_axis is not None and t in (capi.CAPSULE, capi.CYLINDER):
        u = np.asarray(capsule_axis, np.float64) * s
        return capi.make_volume(t, (*(-u), *u, 0.5 * s), position, q)
    return T._shaped(t, s, position, q)


def posed(hm, t, s, x, z, q, pose, amount=None, **kw):
    """The volume with the centre of its position over (x, z): `shallow` (the lowest point 0.1 of the size under the nearest ground), `deep` (the
    position a quarter of the size under it), `clear` (the lowest point 0.1 of the size over the highest ground under its bounds), `lift` (the lowest
    point `amount` over that highest ground) or `under` (the highest point `amount` under the lowest ground under its bounds)."""
    v0 = shaped(t, s, (0.0, 0.0, 0.0), q, **kw)[0]
    mn, mx = bounds64(v0)
    size = size_of(t, s)
    reach = max(mx[0], -mn[0], mx[2], -mn[2])
    if pose == "shallow":
        y = near_height(hm, x, z) - 0.1 * size - mn[1]
    elif pose == "deep":
        y = near_height(hm, x, z) - 0.25 * size
    elif pose in ("clear", "lift"):
        y = top_height(hm, x, z, reach) + (0.1 * size if pose == "clear" else amount) - mn[1]
    else:
        cell = extent(hm)[4]
        n = min(int(np.ceil(2 * reach / (cell / 3.0))) + 1, 41)
        low = min(near_height(hm, x + a, z + b) for a in np.linspace(-reach, reach, n) for b in np.linspace(-reach, reach, n))
        y = low - amount - mx[1]
    return shaped(t, s, (x, y, z), q, **kw)


def case(family, tag, mapname, volume, **extra):
    c = dict(family=family, tag=tag, map=mapname, volume=volume, vt=int(volume["type"][0]))
    c.update(extra)
    return c


# ---- features: the anchors of the grid, shallow and deep, under three rotations and the named poses of boxes and capsules
ANCHORS = ("vertex", "xline", "zline", "diagonal", "centre", "seam_x", "seam_z", "corner4", "hole_rim")


def anchor(hm, kind, k=0):
    """(x, z) of a feature of a 2 x 2 map whose chunk (1, 0) is a hole."""
    x0, z0, x1, z1, cell = extent(hm)
    n = 128
    gx, gz = 37 + 5 * k, n + 41 + 3 * k          # a cell of chunk (0, 1)
    u, v = {"vertex": (gx, gz), "xline": (gx + 0.5, gz), "zline": (gx, gz + 0.5), "diagonal": (gx + 0.5, gz + 0.5), "centre": (gx + 0.3, gz + 0.4),
            "seam_x": (n, n + 50.3), "seam_z": (50.3, n), "corner4": (n, n), "hole_rim": (n, 0.27 * n)}[kind]
    return x0 + u * cell, z0 + v * cell


def features():
    out = []
    for name in ("rolling", "offset"):
        hm = the_map(name)
        s = 2.4 * extent(hm)[4]                   # 0.6: a few cells across
        for a, kind in enumerate(ANCHORS):
            x, z = anchor(hm, kind)
            for pose in ("shallow", "deep"):
                for t in TYPES:
                    rots = [("id", I4), ("yaw45", YAW45), ("random", _rand_q(_rng(5100, a, t, len(pose))))]
                    for rtag, q in rots:
                        out.append(case("features", f"{kind}_{pose}_{rtag}_{NAMES[t]}", name, posed(hm, t, s, x, z, q, pose)))
                for t in (capi.AABB, capi.OBB):
                    out.append(case("features", f"{kind}_{pose}_vertexdown_{NAMES[t]}", name, posed(hm, t, s, x, z, vertex_down(), pose)))
                for atag, axis in (("along_x", (1.0, 0.0, 0.0)), ("along_diagonal", (np.sqrt(0.5), 0.0, np.sqrt(0.5)))):
                    out.append(case("features", f"{kind}_{pose}_{atag}_capsule", name, posed(hm, capi.CAPSULE, s, x, z, I4, pose, capsule_axis=axis)))
            for t in TYPES:                       # (and clear of the ground: the family's volumes without contacts)
                out.append(case("features", f"{kind}_clear_{NAMES[t]}", name, posed(hm, t, s, x, z, YAW45, "clear")))
    return out


# ---- rim: the map's four edges and four corners, straddled and from outside
RIM_SPOTS = (("x_low", -1, 0), ("x_high", 1, 0), ("z_low", 0, -1), ("z_high", 0, 1), ("low_low", -1, -1), ("high_low", 1, -1), ("low_high", -1, 1),
             ("high_high", 1, 1))


def rim():
    out = []
    for name in ("coarse", "offset"):
        hm = the_map(name)
        x0, z0, x1, z1, cell = extent(hm)
        s = 0.3 if name == "coarse" else 0.5
        for spot, sx, sz in RIM_SPOTS:
            # along an edge: 0.3 of the way, 0.7 on the high x edge (the hole chunk (1, 0) lies at high x, low z)
            ex = x0 if sx < 0 else x1 if sx > 0 else x0 + 0.3 * (x1 - x0)
            ez = z0 if sz < 0 else z1 if sz > 0 else z0 + (0.7 if sx > 0 else 0.3) * (z1 - z0)
            for t in TYPES:
                q = I4 if t not in (capi.OBB, capi.HULL) else _rand_q(_rng(5200, t))
                mn, mx = bounds64(shaped(t, s, (0.0, 0.0, 0.0), q)[0])
                r = size_of(t, s) * (0.5 if t != capi.SPHERE else 1.0)
                for place, gap in (("straddle", None), ("near", 0.67 * r), ("far", 1.5 * r)):
                    # the gap between the volume's bounds and the edge: the centre `gap` + its half width outside
                    off_x = 0.0 if gap is None or sx == 0 else sx * (gap + (mx[0] if sx < 0 else -mn[0]))
                    off_z = 0.0 if gap is None or sz == 0 else sz * (gap + (mx[2] if sz < 0 else -mn[2]))
                    v = posed(hm, t, s, ex + off_x, ez + off_z, q, "shallow")
                    out.append(case("rim", f"{spot}_{place}_{NAMES[t]}", name, v, spot=spot, place=place))
    return out


# ---- seam_exact: a bound of an axis-aligned box or sphere exactly on a seam or an edge, and one ulp to either side
def _ulp(x, k):
    return float(np.nextafter(F32(x), F32(np.inf if k > 0 else -np.inf))) if k else float(F32(x))


def seam_exact():
    hm = the_map("exact")
    x0, z0, x1, z1, cell = extent(hm)
    lines = {"x": (("low", x0), ("seam", (x0 + x1) / 2), ("high", x1)), "z": (("low", z0), ("seam", (z0 + z1) / 2), ("high", z1))}
    half, r = 0.375, 0.5                       # the box's half width and the sphere's radius: float32 numbers
    out = []
    for axis in ("x", "z"):
        for which in ("min", "max"):
            for ltag, line in lines[axis]:
                for k in (-1, 0, 1):
                    bound = _ulp(line, k)
                    # the other coordinate: 5.3 into the map from its low edge
                    other = (z0 if axis == "x" else x0) + 5.3
                    for t in (capi.AABB, capi.SPHERE):
                        w = half if t == capi.AABB else r
                        centre = bound + w if which == "min" else bound - w
                        cx, cz = (centre, other) if axis == "x" else (other, centre)
                        h = near_height(hm, cx, cz)
                        tag = f"{which}_{axis}_{ltag}{'+' if k > 0 else '-' if k < 0 else ''}_{NAMES[t]}"
                        if t == capi.AABB:
                            lo = [cx - half, h - 0.1, cz - half]; hi = [cx + half, h + 0.4, cz + half]
                            lo[0 if axis == "x" else 2], hi[0 if axis == "x" else 2] = (bound, bound + 2 * half) if which == "min" else (bound - 2 * half, bound)
                            v = capi.make_volume(capi.AABB, (*lo, *hi))
                        else:
                            v = capi.sphere_volume((cx, h + r - 0.1, cz), r)
                        out.append(case("seam_exact", tag, "exact", v, axis=axis, which=which, line=line, twin=k))
    # raised clear of the ground: the family's volumes without contacts
    for j, (x, z) in enumerate(((40.0, -56.0), (48.0, -40.0), (56.0, -48.0), (48.0, -48.0))):
        h = top_height(hm, x, z, 0.6)
        out.append(case("seam_exact", f"clear{j}_AABB", "exact", capi.make_volume(capi.AABB, (x - half, h + 0.05, z - half, x + half, h + 0.5, z + half)), twin=None))
        out.append(case("seam_exact", f"clear{j}_sphere", "exact", capi.sphere_volume((x, h + r + 0.05, z), r), twin=None))
    return out


# ---- windows: flat boxes whose cell window is chosen, and whose contact count is found by the oracle
def window_box(hm, chunk, cols, rows, sink=0.03, thick=0.1, ground=None):
    """A flat axis-aligned box whose window in chunk (cx, cz) is the columns cols = (a, b) by the rows rows = (c, d), in the window's own units of
    1 / 129 of the chunk (HmVolume::window multiplies by the vertex count); b or d of 129 and more reach into the next chunk (b - 129 there)."""
    c = np.asarray(hm["min_corner"], np.float64); size = float(hm["chunk_size"])
    at = lambda base, k, f: base + (k + f) / 129.0 if k < 129 else base + 1.0 + (k - 129 + f) / 129.0   # noqa: E731
    xa, xb = c[0] + size * at(chunk[0], cols[0], 0.25), c[0] + size * at(chunk[0], cols[1], 0.75)
    za, zb = c[2] + size * at(chunk[1], rows[0], 0.25), c[2] + size * at(chunk[1], rows[1], 0.75)
    h = near_height(hm, (xa + xb) / 2, (za + zb) / 2) if ground is None else ground
    return capi.make_volume(capi.AABB, (xa, h - sink, za, xb, h - sink + thick, zb))


# (tag, chunk, columns, rows, the cells of the window per chunk it touches)
WINDOW_SHAPES = (("w63", (0, 1), (20, 26), (30, 38), [63]), ("w64", (0, 1), (20, 27), (30, 37), [64]), ("w65", (0, 1), (20, 24), (30, 42), [65]),
                 ("w1x65", (0, 1), (50, 50), (30, 94), [65]), ("w128x1", (0, 1), (0, 127), (70, 70), [128]),
                 ("w9x9_aligned", (0, 1), (40, 48), (56, 64), [81]), ("w9x9_shifted", (0, 1), (44, 52), (60, 68), [81]),
                 ("two_chunks", (0, 1), (120, 129 + 8), (40, 48), [72, 81]), ("four_chunks", (0, 0), (119, 129 + 9), (118, 129 + 8), [90, 100, 81, 90]))


def _count_candidates(hm, chunk):
    """Flat boxes of a few cells (about the stash's 16 contacts) and of some 130 cells (about the cap's 255) at a few places and depths."""
    out = []
    for k, (gx, gz) in enumerate(((30, 40), (61, 77), (90, 23), (14, 101), (75, 52), (49, 9))):
        for sink in (0.005, 0.01, 0.02, 0.03, 0.05):
            for w in (2, 3, 4):
                for d in (2, 3, 4):
                    out.append(("small", window_box(hm, chunk, (gx, gx + w - 1), (gz, gz + d - 1), sink)))
            for w in (10, 11, 12):
                for d in (11, 12, 13):
                    out.append(("large", window_box(hm, chunk, (gx, gx + w - 1), (gz, gz + d - 1), sink, thick=0.4)))
    return out


def window_recipes(mapname, chunk_of=lambda c: c):
    """The windows of WINDOW_SHAPES on a map (chunk_of: where the recipe's chunk (0, 0), (0, 1) .. lies there)."""
    hm = the_map(mapname)
    return [case("windows", tag, mapname, window_box(hm, chunk_of(chunk), cols, rows), cells=cells) for tag, chunk, cols, rows, cells in WINDOW_SHAPES]


def windows(oracle_mod):
    hm = the_map("fine")
    out = window_recipes("fine")
    cand = _count_candidates(hm, (1, 1))
    vols = np.concatenate([v for _, v in cand])
    n = np.diff(T.oracle_terrain_contacts(oracle_mod, hm, vols)[0].astype(np.int64))
    for want in (STASH - 1, STASH, STASH + 1, CAP - 1, CAP):
        k = np.flatnonzero(n == want)
        assert len(k), f"no candidate box with {want} contacts (counts found: {sorted(set(n.tolist()))})"
        out.append(case("windows", f"count{want}", "fine", cand[int(k[0])][1], count=want))
    # more than the cap: a 3 m box, and inside its bounds two boxes side by side that have more than 255 contacts between them
    x0, z0, x1, z1, cell = extent(hm)
    x, z = x0 + 0.25 * (x1 - x0), z0 + 0.25 * (z1 - z0)
    h = near_height(hm, x, z)
    out.append(case("windows", "over_cap", "fine", capi.make_volume(capi.AABB, (x - 1.5, h - 0.1, z - 1.5, x + 1.5, h + 0.1, z + 1.5)), count=CAP))
    for j, xa in enumerate((x - 1.4, x + 0.1)):
        out.append(case("windows", f"over_cap_witness{j}", "fine", capi.make_volume(capi.AABB, (xa, h - 0.1, z - 0.6, xa + 0.65, h + 0.1, z + 0.6)), witness=True))
    # clear of the ground: the family's volumes without contacts
    for j, (tag, chunk, cols, rows, cells) in enumerate(WINDOW_SHAPES[:4]):
        v = window_box(hm, chunk, cols, rows)
        top = top_height(hm, float(v["shape"][0, 0] + v["shape"][0, 3]) / 2, float(v["shape"][0, 2] + v["shape"][0, 5]) / 2, 2.5)
        out.append(case("windows", f"{tag}_clear", "fine", window_box(hm, chunk, cols, rows, sink=-0.02, ground=top), cells=cells))
    return out


# ---- maps: a generic placement of every type on each kind of map
def maps():
    out = []
    spots = {"flat": (5.3, 7.7), "tilted": (6.1, 9.4), "floor": (3.3, 11.2), "plateau": (9.9, 4.6), "ripple": (7.3, 8.1), "wide": (0.7, -1.3)}
    for name, (x, z) in spots.items():
        hm = the_map(name)
        s = 0.25 if name == "wide" else 0.4        # (cells of 1 / 16: a larger sphere sunk to its middle has more than 255 contacts)
        for t in TYPES:
            q = _rand_q(_rng(5500, t, len(name)))
            for pose in ("shallow", "deep", "clear"):
                out.append(case("maps", f"{name}_{pose}_{NAMES[t]}", name, posed(hm, t, s, x, z, q, pose)))
            out.append(case("maps", f"{name}_high_{NAMES[t]}", name, posed(hm, t, s, x + 1.5, z, q, "lift", 0.5)))
    hm = the_map("wide")
    # the row's floor: a capsule and a box that lie across the chunks (1, 2), (2, 2) and (3, 2), rising by 0.05 per unit of x so that only the low
    # end dips into the floor (lying flat they would have more than 255 contacts)
    h = near_height(hm, 0.0, 0.2)
    out.append(case("maps", "wide_three_chunks_capsule", "wide", capi.make_volume(capi.CAPSULE, (-6.0, 0.05, 0.0, 6.0, 0.65, 0.0, 0.1), (0.0, h, 0.2))))
    out.append(case("maps", "wide_three_chunks_OBB", "wide", capi.box_volume((0.0, h + 0.3, 1.0), (6.0, 0.05, 0.1), scenes.q_axis_angle((0, 0, 1), 0.05))))
    return out


# ---- many_chunks: 256 and 257 chunks per dimension
def many_chunks():
    out = []
    for cpd in (256, 257):
        name = f"many{cpd}"
        hm = the_map(name)
        lo = MANY_CORNER[0] + 16.0 * (cpd - 2)     # the four chunks cover [lo, lo + 32]^2
        spots = [(lo + a, lo + b) for a in (7.3, 16.0, 24.6) for b in (6.1, 16.0, 25.2)]
        for k, (x, z) in enumerate(spots):
            for t in T.TRIANGLE_TYPES:
                q = I4 if t == capi.AABB else _rand_q(_rng(5600, t, k))
                for stag, s in (("small", 0.2), ("large", 0.7)):
                    out.append(case("many_chunks", f"{cpd}_{k}_{stag}_{NAMES[t]}", name, posed(hm, t, s, x, z, q, "shallow")))
            out.append(case("many_chunks", f"{cpd}_{k}_clear_{NAMES[T.TRIANGLE_TYPES[k % 4]]}", name, posed(hm, T.TRIANGLE_TYPES[k % 4], 0.3, x, z, I4, "clear")))
    return out


def shared_windows():
    """The windows of WINDOW_SHAPES that fit one chunk and small boxes about the stash's size, in chunk (255, 255), which the 256 and the 257 map share:
    [(tag, volume)].  tests keep those to which the oracle gives at most 16 contacts in a window of at most 64 cells."""
    hm = the_map("many256")
    out = [(tag, window_box(hm, (255, 255), cols, rows)) for tag, chunk, cols, rows, cells in WINDOW_SHAPES[:7]]
    out += [(f"{kind}{j}", v) for j, (kind, v) in enumerate(_count_candidates(hm, (255, 255))[::7]) if kind == "small"]
    return out


_SHARED = []


def shared_expected(oracle_mod):
    """(tags, volumes, the oracle's (offsets, records, boxes) on the 256 map, the same on the 257 map) of the shared_windows to which the oracle gives,
    on the 256 map, at most 16 contacts in a window of at most 64 cells: the volumes k_hm_write_stashed writes on the one map and the wave-per-collider
    WRITE pass on the other.  Computed once, read-only."""
    if not _SHARED:
        cand = shared_windows()
        hm = the_map("many256")
        offsets, _, boxes = T.oracle_terrain_contacts(oracle_mod, hm, np.concatenate([v for _, v in cand]))
        n = np.diff(offsets.astype(np.int64))
        keep = [i for i in range(len(cand)) if n[i] <= STASH and T.largest_window(hm, boxes[i]) <= 64]
        vols = np.concatenate([cand[i][1] for i in keep])
        both = [T.oracle_terrain_contacts(oracle_mod, the_map(m), vols) for m in ("many256", "many257")]
        for a in (vols, *both[0], *both[1]):
            a.setflags(write=False)
        _SHARED.extend([[cand[i][0] for i in keep], vols, both[0], both[1]])
    return tuple(_SHARED)


# ---- size: tiny, thin and degenerate volumes
def size():
    hm = the_map("rolling")
    x0, z0, _, _, cell = extent(hm)
    # in chunk (1, 1), 15 units from every other case of the map: in the step's world the massless bodies of the degenerate volumes get NaN poses and
    # hand them to whatever they touch
    x, z = x0 + 188.3 * cell, z0 + 198.4 * cell
    out = []
    for t in FAMILY_TYPES["size"]:
        q = _rand_q(_rng(5700, t))
        for pose in ("shallow", "deep", "clear"):
            out.append(case("size", f"tiny_{pose}_{NAMES[t]}", "rolling", posed(hm, t, 1e-3 * cell, x, z, q, pose)))
    h = near_height(hm, x, z)
    for pose, y in (("sunk", h), ("clear", top_height(hm, x, z, 2.2) + 0.01)):      # a 3 m plate 1 mm thick, through the surface along a contour line
        out.append(case("size", f"plate_{pose}_AABB", "rolling", capi.make_volume(capi.AABB, (x - 1.5, y, z - 1.5, x + 1.5, y + 1e-3, z + 1.5))))
        out.append(case("size", f"plate_{pose}_OBB", "rolling", capi.box_volume((x, y, z), (1.5, 5e-4, 1.5), scenes.q_axis_angle((0, 1, 0), 0.4))))
    # the volumes without a size, each at a spot of its own (4, 5 .. 11 units along x from the others, which they would hand their NaN poses to)
    for j, pose in enumerate(("under", "over")):
        at = [(x + 4.0 + 4 * j + k, z) for k in range(4)]
        ys = [near_height(hm, *p) + (-0.05 if pose == "under" else 0.05) for p in at]
        (xa, za), (xb, zb), (xc, zc), (xd, zd) = at
        out.append(case("size", f"radius0_{pose}_sphere", "rolling", capi.sphere_volume((xa, ys[0], za), 0.0)))
        out.append(case("size", f"length0_{pose}_capsule", "rolling", capi.capsule_volume((xb, ys[1] + 0.1, zb), (xb, ys[1] + 0.1, zb), 0.1)))
        out.append(case("size", f"flat_{pose}_AABB", "rolling", capi.make_volume(capi.AABB, (xc - 0.3, ys[2], zc - 0.2, xc + 0.3, ys[2], zc + 0.2))))
        out.append(case("size", f"flat_{pose}_OBB", "rolling", capi.box_volume((xd, ys[3], zd), (0.3, 0.2, 0.0), scenes.q_axis_angle((1, 0, 0), 0.3))))
    return out


# ---- height_range: above, below and far under the surface
def height_range():
    hm = the_map("rolling")
    out = []
    for t in TYPES:
        x, z = anchor(hm, "centre", 2 + TYPES.index(t) % 3)
        q = _rand_q(_rng(5800, t))
        for tag, pose, amount in (("above1", "lift", 1.0), ("above9.9", "lift", 9.9), ("above10.1", "lift", 10.1), ("under9.9", "under", 9.9), ("under10.1", "under", 10.1),
                                  ("under20", "under", 20.0)):
            out.append(case("height_range", f"{tag}_{NAMES[t]}", "rolling", posed(hm, t, 0.4, x, z, q, pose, amount)))
        # wholly below min_corner.y
        v0 = shaped(t, 0.4, (0.0, 0.0, 0.0), q)[0]
        out.append(case("height_range", f"below_corner_{NAMES[t]}", "rolling", shaped(t, 0.4, (x, float(hm["min_corner"][1]) - 0.5 - bounds64(v0)[1][1], z), q)))
    return out


_GENERATORS = dict(features=features, rim=rim, seam_exact=seam_exact, maps=maps, many_chunks=many_chunks, size=size, height_range=height_range)
_CACHE = {}


def family(oracle_mod, name):
    """The cases of a family (computed once per process; `windows` asks the oracle for the boxes with the contact counts it needs)."""
    if name not in _CACHE:
        _CACHE[name] = windows(oracle_mod) if name == "windows" else _GENERATORS[name]()
    return _CACHE[name]


def family_types(name):
    return FAMILY_TYPES.get(name, TYPES)


def by_map(oracle_mod):
    """{map: [cases of every family on it]} in the order of FAMILIES; an even number of cases gets the first one again: the batches are odd."""
    out = {}
    for f in FAMILIES:
        for c in family(oracle_mod, f):
            out.setdefault(c["map"], []).append(c)
    return {m: cs + ([cs[0]] if len(cs) % 2 == 0 else []) for m, cs in out.items()}


def volumes_of(cases):
    return np.concatenate([c["volume"] for c in cases])


_EXPECTED = {}


def expected(oracle_mod, mapname):
    """(cases, volumes, offsets, records, boxes) of a map: the oracle's answer to all of the map's cases in one world, computed once, read-only."""
    if mapname not in _EXPECTED:
        cases = by_map(oracle_mod)[mapname]
        vols = volumes_of(cases)
        out = T.oracle_terrain_contacts(oracle_mod, the_map(mapname), vols)
        for a in (vols, *out):
            a.setflags(write=False)
        _EXPECTED[mapname] = (cases, vols, *out)
    return _EXPECTED[mapname]


def results(oracle_mod, name):
    """Per case of a family: (case, its records, its world AABB) from expected() of the case's map."""
    out = []
    index = {}
    for c in family(oracle_mod, name):
        if c["map"] not in index:
            cases = expected(oracle_mod, c["map"])[0]
            index[c["map"]] = {id(k): i for i, k in reversed(list(enumerate(cases)))}
        _, _, offsets, recs, boxes = expected(oracle_mod, c["map"])
        i = index[c["map"]][id(c)]
        out.append((c, recs[int(offsets[i]):int(offsets[i + 1])], boxes[i]))
    return out


def step_scene(mapname, vols):
    """The map's volumes as gravity-free dynamic bodies, one collider each."""
    e, ce, c = T.volume_bodies(vols)
    e["gravity_factor"] = 0.0
    return T.terrain_scene(the_map(mapname), e, ce, c)
