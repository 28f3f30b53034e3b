"""The test matrix of the ray cast against the heightmap terrain (mi_world_raycast with the terrain flag of the include mask): the rays at which a float32 walk over
the terrain's cells goes wrong; numpy only, no GPU.  tests/test_raycast_terrain.py checks the matrix itself from the float64 reference alone,
tests/test_gpu_raycast_terrain.py runs it on the GPU.  Built the way tests/raycast_matrix.py is:

  * a ray is posed in float64 and rounded to float32 once, when the case is finished; the reference sees the rounded numbers, the ones the GPU gets;
  * the REFERENCE (cast) is the first crossing of the ray with the collision triangles of raycast_ref.terrain_triangles, every triangle with
    inclusive edges (1e-9 of a cell): the surface as a whole, nothing decides which of two triangles owns a point of their shared edge;
  * a CASE is one map, one ray with its max_t, and a `scale` = max(1, the largest |coordinate| of the origin and of the hit; on a miss, of the
    points where the ray enters and leaves the map's box);
  * delta = 4 x the family's bound x scale is the offset of the derived families and the slack of the ROBUSTNESS FILTER: a case is kept when the
    reference decides hit / miss the same way with every height raised and lowered by delta, and a hit's two shifted times stay within
    delta / |n . d^| + delta of the unshifted one (the same piece of surface, no ridge skimmed).  The filter moves the whole surface, never one
    triangle: a hit on a shared edge or a vertex is well conditioned and stays.  It uses the reference alone, so the GPU comparison has no budget;
  * `limits` and `ordering` are derived from kept hits in closed form and judged by what the reference says of the rounded numbers; `invalid` is
    a miss by the header's rule and is not filtered.
An origin ON the surface (t = 0, the normal -normalize(d)) cannot pass that filter, and on the hills float32 rounding decides on which side of the
surface it lands.  `below` poses it on the `floor` map, whose heights are all 0 counts: the surface is y = min_corner.y exactly in any arithmetic.
Those cases are judged in closed form (the reference's t is exactly 0), like `limits`."""
import numpy as np

import raycast_matrix as RM
import raycast_ref
import sweep_terrain_ref as ST
from d3d12renderer_amd import capi, scenes

FAMILIES = ("generic", "features", "axes", "grazing", "below", "outside", "direction_length", "far", "offset", "limits", "ordering", "invalid")
LENGTHS = RM.LENGTHS
FAR = (1e2, 1e3, 1e4)
# The bound on |t - t_ref| |d|, on the point's distance from o + t d and from the surface and on the normal's distance from an admissible one, PER
# UNIT OF `scale`: 4 x the largest value measured on the MI355X against the float64 reference, rounded up to one digit (MEASURED).
# The cases follow from the bounds through delta, so each figure is the one measured at its own bound.  Ten families measure the same at any bound
# from these up to ten times as wide.  grazing does not: its hits dip 4 delta into a ridge, and which facets they then cross moves the figure:
# 1.0e-6 at its own bound of 4e-6, 4.9e-7 at 3e-6, 6.1e-7 at 2e-6 (and 2.4e-6 at 4e-7 and 8e-7, where the dips are of 2e-4 and 4e-4).  ordering's figure is its sphere's entry (the terrain's own part: 5.8e-8).  Only far
# exceeds raycast_matrix.BOUNDS of the family with the same name (7e-7, from 1.75e-7): 1.8e-7 is one and a half roundings of a coordinate.
MEASURED = {"generic": 1.42e-7, "features": 7.67e-8, "axes": 7.83e-8, "grazing": 1.0e-6, "below": 5.49e-8, "outside": 1.44e-7, "direction_length": 7.31e-8,
            "far": 1.82e-7, "offset": 4.67e-8, "limits": 1.42e-7, "ordering": 8.57e-7}
BOUNDS = {"generic": 6e-7, "features": 4e-7, "axes": 4e-7, "grazing": 4e-6, "below": 3e-7, "outside": 6e-7, "direction_length": 3e-7, "far": 8e-7,
          "offset": 2e-7, "limits": 6e-7, "ordering": 4e-6, "invalid": 0.0}
INF = np.inf
OFFSET_CORNER = (2900.0, 100.0, -3700.0)
HOLE = (1, 0)


def offset_map():
    """The rolling heights (sweep_terrain_ref.rolling_map) with min_corner a few thousand units from the origin on x and z, a hundred on y."""
    return scenes.rolling_heightmap(2, 32.0, 6.0, holes=(HOLE,), min_corner=OFFSET_CORNER)


FLOOR_Y = 2.0


def floor_map():
    """One chunk of 16 m, every height 0 counts, min_corner (0, FLOOR_Y, 0): the plane y = FLOOR_Y, exactly."""
    hm = ST.flat_map()
    hm["chunks"] = {(0, 0): np.zeros((129, 129), np.uint16)}
    hm["min_corner"] = np.array([0.0, FLOOR_Y, 0.0], np.float32)
    return hm


MAPS = dict(ST.MAPS, offset=offset_map, floor=floor_map)


class Map:
    """A map of MAPS in float64: s the cell, n cells per side, x0 / z0 / size the square it covers, H[z, x] the vertex heights in world y (NaN
    where no chunk has one), solid[z, x] the cells that have triangles, and the triangles themselves (a, b, c, unit normals, xz bounds)."""

    def __init__(self, name):
        hm = MAPS[name]()
        self.name, self.hm = name, hm
        self.n, self.s = 128 * hm["chunks_per_dim"], hm["chunk_size"] / 128.0
        self.corner = np.asarray(hm["min_corner"], np.float32).astype(np.float64)
        self.x0, self.z0, self.size = self.corner[0], self.corner[2], self.n * self.s
        self.H = np.full((self.n + 1, self.n + 1), np.nan)
        self.solid = np.zeros((self.n, self.n), bool)
        for (cx, cz), h in hm["chunks"].items():
            self.H[cz * 128:cz * 128 + 129, cx * 128:cx * 128 + 129] = np.asarray(h, np.float64) * (hm["amplitude"] / 65535.0) + self.corner[1]
            self.solid[cz * 128:cz * 128 + 128, cx * 128:cx * 128 + 128] = True
        self.ymin, self.ymax = float(np.nanmin(self.H)), float(np.nanmax(self.H))
        self.a, self.b, self.c = raycast_ref.terrain_triangles(hm)
        nn = np.cross(self.b - self.a, self.c - self.a)
        self.normal = nn / np.linalg.norm(nn, axis=1, keepdims=True)
        v = np.stack([self.a, self.b, self.c])
        self.lo, self.hi = v.min(axis=0)[:, ::2], v.max(axis=0)[:, ::2]

    def height(self, x, z):
        """The triangulated surface's height over (x, z), clamped into the map (NaN in a hole)."""
        u, v = np.clip((x - self.x0) / self.s, 0, self.n), np.clip((z - self.z0) / self.s, 0, self.n)
        gx, gz = min(int(u), self.n - 1), min(int(v), self.n - 1)
        u, v = u - gx, v - gz
        if not self.solid[gz, gx]:
            return np.nan
        A, B, C, D = self.H[gz, gx], self.H[gz + 1, gx], self.H[gz, gx + 1], self.H[gz + 1, gx + 1]
        return A + u * (C - A) + v * (B - A) if u + v <= 1 else D + (1 - u) * (B - D) + (1 - v) * (C - D)

    def holders(self, p, tol):
        """The triangles whose footprint holds (p.x, p.z) to within tol (a length)."""
        m = np.flatnonzero((self.lo[:, 0] <= p[0] + tol) & (self.hi[:, 0] >= p[0] - tol) & (self.lo[:, 1] <= p[2] + tol) & (self.hi[:, 1] >= p[2] - tol))
        u, w = _bary(self.a[m], self.b[m], self.c[m], np.asarray(p, np.float64)[None])
        e = tol / self.s
        return m[(u >= -e) & (w >= -e) & (u + w <= 1 + e)]


_MAPS = {}


def the_map(name):
    if name not in _MAPS:
        _MAPS[name] = Map(name)
    return _MAPS[name]


def _bary(a, b, c, p):
    """Barycentric coordinates (along b - a and c - a) of p's footprint in the footprints of the triangles: the maps' cells are axis-aligned."""
    v0, v1, v2 = (b - a)[:, ::2], (c - a)[:, ::2], (p - a)[:, ::2]
    den = v0[:, 0] * v1[:, 1] - v0[:, 1] * v1[:, 0]
    return (v2[:, 0] * v1[:, 1] - v2[:, 1] * v1[:, 0]) / den, (v0[:, 0] * v2[:, 1] - v0[:, 1] * v2[:, 0]) / den


def _box_span(m, o, d, max_t):
    """[t0, t1] of the ray inside the map's box (1 higher and lower than its heights, 1e-6 wider), within [0, max_t]; None: never."""
    lo = np.array([m.x0 - 1e-6, m.ymin - 1.0, m.z0 - 1e-6]); hi = np.array([m.x0 + m.size + 1e-6, m.ymax + 1.0, m.z0 + m.size + 1e-6])
    t0, t1 = 0.0, max_t
    for k in range(3):
        if d[k] == 0:
            if o[k] < lo[k] or o[k] > hi[k]:
                return None
        else:
            a, b = sorted(((lo[k] - o[k]) / d[k], (hi[k] - o[k]) / d[k]))
            t0, t1 = max(t0, a), min(t1, b)
    return (t0, t1) if t0 <= t1 else None


def cast(m, o, d, max_t=INF, shift=0.0):
    """The first crossing of the ray with map m's surface raised by `shift`: (t, triangle index), or (None, -1).  t in the direction's units."""
    o = np.asarray(o, np.float64) - (0.0, shift, 0.0)
    if not (np.isfinite(o).all() and np.isfinite(d).all() and np.any(d != 0) and max_t >= 0):
        return None, -1
    span = _box_span(m, o, d, max_t)
    if span is None:
        return None, -1
    e0, e1 = o + span[0] * d, o + span[1] * d
    pick = np.flatnonzero((m.hi[:, 0] >= min(e0[0], e1[0]) - 1e-6) & (m.lo[:, 0] <= max(e0[0], e1[0]) + 1e-6) &
                          (m.hi[:, 1] >= min(e0[2], e1[2]) - 1e-6) & (m.lo[:, 1] <= max(e0[2], e1[2]) + 1e-6))
    if not len(pick):
        return None, -1
    a, b, c, n = m.a[pick], m.b[pick], m.c[pick], m.normal[pick]
    dn = n @ d
    with np.errstate(divide="ignore", invalid="ignore"):
        t = ((a - o) * n).sum(axis=1) / dn
        u, w = _bary(a, b, c, o + t[:, None] * d)
        ok = (dn != 0) & (t >= 0) & (t <= max_t) & (u >= -1e-9) & (w >= -1e-9) & (u + w <= 1 + 1e-9)
    if not ok.any():
        return None, -1
    j = int(np.argmin(np.where(ok, t, INF)))
    return float(t[j]), int(pick[j])


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


def finish(family, tag, mapname, o, d, max_t=INF, **extra):
    o32, d32 = np.asarray(o, np.float64).astype(np.float32), np.asarray(d, np.float64).astype(np.float32)
    case = dict(family=family, tag=tag, map=mapname, raw=(np.asarray(o, np.float64), np.asarray(d, np.float64), float(max_t)), o32=o32, d32=d32,
                max_t32=np.float32(max_t), o=o32.astype(np.float64), d=d32.astype(np.float64), max_t=float(np.float32(max_t)), spheres=[])
    case.update(extra)
    return case


def delta(case):
    return 4.0 * BOUNDS[case["family"]] * case["scale"]


def judge(case):
    """The reference's answer and the robustness filter: case["t"] (None on a miss), ["tri"], ["point"], ["scale"], ["kept"]."""
    m, o, d, mt = the_map(case["map"]), case["o"], case["d"], case["max_t"]
    t, j = cast(m, o, d, mt)
    reach = [np.abs(o).max()] if np.isfinite(o).all() else [1.0]
    if t is not None:
        reach.append(np.abs(o + t * d).max())
    elif np.isfinite(o).all() and np.isfinite(d).all() and np.any(d != 0) and mt >= 0:
        span = _box_span(m, o, d, mt)
        if span is not None:
            reach += [np.abs(o + span[0] * d).max(), np.abs(o + span[1] * d).max()]
    case.update(t=t, tri=j, point=None if t is None else o + t * d, scale=max(1.0, float(max(reach))))
    if case["family"] == "invalid":
        case["kept"] = t is None
        return case
    if case.get("on_surface"):        # closed form: the origin lies on the plane exactly, the reference's t is exactly 0
        case["kept"] = t == 0.0
        return case
    dl, length = delta(case), float(np.linalg.norm(d))
    shifted = [cast(m, o, d, mt, s)[0] for s in (dl, -dl)]
    if t is None:
        kept = shifted[0] is None and shifted[1] is None
    else:
        slack = (dl / abs(m.normal[j] @ d / length) + dl) / length
        kept = all(s is not None and abs(s - t) <= slack for s in shifted)
    case["kept"] = bool(kept)
    return case


# ---- rays: a target on the surface, a unit direction of travel, the origin `dist` before the target
def _down(rng, lowest=35.0, kind=None):
    """A random direction of travel that descends by at least `lowest` degrees: steeper than any slope of the maps.  At the vertex where the four
    chunks meet (kind corner4) it heads from the (-x, -z) chunk to the (+x, +z) one or back: a ray that arrives over the hole or leaves into it
    turns from hit to miss when the surface moves by delta, which is the hole's rim (features: rim_corner) and not this vertex."""
    el, az = np.radians(rng.uniform(lowest, 90.0)), rng.uniform(0, 2 * np.pi)
    if kind == "corner4":
        az = np.radians(rng.uniform(15.0, 75.0) + 180.0 * rng.integers(0, 2))
    return np.array([np.cos(el) * np.cos(az), -np.sin(el), np.cos(el) * np.sin(az)])


def _surface(m, x, z):
    return np.array([x, m.height(x, z), z])


def _solid_cell(m, rng, margin=8):
    while True:
        gx, gz = rng.integers(margin, m.n - margin, 2)
        if m.solid[gz - 2:gz + 3, gx - 2:gx + 3].all():
            return int(gx), int(gz)


def _interior(m, rng):
    gx, gz = _solid_cell(m, rng)
    u, v = rng.uniform(0.15, 0.85, 2)
    if abs(u + v - 1) < 0.15:
        u *= 0.5
    return _surface(m, m.x0 + (gx + u) * m.s, m.z0 + (gz + v) * m.s)


def generic(seed=6100, maps=(("flat", 8), ("tilted", 8), ("rolling", 32)), family="generic", max_ts=(40.0, INF)):
    """Random origins above the map, directions over the whole sphere (upward ones miss), half with a finite max_t."""
    out = []
    for name, count in maps:
        m = the_map(name)
        for k in range(count):
            rng = np.random.default_rng([seed, len(name), k])
            o = np.array([m.x0 + rng.uniform(0.1, 0.9) * m.size, m.ymax + rng.uniform(0.5, 4.0), m.z0 + rng.uniform(0.1, 0.9) * m.size])
            d = _unit(rng.normal(size=3))
            if k % 4 != 3:
                d[1] = -abs(d[1]) - 0.3 * (k % 3)
            out.append((family, f"{name}{k}", name, o, _unit(d), max_ts[k % 2]))
    return out


FEATURE_KINDS = ("vertex", "xline", "zline", "diagonal", "seam", "corner4")


def feature_targets(m, rng, kind):
    """A point of the surface on a feature of the 2 x 2-chunk maps.  xline: x on a grid line; zline: z on one; seam: on x = centre (z beyond the
    hole) or z = centre (x before it); corner4: the vertex where the four chunks meet."""
    gx, gz = _solid_cell(m, rng)
    f = rng.uniform(0.1, 0.9)
    half = m.n // 2
    if kind == "vertex":
        u, v = gx, gz
    elif kind == "xline":
        u, v = gx, gz + f
    elif kind == "zline":
        u, v = gx + f, gz
    elif kind == "diagonal":
        u, v = gx + f, gz + 1 - f
    elif kind == "seam":
        u, v = ((half, half + rng.integers(4, half - 8) + rng.choice([0.0, f])) if rng.random() < 0.5 else
                (rng.integers(8, half - 4) + rng.choice([0.0, f]), half))
    else:
        u, v = half, half
    return _surface(m, m.x0 + u * m.s, m.z0 + v * m.s)


def features(seed=6200, name="rolling", family="features", per_kind=10, dist=6.0):
    m = the_map(name)
    out = []
    for kind in FEATURE_KINDS:
        for k in range(per_kind):
            rng = np.random.default_rng([seed, len(kind), k])
            T = feature_targets(m, rng, kind)
            u = _down(rng, kind=kind)
            out.append((family, f"{kind}{k}", name, T - dist * u, u, INF if k % 2 else dist + 2.0, dict(target=T, feature=kind)))
    # the outer border and corners, the rim of the hole: delta inside (a hit) and delta outside (a miss; the ray heads away from the ground)
    dl = 4.0 * BOUNDS[family] * (max(abs(m.x0), abs(m.z0), abs(m.x0 + m.size), abs(m.z0 + m.size)) + dist)
    mid = m.size / 2
    spots = [("border-x", (0.0, 0.37 * m.size), (-1, 0)), ("border+x", (m.size, 0.81 * m.size), (1, 0)), ("border-z", (0.21 * m.size, 0.0), (0, -1)),
             ("border+z", (0.66 * m.size, m.size), (0, 1)), ("corner--", (0.0, 0.0), (-1, -1)), ("corner-+", (0.0, m.size), (-1, 1)), ("corner++", (m.size, m.size), (1, 1)),
             ("rim_x", (mid, 0.27 * m.size), (1, 0)), ("rim_z", (0.77 * m.size, mid), (0, -1)), ("rim_corner", (mid, mid), (1, -1))]
    for k, (tag, (px, pz), (ox, oz)) in enumerate(spots):
        for side, sign in (("in", -1.0), ("out", 1.0)):
            rng = np.random.default_rng([seed, 99, k])
            x, z = m.x0 + px + sign * dl * ox, m.z0 + pz + sign * dl * oz
            y = m.height(m.x0 + px - 1e-9 * ox, m.z0 + pz - 1e-9 * oz)
            u = _down(rng, 50.0)
            h = np.hypot(u[0], u[2])
            u[0], u[2] = (ox * h / np.hypot(ox, oz), oz * h / np.hypot(ox, oz))          # heading outwards: past the border nothing lies below
            T = np.array([x, y, z])
            out.append((family, f"{tag}_{side}", name, T - dist * u, u, INF, dict(target=T, feature="border" if "rim" not in tag else "rim")))
    return out


def axes(seed=6300):
    """Directions with zero components."""
    out = []
    m = the_map("rolling")
    for k in range(18):      # straight down over vertices, edges, diagonals and interiors; |d| not 1 on every third
        rng = np.random.default_rng([seed, k])
        T = feature_targets(m, rng, ("vertex", "xline", "zline", "diagonal", "seam", "corner4")[k % 6]) if k < 12 else _interior(m, rng)
        out.append(("axes", f"down{k}", "rolling", T + (0, rng.uniform(1, 9), 0), (0.0, -1.0 if k % 3 else -2.5, 0.0), INF, dict(target=T)))
    for k in range(4):       # straight up from above: a miss
        T = _interior(m, np.random.default_rng([seed, 50 + k]))
        out.append(("axes", f"up{k}", "rolling", T + (0, 2.0, 0), (0.0, 1.0, 0.0), INF))
    y = m.ymin + 0.6 * (m.ymax - m.ymin)
    half, lo, hi = m.n // 2, m.x0 + 1.0, m.x0 + m.size - 1.0
    for k, g in enumerate((23, 77, half, 171, 230)):     # level rays exactly on a cell line (g = half: on a chunk seam), from either end
        line = m.z0 + g * m.s
        for tag, o, d in ((f"+x{k}", (lo, y, line), (1, 0, 0)), (f"-x{k}", (m.x0 + (m.size / 2 if g < half else m.size) - 1.0, y, line), (-1, 0, 0)),
                          (f"+z{k}", (m.x0 + g * m.s, y, m.z0 + (m.size / 2 if g >= half else 0) + 1.0), (0, 0, 1)), (f"-z{k}", (m.x0 + g * m.s, y, hi), (0, 0, -1))):
            # (x on the seam and z before the centre is the hole's rim, a knife edge sideways: the -z ray stops short of it)
            out.append(("axes", "level" + tag, "rolling", np.array(o, np.float64), np.array(d, np.float64), m.size / 2 - 1.5 if g == half and d[2] < 0 else INF))
    for k, (gx, gz, dx, dz) in enumerate(((10, 140, 1, 1), (120, 250, 1, -1), (100, 20, -1, 1), (250, 250, -1, -1), (20, 130, 1, 1), (128, 128, -1, 1))):
        for j, yy in enumerate((y, m.ymax + 0.5)):       # level diagonal rays through grid vertices: the x and z crossings tie; the higher one misses
            out.append(("axes", f"diag{k}_{j}", "rolling", np.array([m.x0 + gx * m.s, yy, m.z0 + gz * m.s]), np.array([dx, 0.0, dz]) * np.sqrt(0.5), INF))
    for name in ("flat", "rolling"):                     # straight down exactly on the map's outer edge and corner
        e = the_map(name)
        for k, (fx, fz) in enumerate(((0.0, 0.3), (1.0, 0.6), (0.4, 1.0), (0.0, 0.0), (0.0, 1.0))):
            out.append(("axes", f"edge_{name}{k}", name, np.array([e.x0 + fx * e.size, e.ymax + 2.0, e.z0 + fz * e.size]), (0.0, -1.0, 0.0), INF))
    return out


def _profile(m, o, d, t1):
    """The parameters in [0, t1] at which the ray's footprint crosses a grid line or a cell diagonal: between them the surface below is one plane."""
    ts = [0.0, t1]
    for w, base in ((np.array([1.0, 0, 0]), m.x0), (np.array([0, 0, 1.0]), m.z0), (np.array([1.0, 0, 1.0]), m.x0 + m.z0)):
        rate, at = w @ d, w @ o
        if rate != 0:
            k0, k1 = sorted(((at - base) / m.s, (at + t1 * rate - base) / m.s))
            ts += [((k * m.s + base) - at) / rate for k in range(int(np.ceil(k0)), int(np.floor(k1)) + 1)]
    return np.clip(np.array(ts), 0.0, t1)


def grazing(seed=6400):
    """Near-level rays over the rolling map from the (-x, -z) quarter over both seams into the (+x, +z) quarter, more than 200 cells long, that
    clear the highest ridge under them by 4 and 16 delta (misses) or dip as deep into it (hits)."""
    m = the_map("rolling")
    out = []
    for k in range(10):
        rng = np.random.default_rng([seed, k])
        a, b = rng.uniform(3, 12, 2), m.size - rng.uniform(3, 12, 2)          # (x, z) from the map's corner: start and end
        if (m.size / 2 - a[1]) / (b[1] - a[1]) > (m.size / 2 - a[0]) / (b[0] - a[0]):   # the seam z = centre comes first: never over the hole
            a, b = a[::-1], b[::-1]
        start, end = np.array([m.x0 + a[0], 0.0, m.z0 + a[1]]), np.array([m.x0 + b[0], 0.0, m.z0 + b[1]])
        d = end - start
        t1 = float(np.linalg.norm(d))
        d = _unit(d + (0, rng.uniform(-2e-3, 2e-3) * t1, 0))
        dl = 4.0 * BOUNDS["grazing"] * m.size / 2
        t_out = min(((m.x0 if d[0] < 0 else m.x0 + m.size) - start[0]) / d[0], ((m.z0 if d[2] < 0 else m.z0 + m.size) - start[2]) / d[2])
        for mult, reach in ((4, t1), (16, t_out)):     # max_t = the path's length, or none: then the ridge is the highest up to the map's border
            ts = _profile(m, start, d, reach)
            gap = np.array([t * d[1] - m.height(*(start + t * d)[::2]) for t in ts])
            assert np.isfinite(gap).all(), k
            for sign, what in ((1, "miss"), (-1, "hit")):
                o = start + (0, sign * mult * dl - gap.min(), 0)
                out.append(("grazing", f"path{k}_k{mult}{what}", "rolling", o, d, t1 if mult == 4 else INF, dict(path=t1)))
    return out


def below(seed=6500):
    m = the_map("rolling")
    out = []
    for k in range(32):
        rng = np.random.default_rng([seed, k])
        T = _interior(m, rng) if k % 4 else feature_targets(m, rng, FEATURE_KINDS[(k // 4) % 4])
        u = _down(rng)
        if k < 16:       # under the surface, going up: a hit from below
            out.append(("below", f"up{k}", "rolling", T + rng.uniform(0.3, 2.0) * u, -u, INF if k % 2 else 4.0, dict(target=T)))
        else:            # under the surface, going down
            out.append(("below", f"down{k}", "rolling", T + rng.uniform(0.05, 1.0) * u, u, INF))
    # on the surface of the floor map (in a cell, on a cell line, on a vertex, on a diagonal), going down and up, |d| not 1, max_t = 0 too
    spots = ((3.3, 4.7), (5.0, 2.31), (7.125, 9.5), (6.0625, 6.0625), (11.9, 0.6), (2.0, 14.0), (9.45, 9.45), (15.2, 8.8))
    dirs = ((0, -1, 0), (0, 1, 0), (0.3, -0.5, 0.2), (-0.4, 0.7, 0.1), (0, -3, 0), (2, 5, -1), (-0.02, -0.01, 0.03), (0.6, 0.8, 0))
    for k, ((x, z), d) in enumerate(zip(spots, dirs)):
        out.append(("below", f"on{k}", "floor", np.array([x, FLOOR_Y, z]), np.array(d, np.float64), 0.0 if k == 3 else INF, dict(on_surface=True)))
    return out


def outside(seed=6600):
    m = the_map("rolling")
    c, h = m.size / 2, m.ymax
    x0, z0, x1, z1 = m.x0, m.z0, m.x0 + m.size, m.z0 + m.size
    out = []

    def aimed(tag, o, T, max_t=INF):
        out.append(("outside", tag, "rolling", np.asarray(o, np.float64), _unit(np.asarray(T) - np.asarray(o)), max_t))
    for k in range(3):
        rng = np.random.default_rng([seed, k])
        f, g, up = rng.uniform(0.1, 0.4), rng.uniform(2.0, 6.0), rng.uniform(3.0, 8.0)
        aimed(f"side-x{k}", (x0 - g, h + up, z0 + (0.55 + f) * m.size), _surface(m, x0 + rng.uniform(0.5, 6), z0 + (0.55 + f) * m.size + rng.uniform(-3, 3)))
        aimed(f"side+x{k}", (x1 + g, h + up, z1 - f * m.size), _surface(m, x1 - rng.uniform(0.5, 6), z1 - f * m.size + rng.uniform(-3, 3)))
        aimed(f"side-z{k}", (x0 + f * m.size, h + up, z0 - g), _surface(m, x0 + f * m.size + rng.uniform(-3, 3), z0 + rng.uniform(0.5, 6)))
        aimed(f"side+z{k}", (x0 + (0.3 + f) * m.size, h + up, z1 + g), _surface(m, x0 + (0.3 + f) * m.size + rng.uniform(-3, 3), z1 - rng.uniform(0.5, 6)))
        aimed(f"corner--{k}", (x0 - g, h + up, z0 - g * rng.uniform(0.5, 2)), _surface(m, x0 + rng.uniform(0.3, 5), z0 + rng.uniform(0.3, 5)))
        aimed(f"corner-+{k}", (x0 - g, h + up, z1 + g * rng.uniform(0.5, 2)), _surface(m, x0 + rng.uniform(0.3, 5), z1 - rng.uniform(0.3, 5)))
        aimed(f"corner++{k}", (x1 + g, h + up, z1 + g * rng.uniform(0.5, 2)), _surface(m, x1 - rng.uniform(0.3, 5), z1 - rng.uniform(0.3, 5)))
        # over the whole map and out again without a hit; level beside it; parallel to a side just outside it, descending through the heights
        out.append(("outside", f"over{k}", "rolling", np.array([x0 - g, h + up, z0 + f * m.size]), _unit((1.0, rng.uniform(-0.02, 0.05), rng.uniform(0.1, 0.5))), INF))
        out.append(("outside", f"away{k}", "rolling", np.array([x0 - g, h - 1.0, z0 + f * m.size]), _unit((-1.0, -0.2, 0.3)), INF))
        dl = 4.0 * BOUNDS["outside"] * (c + g)
        out.append(("outside", f"beside-x{k}", "rolling", np.array([x0 - dl, h + 1.0, z0 - g]), np.array([0.0, -0.1 - 0.1 * k, 1.0]), INF))
        out.append(("outside", f"beside+z{k}", "rolling", np.array([x1 + g, h + 1.0, z1 + dl]), np.array([-1.0, -0.1 - 0.1 * k, 0.0]), INF))
        # in through the hole chunk's outer sides (+x at low z, -z at high x), over the hole, a hit beyond it
        aimed(f"hole+x{k}", (x1 + g, h + up, z0 + f * c), _surface(m, x0 + c - rng.uniform(1, 8), z0 + f * c + rng.uniform(-2, 2)))
        aimed(f"hole-z{k}", (x0 + c + f * c, h + up, z0 - g), _surface(m, x0 + c + f * c + rng.uniform(-2, 2), z0 + c + rng.uniform(1, 8)))
        aimed(f"hole_through{k}", (x0 + c + f * c, h + up, z0 - g), (x0 + c + f * c, h - 8.0, z0 + 0.8 * c))   # down into the hole: a miss
    return out


def direction_length():
    """Three kept generic hits and a miss at every |d|; max_t scaled to match."""
    base = [c for c in kept("generic") if c["map"] == "rolling"]
    out = []
    for b in [c for c in base if c["t"] is not None][:3] + [c for c in base if c["t"] is None][:1]:
        o, d, mt = b["raw"]
        for length in LENGTHS:
            out.append(("direction_length", f"{b['tag']}_d{length:g}", "rolling", o, _unit(d) * length, mt / length))
    return out


def far(seed=6700):
    """Origins 1e2, 1e3 and 1e4 from the hit, aimed at interiors and at the feature targets."""
    m = the_map("rolling")
    out = []
    for j, dist in enumerate(FAR):
        for kind in ("interior",) + FEATURE_KINDS:
            for k in range(8 if kind == "corner4" else 4):   # (from 1e3 on, rounding takes half of the rays at the four-chunk vertex over the hole)
                rng = np.random.default_rng([seed, j, len(kind), k])
                T = _interior(m, rng) if kind == "interior" else feature_targets(m, rng, kind)
                u = _down(rng, kind=kind)
                out.append(("far", f"{kind}{k}+1e{2 + j}", "rolling", T - dist * u, u, INF if k % 2 else dist * 1.01, dict(target=T, feature=kind)))
    return out


def offset():
    return (generic(6800, (("offset", 24),), "offset", (28.0, 20.0)) + features(6900, "offset", "offset", 8))


def invalid():
    nan, o, d = np.nan, np.array([1.0, 8.0, 2.0]), np.array([0.1, -1.0, 0.2])
    rows = [("nan_d", o, (nan, -1.0, 0.0), INF), ("inf_d", o, (0.0, -INF, 0.0), INF), ("zero_d", o, (0.0, 0.0, 0.0), INF), ("nan_o", (1.0, nan, 2.0), d, INF),
            ("negative_max_t", o, d, -1.0), ("nan_dy", o, (0.1, nan, 0.2), INF), ("inf_o", (INF, 8.0, 2.0), d, INF)]
    return [("invalid", tag, "rolling", np.asarray(a, np.float64), np.asarray(b, np.float64), mt) for tag, a, b, mt in rows]


_GENERATORS = dict(generic=generic, features=features, axes=axes, grazing=grazing, below=below, outside=outside, direction_length=direction_length,
                   far=far, offset=offset, invalid=invalid)
_CACHE = {}


def limits():
    """From the kept hits of generic (reference time t, |d| = L, delta of this family at the base's scale):
      short  max_t = t - delta / L: a miss;   reach  max_t = t + delta / L: the same hit;   zero  max_t = 0: a miss;   inf  max_t = inf: the hit."""
    out = []
    for b in [c for c in kept("generic") if c["t"] is not None][:12]:
        t, L = b["t"], float(np.linalg.norm(b["d"]))
        dl = 4.0 * BOUNDS["limits"] * b["scale"]
        for what, mt in (("short", t - dl / L), ("reach", t + dl / L), ("zero", 0.0), ("inf", INF)):
            c = judge(finish("limits", f"{b['tag']}_{what}", b["map"], b["o"], b["d"], mt))
            # closed form: kept when the reference of the rounded numbers decides as intended with half of delta to spare
            if what == "short":
                c["kept"] = c["t"] is None and t - c["max_t"] > 0.5 * dl / L
            elif what == "reach":
                c["kept"] = c["t"] is not None and c["max_t"] - t > 0.5 * dl / L
            else:
                c["kept"] = (c["t"] is None) == (what == "zero")
            out.append(c)
    return out


SPHERE_R = 0.2


def ordering():
    """One static sphere on the ray of a kept generic hit on the rolling map (a base of its own per case), its entry 4 or 16 delta in front of the
    terrain hit (the sphere wins) or as far behind it (the terrain wins): closest hit = smallest t.  Every ray sees every sphere of the family;
    case["spheres"]: its own (centre, radius); case["sphere_t"]: the first entry into any sphere; case["sphere"]: which one."""
    base = [c for c in kept("generic") if c["map"] == "rolling" and c["t"] is not None][:16]
    out = []
    for k, b in enumerate(base):
        u, L = _unit(b["d"]), float(np.linalg.norm(b["d"]))
        mult, sign, what = (4, 16)[k // 2 % 2], (-1, 1)[k % 2], ("front", "behind")[k % 2]
        dl = 4.0 * BOUNDS["ordering"] * b["scale"]
        centre = b["o"] + (b["t"] * L + sign * mult * dl + SPHERE_R) * u
        out.append(judge(finish("ordering", f"{b['tag']}_{what}{mult}", "rolling", b["o"], b["d"], INF, spheres=[(centre.astype(np.float32), np.float32(SPHERE_R))], front=what == "front")))
    for c in out:
        u, L = _unit(c["d"]), float(np.linalg.norm(c["d"]))
        ts = [float(raycast_ref.ray_sphere(c["o"][None], u[None], x["spheres"][0][0].astype(np.float64), float(x["spheres"][0][1]))[0]) / L for x in out]
        c["sphere"], c["sphere_t"] = int(np.argmin(ts)), min(ts)
        c["sphere_wins"] = bool(c["sphere_t"] < c["t"])
        dl = delta(c)
        c["kept"] = c["kept"] and out[c["sphere"]] is c and c["sphere_wins"] == c["front"] and abs(c["sphere_t"] - c["t"]) * L > 2.0 * dl
    return out


def _make(c):
    return judge(finish(*c[:6], **(c[6] if len(c) > 6 else {})))


def family(name):
    """Every generated case of a family, judged by the reference; computed once per process."""
    if name not in _CACHE:
        _CACHE[name] = limits() if name == "limits" else ordering() if name == "ordering" else [_make(c) for c in _GENERATORS[name]()]
    return _CACHE[name]


def kept(name):
    return [c for c in family(name) if c["kept"]]


def on_target(case):
    """Whether a kept hit is the one its recipe aimed at: the reference's point within 1e-6 x max(scale, |origin - target|) of the target."""
    T = case.get("target")
    return T is not None and case["t"] is not None and np.linalg.norm(case["point"] - T) <= 1e-6 * max(case["scale"], np.linalg.norm(case["o"] - T))


def scene(name):
    """A world of one map.  The rolling map's also holds the `ordering` family's spheres as static colliders: the terrain flag alone (include = 4)
    does not see them."""
    cases = family("ordering") if name == "rolling" else []
    n = len(cases)
    e = scenes.make_entities(n, capi.ENTITY_STATIC)
    col = scenes.make_colliders(n, capi.SPHERE)
    for i, c in enumerate(cases):
        e["position"][i] = c["spheres"][0][0]
        col["shape"][i, :4] = (0.0, 0.0, 0.0, c["spheres"][0][1])
    return scenes.Scene("raycast_terrain_" + name, e, np.arange(n, dtype=np.uint32), col, 10, heightmap=MAPS[name]())
