"""The test matrix of the shape cast against the heightmap terrain (mi_world_sweep with the terrain flag of the include mask): the casts at which a
float32 walk over the terrain's blocks and a float32 GJK cast against its triangles go wrong; numpy only, no GPU.  tests/test_sweep_terrain_matrix.py
checks the matrix itself from the float64 reference alone, tests/test_gpu_sweep_terrain_matrix.py runs it on the GPU.  Built the way
tests/raycast_terrain_matrix.py and tests/sweep_matrix.py are:

  * a volume is one of sweep_matrix's posed shapes, built in float64 and rounded to float32 once, when the case is finished; the reference sees
    the rounded numbers, the ones the GPU gets;
  * the REFERENCE is sweep_terrain_ref.cast: the terrain's triangles as convex shapes through the conservative advancement of sweep_ref;
  * a CASE is one map (raycast_terrain_matrix.MAPS and sweep_terrain_ref.wide_map), one volume, one displacement, an include mask and a
    `scale` = max(1, the largest |coordinate| of the swept bounds);
  * delta = 4 x the family's bound x scale.  Cases are PLACED: the recipe picks a point of the surface, a direction of travel and a volume,
    `place` lets the reference find the touch from back along -d and sets the start so that the touch falls at the chosen fraction of the
    displacement; offsets that decide hit / miss are 4.5 delta, and the case is kept when the reference, on the rounded numbers, finds the
    decision at least 4 delta from flipping (`clearance`: for a miss the closest approach; for a hit the gap at the start and the depth reached
    along the touch's normal by the end, as sweep_terrain_ref.comparison_reference has it; for an initial overlap and a dip into a ridge, that
    the volume still touches after 4 delta along the normal).  A case that fails this is dropped and counted; test_sweep_terrain_matrix.py holds
    the count to one in eight per family and to at least one kept case per volume type.
`lattice` needs no GJK reference: vertical casts of tiny spheres through every kind of line of the grid, judged by Map.height."""
import numpy as np

import overlap_ref as R
import raycast_matrix as RM
import raycast_terrain_matrix as RT
import sweep_matrix as SM
import sweep_ref as S
import sweep_terrain_ref as ST
from d3d12renderer_amd import capi, scenes

FAMILIES = ("generic", "features", "axes", "grazing", "below", "outside", "far", "size_ratio", "wide", "limits", "initial", "direction_length",
            "ordering", "invalid")
TYPES = SM.TYPES
SIX = tuple(range(6))
# The families whose text names the volume types they hold (the others hold all six)
FAMILY_TYPES = {"wide": (R.SPHERE, R.CAPSULE, R.CYLINDER, R.AABB, R.OBB), "invalid": (R.SPHERE, R.HULL)}
# The bound on |t - t_ref| |d|, on the point's distance from the surface and on the shortfall of the separation after backing off along the
# normal, PER UNIT OF `scale`: 4 x the largest value measured on the MI355X against the float64 reference, rounded up to one digit (MEASURED;
# tests/test_gpu_sweep_terrain_matrix.py and INTEGRATION.md 6f state what the figures are).  The cases follow from the bounds through delta: the
# figures are those measured at these bounds.  generic, features, axes, far, size_ratio, limits, initial, direction_length and ordering measure
# under sweep_terrain_ref.BOUND = 6e-6 (4 x 1.44e-6), the bound the terrain cast's comparison set already has, and keep it, tighter than 4 x their
# own figures: at the offset map's coordinates (scale 3 700) a wider bound makes delta longer than the volumes and their travel.  axes is on the
# rolling map only: 8 units of level travel cannot stay 4 delta clear at those coordinates.  Above 6e-6:
#   grazing, below, outside   the cases that dip 4.5 delta into a peak, the hole's rim or the border's free edge end early in t |d| where |n . d^|
#             is a few hundredths (inside the kernel's stall limit of 16 x 2e-6 x scale / |n . d^|), and the figure moves with delta, not
#             monotonically.  Measured at bounds of 6e-6 / 3e-5 / 5e-5: grazing 4.71e-5 / 1.89e-5 / 7.04e-6 (a sphere into a peak in level travel);
#             at 6e-6 / 1e-5 / 2e-5 / 4e-5: below 4.53e-6 / 8.36e-6 / 1.01e-6 / 1.23e-6 (a cylinder onto the hole's rim from below); at 6e-6 / 2e-5 /
#             6e-5: outside 1.27e-5 / 2.56e-6 / 5.06e-7 (a sphere into the border's free edge).  Each bound is one at which 4 x the figure
#             measured there, rounded up, does not exceed it; below's is 4 x its largest figure at any delta
#   wide      the separation of a flat box that meets the far bump's top vertex with its face: a volume without a radius reports the last clip
#             plane's normal, which on a vertex or an edge of the terrain is a separating direction of the triangle hit, not a face's normal
#             (include/mi_physics.h says so).  Its cases do not depend on delta
MEASURED = {"generic": 1.92e-6, "features": 3.13e-6, "axes": 3.50e-6, "grazing": 7.04e-6, "below": 1.23e-6, "outside": 2.56e-6, "far": 1.92e-6,
            "size_ratio": 1.76e-6, "wide": 9.16e-5, "limits": 1.92e-6, "initial": 2.04e-6, "direction_length": 1.61e-6, "ordering": 1.92e-6}
BOUNDS = {f: ST.BOUND for f in FAMILIES}
BOUNDS.update(below=4e-5, grazing=5e-5, outside=2e-5, wide=4e-4)
BOUNDS["invalid"] = 0.0
LATTICE_MEASURED = 2.78e-6     # |t |d| - (y0 - Map.height)| on the rolling map; offset 2.12e-6, floor 1.99e-6; no miss in 15 084 casts of each radius
LATTICE_BOUND = ST.BOUND
TERRAIN_ONLY, COLLIDERS_ONLY, BOTH = 4, 3, 7
HILLS = ("rolling", "offset")
INF = np.inf


def the_map(name):
    return RT.the_map(name)


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


def _rng(*key):
    return np.random.default_rng(list(key))


# ---- volumes
def volume(rng, vt, size=None, variant=0):
    """A posed shape of type vt under a random rotation: half-size in [0.15, 0.5], or of overall size `size` (hulls: the geometry nearest to it)."""
    if vt == R.HULL:
        return SM.hull(SM._rand_q(rng), 0 if size is None else 2 if size < 0.1 else 1 if size > 5 else 0)
    lo, hi = (0.15, 0.5) if size is None else (0.5 * size, 0.5 * size)
    return SM._random_shape(rng, vt, variant, lo, hi)[0]


def centred(posed, at):
    """The posed shape moved so that the centre of its bounds lies at `at`."""
    mn, mx = S.bounds(SM.conv64(posed))
    return SM.shifted(posed, np.asarray(at, np.float64) - (mn + mx) / 2)


def extent(posed):
    mn, mx = S.bounds(SM.conv64(posed))
    return float(np.linalg.norm(mx - mn))


# ---- cases
def finish(family, tag, mapname, posed, d, expect, include=TERRAIN_ONLY, **extra):
    """The case in float32 as the GPU gets it, the reference's shape of those very numbers, and the scale.  expect: "hit", "miss", "initial" or
    "invalid" - what the recipe intends; judge() says what the reference finds."""
    v = capi.make_volume(posed["ctype"], posed["words"], posed["pos"], posed["rot"], posed["hull"])
    d32 = np.asarray(d, np.float64).astype(np.float32)
    case = dict(family=family, tag=tag, map=mapname, vt=posed["label"], posed=posed, volume=v, disp=d32, d=d32.astype(np.float64), expect=expect, include=include)
    if expect != "invalid":
        case["conv"] = SM.convex_of(int(v["type"][0]), v["shape"][0], v["position"][0], v["rotation"][0], posed["hull"])
        case["scale"] = ST.scale_of(case["conv"], case["d"])
    else:
        case["conv"], case["scale"] = None, 1.0
    case.update(extra)
    return case


def delta(case):
    return 4.0 * BOUNDS[case["family"]] * case["scale"]


def delta_at(family, scale):
    return 4.0 * BOUNDS[family] * max(1.0, scale)


def still_touching(mapname, conv, offset):
    """Whether the volume moved by `offset` touches the terrain (its gap is 0 or below: an initial overlap)."""
    return ST.min_gap(mapname, S.moved(conv, offset), 1e-3) <= S.GAP_EPS


def judge(case):
    """The reference's answer on the rounded numbers (case["ref"]: (t, normal, point, initial) or None), case["clearance"]: how far the decision
    is from flipping, and case["kept"]: the reference decides as the recipe intends, at least 4 delta clear."""
    if case["expect"] == "invalid":
        case.update(ref=None, clearance=INF, kept=True)
        return case
    name, conv, d, dl = case["map"], case["conv"], case["d"], delta(case)
    hit = ST.cast(name, conv, d)
    if hit is None:
        c = ST.closest_approach(name, conv, d, 6.0 * dl)
    elif hit[3]:
        # deep enough: the volume still touches when moved 4 delta along `out` (the recipe's direction out of the surface)
        c = 4.0 * dl if case.get("out") is not None and still_touching(name, conv, 4.0 * dl * case["out"]) else 0.0
    else:
        along = -(d @ hit[1])
        c = min(hit[0], 1.0 - hit[0]) * along
        if "lift" in case and not _hits(name, S.moved(conv, 4.0 * dl * case["lift"]), d):    # a dip: raised by 4 delta the cast still hits
            c = 0.0
    said = "miss" if hit is None else "initial" if hit[3] else "hit"
    case.update(ref=hit, clearance=c, kept=bool(said == case["expect"] and c >= 4.0 * dl))
    return case


def _hits(mapname, conv, d):
    return ST.cast(mapname, conv, d) is not None


def approach(mapname, posed, anchor, u, back=None, lead=None):
    """`posed` with the centre of its bounds at anchor - back * u and how far it travels along the unit vector u until it first touches the terrain
    (the float64 reference's cast over back + lead): (shape, travel, hit), or None when there is no touch on that way or it starts in touch."""
    ext = extent(posed)
    back = ext + 1.0 if back is None else back
    lead = ext + 1.0 if lead is None else lead
    start = centred(posed, np.asarray(anchor, np.float64) - back * u)
    hit = ST.cast(mapname, SM.conv64(start), (back + lead) * u)
    if hit is None or hit[3]:
        return None
    return start, hit[0] * (back + lead), hit


def place(mapname, posed, anchor, u, length, t_frac, back=None, lead=None):
    """The volume of `approach` moved on along u so that the touch falls at t_frac of the displacement length * u (t_frac None, or a start that would
    lie before the one the reference searched from: the start stays).  (shape, displacement, hit) or None."""
    u = _unit(u)
    got = approach(mapname, posed, anchor, u, back, lead)
    if got is None:
        return None
    start, travel, hit = got
    on = 0.0 if t_frac is None else max(travel - t_frac * length, 0.0)
    return SM.shifted(start, on * u), length * u, hit


def tuned(gap_at, x0, target, slope=1.0, tol=None, steps=8):
    """The parameter x at which gap_at(x) (a closest approach, rising with x at about `slope`) equals `target`, from x0 on the clear side."""
    tol = 0.02 * target if tol is None else tol
    x = x0
    for _ in range(steps):
        g = gap_at(x)
        if not np.isfinite(g):
            return None
        if abs(g - target) <= tol:
            return x
        x -= (g - target) / slope
    return None


def surface_normal(m, p):
    k = m.holders(p, 1e-7)
    n = m.normal[k].sum(axis=0)
    n = n if n[1] > 0 else -n
    return _unit(n)


def _down(rng, lo=70.0, hi=90.0):
    el, az = np.radians(rng.uniform(lo, hi)), rng.uniform(0, 2 * np.pi)
    return np.array([np.cos(el) * np.cos(az), -np.sin(el), np.cos(el) * np.sin(az)])


def _shallow(rng, n, degrees=10.0):
    """A direction of travel that meets the plane of normal n at `degrees`."""
    t = _unit(np.cross(n, rng.normal(size=3)))
    a = np.radians(degrees)
    return np.cos(a) * t - np.sin(a) * n


# ---- generic: the comparison set's regime, placed
def generic(seed=7100):
    out = []
    for k, what in enumerate(("above", "below", "level", "short", "hole")):
        for vt in SIX:
            name = HILLS[(vt + k) % 2]
            m, rng = the_map(name), _rng(seed, k, vt)
            vol = volume(rng, vt, variant=k % 2)
            T = RT._interior(m, rng)
            if what == "above":
                got = place(name, vol, T, _down(rng, 40.0), 4.0, rng.uniform(0.3, 0.7))
                out.append(("generic", f"above_{TYPES[vt]}", name, got[0], got[1], "hit"))
            elif what == "below":
                got = place(name, vol, T, -_down(rng, 40.0), 4.0, rng.uniform(0.3, 0.7))
                out.append(("generic", f"below_{TYPES[vt]}", name, got[0], got[1], "hit"))
            elif what == "level":
                out.append(("generic", f"level_{TYPES[vt]}", name, centred(vol, (T[0], m.ymax + 0.5 * extent(vol) + rng.uniform(0.3, 1.0), T[2])),
                            (rng.uniform(-6, 6), 0.0, rng.uniform(-6, 6)), "miss"))
            elif what == "short":
                beyond = max(rng.uniform(0.2, 0.5), 8.0 * delta_at("generic", np.abs(T).max() + 4.0))     # the touch lies this far behind the end
                got = place(name, vol, T, _down(rng, 40.0), 1.0, 1.0 + beyond, back=extent(vol) + 1.5 + beyond)
                out.append(("generic", f"short_{TYPES[vt]}", name, got[0], got[1], "miss"))
            else:
                c = m.size / 2
                at = (m.x0 + c + rng.uniform(0.25, 0.75) * c, m.ymax + 1.5, m.z0 + rng.uniform(0.25, 0.75) * c)
                out.append(("generic", f"hole_{TYPES[vt]}", name, centred(vol, at), (rng.uniform(-0.5, 0.5), -(m.ymax - m.ymin) - 4.0, rng.uniform(-0.5, 0.5)), "miss"))
    return out


# ---- features: the touch aimed at the features of the grid
FEATURES = ("vertex", "xedge_mid", "xedge_end", "zedge_mid", "zedge_end", "diag_mid", "diag_end", "block", "seam_x", "seam_z", "corner4",
            "map_corner", "rim", "hole_corner")


def feature_target(m, rng, kind, k=0):
    """(a point of the surface on the feature, the unit direction in the ground plane that leads from it into solid ground or None)."""
    gx, gz = RT._solid_cell(m, rng)
    half, e = m.n // 2, 1e-3
    inward = None
    if kind == "vertex":
        u, v = gx, gz
    elif kind in ("xedge_mid", "xedge_end"):       # an edge along x: z on a grid line
        u, v = gx + (0.5 if kind == "xedge_mid" else e), gz
    elif kind in ("zedge_mid", "zedge_end"):
        u, v = gx, gz + (0.5 if kind == "zedge_mid" else 1.0 - e)
    elif kind in ("diag_mid", "diag_end"):
        f = 0.5 if kind == "diag_mid" else e
        u, v = gx + f, gz + 1.0 - f
    elif kind == "block":
        u, v = (8 * (gx // 8), gz + rng.uniform(0.1, 0.9)) if k % 2 else (gx + rng.uniform(0.1, 0.9), 8 * (gz // 8))
    elif kind == "seam_x":                          # the seam x = centre, beyond the hole
        u, v = half, half + rng.integers(4, half - 8) + rng.choice([0.0, 0.37])
    elif kind == "seam_z":                          # the seam z = centre, before the hole
        u, v = rng.integers(8, half - 4) + rng.choice([0.0, 0.37]), half
    elif kind == "corner4":
        u, v, inward = half, half, _unit((-1.0, 0.0, 1.0))
    elif kind == "map_corner":                      # the three corners of the map that have ground (the fourth is the hole's)
        u, v, inward = ((0, 0, _unit((1.0, 0, 1.0))), (0, m.n, _unit((1.0, 0, -1.0))), (m.n, m.n, _unit((-1.0, 0, -1.0))))[k % 3]
    elif kind == "rim":                             # the hole's rim: x = centre below the hole's z, z = centre along the hole's x
        u, v, inward = ((half, 0.27 * m.n, np.array([-1.0, 0, 0])), (0.77 * m.n, half, np.array([0, 0, 1.0])))[k % 2]
    else:                                           # where the hole's rim z = centre meets the map's border x = max
        u, v, inward = m.n, half, _unit((-1.0, 0, 1.0))
    x, z = m.x0 + u * m.s, m.z0 + v * m.s
    nudge = np.zeros(3) if inward is None else 1e-9 * inward
    return np.array([x, m.height(x + nudge[0], z + nudge[2]), z]), inward


def features(seed=7200):
    """Every feature approached steeply (70 to 90 degrees) and at 10 degrees above the surface, on the rolling and the offset map; the volume types
    in turn.  Then spheres of radius 0 and 1e-3 straight at the inner features and 8 delta inside the free edges.  A hit in every case."""
    out, i = [], 0
    for j, approach in enumerate(("steep", "shallow")):
        for name in HILLS:
            m = the_map(name)
            for f, kind in enumerate(FEATURES):
                vt = i % 6
                i += 1
                for attempt in range(6):
                    rng = _rng(seed, j, len(name), f, attempt)
                    T, inward = feature_target(m, rng, kind, f + j + len(name))
                    if inward is not None:
                        T = T + 1e-9 * inward
                    vol = volume(rng, vt, variant=f % 2)
                    u = _down(rng) if approach == "steep" else _shallow(rng, surface_normal(m, T))
                    got = place(name, vol, T, u, 3.0, rng.uniform(0.35, 0.65), back=extent(vol) + (1.0 if approach == "steep" else 0.6))
                    if got is not None:
                        break
                assert got is not None, (approach, name, kind)
                out.append(("features", f"{approach}_{kind}_{TYPES[vt]}", name, got[0], got[1], "hit", dict(target=T, feature=kind)))
    for name in HILLS:
        m = the_map(name)
        for f, kind in enumerate(FEATURES):
            rng = _rng(seed, 9, len(name), f)
            r = (0.0, 1e-3)[(f + len(name)) % 2]
            T, inward = feature_target(m, rng, kind, f)
            if inward is not None:
                T = T + 8.0 * delta_at("features", np.abs(T).max() + 3.0) * inward
                T[1] = m.height(T[0], T[2])
            u = _down(rng)
            out.append(("features", f"point_{kind}_r{r:g}", name, SM.shifted(SM.sphere(r), T - (1.5 + r) * u), 3.0 * u, "hit", dict(target=T, feature=kind, tiny=True, ruled_normal=r == 0.0)))
    return out


# ---- axes: displacements with zero components and ties
def axes(seed=7300):
    s = np.sqrt(0.5)
    specs = [("+x", (1, 0, 0)), ("-x", (-1, 0, 0)), ("+z", (0, 0, 1)), ("-z", (0, 0, -1)), ("-y", (0, -1, 0)), ("+y", (0, 1, 0)),
             ("x0", _unit((0, -1, 0.8))), ("z0", _unit((-0.7, -1, 0))), ("x0up", _unit((0, 1, 0.5))), ("z0up", _unit((0.5, 1, 0))),
             ("tie++", _unit((s, -0.6, s))), ("tie+-", _unit((s, -0.6, -s))), ("tie-+", _unit((-s, -0.6, s))), ("tie--", _unit((-s, -0.6, -s))),
             ("tie++level", (s, 0, s)), ("tie--level", (-s, 0, -s))]
    out = []
    for k, (tag, u) in enumerate(specs):
        u = np.asarray(u, np.float64)
        for j in range(2):
            vt, name = (2 * k + j) % 6, "rolling"
            m = the_map(name)
            level = u[1] == 0
            for attempt in range(80):
                rng = _rng(seed, k, j, attempt)
                vol = volume(rng, vt, variant=j)
                T = RT._interior(m, rng)
                if level:        # onto a slope that faces the travel, the volume's middle a little above the point: eight units of travel from 3 before it
                    if surface_normal(m, T) @ u > -0.2:
                        continue
                    got = place(name, vol, T + (0, 0.3 * extent(vol), 0), u, 8.0, None, back=3.0, lead=3.0)
                else:
                    got = place(name, vol, T, u, 4.0, rng.uniform(0.3, 0.7))
                if got is not None:
                    break
            assert got is not None, tag
            # (a float32 displacement along an axis is exact; the ties are equal in float32 by construction: the same number in both components)
            d = got[1].copy()
            if tag.startswith("tie"):
                d[2] = np.sign(d[2]) * abs(np.float32(d[0]))
                d[0] = np.float32(d[0])
            out.append(("axes", f"{tag}_{TYPES[vt]}", name, got[0], d, "hit"))
    # vertical casts of volumes 3 units wide: an AABB, an OBB turned about y, a capsule and a cylinder lying along x and along z
    wide = [SM.aabb((1.5, 0.2, 0.4)), SM.obb((0.4, 0.2, 1.5), scenes.q_axis_angle((0, 1, 0), 0.3), 1), SM.capsule(1.3, 0.2, 0), SM.capsule(1.3, 0.2, 2),
            SM.cylinder(1.5, 0.25, 0), SM.cylinder(1.5, 0.25, 2)]
    for k, vol in enumerate(wide):
        name = "rolling"
        m, rng = the_map(name), _rng(seed, 77, k)
        got = place(name, vol, RT._interior(m, rng), (0.0, -1.0, 0.0), 3.0, 0.5, back=2.5)
        out.append(("axes", f"vertical_wide{k}_{TYPES[vol['label']]}", name, got[0], got[1], "hit"))
    return out


# ---- grazing: over a ridge and over a peak vertex, 4.5 delta clear and 4.5 delta deep
def _peaks(m):
    """Interior vertices higher than their eight neighbours, in solid ground."""
    H = np.where(np.isnan(m.H), -INF, m.H)
    c = H[1:-1, 1:-1]
    top = np.ones_like(c, bool)
    for dz in (0, 1, 2):
        for dx in (0, 1, 2):
            if (dz, dx) != (1, 1):
                top &= c > H[dz:dz + c.shape[0], dx:dx + c.shape[1]]
    gz, gx = np.nonzero(top)
    keep = [(x + 1, z + 1) for x, z in zip(gx, gz) if 10 < x < m.n - 10 and 10 < z < m.n - 10 and m.solid[z - 8:z + 10, x - 8:x + 10].all()]
    return keep


def grazing(seed=7400):
    """A volume carried level over the hills along 5 units: over a peak vertex (the second six) or wherever a random path's highest ridge is (the first six),
    at the height at which its closest approach is 4.5 delta (a miss), and 9 delta lower (a hit that dips 4.5 delta)."""
    out = []
    for k in range(12):
        vt, name = k % 6, "rolling"
        m, rng = the_map(name), _rng(seed, k)
        vol = volume(rng, vt, variant=k % 2)
        if k // 6:
            peaks = _peaks(m)
            gx, gz = peaks[int(rng.integers(len(peaks)))]
            mid = np.array([m.x0 + gx * m.s, m.H[gz, gx], m.z0 + gz * m.s])
        else:
            mid = RT._interior(m, rng)
        scale = max(1.0, np.abs(mid).max() + 3.0)
        dl = delta_at("grazing", scale)
        for attempt in range(8):     # a heading on which the ground at both ends of the way lies low enough for the dipping cast to start and end clear
            az = rng.uniform(0, 2 * np.pi)
            u = np.array([np.cos(az), 0.0, np.sin(az)])
            d = 5.0 * u
            base = centred(vol, mid - 2.5 * u)
            conv = SM.conv64(base)
            top = max(m.height(*(mid + s * u)[::2]) for s in np.linspace(-3.5, 3.5, 57))
            y0 = top - mid[1] + 0.5 * extent(vol) + 0.2
            y = tuned(lambda h: ST.closest_approach(name, S.moved(conv, (0, h, 0)), d, 3.0), y0, 4.5 * dl)
            assert y is not None, k
            low = S.moved(conv, (0, y - 9.0 * dl, 0))
            if min(ST.min_gap(name, low, 1.0), ST.min_gap(name, S.moved(low, d), 1.0)) > 6.0 * dl:
                break
        what = "peak" if k // 6 else "ridge"
        out.append(("grazing", f"{what}{k}_miss_{TYPES[vt]}", name, SM.shifted(base, (0, y, 0)), d, "miss"))
        out.append(("grazing", f"{what}{k}_hit_{TYPES[vt]}", name, SM.shifted(base, (0, y - 9.0 * dl, 0)), d, "hit", dict(lift=np.array([0.0, 1.0, 0.0]))))
    return out


# ---- below: from under the surface, through the hole, on the floor
def below(seed=7500):
    out = []
    for vt in SIX:
        name = "rolling"
        m, rng = the_map(name), _rng(seed, vt)
        vol = volume(rng, vt)
        T = RT._interior(m, rng)
        got = place(name, vol, T, -_down(rng, 50.0), 3.0, rng.uniform(0.3, 0.7))
        out.append(("below", f"up_{TYPES[vt]}", name, got[0], got[1], "hit", dict(normal_down=True)))
        T = RT._interior(m, rng)
        out.append(("below", f"down_{TYPES[vt]}", name, centred(vol, T - (0, 0.5 * extent(vol) + 0.3, 0)), 3.0 * _down(rng, 50.0), "miss"))
        # up through the hole beside its rim x = centre: 4.5 delta clear of the rim's free edge (a miss), 4.5 delta over it (struck from below)
        z = m.z0 + rng.uniform(0.2, 0.4) * m.size
        xr = m.x0 + m.size / 2
        yr = m.height(xr - 1e-9, z)
        d = np.array([0.0, 3.0, 0.0])
        base = centred(vol, (xr, yr - 1.5, z))
        conv = SM.conv64(base)
        dl = delta_at("below", max(abs(xr) + 2.0, abs(z) + 2.0))
        half_x = 0.5 * (S.bounds(conv)[1][0] - S.bounds(conv)[0][0])
        x = tuned(lambda o: ST.closest_approach(name, S.moved(conv, (o, 0, 0)), d, 1.0), half_x + 0.1, 4.5 * dl)
        assert x is not None, vt
        out.append(("below", f"hole_clear_{TYPES[vt]}", name, SM.shifted(base, (x, 0, 0)), d, "miss"))
        out.append(("below", f"hole_rim_{TYPES[vt]}", name, SM.shifted(base, (x - 9.0 * dl, 0, 0)), d, "hit", dict(lift=np.array([1.0, 0.0, 0.0]))))
        # from inside the hole sideways into the rim's free edge, at the surface's height
        got = place(name, vol, (xr, yr, z), (-1.0, 0.0, 0.0), 3.0, 0.5, back=extent(vol) + 1.0, lead=1.0)
        out.append(("below", f"hole_side_{TYPES[vt]}", name, got[0], got[1], "hit"))
    # the floor map (y = 2 exactly): the lowest point of the volume exactly on the plane; every number here is exact in float32
    F = RT.FLOOR_Y
    on = [("sphere", SM.shifted(SM.sphere(0.5), (3.25, F + 0.5, 4.75))), ("capsule", SM.shifted(SM.capsule(0.5, 0.25, 1), (7.125, F + 0.75, 9.5))),
          ("cylinder", SM.shifted(SM.cylinder(0.5, 0.25, 1), (6.0625, F + 0.5, 6.0625))), ("AABB", SM.shifted(SM.aabb((0.5, 0.25, 0.375)), (11.5, F + 0.25, 2.25)))]
    for tag, vol in on:
        for j, d in enumerate(((0.0, -1.0, 0.0), (0.5, 0.0, 0.25), (0.25, -0.5, 0.0))):
            # (judged in closed form, not by a clearance: `out` = 0 makes judge() pass them; test_sweep_terrain_matrix.py requires the reference's gap to be 0 exactly)
            out.append(("below", f"on_floor_{tag}{j}", "floor", vol, d, "initial", dict(on_surface=True, out=np.zeros(3))))
    return out


# ---- outside: the map's border
def outside(seed=7600):
    out = []
    for vt in SIX:
        name = "rolling"
        m, rng = the_map(name), _rng(seed, vt)
        vol = volume(rng, vt)
        ext = extent(vol)
        z = m.z0 + rng.uniform(0.55, 0.9) * m.size          # (beyond the hole's rows)
        edge = np.array([m.x0, m.height(m.x0, z), z])        # a point of the border x = min
        dl = delta_at("outside", max(abs(m.x0), abs(z)) + 4.0)
        # from outside inwards, coming down onto the ground a little inside
        T = RT._surface(m, m.x0 + rng.uniform(0.5, 1.5), z)
        got = place(name, vol, T, _unit((1.0, -0.7, rng.uniform(-0.2, 0.2))), 5.0, 0.6, back=4.0)
        out.append(("outside", f"inwards_{TYPES[vt]}", name, got[0], got[1], "hit"))
        # from inside outwards and down, ending below the surface's level beyond the border: over the free edge by 4.5 delta, and into it
        u = _unit((-1.0, -0.5, rng.uniform(-0.1, 0.1)))
        d = 5.0 * u
        base = centred(vol, edge - 2.5 * u)
        conv = SM.conv64(base)
        top = max(m.height(*(edge + s * u)[::2]) - (edge + s * u)[1] for s in np.linspace(-2.5 - ext, 0.0, 33))
        y = tuned(lambda h: ST.closest_approach(name, S.moved(conv, (0, h, 0)), d, 1.0), max(top, 0.0) + 0.5 * ext + 0.2, 4.5 * dl)
        assert y is not None, vt
        out.append(("outside", f"outwards_over_{TYPES[vt]}", name, SM.shifted(base, (0, y, 0)), d, "miss"))
        out.append(("outside", f"outwards_into_{TYPES[vt]}", name, SM.shifted(base, (0, y - 9.0 * dl, 0)), d, "hit", dict(lift=np.array([0.0, 1.0, 0.0]))))
        # level, from outside into the border's free edge at the surface's height
        got = place(name, vol, edge, (1.0, 0.0, 0.0), 3.0, 0.5, back=ext + 1.0, lead=1.0)
        out.append(("outside", f"edge_side_{TYPES[vt]}", name, got[0], got[1], "hit"))
        # straight down with the footprint half off the map
        got = place(name, vol, edge, (0.0, -1.0, 0.0), 3.0, 0.5)
        out.append(("outside", f"half_off_{TYPES[vt]}", name, got[0], got[1], "hit"))
        # straight down beside the map: 4.5 delta and 1 unit from the border
        d = np.array([0.0, -4.0, 0.0])
        base = centred(vol, edge + (0, 2.0, 0))
        conv = SM.conv64(base)
        half_x = 0.5 * (S.bounds(conv)[1][0] - S.bounds(conv)[0][0])
        x = tuned(lambda o: ST.closest_approach(name, S.moved(conv, (-o, 0, 0)), d, 1.0), half_x + 0.1, 4.5 * dl)
        assert x is not None, vt
        out.append(("outside", f"beside_close_{TYPES[vt]}", name, SM.shifted(base, (-x, 0, 0)), d, "miss"))
        out.append(("outside", f"beside_unit_{TYPES[vt]}", name, SM.shifted(base, (-half_x - 1.0, 0, 0)), d, "miss"))
    return out


# ---- far: starts 1e2 to 1e4 from the touch; small volumes at the offset map's coordinates
FAR = (1e2, 1e3, 1e4)


def far(seed=7700):
    out = []
    for j, dist in enumerate(FAR):
        for name in HILLS:
            for vt in SIX:
                m, rng = the_map(name), _rng(seed, j, len(name), vt)
                vol = volume(rng, vt, variant=j % 2)
                T = RT._interior(m, rng)
                u = _down(rng, 60.0)
                got = approach(name, vol, T, u)
                assert got is not None, (dist, name, vt)
                # the same touch from `dist` back: the displacement 1.02 x as long (the end 0.02 x dist past it)
                out.append(("far", f"{TYPES[vt]}+1e{2 + j}", name, SM.shifted(got[0], (got[1] - dist) * u), 1.02 * dist * u, "hit"))
    for k, size in enumerate((1e-2, 3e-2, 0.1, 0.3, 1.0, 1e-2)):
        vt = k % 6
        m, rng = the_map("offset"), _rng(seed, 9, k)
        got = place("offset", volume(rng, vt, size), RT._interior(m, rng), _down(rng, 60.0), 4.0, 0.5)
        out.append(("far", f"offset_size{size:g}_{TYPES[vt]}", "offset", got[0], got[1], "hit"))
    return out


# ---- size ratio
def size_ratio(seed=7800):
    out = []
    m = the_map("rolling")
    for vt in SIX:
        # a volume of 1e-2, a fortieth of a cell, onto a face, an edge and a vertex
        for k, kind in enumerate(("face", "xedge_mid", "vertex")):
            rng = _rng(seed, vt, k)
            T = RT._interior(m, rng) if kind == "face" else feature_target(m, rng, kind)[0]
            got = place("rolling", volume(rng, vt, 1e-2, k % 2), T, _down(rng), 1.0, 0.5, back=0.5, lead=0.5)
            out.append(("size_ratio", f"tiny_{kind}_{TYPES[vt]}", "rolling", got[0], got[1], "hit", dict(tiny=True)))
        # volumes 20 and 40 units wide (hulls: the 36-unit geometry) down onto the hills: the touch is the highest hilltop under them
        for size in (20.0, 40.0):
            rng = _rng(seed, vt, int(size))
            vol = volume(rng, vt, size)
            if vt in (R.CAPSULE, R.CYLINDER):    # lying, so that the footprint is as wide as the size
                vol = (SM.capsule if vt == R.CAPSULE else SM.cylinder)(0.5 * size, 1.0, 0, scenes.q_axis_angle((0, 1, 0), rng.uniform(0, np.pi)))
            if vt in (R.AABB, R.OBB):            # a slab
                vol = SM.aabb((0.5 * size, 0.5, 0.3 * size)) if vt == R.AABB else SM.obb((0.5 * size, 0.5, 0.3 * size), scenes.q_axis_angle(_unit((0.1, 1, 0.05)), 0.7), 1)
            conv = SM.conv64(centred(vol, (0, 0, 0)))
            mn, mx = S.bounds(conv)
            at = np.array([rng.uniform(-31 - mn[0], 31 - mx[0]) if mx[0] - mn[0] < 62 else 0.0, 0.0, rng.uniform(2 - mn[2], 31 - mx[2]) if mx[2] - mn[2] < 29 else 16.0])
            # from a little above the highest ground under its bounds
            lo, hi = np.clip(np.floor((at + mn - (m.x0, 0, m.z0)) / m.s).astype(int), 0, m.n), np.clip(np.ceil((at + mx - (m.x0, 0, m.z0)) / m.s).astype(int), 0, m.n)
            top = np.nanmax(m.H[lo[2]:hi[2] + 1, lo[0]:hi[0] + 1])
            start = centred(vol, (at[0], top + 0.2 - mn[1], at[2]))
            hit = ST.cast("rolling", SM.conv64(start), (0.0, -4.0, 0.0))
            assert hit is not None and not hit[3], (vt, size)
            travel = hit[0] * 4.0
            out.append(("size_ratio", f"big{size:g}_{TYPES[vt]}", "rolling", SM.shifted(start, (0, 0.5 - travel, 0)), (0.0, -1.0, 0.0), "hit"))
    # a capsule 60 units long lying across both seams (from the (-x, +z) chunk over x = 0, its end over z = 0 beside the hole), straight down
    vol = SM.capsule(30.0, 0.4, 0, scenes.q_axis_angle((0, 1, 0), 0.1))
    mn, mx = S.bounds(SM.conv64(vol))
    top = np.nanmax(m.H[m.n // 2:, :])
    start = centred(vol, (0.0, top + 0.7, 3.5))
    hit = ST.cast("rolling", SM.conv64(start), (0.0, -4.0, 0.0))
    assert hit is not None and not hit[3]
    out.append(("size_ratio", "capsule60_seams", "rolling", SM.shifted(start, (0, 0.5 - 4.0 * hit[0], 0)), (0.0, -1.0, 0.0), "hit"))
    return out


# ---- wide: a footprint of more than 64 blocks across the travel
def footprint_blocks(case, pad_rel=0.0):
    """(first, last) block of the cast's footprint along the axis across the travel, by the kernel's own formula (k_q_sweep_terrain: the swept
    bounds in cells, clamped to the map, in blocks of 8; the dominant axis is x when |d.x| >= |d.z|); the kernel's padding of a few ulps left out."""
    hm = ST.map_of(case["map"])
    n, cell = 128 * hm["chunks_per_dim"], np.float32(hm["chunk_size"] / 128.0)
    mn, mx = S.bounds(("swept", case["conv"], case["d"]))
    w = 2 if abs(case["disp"][0]) >= abs(case["disp"][2]) else 0
    lo = np.float32(mn[w]) - np.float32(hm["min_corner"][w])
    hi = np.float32(mx[w]) - np.float32(hm["min_corner"][w])
    cells = [int(min(max(np.floor(v / cell), 0), n - 1)) for v in (lo, hi)]
    return cells[0] >> 3, cells[1] >> 3


def wide(seed=7900):
    """On the wide map: volumes 38 units (more than 600 cells) long lying level along the row (travel dominant in z: the row's x runs across the
    travel) or along the column (travel vertical, or |d.x| = |d.z|), coming down onto the bump at the far end: the only touch lies in the second
    pass over the blocks across the travel.  A sphere that wide meets the far bump with its flank.  No hull: the largest geometry of the matrix worlds is 33 units wide, under 520 cells.  Partners tilted so
    that the near end is the lower one and touches the near bump: the same footprint, the touch in the first 64 blocks.  Every displacement ends
    above the floor: only the bumps rise into the swept bounds."""
    out = []
    top = {counts: counts * 24.0 / 65535.0 for _, counts in ST.WIDE_BUMPS}
    far_at = -20.0 + (ST.WIDE_BUMPS[1][0] + 1) * ST.WIDE_CELL
    half = 19.0
    shapes = [
        ("capsule_x", SM.capsule(half, 0.3, 0), (0.1, -1.0, 0.6), "x", None), ("capsule_z", SM.capsule(half, 0.3, 2), (0.0, -1.0, 0.0), "z", None),
        ("cylinder_x", SM.cylinder(half, 0.3, 0), (0.0, -1.0, 0.5), "x", None), ("cylinder_z", SM.cylinder(half, 0.3, 2), (0.5, -1.0, 0.5), "z", None),
        ("AABB_x", SM.aabb((half, 0.1, 0.4)), (0.3, -1.0, -0.6), "x", None), ("AABB_z", SM.aabb((0.4, 0.1, half)), (0.0, -1.0, 0.0), "z", None),
        ("OBB_x", SM.obb((half, 0.1, 0.4), scenes.q_axis_angle((1, 0, 0), 0.4), 1), (0.0, -1.0, -0.7), "x", None),
        ("OBB_z", SM.obb((0.4, 0.1, half), scenes.q_axis_angle((0, 0, 1), 0.4), 0), (0.6, -1.0, 0.6), "z", None),
        ("sphere_x", SM.sphere(19.0), (0.0, -1.0, 0.4), "x", 15.0), ("sphere_z", SM.sphere(19.0), (0.0, -1.0, 0.0), "z", 15.0),
    ]
    for tag, vol, u, along, flank in shapes:
        u = _unit(u)
        mn, mx = S.bounds(SM.conv64(vol))
        if flank is None:     # level and centred on the map: its far end over the far bump
            at, y = 0.0, top[ST.WIDE_FAR] + 0.5 * (mx[1] - mn[1])
        else:                 # a round volume, its middle `flank` before the bump: its lowest point stays far above the floor
            r = 0.5 * (mx[0] - mn[0])
            at, y = far_at - flank, top[ST.WIDE_FAR] + np.sqrt(r * r - flank * flank)
        # (from 2 back along -u of where it would rest on the bump, so that the travel's sideways part brings it over the bump)
        start = centred(vol, np.array((at, y, 0.0) if along == "x" else (0.0, y, at)) - 2.0 * u)
        hit = ST.cast("wide", SM.conv64(start), 8.0 * u)
        assert hit is not None and not hit[3], tag
        out.append(("wide", f"far_{tag}", "wide", SM.shifted(start, (hit[0] * 8.0 - 1.0) * u), 2.0 * u, "hit", dict(second_pass=True)))
    tilt = 0.4     # radians: the near end 2 x 20.5 x sin(tilt) = 16 lower than the far end, the near bump 11 lower than the far one
    long = half / np.cos(tilt)
    partners = [("capsule_x", SM.capsule(long, 0.3, 0, scenes.q_axis_angle((0, 0, 1), tilt)), (0.1, -1.0, 0.6), "x"),
                ("cylinder_z", SM.cylinder(long, 0.3, 2, scenes.q_axis_angle((1, 0, 0), -tilt)), (0.0, -1.0, 0.0), "z"),
                ("OBB_x", SM.obb((long, 0.1, 0.4), scenes.q_axis_angle((0, 0, 1), tilt), 1), (0.0, -1.0, -0.7), "x")]
    for tag, vol, u, along in partners:
        u = _unit(u)
        mn, mx = S.bounds(SM.conv64(vol))
        y = top[ST.WIDE_NEAR] + 0.5 * (mx[1] - mn[1])
        start = centred(vol, np.array((0.0, y, 0.0)) - 2.0 * u)
        hit = ST.cast("wide", SM.conv64(start), 8.0 * u)
        assert hit is not None and not hit[3], tag
        out.append(("wide", f"near_{tag}", "wide", SM.shifted(start, (hit[0] * 8.0 - 1.0) * u), 2.0 * u, "hit", dict(second_pass=False)))
    return out


# ---- derived families
def _bases(per_type=2, families=("generic", "features"), maps=("rolling",)):
    """Kept plain hits of the base families: `per_type` of every volume type from each family (the tiny spheres apart).  The rolling map only: at the
    offset map's coordinates 4.5 delta is longer than the volumes are."""
    out = []
    for f in families:
        for vt in SIX:
            hits = [c for c in kept(f) if c["vt"] == vt and c["expect"] == "hit" and (maps is None or c["map"] in maps) and not c["tag"].startswith("point_")]
            out += hits[:per_type]
    return out


def limits():
    """The displacement of a kept hit cut so that the touch lies 4.5 delta (measured along the touch's normal) beyond its end: a miss; and so that
    it lies as far before the end: a hit with t near 1."""
    out = []
    for b in _bases():
        t, n = b["ref"][0], b["ref"][1]
        L = float(np.linalg.norm(b["d"]))
        u = b["d"] / L
        step = 4.5 * delta_at("limits", b["scale"]) / -(u @ n)
        out.append(judge(finish("limits", f"{b['family']}_{b['tag']}_short", b["map"], b["posed"], (t * L - step) * u, "miss", base=b)))
        out.append(judge(finish("limits", f"{b['family']}_{b['tag']}_reach", b["map"], b["posed"], (t * L + step) * u, "hit", base=b)))
    return out


def initial(seed=8100):
    """From kept hits: the volume at its touch, pushed 4.5 delta into the surface along the touch's normal (an initial overlap) or 4.5 delta out of it
    (a hit after a short way, no flag).  Then volumes that straddle the surface with their centre below it, boxes that enclose a hilltop, and zero
    displacements, touching and clear."""
    out = []
    for b in _bases():
        t, n = b["ref"][0], b["ref"][1]
        step = 4.5 * delta_at("initial", b["scale"])
        at_touch = SM.shifted(b["posed"], t * b["d"])
        out.append(judge(finish("initial", f"{b['family']}_{b['tag']}_deep", b["map"], SM.shifted(at_touch, -step * n), b["d"], "initial", out=n)))
        out.append(judge(finish("initial", f"{b['family']}_{b['tag']}_clear", b["map"], SM.shifted(at_touch, step * n), b["d"], "hit")))
    m = the_map("rolling")
    for vt in SIX:
        rng = _rng(seed, vt)
        vol = volume(rng, vt)
        T = RT._interior(m, rng)
        n = surface_normal(m, T)
        if vt != R.HULL:     # (a hull's origin is not its centre)
            out.append(judge(finish("initial", f"straddle_{TYPES[vt]}", "rolling", centred(vol, T - 0.05 * n), 2.0 * _down(rng, 30.0), "initial", out=n)))
        T2 = RT._interior(m, rng)
        n2 = surface_normal(m, T2)
        out.append(judge(finish("initial", f"zero_touching_{TYPES[vt]}", "rolling", centred(vol, T2 + 0.02 * n2), np.zeros(3), "initial", out=n2)))
        out.append(judge(finish("initial", f"zero_clear_{TYPES[vt]}", "rolling", centred(vol, T2 + (0.5 * extent(vol) + 0.3) * n2), np.zeros(3), "miss")))
    peaks = _peaks(m)
    for k in range(3):       # a box around a hilltop: the peak inside it, its bottom face below the surface all round
        gx, gz = peaks[(7 * k + 3) % len(peaks)]
        P = np.array([m.x0 + gx * m.s, m.H[gz, gx], m.z0 + gz * m.s])
        box = SM.aabb((0.6, 0.4, 0.6)) if k < 2 else SM.obb((0.6, 0.4, 0.6), scenes.q_axis_angle((0, 1, 0), 0.5), 1)
        out.append(judge(finish("initial", f"encloses_peak{k}", "rolling", SM.shifted(box, P - (0, 0.1, 0)), (0.3, -1.0, 0.2), "initial", out=np.array([0.0, 1.0, 0.0]))))
    return out


def direction_length(seed=8200):
    """One touch each on a face, an edge and a vertex of the rolling map, per |d| of raycast_matrix.LENGTHS: the touch half way where that leaves the
    start 4.5 delta clear, else a miss that ends 4.5 delta (along the normal) before it.  The volume types in turn."""
    out = []
    m = the_map("rolling")
    i = 0
    for k, kind in enumerate(("face", "xedge_mid", "vertex")):
        for length in RM.LENGTHS:
            vt = i % 6
            i += 1
            rng = _rng(seed, k, vt)
            T = RT._interior(m, rng) if kind == "face" else feature_target(m, rng, kind)[0]
            u = _down(rng, 60.0)
            got = approach("rolling", volume(rng, vt), T, u)
            assert got is not None
            got = (SM.shifted(got[0], got[1] * u), None, got[2])          # at the touch
            n = got[2][1]
            scale = max(1.0, np.abs(T).max() + 2.0 + length)
            step = 4.5 * delta_at("direction_length", scale) / -(u @ n)
            if 0.5 * length >= step:
                out.append(("direction_length", f"{kind}_d{length:g}_{TYPES[vt]}", "rolling", SM.shifted(got[0], -0.5 * length * u), length * u, "hit"))
            else:
                out.append(("direction_length", f"{kind}_d{length:g}_{TYPES[vt]}", "rolling", SM.shifted(got[0], -(length + step) * u), length * u, "miss"))
    return out


def ordering():
    """A static sphere or box per case on the way of a kept generic hit on the rolling map, placed by the float64 pair cast so that the volume touches
    it 4.5 delta (of travel) before the terrain or as far behind it.  Every cast sees every collider of the family: case["col_t"] and ["col"] are
    the first touch among all of them, the record must name the nearer of that and the terrain (include 7), each alone with include 3 and 4."""
    base = [c for c in kept("generic") + kept("features") if c["map"] == "rolling" and c["expect"] == "hit" and not c["tag"].startswith("point_")]
    picked = [c for vt in SIX for c in [b for b in base if b["vt"] == vt][:2]]
    out = []
    for k, b in enumerate(picked):
        L = float(np.linalg.norm(b["d"]))
        u = b["d"] / L
        step = 4.5 * delta_at("ordering", b["scale"]) * (-1.0 if k % 2 == 0 else 1.0)      # even: the collider in front
        col = SM.sphere(0.2) if k % 4 < 2 else SM.aabb((0.2, 0.15, 0.25))
        mn, mx = S.bounds(b["conv"])
        col = SM.shifted(col, (mn + mx) / 2 + (b["ref"][0] * L + 0.5 * np.linalg.norm(mx - mn) + 1.0) * u)     # ahead of the volume at its touch
        hit = S.time_of_impact(b["conv"], SM.conv64(col), 3.0 * L * u)
        assert hit is not None and not hit[3], b["tag"]
        col = SM.shifted(col, (b["ref"][0] * L + step - hit[0] * 3.0 * L) * u)
        c = finish("ordering", f"{b['tag']}_{'front' if k % 2 == 0 else 'behind'}", "rolling", b["posed"], b["d"], "hit", BOTH, base=b, front=k % 2 == 0)
        words = np.zeros(12, np.float32); words[:len(col["words"])] = col["words"]
        c.update(col_type=col["ctype"], col_words=words, col_pos=col["pos"].astype(np.float32), col_rot=col["rot"].astype(np.float32), col_hull=0)
        c["cconv"] = SM.convex_of(col["ctype"], words, c["col_pos"], c["col_rot"], 0)
        out.append(c)
    colliders = [c["cconv"] for c in out]
    for i, c in enumerate(out):
        L, dl = float(np.linalg.norm(c["d"])), delta(c)
        c["ref"] = ST.cast("rolling", c["conv"], c["d"])
        first = S.cast(c["conv"], c["d"], colliders)
        c["col"], c["col_ref"] = (first[0], first[1:]) if first is not None else (None, None)
        ok = c["ref"] is not None and not c["ref"][3] and first is not None and first[0] == i and not first[4]
        c["clearance"] = abs(first[1] - c["ref"][0]) * L if ok else 0.0
        c["collider_wins"] = bool(ok and first[1] < c["ref"][0])
        c["kept"] = bool(ok and c["collider_wins"] == c["front"] and c["clearance"] >= 4.0 * dl)
    return out


def invalid():
    nan = np.nan
    ball = SM.shifted(SM.sphere(0.5), (6.0, 6.0, 6.0))
    rows = [("nan_d", ball, (nan, -1.0, 0.0)), ("inf_d", ball, (0.0, -INF, 0.0)), ("nan_dz", ball, (0.0, -8.0, nan)),
            ("nan_position", SM.shifted(SM.sphere(0.5), (6.0, nan, 6.0)), (0.0, -8.0, 0.0)), ("inf_position", SM.shifted(SM.sphere(0.5), (INF, 6.0, 6.0)), (0.0, -8.0, 0.0)),
            ("inf_radius", SM.shifted(SM.sphere(INF), (6.0, 6.0, 6.0)), (0.0, -8.0, 0.0)), ("nan_radius", SM.shifted(SM.sphere(nan), (6.0, 6.0, 6.0)), (0.0, -8.0, 0.0)),
            ("negative_radius", SM.shifted(SM.sphere(-1.0), (6.0, 6.0, 6.0)), (0.0, -8.0, 0.0)),
            ("unknown_hull", SM.shifted(SM.hull(SM.I4, 99), (6.0, 6.0, 6.0)), (0.0, -8.0, 0.0))]
    return [("invalid", tag, "rolling", vol, d, "invalid") for tag, vol, d in rows]


_GENERATORS = dict(generic=generic, features=features, axes=axes, grazing=grazing, below=below, outside=outside, far=far, size_ratio=size_ratio, wide=wide,
                   direction_length=direction_length, invalid=invalid)
_DERIVED = dict(limits=limits, initial=initial, ordering=ordering)
_CACHE = {}


def family(name):
    """Every generated case of a family, judged by the reference; computed once per process."""
    if name not in _CACHE:
        _CACHE[name] = _DERIVED[name]() if name in _DERIVED else [judge(finish(*c[:6], **(c[6] if len(c) > 6 else {}))) for c in _GENERATORS[name]()]
    return _CACHE[name]


def kept(name):
    return [c for c in family(name) if c["kept"]]


def scene(mapname):
    """A world of one map with sweep_matrix's hull geometries.  The rolling map's also holds the `ordering` family's colliders as static entities:
    the terrain flag alone (include = 4) does not see them."""
    cases = family("ordering") if mapname == "rolling" else []
    sc = SM.scene_of(cases, "sweep_terrain_matrix_" + mapname)
    sc.heightmap = ST.map_of(mapname)
    return sc


# ---- lattice: vertical casts of tiny spheres through every kind of line of the grid
LATTICE_MAPS = ("rolling", "offset", "floor")
LATTICE_RADII = (0.0, 1e-3)


def _ulps(x, k):
    x = np.float32(x)
    for _ in range(abs(k)):
        x = np.nextafter(x, np.float32(np.inf if k > 0 else -np.inf))
    return x


def lattice(mapname, seed=8400):
    """(x, z float32 [N], height float64 [N], kinds [N]) of the casts' footprints on a map: per kind of line a few dozen spots, each at 0, +-1 and
    +-2 float32 ulps across the line (both coordinates for a vertex); every spot lies over solid ground by 2 ulps at least: the band along the map's
    border and the hole's rim is posed 2 ulps inside and straddled inwards only."""
    m = the_map(mapname)
    rng = _rng(seed, len(mapname))
    half, n = m.n // 2, m.n
    two = 2 if "chunks" in m.hm and len(m.hm["chunks"]) > 1 else 1       # (2 x 2 chunks or one)
    spots = []     # (kind, u, v, straddle x, straddle z) in cells
    for _ in range(40):
        gx, gz = RT._solid_cell(m, rng, margin=3)
        f = rng.uniform(0.05, 0.95)
        spots += [("vertex", gx, gz, True, True), ("xline", gx, gz + f, True, False), ("zline", gx + f, gz, False, True), ("diagonal", gx + f, gz + 1 - f, True, True),
                  ("block", 8 * (gx // 8), 8 * (gz // 8) + (f if _ % 2 else 0), True, True)]
    if two == 2:
        for _ in range(40):
            f = rng.uniform(0.0, 1.0)
            spots += [("seam", half, half + 2 + int(rng.integers(0, half - 4)) + (f if _ % 2 else 0), True, True),
                      ("seam", 2 + int(rng.integers(0, half - 4)) + (f if _ % 2 else 0), half, True, True)]
        spots += [("chunk_vertex", half, half, True, True)] * 1
    xs, zs, kinds = [], [], []
    for kind, u, v, sx, sz in spots:
        x, z = np.float32(m.x0 + u * m.s), np.float32(m.z0 + v * m.s)
        for kx in ((-2, -1, 0, 1, 2) if sx else (0,)):
            for kz in ((-2, -1, 0, 1, 2) if sz else (0,)):
                xs.append(_ulps(x, kx)); zs.append(_ulps(z, kz)); kinds.append(kind)
    # the band 2 ulps inside the border and the rim
    x_lo, x_hi, z_lo, z_hi = _ulps(m.x0, 2), _ulps(m.x0 + m.size, -2), _ulps(m.z0, 2), _ulps(m.z0 + m.size, -2)
    for _ in range(60):
        f = rng.uniform(0.02, 0.98)
        if two == 2:     # the hole is the chunk x > centre, z < centre
            cx, cz = np.float32(m.x0 + m.size / 2), np.float32(m.z0 + m.size / 2)
            band = [(x_lo, m.z0 + f * m.size), (x_hi, m.z0 + (0.5 + 0.5 * f) * m.size), (m.x0 + 0.5 * f * m.size, z_lo), (m.x0 + f * m.size, z_hi),
                    (_ulps(cx, -2), m.z0 + 0.5 * f * m.size), (m.x0 + (0.5 + 0.5 * f) * m.size, _ulps(cz, 2))]
        else:
            band = [(x_lo, m.z0 + f * m.size), (x_hi, m.z0 + f * m.size), (m.x0 + f * m.size, z_lo), (m.x0 + f * m.size, z_hi)]
        for x, z in band:
            xs.append(np.float32(x)); zs.append(np.float32(z)); kinds.append("border")
    xs, zs = np.array(xs, np.float32), np.array(zs, np.float32)
    h = np.array([m.height(float(x), float(z)) for x, z in zip(xs, zs)])
    # (Map.height clamps into the map: a spot a step outside a block line that is the map's border is no ground, nor is one over the hole's quarter)
    x64, z64 = xs.astype(np.float64), zs.astype(np.float64)
    solid = np.isfinite(h) & (x64 >= m.x0) & (x64 <= m.x0 + m.size) & (z64 >= m.z0) & (z64 <= m.z0 + m.size)
    return xs[solid], zs[solid], h[solid], [k for k, s in zip(kinds, solid) if s]
