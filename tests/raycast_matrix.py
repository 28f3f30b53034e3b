"""The test matrix of the ray cast (mi_world_raycast): every collider type, one collider at a time, at the rays where a float32 closed form
goes wrong; numpy only, no GPU.  tests/test_raycast.py checks the matrix itself from the exact float64 reference of tests/raycast_exact.py
alone, tests/test_gpu_raycast.py runs it on the GPU.  Built the way tests/sweep_matrix.py is, whose shape builders and hull geometries it uses:

  * a COLLIDER is posed in float64 and rounded to float32 once, when the case is finished, and so are the ray's origin, direction and max_t;
    the reference sees the rounded numbers, the same ones the GPU gets;
  * a CASE is one collider (the `ordering` family: two or three), one ray with its max_t, and a `scale` = max(1, the largest |coordinate| of
    the collider's bounds, of the origin and of the hit or closest point);
  * delta = 4 x the family's bound x scale is the offset of the grazing and derived families and the slack of the ROBUSTNESS FILTER: a case is
    kept only if the reference decides hit / miss the same way with the collider shrunk and grown by delta (its closest approach to the ray's
    segment is more than delta clear, or more than delta deep) and a hit's origin lies more than delta outside (the `inside` family: inside).
    The filter uses the reference alone, so the GPU comparison leaves no kept case out and has no budget;
  * `limits` is derived from kept hits in closed form (the reference time is known) and judged by what the exact reference says of the
    rounded numbers."""
import numpy as np

import overlap_ref as R
import raycast_exact as X
import sweep_matrix as SM
from d3d12renderer_amd import capi, scenes

KINDS = ("sphere", "capsule", "cylinder", "AABB", "box", "OBB", "hull")   # box = an AABB collider turned by its entity's pose, OBB = by its shape words
_LABEL = (R.SPHERE, R.CAPSULE, R.CYLINDER, R.AABB, R.OBB, R.OBB, R.HULL)
_VARIANT = (0, 0, 0, 0, 0, 1, 0)
FAMILIES = ("generic", "grazing", "features", "axes", "direction_length", "far", "size_ratio", "limits", "inside", "ordering")
LENGTHS = (1e-3, 1e-2, 0.1, 1.0, 30.0, 1e3, 1e4)
# The bound on |t - t_ref| |d|, on the point's distance from o + t d and from the collider's surface and on the normal's separation, PER UNIT
# OF `scale`: 4 x the largest value measured on the MI355X against the exact float64 reference, rounded up to one digit (the measured figures:
# MEASURED below).  None exceeds sweep_matrix.BOUNDS of the family with the same name.  grazing is measured at its own bound
# (delta, so the depth of its hits, follows from it): 1.6e-4 at 1e-6, 3.5e-5 at 1e-4, 2.7e-5 at 2e-4.  axes leaves out the two cases of
# test_gpu_raycast.KNOWN_ILL_CONDITIONED (8.2e-5, 6.8e-5).
MEASURED = {"generic": 5.04e-6, "grazing": 2.65e-5, "features": 8.59e-6, "axes": 1.38e-5, "direction_length": 2.49e-6, "far": 1.75e-7, "size_ratio": 1.82e-7,
            "limits": 5.04e-6, "inside": 8.49e-8, "ordering": 3.31e-6}
BOUNDS = {"generic": 3e-5, "grazing": 2e-4, "features": 4e-5, "axes": 6e-5, "direction_length": 1e-5, "far": 7e-7, "size_ratio": 8e-7, "limits": 3e-5,
          "inside": 4e-7, "ordering": 2e-5}
INF = np.inf
I4 = SM.I4


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


def _perp(rng, u):
    return _unit(np.cross(u, rng.normal(size=3)))


def exact64(col):
    """The exact reference's shape of a posed collider before rounding (placement only; the comparison uses the rounded one)."""
    return X.shape_of(col["ctype"], col["words"], col["pos"], col["rot"], SM.hulls()[col["hull"]])


def _round(col):
    words = np.zeros(12, np.float32); words[:len(col["words"])] = col["words"]
    pos, rot = col["pos"].astype(np.float32), col["rot"].astype(np.float32)
    return dict(ctype=col["ctype"], words=words, pos=pos, rot=rot, hull=col["hull"], shape=X.shape_of(col["ctype"], words, pos, rot, SM.hulls()[col["hull"]]))


def finish(family, tag, kind, col, o, d, max_t=INF, **extra):
    """The case in float32 as the GPU gets it and the exact reference's shapes of those very numbers.  col: one posed collider or a list."""
    cols = col if isinstance(col, list) else [col]
    o32, d32 = np.asarray(o, np.float64).astype(np.float32), np.asarray(d, np.float64).astype(np.float32)
    case = dict(family=family, tag=tag, kind=kind, raw=(cols, np.asarray(o, np.float64), np.asarray(d, np.float64), float(max_t)), cols=[_round(c) for c in cols],
                o32=o32, d32=d32, max_t32=np.float32(max_t), o=o32.astype(np.float64), d=d32.astype(np.float64), max_t=float(np.float32(max_t)))
    case.update(extra)
    return case


def delta(case):
    return 4.0 * BOUNDS[case["family"]] * case["scale"]


def judge(case):
    """The exact reference's answer and the robustness filter.  case["ref"] = raycast_exact.cast of the winning collider (t None on a miss),
    case["win"] = its place among the case's colliders, case["approach"] = the signed closest approach of the ray's segment to it,
    case["normals"] = the outward normals of every surface entered within delta of the entry (one, away from edges), case["kept"]."""
    o, d, mt = case["o"], case["d"], case["max_t"]
    refs = [X.cast(c["shape"], o, d, mt) for c in case["cols"]]
    hits = [(r["t"], i) for i, r in enumerate(refs) if r["t"] is not None]
    win = min(hits)[1] if hits else None
    if len(hits) > 1 and case.get("identical"):
        win = max(i for t, i in hits if t == min(hits)[0])      # byte-identical colliders: the lower WORLD index is the later one created
    shape = case["cols"][win if win is not None else 0]["shape"]
    ref = refs[win if win is not None else 0]
    approach, s = X.closest_approach(shape, o, d, mt)
    reach = [np.abs(b).max() for c in case["cols"] for b in X.bounds(c["shape"])] + [np.abs(o).max(), np.abs(ref["point"] if ref["t"] is not None else o + s * d).max()]
    case.update(ref=ref, win=win, approach=approach, scale=max(1.0, float(max(reach))))
    dl, length = delta(case), float(np.linalg.norm(d))
    start = X.sdf(shape, o)
    if case["family"] == "inside":
        kept = start < -dl
        exits = [n for t, n in ref["exits"] if (t - ref["t_exit"]) * length <= dl] if ref["t"] is not None else []
        case["exit_normals"] = exits
    elif ref["t"] is None:
        kept = all(X.closest_approach(c["shape"], o, d, mt)[0] > dl for c in case["cols"])
    else:
        kept = approach < -dl and start > dl
        if len(hits) > 1 and not case.get("identical"):          # the runner-up trails by more than twice the slack of either entry
            kept = kept and sorted(hits)[1][0] - ref["t"] > 2.0 * dl / length
    t_in = max((t for t, _ in ref["entries"]), default=0.0)
    case["normals"] = [n for t, n in ref["entries"] if (t_in - t) * length <= dl]
    case["kept"] = bool(kept)
    return case


# ---- colliders
def _random_collider(rng, kind, lo=0.05, hi=0.5, hull_geometry=0):
    return SM._random_shape(rng, _LABEL[kind], _VARIANT[kind], lo, hi, hull_geometry)[0]


def _centre(shape):
    """(a point well inside, the radius of the ball about it that the solid contains, the radius of the one that contains the solid)."""
    mn, mx = X.bounds(shape)
    c = (mn + mx) / 2 if shape[0] != X.HULL else shape[1][0].mean(axis=0)
    return c, -X.sdf(shape, c), float(np.linalg.norm(mx - mn) / 2)


# ---- generic: random pose, sizes 0.1 to 1, the origin about 6 units away, aimed at the shape with a random lateral offset: four hits, two misses
def generic(seed=5100, samples=6):
    out = []
    for kind in range(7):
        for k in range(samples):
            rng = np.random.default_rng([seed, kind, k])
            col = SM.shifted(_random_collider(rng, kind), rng.uniform(-1, 1, 3))
            c, inner, outer = _centre(exact64(col))
            u = _unit(rng.normal(size=3)); w = _perp(rng, u)
            lateral = rng.uniform(0, 0.8) * inner if k % 3 != 2 else outer * rng.uniform(1.15, 1.6)
            out.append(("generic", f"s{k}", kind, col, c - 6.0 * u + lateral * w, u, INF if k % 2 else 8.5))
    return out


# ---- silhouette features: a point T on the surface, an outward normal w there and a direction u along the surface (u . w = 0)
def _hull_features(shape, tris):
    """(a vertex with the mean normal of its faces, the midpoint of an edge between two faces that are not coplanar with the mean of their normals
    and the edge's direction, the midpoint of the edge that comes nearest to coplanar likewise)."""
    verts, normals = shape[1][0], shape[1][1]
    tris = [tuple(int(i) for i in t) for t in tris]
    v = max(range(len(verts)), key=lambda i: sum(i in t for t in tris))
    vertex = (verts[v], _unit(sum(normals[i] for i, t in enumerate(tris) if v in t)))
    edges = {}
    for i, t in enumerate(tris):
        for e in ((t[0], t[1]), (t[1], t[2]), (t[2], t[0])):
            edges.setdefault(frozenset(e), []).append(i)
    pairs = sorted((float(normals[f[0]] @ normals[f[1]]), tuple(sorted(e))) for e, f in edges.items() if len(f) == 2)
    out = [vertex]
    for _, (p, q) in (pairs[0], pairs[-1]):
        f = edges[frozenset((p, q))]
        out.append(((verts[p] + verts[q]) / 2, _unit(normals[f[0]] + normals[f[1]]), _unit(verts[q] - verts[p])))
    return out


def features_of(kind, shape, rng, tris=None):
    """[(name, T, w, u)] of the shape's silhouette features: sphere limb; capsule side and seam; cylinder side and rim; box edge and corner;
    hull vertex, sharp edge and the shared edge of its two most nearly coplanar triangles."""
    t, p = shape
    if t == X.SPHERE:
        w = _unit(rng.normal(size=3))
        w2 = _perp(rng, w)
        return [("limb", p[0] + p[1] * w, w, _perp(rng, w)), ("limb2", p[0] + p[1] * w2, w2, _perp(rng, w2))]
    if t in (X.CAPSULE, X.CYLINDER):
        a, b, r = p
        ua = _unit(b - a); w = _perp(rng, ua); along = np.cross(ua, w)
        side = ("side", (a + b) / 2 + 0.3 * (b - a) + r * w, w, _unit(along + 0.5 * ua))
        if t == X.CAPSULE:
            return [side, ("seam", b + r * w, w, along), ("end", b + r * _unit(w + ua), _unit(w + ua), along)]
        return [side, ("rim", b + r * w, _unit(w + ua), _unit(ua - w)), ("rim_along", a + r * w, _unit(w - ua), along)]
    if t == X.OBB:
        c, half, Rm = p
        return [("edge", c + Rm @ (half * (1, 1, 0.3)), _unit(Rm @ (1, 1, 0)), _unit(Rm @ (1, -1, 0.7))),
                ("corner", c + Rm @ (half * (1, -1, 1)), _unit(Rm @ (1, -1, 1)), _unit(Rm @ (1, 1, 0)))]
    vertex, sharp, flat = _hull_features(shape, tris)
    return [("vertex", vertex[0], vertex[1], _perp(rng, vertex[1])), ("edge", sharp[0], sharp[1], _unit(np.cross(sharp[2], sharp[1]) + 0.5 * sharp[2])),
            ("shared_edge", flat[0], flat[1], _unit(np.cross(flat[2], flat[1])))]


def _feature_setups(seed):
    for kind in range(7):
        rng = np.random.default_rng([seed, kind])
        col = SM.shifted(_random_collider(rng, kind, 0.2, 0.5), rng.uniform(-1, 1, 3))
        shape = exact64(col)
        for name, T, w, u in features_of(kind, shape, rng, SM.hulls()[col["hull"]][1]):
            yield kind, col, shape, name, T, w, u


# ---- grazing: the ray runs along the surface at a silhouette feature, its lateral offset solved from the reference's closest approach
def _solve(f, lo, hi):
    """The root of an increasing f between lo (f < 0) and hi (f > 0) by bisection."""
    assert f(lo) < 0 < f(hi)
    for _ in range(34):
        mid = (lo + hi) / 2
        lo, hi = (mid, hi) if f(mid) < 0 else (lo, mid)
    return (lo + hi) / 2


def grazing(seed=5200):
    """Per feature: the ray 4 delta and 16 delta clear (misses) and as deep (hits)."""
    out = []
    for kind, col, shape, name, T, w, u in _feature_setups(seed):
        start = T - 6.0 * u
        scale = max(1.0, max(np.abs(b).max() for b in X.bounds(shape)), np.abs(start).max(), np.abs(T).max())
        dl = 4.0 * BOUNDS["grazing"] * scale
        inner = _centre(shape)[1]
        for mult in (4, 16):
            for sign, what in ((1, "miss"), (-1, "hit")):
                f = lambda x: X.closest_approach(shape, start + x * w, u, 9.0)[0] - sign * mult * dl   # noqa: E731
                x = _solve(f, min((-k * 0.25 * inner for k in range(1, 9)), key=f), 0.5)               # (from the deepest of a few offsets)
                out.append(("grazing", f"{name}_k{mult}{what}", kind, col, start + x * w, u, 9.0 if mult == 4 else INF))
    return out


# ---- features: rays aimed exactly at edges, corners, rims, seams and vertices; rays with zero direction components; the cylinder's special rays
def _upright(kind, rng):
    """A capsule / cylinder along +y under the identity rotation (rotateFromTo's identity branch), only translated."""
    h, r = rng.uniform(0.2, 0.5), rng.uniform(0.1, 0.3)
    return SM.shifted((SM.capsule if kind == 1 else SM.cylinder)(h, r), rng.uniform(-1, 1, 3)), h, r


def features(seed=5300):
    out = []
    for kind, col, shape, name, T, w, u in _feature_setups(seed):
        for k, v in enumerate((w, _unit(w + 0.4 * u))):           # head-on and oblique: the far side of the feature is a hit either way
            out.append(("features", f"{name}_{'ho'[k]}", kind, col, T + 6.0 * v, -v, INF if k else 7.0))
    for kind in range(7):   # axis-parallel rays: exactly zero direction components, |d| exactly 1
        rng = np.random.default_rng([seed, kind, 1])
        col = SM.shifted(_random_collider(rng, kind, 0.2, 0.5), rng.uniform(-1, 1, 3))
        c, inner, outer = _centre(exact64(col))
        for axis, sign in ((0, 1.0), (1, -1.0), (2, 1.0), (1, 1.0)):
            e = np.zeros(3); e[axis] = sign
            off = 0.5 * inner * _unit(np.roll((0.0, 0.6, 0.8), axis)) if sign * axis != 1 else 1.5 * outer * _unit(np.roll((0.0, 0.6, 0.8), axis))
            out.append(("features", f"axis{'+-'[sign < 0]}{'xyz'[axis]}", kind, col, c + 6.0 * e + off, -e, INF))
    for kind in (1, 2):     # parallel to the axis inside and outside the radius, exactly perpendicular to it, the end / cap hit flat on
        rng = np.random.default_rng([seed, kind, 2])
        col, h, r = _upright(kind, rng)
        c = col["pos"]
        for tag, o, d in (("down_inside", (0.4 * r, 5.0, 0.3 * r), (0, -1, 0)), ("up_inside", (-0.5 * r, -5.0, 0.2 * r), (0, 1, 0)), ("centre_down", (0, 5.0, 0), (0, -2, 0)),
                          ("down_outside", (1.3 * r, 5.0, 0.0), (0, -1, 0)), ("across", (-5.0, 0.4 * h, 0.3 * r), (1, 0, 0)), ("across_z", (0.5 * r, -0.7 * h, 5.0), (0, 0, -0.5)),
                          ("across_above", (-5.0, h + 1.5 * r, 0.0), (1, 0, 0))):
            out.append(("features", tag, kind, col, c + np.asarray(o, np.float64), np.asarray(d, np.float64), INF))
    return out


# ---- axes (capsule and cylinder): the segment along every axis and next to rotateFromTo's half-turn branch, a side ray and an end ray each
def axes(seed=5400):
    out = []
    tilt = lambda a: np.array([np.sin(a) * 0.6, -np.cos(a), np.sin(a) * 0.8])   # noqa: E731  (the angle a off -y)
    dirs = [("+x", (1, 0, 0)), ("-x", (-1, 0, 0)), ("+y", (0, 1, 0)), ("-y", (0, -1, 0)), ("+z", (0, 0, 1)), ("-z", (0, 0, -1)), ("-y+1e-3", tilt(1e-3)), ("-y+1e-2", tilt(1e-2))]
    for kind in (1, 2):
        for k, (name, ax) in enumerate(dirs):
            rng = np.random.default_rng([seed, kind, k])
            h, r = rng.uniform(0.2, 0.5), rng.uniform(0.1, 0.3)
            ax = np.asarray(ax, np.float64)
            mid = rng.uniform(-0.2, 0.2, 3)
            col = SM.shifted(SM._posed(_LABEL[kind], (capi.CAPSULE, capi.CYLINDER)[kind - 1], [*(mid - h * ax), *(mid + h * ax), r]), rng.uniform(-1, 1, 3))
            c = col["pos"] + mid
            w = _perp(rng, ax)
            side = _unit(w + 0.3 * ax)
            out.append(("axes", f"{name}_side", kind, col, c + 0.4 * h * ax + 0.5 * r * np.cross(ax, w) + 6.0 * side, -side, INF))
            end = _unit(ax + 0.1 * w)
            out.append(("axes", f"{name}_end", kind, col, c + 0.4 * r * w + 6.0 * end, -end, 8.0))
            out.append(("axes", f"{name}_back", kind, col, c - 0.3 * r * w - 6.0 * end, end, INF))
    return out


# ---- direction length: one kept generic hit and one kept generic miss per type at every |d|, max_t = inf
def direction_length():
    out = []
    for kind in range(7):
        cases = [c for c in kept("generic") if c["kind"] == kind]
        for base in ([c for c in cases if c["win"] is not None][:1] + [c for c in cases if c["win"] is None][:1]):
            cols, o, d, _ = base["raw"]
            for length in LENGTHS:
                out.append(("direction_length", f"{base['tag']}_d{length:g}", kind, cols, o, _unit(d) * length, INF))
    return out


# ---- far: generic and features cases translated as a whole, in float64 before rounding, by the sweep matrix's offsets
def far():
    out = []
    for k, (_, tag, kind, col, o, d, mt) in enumerate(generic() + features()):
        for j, off in enumerate(SM.FAR_OFFSETS):
            if (k + j) % 2 == 0 or tag.startswith("axis") or "_" not in tag:
                out.append(("far", f"{tag}+1e{2 + j}", kind, SM.shifted(col, off), np.asarray(o, np.float64) + off, d, mt))
    return out


# ---- size ratio: a collider of 1e-2 from 20 and from 1e3 units away; a 50-unit round shape, a 200-unit box, the 30 x hull hit off-centre from nearby
def size_ratio(seed=5600):
    out = []
    skew = scenes.q_axis_angle(_unit((1, 2, 3)), np.pi / 6)
    for kind in range(7):
        for k, dist in enumerate((20.0, 1e3, 20.0)):
            rng = np.random.default_rng([seed, kind, k])
            col = SM.shifted(SM._sized(rng, _LABEL[kind], 1e-2, _VARIANT[kind]), rng.uniform(-1, 1, 3))
            c, inner, outer = _centre(exact64(col))
            u = _unit(rng.normal(size=3)); w = _perp(rng, u)
            out.append(("size_ratio", f"tiny{k}", kind, col, c - dist * u + (0.1 * inner if k < 2 else 0.5 + outer) * w, u, INF))
        for k in range(3):
            rng = np.random.default_rng([seed, kind, 3 + k])
            if kind >= 3 and kind < 6:
                col = SM.aabb((100.0, 10.0, 100.0)) if kind == 3 else SM.obb((100.0, 10.0, 100.0), skew, _VARIANT[kind])
                g = R.qmat(skew) if kind > 3 else np.eye(3)
                aim = g @ np.array(((35.0, 9.0, -22.0), (-60.0, 9.0, 41.0), (80.0, 2.0, 99.0))[k])
                u = g @ _unit(((0.3, -1.0, 0.2), (-0.2, -1.0, -0.4), (0.1, -0.3, -1.0))[k])
            elif kind == 6:
                col = SM.hull(SM._rand_q(rng), 1)
                aim = _centre(exact64(col))[0] + rng.uniform(-8, 8, 3); u = _unit(rng.normal(size=3))
            else:
                col = SM.sphere(25.0) if kind == 0 else SM.capsule(25.0, 10.0, 1, SM._rand_q(rng)) if kind == 1 else SM.cylinder(25.0, 15.0, 1, SM._rand_q(rng))
                shape = exact64(col)
                aim = (_unit(rng.normal(size=3)) * 15.0 if kind == 0 else
                       shape[1][0] + (0.5 + 0.36 * (k - 1)) * (shape[1][1] - shape[1][0]) + _perp(rng, shape[1][1] - shape[1][0]) * 6.0)
                u = _unit(rng.normal(size=3))
            cc = rng.uniform(-3, 3, 3)
            col = SM.shifted(col, cc); aim = aim + cc
            entry = X.cast(exact64(col), aim - 400.0 * u, u)
            assert entry["t"] is not None and not entry["inside"], (kind, k)
            reach = 3.0 + 1.5 * k
            out.append(("size_ratio", f"big{k}", kind, col, entry["point"] - reach * u, u, INF if k else 2.0 * reach))
    return out


# ---- inside: the origin in the solid, one case per sub-part; what the header of mi_world_raycast documents (expect: "t0", "miss", "exit")
def inside(seed=5800):
    out = []
    rng = np.random.default_rng(seed)
    place = lambda col: SM.shifted(col, rng.uniform(-1, 1, 3))   # noqa: E731
    col = place(SM.sphere(0.4))
    for k in range(3):
        out.append(("inside", f"sphere{k}", 0, col, col["pos"] + rng.uniform(-0.15, 0.15, 3), _unit(rng.normal(size=3)) * (1.0, 0.01, 50.0)[k], INF, dict(expect="t0")))
    for kind in (1, 2):   # upright: the cylinder test's frame is the entity's, so what it does is read off the direction's y
        col, h, r = _upright(kind, rng)
        c = col["pos"]
        mid = c + (0.2 * r, 0.3 * h, -0.1 * r)
        # in the middle: a direction with an axial part makes the cylinder test answer with the cap BEHIND the origin, a negative t: no hit;
        # exactly perpendicular to the axis neither cap is tried: t = 0
        out.append(("inside", "middle_down", kind, col, mid, (0.05, -1.0, 0.02), INF, dict(expect="miss")))
        out.append(("inside", "middle_up", kind, col, mid, (0.0, 3.0, 0.0), INF, dict(expect="miss")))
        out.append(("inside", "middle_across", kind, col, mid, (1.0, 0.0, 0.0), INF, dict(expect="t0")))
        out.append(("inside", "middle_across_z", kind, col, mid, (0.0, 0.0, -0.2), INF, dict(expect="t0")))
        if kind == 1:   # in an end sphere, beyond the segment's end: t = 0 unless the cylinder part answers first (outwards: its cap behind, no hit)
            end = c + (0.1 * r, h + 0.5 * r, 0.1 * r)
            out.append(("inside", "end_across", kind, col, end, (1.0, 0.0, 0.0), INF, dict(expect="t0")))
            out.append(("inside", "end_inwards", kind, col, end, (0.0, -1.0, 0.0), INF, dict(expect="t0")))
            out.append(("inside", "end_outwards", kind, col, end, (0.0, 1.0, 0.0), INF, dict(expect="miss")))
    for kind in (3, 4, 5):
        col = place(_random_collider(rng, kind, 0.3, 0.5))
        c, inner, _ = _centre(exact64(col))
        for k in range(3):
            out.append(("inside", f"box{k}", kind, col, c + 0.4 * inner * _unit(rng.normal(size=3)), _unit(rng.normal(size=3)) * (1.0, 0.01, 50.0)[k], INF, dict(expect="miss")))
    col = place(SM.hull(SM._rand_q(rng)))
    c, inner, _ = _centre(exact64(col))
    for k in range(4):
        out.append(("inside", f"hull{k}", 6, col, c + 0.4 * inner * _unit(rng.normal(size=3)), _unit(rng.normal(size=3)) * (1.0, 0.01, 50.0, 1.0)[k], INF, dict(expect="exit")))
    return out


# ---- ordering: two and three colliders in line along one ray under one entity range, their entries 4 delta and 16 delta apart
def ordering(seed=5900):
    out = []
    rows = [((0, 3), 4), ((4, 1), 16), ((2, 6, 0), 4), ((5, 0, 1), 16), ((6, 2), 4), ((1, 5, 3), 16), ((3, 4), 4)]
    for k, (kinds, mult) in enumerate(rows):
        rng = np.random.default_rng([seed, k])
        u = _unit(rng.normal(size=3)) if 3 not in kinds else _unit((0.3, -1.0, 0.2))
        o = rng.uniform(-1, 1, 3) - 6.0 * u
        dl = 4.0 * BOUNDS["ordering"] * 8.0
        cols = []
        for j, kind in enumerate(rng.permutation(len(kinds))):
            col = _random_collider(rng, kinds[kind], 0.2, 0.5)
            col = SM.shifted(col, o + 6.0 * u - _centre(exact64(col))[0])
            col = SM.shifted(col, (6.0 + kind * mult * dl - X.cast(exact64(col), o, u)["t"]) * u)
            cols.append(col)
        out.append(("ordering", f"row{k}_k{mult}", kinds[0], cols, o, u, INF))
    rng = np.random.default_rng([seed, 99])
    col = SM.shifted(SM.sphere(0.3), rng.uniform(-1, 1, 3))
    out.append(("ordering", "identical", 0, [col, dict(col), dict(col)], col["pos"] - 5.0 * _unit((1, 2, 2)) + (0.05, 0, 0), _unit((1, 2, 2)), INF, dict(identical=True)))
    # the nearest collider is as large as shape_zoo's ground (the query grid's large list); a small sphere's entry lies 16 delta behind its top
    u = _unit((0.2, -1.0, 0.1)); o = np.array((3.0, 5.0, -2.0))
    dl = 4.0 * BOUNDS["ordering"] * 100.0
    ground = SM.shifted(SM.aabb((100.0, 2.0, 100.0)), (0, -2.0, 0))
    ball = SM.shifted(SM.sphere(0.3), o + 5.0 * u)
    ball = SM.shifted(ball, (X.cast(exact64(ground), o, u)["t"] + 16 * dl - X.cast(exact64(ball), o, u)["t"]) * u)
    out.append(("ordering", "large_list", 3, [ball, ground], o, u, INF))
    return out


# ---- the families, judged once per process
_GENERATORS = dict(generic=generic, grazing=grazing, features=features, axes=axes, direction_length=direction_length, far=far, size_ratio=size_ratio,
                   inside=inside, ordering=ordering)
_CACHE = {}


def _make(c):
    extra = c[7] if len(c) > 7 else {}
    return judge(finish(*c[:7], **extra))


def limits():
    """From the kept hits of generic and direction_length (reference time t, |d| = L, delta of this family at the base's scale):
      short   max_t = t - delta / L: a miss;    reach   max_t = t + delta / L: the same hit;
      near    the origin moved forward to delta in front of the surface: a hit at t = delta / L."""
    out = []
    for base in kept("generic") + kept("direction_length"):
        if base["win"] is None:
            continue
        cols, o, d, _ = base["raw"]
        t, L = base["ref"]["t"], float(np.linalg.norm(base["d"]))
        dl = 4.0 * BOUNDS["limits"] * base["scale"]
        tag = base["tag"] if base["family"] == "direction_length" else base["tag"] + "_d1"
        for what, c in (("short", finish("limits", f"{tag}_short", base["kind"], cols, base["o"], base["d"], t - dl / L, expect=None)),
                        ("reach", finish("limits", f"{tag}_reach", base["kind"], cols, base["o"], base["d"], t + dl / L, expect=t)),
                        ("near", finish("limits", f"{tag}_near", base["kind"], cols, base["o"] + (t - dl / L) * base["d"], base["d"], INF, expect=dl / L))):
            c = judge(c)
            # closed form: no filter; kept when the exact reference of the rounded numbers decides as intended, with half of delta to spare
            ref_t = c["ref"]["t"]
            if what == "short":
                c["kept"] = ref_t is None and X.cast(c["cols"][0]["shape"], c["o"], c["d"])["t"] - c["max_t"] > 0.5 * dl / L
            elif what == "reach":
                c["kept"] = ref_t is not None and c["max_t"] - ref_t > 0.5 * dl / L
            else:
                c["kept"] = ref_t is not None and not c["ref"]["inside"] and ref_t * L > 0.5 * dl
            out.append(c)
    return out


def family(name):
    """Every generated case of a family, judged by the exact reference (case["ref"], case["kept"]); computed once per process."""
    if name not in _CACHE:
        _CACHE[name] = limits() if name == "limits" else [_make(c) for c in _GENERATORS[name]()]
    return _CACHE[name]


def kept(name):
    """The cases the GPU comparison runs."""
    return [c for c in family(name) if c["kept"]]


def counts(cases):
    """Per collider kind: [generated, kept, kept hits, kept misses]."""
    table = {k: [0, 0, 0, 0] for k in range(7)}
    for c in cases:
        m = table[c["kind"]]
        m[0] += 1; m[1] += c["kept"]; m[2] += bool(c["kept"] and c["win"] is not None); m[3] += bool(c["kept"] and c["win"] is None)
    return table


# ---- a world of one family: one static entity with one collider per collider of every case; ray i sees the entities of case i
def scene_of(cases, name="raycast_matrix"):
    """(the scene, per case the entity range [first, first + colliders))."""
    flat = [(c, k) for c in cases for k in c["cols"]]
    n = len(flat)
    e = scenes.make_entities(n, capi.ENTITY_STATIC)
    col = scenes.make_colliders(n, capi.SPHERE)
    for i, (_, k) in enumerate(flat):
        e["position"][i] = k["pos"]; e["rotation"][i] = k["rot"]
        col["type"][i] = k["ctype"]; col["shape"][i, :12] = k["words"]; col["hull_geometry"][i] = k["hull"]
    firsts = np.cumsum([0] + [len(c["cols"]) for c in cases])
    ranges = np.array([(firsts[i], firsts[i + 1]) for i in range(len(cases))], np.uint32)
    return scenes.Scene(name, e, np.arange(n, dtype=np.uint32), col, 10, hulls=list(SM.hulls())), ranges
