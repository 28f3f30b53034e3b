"""The pair-level test matrix of the shape cast (mi_world_sweep): every volume type against every collider type, one collider at a time, at the
configurations where a float32 GJK ray cast goes wrong; numpy only, no GPU.  tests/test_sweep.py checks the matrix itself from the float64
reference of tests/sweep_ref.py alone, tests/test_gpu_sweep.py runs it on the GPU.

  * a SHAPE is built in float64 (`_posed`: collider type, shape words, pose, hull geometry), moved and turned in float64, and rounded to float32
    once, when the case is finished; the reference sees the rounded numbers, the same ones the GPU gets;
  * a CASE is a volume, a displacement, one collider and a `scale` = max(1, the largest |coordinate| either shape reaches during the cast);
  * the BASE families (generic, aligned, grazing, far, size_ratio, displacement) hold all 36 pairs; the DERIVED ones rescale a base hit in
    closed form (its reference time is known) and cost no reference work;
  * delta = 4 x the family's bound x scale is the offset of the grazing and derived families and the slack of the ROBUSTNESS FILTER: a base
    case is kept only if the reference decides hit / miss the same way with the shapes shrunk and grown by delta and no hit starts
    overlapping, so the GPU comparison leaves no case out."""
import numpy as np

import overlap_ref as R
import sweep_ref as S
from d3d12renderer_amd import capi, scenes

TYPES = ("sphere", "capsule", "cylinder", "AABB", "OBB", "hull")   # the matrix's axes, in the order of overlap_ref's type constants
PAIRS = [(v, c) for v in range(6) for c in range(6)]
BASE_FAMILIES = ("generic", "aligned", "grazing", "far", "size_ratio", "displacement")
DERIVED_FAMILIES = ("starts_just_clear", "starts_just_inside", "ends_just_short", "just_reaches", "zero_radius", "far_starts_just_clear", "far_starts_just_inside")
# The bound on |t - t_ref| * |d|, on the point's distance from the collider and on the normal's separation, PER UNIT OF `scale`.  The families
# whose coordinates stay in the regime of the cast set of test_gpu_sweep.py use its BOUND; the scaled ones 4 x the largest value measured on the
# GPU against the float64 reference, rounded up to one digit (measured: far 1.23e-5, size_ratio 1.66e-6 without the two casts that end
# unconverged - test_gpu_sweep.KNOWN_UNCONVERGED holds those to their own figures -, displacement 1.99e-6; what they are: the comment at
# BOUND in test_gpu_sweep.py).
UNIT_BOUND = 3e-4
BOUNDS = {"generic": UNIT_BOUND, "aligned": UNIT_BOUND, "grazing": UNIT_BOUND, "far": 5e-5, "size_ratio": 7e-6, "displacement": 8e-6}
BOUNDS.update({f: BOUNDS["far"] if f.startswith("far_") else UNIT_BOUND for f in DERIVED_FAMILIES})
I4 = np.array([0.0, 0.0, 0.0, 1.0])
FAR_OFFSETS = (np.array([137.3, -211.7, 98.1]), np.array([1031.1, 877.3, -1204.9]))

_HULLS = []


PRISM_SIDES = 65


def _outward(verts, tris):
    """The triangles wound so that their normals point away from the vertex centroid."""
    c = verts.mean(axis=0); out = []
    for a, b, cc in tris:
        n = np.cross(verts[b] - verts[a], verts[cc] - verts[a])
        out.append((a, cc, b) if np.dot(n, verts[a] - c) < 0 else (a, b, cc))
    return np.asarray(out, np.uint32)


def _cube_hull():
    """The unit cube (half-size 0.5) as a hull of 8 vertices: every support direction along an axis ties four ways, exactly."""
    v = np.array([(x, y, z) for x in (-0.5, 0.5) for y in (-0.5, 0.5) for z in (-0.5, 0.5)], np.float64)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    return v.astype(np.float32), _outward(v, [t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))])


def _prism_hull(n=PRISM_SIDES, radius=0.5, half=0.3):
    """A prism over a regular n-gon, 2 n = 130 vertices: vertex i of the bottom cap (y = -half) and n + i of the top cap are mirror images, the
    n vertices of a cap are coplanar exactly, and a scan in strides of 64 lanes visits every lane at least twice."""
    ang = 2.0 * np.pi * np.arange(n) / n
    ring = np.stack([radius * np.cos(ang), np.zeros(n), radius * np.sin(ang)], axis=1)
    v = np.concatenate([ring - (0, half, 0), ring + (0, half, 0)])
    tris = [(0, i, i + 1) for i in range(1, n - 1)] + [(n, n + i, n + i + 1) for i in range(1, n - 1)]
    tris += [t for i in range(n) for j in [(i + 1) % n] for t in ((i, j, n + j), (i, n + j, n + i))]
    return v.astype(np.float32), _outward(v.astype(np.float32).astype(np.float64), tris)


def hulls():
    """The hull geometries of every matrix world: 0 = overlap_ref.volume_hull() (radius 0.6); 1 = the same 30 times larger with its vertices
    tens of units from its origin; 2 = the same at a size of 1e-2; 3 = the unit cube; 4 = a prism of 130 vertices (tests/contact_matrix.py)."""
    if not _HULLS:
        v, t = R.volume_hull()
        _HULLS.extend([(v, t), ((v.astype(np.float64) * 30.0 + (25.0, 10.0, -15.0)).astype(np.float32), t), ((v.astype(np.float64) / 120.0).astype(np.float32), t),
                       _cube_hull(), _prism_hull()])
    return _HULLS


# ---- shapes in float64
def _posed(label, ctype, words, pos=(0, 0, 0), rot=I4, hull=0):
    return dict(label=label, ctype=ctype, words=np.asarray(words, np.float64), pos=np.asarray(pos, np.float64), rot=np.asarray(rot, np.float64), hull=hull)


def _axis(i, h):
    a = np.zeros(3); a[i] = h
    return a


def sphere(r):
    return _posed(R.SPHERE, capi.SPHERE, [0, 0, 0, r])


def capsule(h, r, axis=1, rot=I4):
    return _posed(R.CAPSULE, capi.CAPSULE, [*-_axis(axis, h), *_axis(axis, h), r], rot=rot)


def cylinder(h, r, axis=1, rot=I4):
    return _posed(R.CYLINDER, capi.CYLINDER, [*-_axis(axis, h), *_axis(axis, h), r], rot=rot)


def aabb(half):
    half = np.asarray(half, np.float64)
    return _posed(R.AABB, capi.AABB, [*-half, *half])


def obb(half, q, variant=0):
    """A box under the rotation q: an AABB collider turned by its pose (variant 0) or an OBB collider turned by its shape words (1)."""
    half = np.asarray(half, np.float64)
    return _posed(R.OBB, capi.AABB, [*-half, *half], rot=q) if variant == 0 else _posed(R.OBB, capi.OBB, [*q, 0, 0, 0, *half])


def hull(q=I4, geometry=0):
    return _posed(R.HULL, capi.HULL, [0, 0, 0, 1, 0, 0, 0], rot=q, hull=geometry)


def shifted(p, off):
    return dict(p, pos=p["pos"] + np.asarray(off, np.float64))


def turned(p, g):
    """The shape turned about the world's origin by the quaternion g (never an AABB unless g is the identity)."""
    if np.array_equal(g, I4):
        return p
    assert p["label"] != R.AABB
    return dict(p, pos=R.qmat(g) @ p["pos"], rot=scenes.q_mul(g, p["rot"]))


def convex_of(ctype, words, pos, rot, hull_geometry):
    return S.convex(R.world_shape(ctype, words, pos, rot), hulls()[hull_geometry][0] if ctype == capi.HULL else None)


def conv64(p):
    """The reference's shape of a posed shape before rounding (placement only; the comparison uses the rounded one)."""
    return convex_of(p["ctype"], p["words"], p["pos"], p["rot"], p["hull"])


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


def _rand_q(rng):
    return _unit(rng.normal(size=4))


def _perp(rng, u):
    w = np.cross(u, rng.normal(size=3))
    return _unit(w)


# ---- cases
def finish(family, tag, vol, col, d, ref=None):
    """The case in float32 as the GPU gets it, the reference's shapes of those very numbers, and the scale."""
    v = capi.make_volume(vol["ctype"], vol["words"], vol["pos"], vol["rot"], vol["hull"])
    d32 = np.asarray(d, np.float64).astype(np.float32)
    words = np.zeros(12, np.float32); words[:len(col["words"])] = col["words"]
    pos, rot = col["pos"].astype(np.float32), col["rot"].astype(np.float32)
    vconv = convex_of(int(v["type"][0]), v["shape"][0], v["position"][0], v["rotation"][0], vol["hull"])
    cconv = convex_of(col["ctype"], words, pos, rot, col["hull"])
    dd = d32.astype(np.float64)
    reach = [np.abs(b).max() for s in (vconv, S.moved(vconv, dd), cconv) for b in S.bounds(s)]
    return dict(family=family, tag=tag, vt=vol["label"], ct=col["label"], vol=vol, col=col, volume=v, disp=d32, d=dd, col_type=col["ctype"], col_words=words,
                col_pos=pos, col_rot=rot, col_hull=col["hull"], vconv=vconv, cconv=cconv, scale=max(1.0, float(max(reach))), ref=ref)


def delta(case):
    return 4.0 * BOUNDS[case["family"]] * case["scale"]


def judge(case):
    """The reference's answer and the robustness filter: case["ref"] = the hit (t, normal, point, initial) or None, case["kept"] = the decision
    is the same with the shapes shrunk and grown by delta and a hit does not start within delta of touching."""
    dl = delta(case)
    hit = S.time_of_impact(case["vconv"], case["cconv"], case["d"])
    case["ref"] = hit
    if hit is None:
        case["kept"] = S.closest_approach(case["vconv"], case["cconv"], case["d"]) > dl   # (= the cast of the shapes grown by delta misses too)
    else:
        case["kept"] = (not hit[3] and S.gap(case["vconv"], case["cconv"]) > dl and
                        S.time_of_impact(case["vconv"], case["cconv"], case["d"], slack=-dl, plain=hit) is not None)
    return case


def _approach(vol, col, u, reach):
    """How far `vol` travels along the unit vector u until it touches `col` (float64 shapes; reach = the longest travel tried), or None."""
    hit = S.time_of_impact(conv64(vol), conv64(col), reach * u)
    return None if hit is None or hit[3] else hit[0] * reach


# ---- generic: random orientations, sizes 0.1 to 1, started about 6 units away and aimed at the collider with a small lateral offset
def _random_shape(rng, label, variant, lo=0.05, hi=0.5, hull_geometry=0):
    """(shape, radius of a ball about its centre that it contains) with half-size in [lo, hi]."""
    h = rng.uniform(lo, hi); q = _rand_q(rng)
    if label == R.SPHERE:
        return sphere(h), h
    if label == R.CAPSULE:
        return capsule(h, 0.4 * h, 1, q), 0.4 * h
    if label == R.CYLINDER:
        return cylinder(h, 0.6 * h, 1, q), 0.6 * h
    half = h * rng.uniform(0.5, 1.0, 3)
    if label == R.AABB:
        return aabb(half), half.min()
    if label == R.OBB:
        return obb(half, q, variant), half.min()
    return hull(q, hull_geometry), 0.0   # (its origin is not its centre: no ball is claimed)


def _generic_setup(seed, vt, ct, k):
    rng = np.random.default_rng([seed, vt, ct, k])
    vol, rv = _random_shape(rng, vt, k % 2)
    col, rc = _random_shape(rng, ct, (k + 1) % 2)
    cc = rng.uniform(-1, 1, 3); u = _unit(rng.normal(size=3)); w = _perp(rng, u)
    return rng, vol, shifted(col, cc), cc, u, w, rv + rc


def generic(seed=4100, samples=3):
    out = []
    for vt, ct in PAIRS:
        for k in range(samples):
            rng, vol, col, cc, u, w, inner = _generic_setup(seed, vt, ct, k)
            out.append(("generic", f"s{k}", shifted(vol, cc - 6.0 * u + rng.uniform(0, 0.6) * inner * w), col, 8.5 * u))
    return out


# ---- grazing: the generic set-up, the lateral offset chosen from the reference so that the path's closest approach is +-k delta from touching
def _root_from_outside(f, x0, x1, tol):
    """The root of a convex increasing f by the secant rule from two points beyond it (the iterates then stay beyond it)."""
    f0, f1 = f(x0), f(x1)
    for _ in range(30):
        if abs(f1) <= tol:
            return x1
        x0, f0, x1 = x1, f1, x1 - f1 * (x1 - x0) / (f1 - f0)
        f1 = f(x1)
    raise RuntimeError("no root")


def grazing(seed=4200):
    """Per pair two set-ups: k = 4 for the first, k = 16 for the second, each as a miss (k delta clear) and as a hit (k delta deep)."""
    out = []
    for vt, ct in PAIRS:
        for k, mult in enumerate((4, 16)):
            rng, vol, col, cc, u, w, _ = _generic_setup(seed, vt, ct, k)
            base = shifted(vol, cc - 6.0 * u)
            d = 8.5 * u
            vc, c = conv64(base), conv64(col)

            def clear_by(o, m):   # the closest approach at the lateral offset o, less m x delta there
                v = S.moved(vc, o * w)
                reach = max(np.abs(b).max() for s in (v, S.moved(v, d), c) for b in S.bounds(s))
                return S.closest_approach(v, c, d) - m * 4.0 * BOUNDS["grazing"] * max(1.0, reach)
            o2 = _root_from_outside(lambda o: clear_by(o, 2 * mult), 4.0, 3.5, 2e-5)     # (to half a percent of delta: the offsets need no more)
            o1 = _root_from_outside(lambda o: clear_by(o, mult), o2, o2 + 0.05, 2e-5)
            out.append(("grazing", f"k{mult}miss", shifted(base, o1 * w), col, d))
            # the hit side: as deep as the miss side is clear, by the slope of the closest approach between k delta and 2 k delta
            out.append(("grazing", f"k{mult}hit", shifted(base, (3.0 * o1 - 2.0 * o2) * w), col, d))
    return out


# ---- aligned: shared axes, degenerate feature pairs
def _hull_face_rotation(geometry, face, towards):
    """(quaternion, the face's centroid after it) turning the outward normal of triangle `face` of the hull geometry onto `towards`."""
    verts, tris = hulls()[geometry]
    a, b, c = (verts[i].astype(np.float64) for i in tris[face])
    n = _unit(np.cross(b - a, c - a)); t = _unit(towards)
    axis = np.cross(n, t); s = np.linalg.norm(axis)
    q = scenes.q_axis_angle(axis / s, np.arctan2(s, n @ t)) if s > 1e-9 else (I4 if n @ t > 0 else np.array([1.0, 0, 0, 0]))
    return q, R.qmat(q) @ ((a + b + c) / 3)


def _aligned_shape(rng, label, k, is_volume, variant):
    h = rng.uniform(0.2, 0.5)
    if label == R.SPHERE:
        return sphere(h)
    if label == R.CAPSULE:
        return capsule(h, 0.4 * h, 0)                 # along x: parallel to the faces, the x edges and the other capsule
    if label == R.CYLINDER:
        return cylinder(h, 0.6 * h, (1, 0, 2)[k])    # k 0: caps flat onto what is above / below; otherwise its side along it
    half = h * rng.uniform(0.5, 1.0, 3)
    if label == R.AABB:
        return aabb(half)
    if label == R.OBB:   # the same axes through a half or quarter turn (the half turn is exact in float32)
        return obb(half, (np.array([1.0, 0, 0, 0]), scenes.q_axis_angle((0, 0, 1), np.pi / 2), scenes.q_axis_angle((1, 0, 0), np.pi / 2))[k], variant)
    q, centroid = _hull_face_rotation(0, int(rng.integers(len(hulls()[0][1]))), (0, -1, 0) if is_volume else (0, 1, 0))
    return shifted(hull(q), (-centroid[0], 0, -centroid[2]))   # a face flat against the other shape, its centroid on the y axis


def aligned(seed=4300):
    """Per pair: k 0 = centred, flat onto flat, displacement exactly along -y; k 1 = half-overlapping along x, the volume's lower z edge aimed at
    the collider's upper z edge, displacement exactly along the face diagonal (0, -1, -1); k 2 = half-overlapping in x and z, along -y, and the
    whole configuration under one random rotation (pairs with an AABB stay axis-aligned)."""
    out = []
    for vt, ct in PAIRS:
        for k in range(3):
            rng = np.random.default_rng([seed, vt, ct, k])
            vol, col = _aligned_shape(rng, vt, k, True, k % 2), _aligned_shape(rng, ct, k, False, (k + 1) % 2)
            (vmn, vmx), (cmn, cmx) = S.bounds(conv64(vol)), S.bounds(conv64(col))
            vh, ch = (vmx - vmn) / 2, (cmx - cmn) / 2
            if k == 1:
                u = np.array([0.0, -1.0, -1.0]) / np.sqrt(2.0)
                off = np.array([0.5 * vh[0], cmx[1] - vmn[1] + 4.0, cmx[2] - vmn[2] + 4.0])
            else:
                u = np.array([0.0, -1.0, 0.0])
                off = np.array([0.0, cmx[1] - vmn[1] + 5.0, 0.0]) if k == 0 else np.array([0.5 * (vh[0] + ch[0]), cmx[1] - vmn[1] + 5.0, 0.5 * min(vh[2], ch[2])])
            vol = shifted(vol, off)
            g = _rand_q(rng) if k == 2 and R.AABB not in (vt, ct) else I4
            cc = rng.uniform(-1, 1, 3)
            out.append(("aligned", f"s{k}", shifted(turned(vol, g), cc), shifted(turned(col, g), cc), R.qmat(g) @ (8.0 * u)))
    return out


# ---- far: generic and aligned cases translated as a whole, in float64 before rounding
def far():
    gen, ali = generic(samples=1), aligned()
    out = []
    for i in range(36):
        for k, ((_, tag, vol, col, d), off) in enumerate(((gen[i], FAR_OFFSETS[0]), (ali[3 * i], FAR_OFFSETS[1]), (ali[3 * i + 2], FAR_OFFSETS[0]), (ali[3 * i + 1], FAR_OFFSETS[1]))):
            out.append(("far", f"{'ga'[k > 0]}{tag}+1e{2 + k % 2}", shifted(vol, off), shifted(col, off), d))
    return out


# ---- size ratio
def _sized(rng, label, size, variant):
    """A shape of that overall size (half of it as its half-size) under a random rotation; hulls: the geometry nearest to it."""
    if label == R.HULL:
        return hull(_rand_q(rng), 2 if size < 0.1 else 1 if size > 5 else 0)
    return _random_shape(rng, label, variant, 0.5 * size, 0.5 * size)[0]


def size_ratio(seed=4500):
    """Per pair: k 0, 1 = a volume of size 1e-2 onto a box 200 units wide (landing tens of units off its centre; the OBB turned 30 degrees about a
    skew axis), onto a 50-unit sphere / capsule / cylinder, onto the hull geometry whose vertices lie tens of units from its origin; k 2 = a
    20-unit volume onto a collider of size 1e-2."""
    out = []
    skew = scenes.q_axis_angle(_unit((1, 2, 3)), np.pi / 6)
    for vt, ct in PAIRS:
        for k in range(3):
            rng = np.random.default_rng([seed, vt, ct, k])
            u = _unit(rng.normal(size=3))
            if k == 2:
                vol, col, aim = _sized(rng, vt, 20.0, 0), _sized(rng, ct, 1e-2, 1), rng.uniform(-2, 2, 3)
            else:
                vol = _sized(rng, vt, 1e-2, k)
                if ct in (R.AABB, R.OBB):
                    col = aabb((100.0, 10.0, 100.0)) if ct == R.AABB else obb((100.0, 10.0, 100.0), skew, k)
                    g = R.qmat(skew) if ct == R.OBB else np.eye(3)
                    aim = g @ np.array(((35.0, 10.0, -22.0), (-60.0, 10.0, 41.0))[k])     # on the top face
                    u = g @ _unit((0.3, -1.0, (0.2, -0.4)[k]))
                elif ct == R.HULL:
                    col = hull(_rand_q(rng), 1)
                    aim = conv64(col)[1].mean(axis=0) + rng.uniform(-4, 4, 3)
                else:
                    col = sphere(25.0) if ct == R.SPHERE else capsule(25.0, 10.0, 1, _rand_q(rng)) if ct == R.CAPSULE else cylinder(25.0, 15.0, 1, _rand_q(rng))
                    aim = rng.uniform(-6, 6, 3)
            cc = rng.uniform(-3, 3, 3)
            col = shifted(col, cc); aim = aim + cc
            (vmn, vmx), (cmn, cmx) = S.bounds(conv64(vol)), S.bounds(conv64(col))
            back = np.linalg.norm(vmx - vmn) + np.linalg.norm(cmx - cmn) + 5.0
            vol = shifted(vol, aim - back * u - (vmn + vmx) / 2)                # its bounds' centre on the line through `aim`, clear of the collider
            travel = _approach(vol, col, u, 2.0 * back)
            assert travel is not None, (vt, ct, k)
            reach = 3.0 if k < 2 else 6.0
            out.append(("size_ratio", ("tiny", "tiny", "big")[k] + str(k), shifted(vol, (travel - reach) * u), col, 1.5 * reach * u))
    return out


# ---- displacement length: one start and direction per pair, |d| from 1e-3 to 1e4, the collider placed so that t lands near 0, near 1, in between
DISPLACEMENTS = ((1e4, 0.01), (30.0, 0.5), (0.1, 0.8), (1e3, 0.99), (1e-3, None))   # (|d|, t of the touch; None: the collider 0.05 ahead, a miss)


def displacement(seed=4600):
    out = []
    for vt, ct in PAIRS:
        rng, vol, col, cc, u, w, inner = _generic_setup(seed, vt, ct, 0)
        vol = shifted(vol, rng.uniform(-1, 1, 3))
        col = shifted(col, vol["pos"] + 6.0 * u + rng.uniform(0, 0.6) * inner * w - col["pos"])
        travel = _approach(vol, col, u, 12.0)
        assert travel is not None, (vt, ct)
        for k, (length, t) in enumerate(DISPLACEMENTS):
            if t is None and (vt + ct) % 2:
                continue
            out.append(("displacement", f"d{length:g}", vol, shifted(col, ((0.05 if t is None else t * length) - travel) * u), length * u))
    return out


# ---- the families, judged once per process
_GENERATORS = dict(generic=generic, aligned=aligned, grazing=grazing, far=far, size_ratio=size_ratio, displacement=displacement)
_CACHE = {}


def family(name):
    """Every generated case of a base family, judged by the reference (case["ref"], case["kept"]); computed once per process."""
    if name not in _CACHE:
        _CACHE[name] = [judge(finish(*c)) for c in _GENERATORS[name]()]
    return _CACHE[name]


def kept(name):
    """The cases the GPU comparison runs: the base families and the zero-radius spheres as far as the robustness filter keeps them, the
    closed-form families whole (their base cases passed it)."""
    cases = family(name) if name in BASE_FAMILIES else derived(name)
    return [c for c in cases if c["kept"]] if name in BASE_FAMILIES or name == "zero_radius" else cases


def derived(name):
    """Closed-form rescalings of the kept hits of generic and aligned (reference time t, travelled distance t |d|):
      starts_just_clear   the start moved forward to t - delta / |d|: a hit after delta, no initial overlap   (expect = t of the new cast)
      starts_just_inside  the start moved to t + delta / |d|: t = 0 with the initial-overlap flag
      ends_just_short     d shortened to t - delta / |d| of itself: a miss
      just_reaches        d shortened to t + delta / |d| of itself: a hit with t near 1
      zero_radius         the sphere volumes shrunk to a point: a ray (judged by the reference like a base case)
    far_starts_just_clear and far_starts_just_inside are the first two made of the kept hits of far, with its delta: coordinates of 1e2 and 1e3."""
    if name not in _CACHE:
        out = []
        kind = name[4:] if name.startswith("far_") else name
        for base in (kept("far") if name.startswith("far_") else kept("generic") + kept("aligned")):
            if base["ref"] is None:
                continue
            t, dl, length = base["ref"][0], delta(base), float(np.linalg.norm(base["d"]))
            vol, col, d = base["vol"], base["col"], base["d"]
            if kind == "zero_radius":
                if base["vt"] == R.SPHERE:
                    out.append(judge(finish(name, base["family"] + base["tag"], dict(vol, words=vol["words"] * (1, 1, 1, 0)), col, d)))
                continue
            if kind == "starts_just_clear":
                c = finish(name, base["tag"], shifted(vol, (t - dl / length) * d), col, d); c["expect"] = dl / length
            elif kind == "starts_just_inside":
                c = finish(name, base["tag"], shifted(vol, (t + dl / length) * d), col, d); c["expect"] = 0.0
            elif kind == "ends_just_short":
                c = finish(name, base["tag"], vol, col, d * (t - dl / length)); c["expect"] = None
            else:
                c = finish(name, base["tag"], vol, col, d * (t + dl / length)); c["expect"] = t / (t + dl / length)
            c["base"] = base
            out.append(c)
        _CACHE[name] = out
    return _CACHE[name]


def counts(cases):
    """Per pair (volume type, collider type): [generated, kept, kept hits]."""
    table = {p: [0, 0, 0] for p in PAIRS}
    for c in cases:
        m = table[(c["vt"], c["ct"])]
        m[0] += 1; m[1] += bool(c["kept"]); m[2] += bool(c["kept"] and c["ref"] is not None)
    return table


# ---- a world of one family: one static entity with one collider per case
def scene_of(cases, name="sweep_matrix"):
    n = len(cases)
    e = scenes.make_entities(n, capi.ENTITY_STATIC)
    c = scenes.make_colliders(n, capi.SPHERE)
    for i, case in enumerate(cases):
        e["position"][i] = case["col_pos"]; e["rotation"][i] = case["col_rot"]
        c["type"][i] = case["col_type"]; c["shape"][i, :12] = case["col_words"]; c["hull_geometry"][i] = case["col_hull"]
    return scenes.Scene(name, e, np.arange(n, dtype=np.uint32), c, 10, hulls=list(hulls()))
