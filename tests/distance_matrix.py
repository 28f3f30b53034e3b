"""The pair-level test matrix of the distance query (mi_world_distance): every volume type against every collider type, one collider at a time,
at the configurations where a float32 GJK distance goes wrong; numpy only, no GPU.  tests/test_distance.py checks the matrix itself from the
float64 reference of tests/sweep_ref.py alone, tests/test_gpu_distance.py runs it on the GPU.

  * a SHAPE comes from the builders of tests/sweep_matrix.py: built, moved and turned in float64 and rounded to float32 once, when the case is
    finished; the reference sees the rounded numbers, the same ones the GPU gets;
  * a CASE is a volume, one collider, a largest distance (None = unbounded) and a `scale` = max(1, the largest |coordinate| of either shape);
  * every case is PLACED: the volume is moved along a line until the float64 gap of the two shapes is the one the family asks for (Newton on
    the gap, which is convex along a line and whose slope is the closest direction's component along it), so the gap of every case is known
    and none has to be filtered out: case["placed"] is the gap asked for, case["gap64"] what the reference measures at the placement, and
    case["ref"] the gap of the rounded shapes, which the GPU is compared with;
  * delta = 4 x the family's bound x scale: the gaps of `near`, the margins of `cut` about the largest distance and the depth of
    `just_overlapping` are 4 delta or more, so the expected decision holds however the GPU's error (within the bound) falls.
  * `just_overlapping` is placed 0.25 apart and then moved towards the collider along the closest direction n by 0.25 + 4 delta: 4 delta deep
    along n, exact while the closest features stay the same (round and flat pairs), an upper bound of the depth elsewhere; case["back"] is n."""
import numpy as np

import overlap_ref as R
import sweep_matrix as M
import sweep_ref as S

TYPES, PAIRS, FAR_OFFSETS = M.TYPES, M.PAIRS, M.FAR_OFFSETS
FAMILIES = ("generic", "aligned", "near", "far", "size_ratio", "separation", "cut", "just_overlapping")
# The bound on |distance - reference|, on both points' distances from their shapes, on ||point_volume - point_collider| - distance| and on
# |point_volume - point_collider - distance x normal|, PER UNIT OF `scale`: 4 x the largest value measured on the MI355X against the float64
# reference, rounded up to one digit.  Measured (the largest of those measures per family; it is |distance - reference| in each): generic
# 6.76e-7, aligned 1.23e-6, near 1.04e-6, far 1.75e-6, size_ratio 6.07e-6 (a 1e-2 box over the curved side of a cylinder of radius 15),
# separation 9.77e-7, cut 1.32e-6; the points stay within 1.1e-7 of their shapes and of each other's distance in every family.
# just_overlapping asserts a decision only and takes generic's bound for its depth (the same shapes in the same regime).  What the figures
# are: the comment at the bounds in tests/test_gpu_distance.py, INTEGRATION.md 6g.
BOUNDS = {"generic": 3e-6, "aligned": 5e-6, "near": 5e-6, "far": 7e-6, "size_ratio": 3e-5, "separation": 4e-6, "cut": 6e-6, "just_overlapping": 3e-6}
PLACE_TOL = 1e-10


def _centre(conv):
    mn, mx = S.bounds(conv)
    return (mn + mx) / 2, float(np.linalg.norm(mx - mn)) / 2


def closest(a, b):
    """(gap, unit direction from b to a, point on b's surface, point on a's surface) of two shapes by the reference."""
    dist, n, pb = S.core_distance(a, b)
    return dist - S.margin(a) - S.margin(b), n, pb + S.margin(b) * n, pb + (dist - S.margin(a)) * n


def place(vol, col, anchor, u, target, lateral=(0, 0, 0)):
    """`vol` moved so that its bounds' centre lies at anchor + lateral + s u, s chosen from outside so that the float64 gap to `col` is `target`."""
    u = M._unit(u)
    c = M.conv64(col)
    cc, cr = _centre(c)
    vc0, vr = _centre(M.conv64(vol))
    base = M.shifted(vol, np.asarray(anchor, np.float64) + np.asarray(lateral, np.float64) - vc0)
    vc = M.conv64(base)
    s = vr + cr + float(np.linalg.norm(np.asarray(anchor) + np.asarray(lateral) - cc)) + target + 1.0
    for _ in range(60):
        g, n, _, _ = closest(S.moved(vc, s * u), c)
        f = g - target
        if abs(f) <= PLACE_TOL:
            return M.shifted(base, s * u)
        slope = float(n @ u)
        assert slope > 1e-3, "the line leaves the collider sideways"
        s -= f / slope
    raise RuntimeError("placement did not converge")


def finish(family, tag, vol, col, placed, max_distance=None, expect="hit", back=None):
    c = M.finish(family, tag, vol, col, np.zeros(3))
    g64 = closest(M.conv64(vol), M.conv64(col))[0]
    ref = closest(c["vconv"], c["cconv"])
    c.update(placed=placed, gap64=g64, ref=ref[0], ref_normal=ref[1], ref_point_collider=ref[2], ref_point_volume=ref[3], expect=expect, back=back,
             max_distance=None if max_distance is None else np.float32(max_distance))
    return c


def delta(family, scale):
    return 4.0 * BOUNDS[family] * scale


def _scale_at(vol, col):
    return M.finish("generic", "", vol, col, np.zeros(3))["scale"]


# ---- set-ups: (volume, collider, anchor, outward direction, lateral offset)
def _generic(seed, vt, ct, k):
    rng, vol, col, cc, u, w, inner = M._generic_setup(seed, vt, ct, k)
    return rng, vol, col, _centre(M.conv64(col))[0], u, rng.uniform(0, 0.6) * inner * w


def _aligned(seed, vt, ct, k):
    """tests/sweep_matrix.py's aligned configurations: k 0 = centred, flat onto flat, apart along y; k 1 = half-overlapping along x, the volume's lower z
    edge over the collider's upper z edge, apart along the face diagonal (0, 1, 1); k 2 = half-overlapping in x and z, apart along y, the whole
    configuration under one random rotation (pairs with an AABB stay axis-aligned).  Returns the shapes before that rotation and the rotation."""
    rng = np.random.default_rng([seed, vt, ct, k])
    vol, col = M._aligned_shape(rng, vt, k, True, k % 2), M._aligned_shape(rng, ct, k, False, (k + 1) % 2)
    (vmn, vmx), (cmn, cmx) = S.bounds(M.conv64(vol)), S.bounds(M.conv64(col))
    vh, ch = (vmx - vmn) / 2, (cmx - cmn) / 2
    cc = (cmn + cmx) / 2
    if k == 1:
        u = np.array([0.0, 1.0, 1.0]) / np.sqrt(2.0)
        lat = np.array([0.5 * vh[0], ch[1] + vh[1], ch[2] + vh[2]])   # the two edges on each other; from there along the diagonal
    else:
        u = np.array([0.0, 1.0, 0.0])
        lat = np.zeros(3) if k == 0 else np.array([0.5 * (vh[0] + ch[0]), 0.0, 0.5 * min(vh[2], ch[2])])
    g = M._rand_q(rng) if k == 2 and R.AABB not in (vt, ct) else M.I4
    return rng, vol, col, cc, u, lat, g, rng.uniform(-1, 1, 3)


def _turn(vol, col, g, shift):
    return M.shifted(M.turned(vol, g), shift), M.shifted(M.turned(col, g), shift)


def generic(seed=5100):
    out = []
    for vt, ct in PAIRS:
        for k in range(2):
            rng, vol, col, anchor, u, lat = _generic(seed, vt, ct, k)
            target = float(rng.uniform(0.2, 3.0))
            out.append(finish("generic", f"s{k}", place(vol, col, anchor, u, target, lat), col, target))
    return out


def aligned(seed=5200):
    out = []
    for vt, ct in PAIRS:
        for k in range(3):
            rng, vol, col, anchor, u, lat, g, shift = _aligned(seed, vt, ct, k)
            target = float(rng.uniform(0.2, 2.0))
            out.append(finish("aligned", f"s{k}", *_turn(place(vol, col, anchor, u, target, lat), col, g, shift), target))
    return out


def near(seed=5300):
    """A gap of 6 delta (generic) and of 12 delta (flat onto flat)."""
    out = []
    for vt, ct in PAIRS:
        rng, vol, col, anchor, u, lat = _generic(seed, vt, ct, 0)
        target = 6.0 * delta("near", _scale_at(place(vol, col, anchor, u, 0.01, lat), col))
        out.append(finish("near", "generic", place(vol, col, anchor, u, target, lat), col, target))
        rng, vol, col, anchor, u, lat, g, shift = _aligned(seed, vt, ct, 0)
        target = 12.0 * delta("near", _scale_at(*_turn(place(vol, col, anchor, u, 0.01, lat), col, g, shift)))
        out.append(finish("near", "flat", *_turn(place(vol, col, anchor, u, target, lat), col, g, shift), target))
    return out


def far(seed=5400):
    """Generic and aligned cases translated as a whole, in float64 before rounding, to coordinates of 1e2 and 1e3."""
    out = []
    for vt, ct in PAIRS:
        rng, vol, col, anchor, u, lat = _generic(seed, vt, ct, 0)
        target = float(rng.uniform(0.2, 3.0))
        out.append(finish("far", "generic+1e2", M.shifted(place(vol, col, anchor, u, target, lat), FAR_OFFSETS[0]), M.shifted(col, FAR_OFFSETS[0]), target))
        for k, off in ((0, FAR_OFFSETS[1]), (2, FAR_OFFSETS[0])):
            rng, vol, col, anchor, u, lat, g, shift = _aligned(seed, vt, ct, k)
            target = float(rng.uniform(0.2, 2.0))
            out.append(finish("far", f"aligned{k}+1e{3 - k // 2}", *_turn(place(vol, col, anchor, u, target, lat), col, g, shift + off), target))
    return out


def size_ratio(seed=5500):
    """tests/sweep_matrix.py's size ratios: k 0, 1 = a volume of size 1e-2 over a box 200 units wide (tens of units off its centre; the OBB turned 30 degrees
    about a skew axis), over a 50-unit sphere / capsule / cylinder, over the hull geometry whose vertices lie tens of units from its origin;
    k 2 = a 20-unit volume over a collider of size 1e-2.  Gaps of 0.1, 3 and 0.5."""
    from d3d12renderer_amd import scenes
    out = []
    skew = scenes.q_axis_angle(M._unit((1, 2, 3)), np.pi / 6)
    for vt, ct in PAIRS:
        for k in range(3):
            rng = np.random.default_rng([seed, vt, ct, k])
            u = M._unit(rng.normal(size=3))
            if k == 2:
                vol, col, aim = M._sized(rng, vt, 20.0, 0), M._sized(rng, ct, 1e-2, 1), np.zeros(3)
                aim = _centre(M.conv64(col))[0]
            else:
                vol = M._sized(rng, vt, 1e-2, k)
                if ct in (R.AABB, R.OBB):
                    col = M.aabb((100.0, 10.0, 100.0)) if ct == R.AABB else M.obb((100.0, 10.0, 100.0), skew, k)
                    g = R.qmat(skew) if ct == R.OBB else np.eye(3)
                    aim = g @ np.array(((35.0, 10.0, -22.0), (-60.0, 10.0, 41.0))[k])     # on the top face
                    u = g @ M._unit((-0.3, 1.0, (-0.2, 0.4)[k]))
                elif ct == R.HULL:
                    col = M.hull(M._rand_q(rng), 1)
                    aim = M.conv64(col)[1].mean(axis=0) + rng.uniform(-4, 4, 3)
                else:
                    col = M.sphere(25.0) if ct == R.SPHERE else M.capsule(25.0, 10.0, 1, M._rand_q(rng)) if ct == R.CAPSULE else M.cylinder(25.0, 15.0, 1, M._rand_q(rng))
                    aim = rng.uniform(-6, 6, 3)
            cc = rng.uniform(-3, 3, 3)
            target = (0.1, 3.0, 0.5)[k]
            out.append(finish("size_ratio", ("tiny", "tiny", "big")[k] + str(k), place(vol, M.shifted(col, cc), aim + cc, u, target), M.shifted(col, cc), target))
    return out


def separation(seed=5600):
    """Gaps of 10, 100 and 1000 times the volume's size."""
    out = []
    for vt, ct in PAIRS:
        for k in range(2):
            rng, vol, col, anchor, u, lat = _generic(seed, vt, ct, k)
            size = 2.0 * _centre(M.conv64(vol))[1]
            target = (10.0, 100.0, 1000.0)[(vt + ct + k) % 3] * size
            out.append(finish("separation", f"x{target / size:g}", place(vol, col, anchor, u, target, lat), col, target))
    return out


def cut(seed=5700):
    """One placement per pair, asked twice: with the largest distance 4 delta below the gap of the rounded shapes (a miss) and 4 delta above it (a hit)."""
    out = []
    for vt, ct in PAIRS:
        rng, vol, col, anchor, u, lat = _generic(seed, vt, ct, 0)
        target = float(rng.uniform(0.3, 2.0))
        vol = place(vol, col, anchor, u, target, lat)
        probe = finish("cut", "", vol, col, target)
        dl = 4.0 * delta("cut", probe["scale"])
        out.append(finish("cut", "below", vol, col, target, probe["ref"] - dl, "miss"))
        out.append(finish("cut", "above", vol, col, target, probe["ref"] + dl, "hit"))
    return out


START_GAP = 0.25


def just_overlapping(seed=5800):
    out = []
    for vt, ct in PAIRS:
        for kind in ("generic", "flat"):
            if kind == "generic":
                rng, vol, col, anchor, u, lat = _generic(seed, vt, ct, 0)
                vol = place(vol, col, anchor, u, START_GAP, lat)
            else:
                rng, vol, col, anchor, u, lat, g, shift = _aligned(seed, vt, ct, 0)
                vol, col = _turn(place(vol, col, anchor, u, START_GAP, lat), col, g, shift)
            n = closest(M.conv64(vol), M.conv64(col))[1]
            depth = 4.0 * delta("just_overlapping", _scale_at(M.shifted(vol, -START_GAP * n), col))   # (the scale where the shapes touch)
            out.append(finish("just_overlapping", kind, M.shifted(vol, -(START_GAP + depth) * n), col, -depth, None, "overlap", back=n))
    return out


_GENERATORS = dict(generic=generic, aligned=aligned, near=near, far=far, size_ratio=size_ratio, separation=separation, cut=cut, just_overlapping=just_overlapping)
_CACHE = {}


def family(name):
    """Every case of a family (none is left out), computed once per process."""
    if name not in _CACHE:
        _CACHE[name] = _GENERATORS[name]()
    return _CACHE[name]


scene_of = M.scene_of
