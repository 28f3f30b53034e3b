"""Shape-cast scene queries without a GPU: the ABI (header, exports, the record's layout), the float64 yardstick of tests/sweep_ref.py
against closed forms, and the conditions the GPU tests' cast set and pair-level matrix (tests/sweep_matrix.py) have to meet — all computed
by the reference alone."""
import re
from pathlib import Path

import numpy as np
import pytest

import overlap_ref as R
import sweep_matrix as M
import sweep_ref as S
from overlap_ref import AABB, CAPSULE, CYLINDER, HULL, OBB, SPHERE

ROOT = Path(__file__).resolve().parent.parent
SWEEP_SYMBOLS = ("mi_world_sweep", "mi_world_sweep_device_async", "mi_debug_sweep_exhaustive")
I = (0, 0, 0, 1)


def test_header_declares_and_library_exports_the_sweep_api(mi_lib):
    text = (ROOT / "include" / "mi_physics.h").read_text()
    declared = set(re.findall(r"MI_API\s+[\w\s\*]+?\b(mi_\w+)\s*\(", text))
    for name in SWEEP_SYMBOLS:
        assert name in declared, name
    L = mi_lib.library()
    missing = [n for n in SWEEP_SYMBOLS if not hasattr(L.lib, n)]
    assert not missing, missing
    from d3d12renderer_amd import capi
    dt = capi.sweep_hit_dtype
    assert dt.itemsize == 48
    assert [(n, dt.fields[n][1]) for n in dt.names] == [("entity", 0), ("collider", 4), ("t", 8), ("object_type", 12), ("point", 16), ("flags", 28),
                                                        ("normal", 32), ("volume", 44)]
    assert "} mi_sweep_hit;" in text and re.search(r"enum \{ \w+_INITIAL_OVERLAP = 1, \w+_UNCONVERGED = 2 \}", text)   # (the flag names, spelt so that the knob census does not take them for environment variables)
    assert capi.SWEEP_INITIAL_OVERLAP == 1 and capi.SWEEP_UNCONVERGED == 2
    for method in ("sweep", "debug_sweep_exhaustive", "sweep_device_async"):
        assert hasattr(capi.World, method), method


def _shape(ctype, words, position=(0, 0, 0), rotation=I, hull=None):
    return S.convex(R.world_shape(ctype, np.asarray(words, float), position, rotation), hull)


def _random_quaternion(rng):
    q = rng.normal(size=4)
    return (q / np.linalg.norm(q)).astype(np.float32)


def test_gap_equals_the_closed_forms():
    """770 sphere-capsule pairs to 1e-12 (float64 round-off) and 777 sphere-OBB pairs to 1e-6 (overlap_ref.qmat of a float32 quaternion is
    not exactly orthonormal: signed_gap measures in the box's own skewed frame).  AABB-AABB is not compared: that signed_gap is the largest
    slab gap, not a distance."""
    rng = np.random.default_rng(31)
    worst = [0.0, 0.0]
    for i in range(770 + 777):
        c = rng.uniform(-3, 3, 3); r = rng.uniform(0.0, 0.8)
        a = R.world_shape(SPHERE, [*c, r], (0, 0, 0), I)
        if i < 770:
            b = R.world_shape(CAPSULE, [*rng.uniform(-1, 1, 3), *rng.uniform(-1, 1, 3), rng.uniform(0.05, 0.5)], rng.uniform(-1, 1, 3), _random_quaternion(rng))
        else:
            b = R.world_shape(OBB, [*_random_quaternion(rng), *rng.uniform(-0.3, 0.3, 3), *rng.uniform(0.1, 1.0, 3)], rng.uniform(-1, 1, 3), _random_quaternion(rng))
        want = R.signed_gap(a, b)
        if want <= 0 and (i >= 770 or want <= -(r + b[1][2])):
            continue   # (the cores meet: the gap of a core-plus-margin shape is only defined down to minus the margins)
        got = S.gap(S.convex(a), S.convex(b))
        worst[i >= 770] = max(worst[i >= 770], abs(got - want))
    print(f"largest |gap - closed form|: sphere-capsule {worst[0]:.2e}, sphere-OBB {worst[1]:.2e}")
    assert worst[0] <= 1e-12 and worst[1] <= 1e-6


def test_time_of_impact_equals_the_closed_forms():
    hull = R.volume_hull()[0]
    lowest = float(hull[:, 1].min())
    box = _shape(AABB, [-1, -1, -1, 1, 1, 1], (10, 0, 0))
    cases = [
        # box -> box along an axis: t = gap / |d|
        (_shape(AABB, [-0.5, -0.5, -0.5, 0.5, 0.5, 0.5], (5, 0.2, 0.1)), box, (6, 0, 0), (9 - 5.5) / 6, (-1, 0, 0)),
        (_shape(AABB, [-0.5, -0.5, -0.5, 0.5, 0.5, 0.5], (10, 5, 0)), box, (0, -6, 0), (5 - 0.5 - 1) / 6, (0, 1, 0)),
        # cylinder side -> box face, cylinder cap -> box top
        (_shape(CYLINDER, [5, -0.5, 0, 5, 0.5, 0, 0.3]), box, (5, 0, 0), (9 - 5.3) / 5, (-1, 0, 0)),
        (_shape(CYLINDER, [10, 3, 0, 10, 4, 0, 0.3]), box, (0, -4, 0), (3 - 1) / 4, (0, 1, 0)),
        # hull -> box from above: its lowest vertex lands on the top face
        (_shape(HULL, [0, 0, 0, 1, 0, 0, 0], (10, 6, 0), I, hull), box, (0, -8, 0), (6 + lowest - 1) / 8, (0, 1, 0)),
        # capsule end-on -> box face; sphere -> sphere head-on and off-axis
        (_shape(CAPSULE, [5, 0, 0, 6, 0, 0, 0.2]), box, (5, 0, 0), (9 - 6.2) / 5, (-1, 0, 0)),
        (_shape(SPHERE, [-5, 0, 0, 0.25]), _shape(SPHERE, [0, 0, 0, 0.5]), (8, 0, 0), 4.25 / 8, (-1, 0, 0)),
        (_shape(SPHERE, [-5, 0.3, 0, 0.25]), _shape(SPHERE, [0, 0, 0, 0.5]), (8, 0, 0), (5 - np.sqrt(0.75 ** 2 - 0.3 ** 2)) / 8, None),
    ]
    for vol, col, d, want_t, want_n in cases:
        t, n, point, initial = S.time_of_impact(vol, col, d)
        assert abs(t - want_t) * np.linalg.norm(d) <= 1e-10 and not initial, (t, want_t)
        if want_n is not None:
            assert np.allclose(n, want_n, atol=1e-6), (n, want_n)
        assert abs(np.linalg.norm(n) - 1) <= 1e-12 and abs(S.point_gap(point, col)) <= 1e-9
    assert S.time_of_impact(_shape(SPHERE, [-5, 0, 0, 0.25]), _shape(SPHERE, [0, 0, 0, 0.5]), (4.2499, 0, 0)) is None          # stops just short
    assert S.time_of_impact(_shape(SPHERE, [-5, 0, 0, 0.25]), _shape(SPHERE, [0, 0, 0, 0.5]), (-8, 0, 0)) is None             # moves away
    assert S.time_of_impact(_shape(SPHERE, [-0.5, 0, 0, 0.25]), _shape(SPHERE, [0, 0, 0, 0.5]), (1, 0, 0))[3]                 # starts inside


def test_signed_gap_is_zero_at_the_hit_pose():
    """The closed-form pairs of overlap_ref at the reference's own time of impact: the volume moved there touches the collider."""
    rng = np.random.default_rng(32)
    hits = 0
    for i in range(60):
        kind = i % 3
        target = rng.uniform(-1, 1, 3)
        start = target + 6.0 * (lambda u: u / np.linalg.norm(u))(rng.normal(size=3))
        d = 1.5 * (target - start) + rng.uniform(-0.4, 0.4, 3)
        vol_ws = (R.world_shape(SPHERE, [0, 0, 0, rng.uniform(0.0, 0.5)], start, I) if kind != 2 else
                  R.world_shape(CAPSULE, [0, -0.4, 0, 0, 0.4, 0, 0.2], start, _random_quaternion(rng)))
        col_ws = (R.world_shape(SPHERE, [0, 0, 0, 0.6], target, I) if kind == 0 else
                  R.world_shape(OBB, [*_random_quaternion(rng), 0, 0, 0, *rng.uniform(0.3, 0.9, 3)], target, I) if kind == 1 else
                  R.world_shape(CAPSULE, [0, -0.6, 0, 0, 0.6, 0, 0.3], target, _random_quaternion(rng)))
        hit = S.time_of_impact(S.convex(vol_ws), S.convex(col_ws), d)
        if hit is None:
            continue
        hits += 1
        t = hit[0]
        moved = (vol_ws[0], tuple(p + t * d if isinstance(p, np.ndarray) and p.shape == (3,) else p for p in vol_ws[1]))
        assert abs(R.signed_gap(moved, col_ws)) <= (1e-6 if kind == 1 else 1e-9), (kind, R.signed_gap(moved, col_ws))
    assert hits >= 40


@pytest.mark.parametrize("seed", [909, 911])
def test_cast_set_is_a_valid_yardstick(seed):
    """What the GPU comparison relies on, from the reference alone: nearly every cast hits, none starts overlapping, and the winner leads
    the runner-up by far more than any float32 error — so no cast is ever left out of a comparison."""
    ref = S.cast_set_reference(seed)
    n = len(ref["volumes"])
    hits = [h for h in ref["hits"] if h is not None]
    print(f"seed {seed}: {len(hits)} of {n} casts hit, {sum(h[4] for h in hits)} initial overlaps, smallest lead {min(ref['leads']):.3f}")
    assert n == 48 and set(int(t) for t in ref["volumes"]["type"]) == set(range(6))
    assert len(hits) >= 0.9 * n
    assert not any(h[4] for h in hits)
    assert min(ref["leads"]) >= 1e-2


# ---- the pair-level matrix (tests/sweep_matrix.py)
@pytest.mark.parametrize("name", M.BASE_FAMILIES)
def test_matrix_family_is_a_valid_yardstick(name):
    """What the GPU comparison of a family relies on, from the reference alone: all 36 pairs survive the robustness filter (the decision is the
    same with the shapes shrunk and grown by delta = 4 x the family's bound x scale; no hit starts within delta) with at least 2 cases each,
    at most 10 % of the generated cases are filtered out, and the family holds the hits and misses it is meant to."""
    cases = M.family(name)
    table = M.counts(cases)
    n, kept = len(cases), [c for c in cases if c["kept"]]
    hits = sum(c["ref"] is not None for c in kept)
    print(f"{name}: {n} cases, {n - len(kept)} filtered out ({100.0 * (n - len(kept)) / n:.1f} %), {hits} hits and {len(kept) - hits} misses kept, "
          f"scale up to {max(c['scale'] for c in cases):.3g}, delta {min(M.delta(c) for c in cases):.2e} .. {max(M.delta(c) for c in cases):.2e}")
    for vt in range(6):
        print(f"  {M.TYPES[vt]:>8} ->  " + "  ".join(f"{M.TYPES[ct]} {table[(vt, ct)][1]}/{table[(vt, ct)][0]} ({table[(vt, ct)][2]} hit)" for ct in range(6)))
    assert set(table) == set(M.PAIRS) and all(m[0] >= 3 for m in table.values()), "a pair has fewer than 3 samples"
    assert all(m[1] >= 2 for m in table.values()), [p for p, m in table.items() if m[1] < 2]
    assert n - len(kept) <= 0.1 * n
    assert not any(c["ref"][3] for c in kept if c["ref"] is not None)
    if name == "grazing":
        assert 0.4 * len(kept) <= hits <= 0.6 * len(kept)
        for c in kept:   # the closest approach is where the family puts it: k delta clear, or a hit that the cast shrunk by delta still makes
            k = int(c["tag"][1:].rstrip("hitms"))
            assert (c["ref"] is None) == c["tag"].endswith("miss"), c["tag"]
            if c["ref"] is None:
                assert abs(S.closest_approach(c["vconv"], c["cconv"], c["d"]) - k * M.delta(c)) <= 0.05 * M.delta(c), c["tag"]
    else:
        assert hits >= 0.8 * len(kept)
    if name == "far":
        assert min(c["scale"] for c in cases) >= 90 and max(c["scale"] for c in cases) >= 900
    if name == "displacement":
        lengths = sorted(set(float(np.linalg.norm(c["d"])) for c in kept))
        ts = [c["ref"][0] for c in kept if c["ref"] is not None]
        assert lengths[0] <= 1.1e-3 and lengths[-1] >= 0.9e4 and min(ts) <= 0.02 and max(ts) >= 0.98 and any(0.3 <= t <= 0.7 for t in ts)


def _point_cylinder_distance(p, a, b, r):
    """Distance of a point outside a solid cylinder (axis a..b, radius r) from it."""
    u = (b - a) / np.linalg.norm(b - a)
    h = (p - (a + b) / 2) @ u
    rho = np.linalg.norm(p - (a + b) / 2 - h * u)
    return float(np.hypot(max(rho - r, 0.0), max(abs(h) - np.linalg.norm(b - a) / 2, 0.0)))


def test_matrix_reference_equals_the_closed_forms():
    """Where a closed form exists the reference agrees with it to 1e-9 in travelled distance, on the rounded float32 inputs both see:
      * aligned k 0 (centred, exactly along -y, flat or round onto flat: box / cylinder cap / capsule side / sphere onto a box face or a
        cylinder cap) travels the gap of the two bounds along y;
      * two axis-aligned boxes (AABB on AABB in generic and in aligned k 0, 1, 2: face on face, edge onto the parallel edge along the face
        diagonal, half-overlapping faces; with the OBBs of aligned k 0, whose half turn is exact in float32) touch when the displacement
        enters the collider grown by the volume's half-extents: the slab test;
      * a sphere against a sphere, capsule or AABB (generic and aligned), against the exactly turned OBB of aligned k 0 and against a
        cylinder ends at gap 0 (overlap_ref.signed_gap; the point-cylinder distance above).
    Not compared: a sphere against the other OBBs (overlap_ref.qmat of a rounded quaternion is orthonormal to 1e-7 only and signed_gap
    measures in that skewed frame: 1e-6, test_gap_equals_the_closed_forms), against a hull (no closed form short of another polytope
    distance algorithm), and the quarter-turned OBBs of aligned k 1 and 2 (their faces are tilted by 6e-8)."""
    worst = [0.0, 0.0, 0.0]; seen = [0, 0, 0]
    for c in M.family("aligned"):
        flat_below = c["ct"] in (AABB, OBB) or (c["ct"] == CYLINDER and c["vt"] in (CYLINDER, AABB, OBB))
        if c["tag"] == "s0" and c["vt"] != HULL and flat_below:
            want = S.bounds(c["vconv"])[0][1] - S.bounds(c["cconv"])[1][1]
            worst[0] = max(worst[0], abs(c["ref"][0] * np.linalg.norm(c["d"]) - want)); seen[0] += 1
    for c in M.family("generic") + M.family("aligned"):
        boxes = (AABB,) if c["family"] == "generic" or c["tag"] != "s0" else (AABB, OBB)
        if c["vt"] in boxes and c["ct"] in boxes:
            (vmn, vmx), (cmn, cmx) = S.bounds(c["vconv"]), S.bounds(c["cconv"])
            want = S.slab_entry(cmn, cmx, (vmx - vmn) / 2, (vmn + vmx) / 2, c["d"])
            assert want is not None and c["ref"] is not None, (c["family"], c["tag"])
            worst[2] = max(worst[2], abs(c["ref"][0] - want) * np.linalg.norm(c["d"])); seen[2] += 1
        exact_obb = c["ct"] == OBB and c["family"] == "aligned" and c["tag"] == "s0"
        if c["vt"] == SPHERE and (c["ct"] in (SPHERE, CAPSULE, CYLINDER, AABB) or exact_obb) and c["ref"] is not None:
            t, n = c["ref"][0], c["ref"][1]
            v = c["volume"][0].copy(); v["position"] = 0
            ws = R.volume_world_shape(v)
            ws = (ws[0], (ws[1][0] + c["volume"]["position"][0].astype(np.float64) + t * c["d"], ws[1][1]))
            cw = R.world_shape(c["col_type"], c["col_words"], c["col_pos"], c["col_rot"])
            gap = _point_cylinder_distance(ws[1][0], *cw[1]) - ws[1][1] if c["ct"] == CYLINDER else R.signed_gap(ws, cw)
            d_hat = c["d"] / np.linalg.norm(c["d"])
            worst[1] = max(worst[1], abs(gap) / -(d_hat @ n)); seen[1] += 1
    print(f"aligned flat contacts: {seen[0]} cases, largest |travel - bounds gap| {worst[0]:.2e}; box on box: {seen[2]} cases, largest |travel - slab entry| {worst[2]:.2e}; "
          f"sphere casts: {seen[1]} cases, largest |gap at the hit| / |d.n| {worst[1]:.2e}")
    assert seen[0] >= 12 and seen[1] >= 25 and seen[2] >= 9
    assert max(worst) <= 1e-9


def test_matrix_derived_families():
    """The derived families rescale kept hits in closed form; what they expect follows from the base case's reference time alone."""
    base = sum(c["ref"] is not None for c in M.kept("generic") + M.kept("aligned"))
    for name in ("starts_just_clear", "starts_just_inside", "ends_just_short", "just_reaches"):
        cases = M.derived(name)
        assert len(cases) == base and set((c["vt"], c["ct"]) for c in cases) == set(M.PAIRS)
    far = sum(c["ref"] is not None for c in M.kept("far"))
    for name in [f for f in M.DERIVED_FAMILIES if f.startswith("far_")]:
        cases = M.derived(name)
        assert len(cases) == far and set((c["vt"], c["ct"]) for c in cases) == set(M.PAIRS) and min(c["scale"] for c in cases) >= 90
    rays = M.derived("zero_radius")
    print(f"derived: {base} cases per family, {len(rays)} zero-radius spheres ({sum(c['kept'] for c in rays)} kept)")
    assert set(c["ct"] for c in rays if c["kept"]) == set(range(6)) and all(c["volume"]["shape"][0, 3] == 0 for c in rays)
    # a sample: the rescaling against the reference itself, to the rounding of the moved start to float32 (3e-7 x its coordinates)
    for c in M.derived("just_reaches")[:12] + M.derived("starts_just_clear")[:12] + M.derived("far_starts_just_clear")[:12]:
        hit = S.time_of_impact(c["vconv"], c["cconv"], c["d"])
        assert hit is not None and not hit[3] and abs(hit[0] - c["expect"]) * np.linalg.norm(c["d"]) <= 1e-5 * max(1.0, c["scale"] / 30), (c["family"], c["tag"], hit[0], c["expect"])
    for c in M.derived("ends_just_short")[:12]:
        assert S.time_of_impact(c["vconv"], c["cconv"], c["d"]) is None
    for c in M.derived("starts_just_inside")[:12] + M.derived("far_starts_just_inside")[:12]:
        assert S.time_of_impact(c["vconv"], c["cconv"], c["d"])[3]


def test_slack_and_closest_approach_equal_the_closed_forms():
    a, b = _shape(SPHERE, [-5, 0.3, 0, 0.25]), _shape(SPHERE, [0, 0, 0, 0.5])
    assert abs(S.closest_approach(a, b, (8, 0, 0)) - (0.3 - 0.75)) <= 1e-12 and abs(S.closest_approach(a, b, (2, 0, 0)) - (np.hypot(3, 0.3) - 0.75)) <= 1e-12
    for slack in (-0.1, 0.1):
        t = S.time_of_impact(a, b, (8, 0, 0), slack=slack)[0]
        assert abs(t * 8 - (5 - np.sqrt((0.75 + slack) ** 2 - 0.3 ** 2))) <= 1e-9
    box, small = _shape(AABB, [-1, -1, -1, 1, 1, 1], (10, 0, 0)), _shape(AABB, [-0.5, -0.5, -0.5, 0.5, 0.5, 0.5], (5, 0.2, 0.1))
    assert abs(S.closest_approach(small, box, (2, 0, 0)) - 1.5) <= 1e-12
    assert abs(S.time_of_impact(small, box, (6, 0, 0), slack=-0.25)[0] * 6 - 3.75) <= 1e-9    # without a margin: 0.25 deep along the touch's normal
    assert S.time_of_impact(small, box, (3.6, 0, 0), slack=-0.25) is None and S.time_of_impact(small, box, (3.4, 0, 0), slack=0.25) is not None
