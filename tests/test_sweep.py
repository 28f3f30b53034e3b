"""Shape-cast scene queries without a GPU: the ABI (header, exports, the record's layout), the float64 yardstick of tests/sweep_ref.py
against closed forms, and the conditions the GPU tests' cast set has to meet — all computed by the reference alone."""
import re
from pathlib import Path

import numpy as np
import pytest

import overlap_ref as R
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
