"""Shape casts against the heightmap terrain without a GPU: the float64 yardstick of tests/sweep_terrain_ref.py against closed forms (the flat
map from above and from below, a sphere onto the tilted plane), and the conditions the GPU test's comparison set has to meet — all computed by
the reference alone."""
import numpy as np

import overlap_ref as R
import sweep_ref as S
import sweep_terrain_ref as ST
from overlap_ref import AABB, CAPSULE, SPHERE

I = (0, 0, 0, 1)
H = ST.FLAT_Y


def _shape(ctype, words, position=(0, 0, 0)):
    return S.convex(R.world_shape(ctype, np.asarray(words, float), position, I))


def test_the_yardstick_equals_the_closed_forms_on_the_flat_map():
    """Sphere, box and capsule (upright and lying) onto the plane y = 32768 * 4 / 65535, from above and from below, to 1e-7 in t; the normal points
    from the terrain to the volume (down for a volume that comes from below), the point lies in the plane."""
    cases = [   # (volume, displacement, lowest / highest extent of the volume along y about its start)
        (_shape(SPHERE, [0, 0, 0, 0.5], (3.3, 5.0, 4.7)), (0.3, -4.0, 0.2), 0.5),
        (_shape(AABB, [-0.4, -0.3, -0.5, 0.4, 0.3, 0.5], (6.1, 4.0, 9.2)), (0.0, -3.0, 0.0), 0.3),
        (_shape(AABB, [-0.4, -0.3, -0.5, 0.4, 0.3, 0.5], (6.1, 4.0, 9.2)), (0.7, -3.0, -0.4), 0.3),
        (_shape(CAPSULE, [0, -0.5, 0, 0, 0.5, 0, 0.4], (8.0, 4.5, 8.0)), (0.0, -3.0, 0.5), 0.9),
        (_shape(CAPSULE, [-0.5, 0, 0, 0.5, 0, 0, 0.4], (8.0, 4.5, 8.0)), (0.2, -3.0, 0.0), 0.4),
        (_shape(SPHERE, [0, 0, 0, 0.5], (3.3, -1.0, 4.7)), (0.3, 4.0, 0.2), 0.5),
        (_shape(AABB, [-0.4, -0.3, -0.5, 0.4, 0.3, 0.5], (6.1, 0.0, 9.2)), (0.1, 3.0, 0.0), 0.3),
        (_shape(CAPSULE, [0, -0.5, 0, 0, 0.5, 0, 0.4], (8.0, -0.5, 8.0)), (0.0, 3.0, 0.5), 0.9),
    ]
    worst = 0.0
    for vol, d, ext in cases:
        y0 = float(S.bounds(vol)[0][1] + S.bounds(vol)[1][1]) / 2
        up = d[1] > 0
        want = (H - ext - y0) / d[1] if up else (y0 - ext - H) / -d[1]
        t, n, p, initial = ST.cast("flat", vol, d)
        worst = max(worst, abs(t - want))
        assert not initial and abs(t - want) <= 1e-7, (t, want)
        assert np.allclose(n, (0, -1 if up else 1, 0), atol=1e-7) and abs(p[1] - H) <= 1e-7, (n, p)
    print(f"flat map: largest |t - closed form| {worst:.2e}")
    # stops short, moves away, level above; resting in the plane; wholly below and moving down
    ball = _shape(SPHERE, [0, 0, 0, 0.5], (3.3, 5.0, 4.7))
    assert ST.cast("flat", ball, (0, -(4.5 - H) + 1e-3, 0)) is None and ST.cast("flat", ball, (0, 2, 0)) is None and ST.cast("flat", ball, (3, 0, 1)) is None
    assert ST.cast("flat", _shape(SPHERE, [0, 0, 0, 0.5], (3.3, H + 0.2, 4.7)), (0, -1, 0))[3]
    assert ST.cast("flat", _shape(SPHERE, [0, 0, 0, 0.5], (3.3, -1.0, 4.7)), (0, -1, 0)) is None
    # outside the map there is nothing
    assert ST.cast("flat", _shape(SPHERE, [0, 0, 0, 0.5], (-3.0, 5.0, 4.7)), (0, -8, 0)) is None


def test_the_yardstick_equals_the_closed_form_on_the_tilted_plane():
    """A sphere onto the plane through the origin with normal n: t = (n.(c - p0) - r) / -(n.d), to 1e-7."""
    n = ST.TILT_NORMAL
    v, _, _ = ST.triangles("tilted")
    assert np.abs(v.reshape(-1, 3) @ n).max() <= 1e-12   # (exactly planar: 500 counts per vertex)
    rng = np.random.default_rng(5)
    for _ in range(6):
        c = np.array([rng.uniform(4, 12), rng.uniform(6, 8), rng.uniform(4, 12)]); r = rng.uniform(0.1, 0.8)
        d = np.array([rng.uniform(-1, 1), -7.0, rng.uniform(-1, 1)])
        want = (n @ c - r) / -(n @ d)
        t, nn, p, initial = ST.cast("tilted", _shape(SPHERE, [0, 0, 0, r], c), d)
        assert not initial and abs(t - want) <= 1e-7 and np.allclose(nn, n, atol=1e-7) and abs(n @ p) <= 1e-7, (t, want, nn, p)


def test_the_comparison_set_is_a_valid_yardstick():
    """What the GPU comparison relies on, from the reference alone: 48 casts, eight per volume type; every type hits at least once; at least a third of
    the casts hit and at least a sixth miss; no hit starts overlapping; and no decision lies within 16 bounds of flipping (a miss stays that clear of
    the terrain, a hit starts that far from it and would go that deep) — so the GPU test leaves out no hit / miss decision."""
    ref = ST.comparison_reference()
    vols, hits = ref["volumes"], ref["hits"]
    n = len(vols)
    assert n == 48 and all((vols["type"] == t).sum() == 8 for t in range(6))
    hit_types = set(int(vols["type"][i]) for i in range(n) if hits[i] is not None)
    n_hit = sum(h is not None for h in hits)
    margins = [ref["clearance"][i] / (ST.BOUND * ref["scales"][i]) for i in range(n)]
    below = sum(h is not None and h[1][1] < 0 for h in hits)
    print(f"comparison set: {n_hit} of {n} casts hit ({below} from below), smallest clearance {min(margins):.1f} bounds, scales up to {max(ref['scales']):.1f}")
    assert hit_types == set(range(6))
    assert n_hit >= n / 3 and n - n_hit >= n / 6 and below >= 3
    assert not any(h[3] for h in hits if h is not None)
    assert min(margins) >= 16.0
