"""The distance query's test matrix (tests/distance_matrix.py) checked from the float64 reference alone (tests/sweep_ref.py); no GPU.
Every pair in every family, every placed gap what the reference measures, every gap 4 delta clear of 0 and of its largest distance (so the
GPU comparison leaves no case out), the reference against closed forms, and the record's layout."""
import numpy as np
import pytest

import distance_matrix as D
import sweep_matrix as M
import sweep_ref as S


@pytest.mark.parametrize("name", D.FAMILIES)
def test_family_holds_every_pair_at_a_known_gap(name):
    cases = D.family(name)
    assert set((c["vt"], c["ct"]) for c in cases) == set(D.PAIRS)
    worst = 0.0
    for c in cases:
        who = f"{name} {D.TYPES[c['vt']]} -> {D.TYPES[c['ct']]} {c['tag']}"
        dl = D.delta(name, c["scale"])
        if name == "just_overlapping":
            # 4 delta deep along the closest direction n: the reference sees the shapes meet, and still meet when the volume is taken half of that back;
            # taken back by the whole depth and the gap it was placed at, they are that gap apart again
            n, vol = c["back"], M.conv64(c["vol"])
            assert c["expect"] == "overlap" and -c["placed"] >= 4.0 * dl * (1 - 1e-3), who
            dl = -c["placed"]
            assert S.gap(c["vconv"], c["cconv"]) <= 0.0 and S.gap(S.moved(c["vconv"], 0.5 * dl * n), c["cconv"]) <= 0.0, who
            assert abs(S.gap(S.moved(vol, (dl + D.START_GAP) * n), M.conv64(c["col"])) - D.START_GAP) <= 1e-9, who
            if S.margin(c["vconv"]) > 0 and S.margin(c["cconv"]) > 0:   # round pairs: the reference measures the depth itself
                assert abs(c["gap64"] + dl) <= 1e-9, (who, c["gap64"], dl)
            continue
        err = abs(S.gap(M.conv64(c["vol"]), M.conv64(c["col"])) - c["placed"])
        worst = max(worst, err)
        assert err <= 1e-9 and c["gap64"] == pytest.approx(c["placed"], abs=1e-9), (who, err)
        assert abs(c["ref"] - c["placed"]) <= 4e-7 * c["scale"], who   # (the rounding to float32 moves the shapes by half an ulp of their coordinates)
        assert c["ref"] >= 4.0 * dl, (who, c["ref"], dl)
        if c["max_distance"] is not None:
            assert abs(float(c["max_distance"]) - c["ref"]) >= 4.0 * dl * (1 - 1e-3) - 1e-7 * c["scale"], who
            assert (c["expect"] == "hit") == (float(c["max_distance"]) > c["ref"]), who
        else:
            assert c["expect"] == "hit", who
    print(f"{name}: {len(cases)} cases, largest |gap - placed| {worst:.2e}")


def test_cut_asks_both_sides_of_every_pair():
    for a, b in zip(D.family("cut")[::2], D.family("cut")[1::2]):
        assert (a["vt"], a["ct"], a["expect"], b["expect"]) == (b["vt"], b["ct"], "miss", "hit") and a["volume"].tobytes() == b["volume"].tobytes()


def test_reference_matches_closed_forms():
    q = np.array([0.0, 0.0, np.sin(0.3), np.cos(0.3)])
    box = M.conv64(M.shifted(M.aabb((1.0, 0.5, 0.7)), (10, 0, 0)))
    rows = [   # (a, b, gap, direction from b to a or None)
        (M.conv64(M.shifted(M.sphere(0.25), (3, 4, 0))), M.conv64(M.sphere(0.5)), 5 - 0.75, (0.6, 0.8, 0)),                                  # sphere - sphere
        (M.conv64(M.shifted(M.sphere(0.25), (13, 0.1, 0.2))), box, 2 - 0.25, (1, 0, 0)),                                                      # sphere - box face
        (M.conv64(M.shifted(M.sphere(0.25), (12, 1.5, 0.2))), box, np.sqrt(2) - 0.25, (np.sqrt(0.5), np.sqrt(0.5), 0)),                       # ... edge
        (M.conv64(M.shifted(M.sphere(0.25), (12, 1.5, 1.7))), box, np.sqrt(3) - 0.25, np.ones(3) / np.sqrt(3)),                               # ... corner
        (M.conv64(M.shifted(M.capsule(1.0, 0.2, 0), (0, 2, 0))), M.conv64(M.capsule(1.0, 0.3, 2)), 2 - 0.5, (0, 1, 0)),                       # skew capsules: axes x and z, 2 apart in y
        (M.conv64(M.shifted(M.aabb((0.5, 0.5, 0.5)), (13, 0.2, 0.1))), box, 1.5, (1, 0, 0)),                                                  # box - box, faces
        (M.conv64(M.shifted(M.aabb((0.5, 0.5, 0.5)), (13, 3, 0.1))), box, np.hypot(1.5, 2.0), (0.6, 0.8, 0)),                                 # ... edges
        (M.conv64(M.shifted(M.obb((0.5, 0.5, 0.5), q, 1), (14, 0, 0))), box, 3 - 0.5 * (np.cos(0.6) + np.sin(0.6)), (1, 0, 0)),             # a turned box, edge towards the face
    ]
    for i, (a, b, gap, n) in enumerate(rows):
        g, n_ref, pb, pa = D.closest(a, b)
        assert abs(g - gap) <= 1e-12 and np.linalg.norm(n_ref - n) <= 1e-9, (i, g, gap, n_ref)
        assert abs(S.gap(a, b) - gap) <= 1e-12 and np.linalg.norm((pa - pb) - g * n_ref) <= 1e-12, i
        assert abs(S.point_gap(pb, b)) <= 1e-12 and abs(S.point_gap(pa, a)) <= 1e-12, i


def test_record_layout():
    from d3d12renderer_amd import capi
    t = capi.distance_hit_dtype
    assert t.itemsize == 64
    assert [t.fields[n][1] for n in ("entity", "collider", "distance", "object_type", "point_collider", "flags", "point_volume", "volume", "normal", "pad")] == [0, 4, 8, 12, 16, 28, 32, 44, 48, 60]
    assert (capi.DISTANCE_OVERLAP, capi.DISTANCE_UNCONVERGED) == (1, 2)
