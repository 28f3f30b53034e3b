"""The comparison set of the terrain distance queries (tests/terrain_distance_ref.py) is a valid yardstick for tests/test_gpu_terrain_distance.py:
every decision the GPU test asserts is far enough from flipping that the accuracy bound cannot flip it, nothing is left out, and the set kept
under tests/golden is what the reference computes.  Also: the blocking binding rejects wrong argument shapes.  No GPU."""
import numpy as np
import pytest

import overlap_ref as R
import terrain_distance_ref as TD


def test_comparison_set_is_a_valid_yardstick():
    c = TD.comparison_reference()
    n = len(c["volumes"])
    assert n == 48 and len(TD.GROUPS) == 8
    assert [int(t) for t in c["volumes"]["type"]] == [i % 6 for i in range(n)]   # eight of each type, one per group
    per_group = {g: [c["expect"][i] for i in range(n) if c["groups"][i] == g] for g in TD.GROUPS}
    assert per_group["cutting"] == ["overlap"] * 6 and per_group["short"] == ["miss"] * 6
    for g in ("above", "below", "beside", "hole", "beyond", "near"):
        assert per_group[g] == ["hit"] * 6, (g, per_group[g])
    # the groups are where they say they are: outside the map, over the hole
    pos = c["volumes"]["position"].astype(np.float64)
    beside = [i for i in range(n) if c["groups"][i] == "beside"]
    assert all(np.abs(pos[i, [0, 2]]).max() > 32.4 and np.abs(pos[i, [0, 2]]).max() < 36.0 for i in beside)
    hole = [i for i in range(n) if c["groups"][i] == "hole"]
    assert all(0 < pos[i, 0] < 32 and -32 < pos[i, 2] < 0 for i in hole)
    assert all(pos[i, 1] < -1.9 for i in range(n) if c["groups"][i] == "below")
    worst = 0.0
    for i in range(n):
        ref, max_d, scale, what = float(c["ref"][i]), float(c["max_distances"][i]), c["scales"][i], (i, c["groups"][i], c["expect"][i])
        need = 16 * TD.BOUND * scale
        worst = max(worst, need)
        if c["expect"][i] == "overlap":
            assert TD.overlap_holds(c, i), what
            # (1e-3 is the smallest of the three margins: it exceeds 16 bounds only because the cutting group stands near the origin, scales below 4)
            assert TD.OVERLAP_MARGIN > need, (what, need)
            continue
        assert ref >= TD.GAP_MARGIN and TD.GAP_MARGIN > need, (what, ref, need)
        if np.isfinite(max_d):     # a hit / miss decision by the largest distance
            assert abs(ref - max_d) >= TD.DECISION_MARGIN and TD.DECISION_MARGIN > need, (what, ref, max_d, need)
            assert (ref <= max_d) == (c["expect"][i] == "hit")
    assert sum(np.isfinite(c["max_distances"])) == 12
    print(f"largest 16 x BOUND x scale of the set: {worst:.2e}")


def test_golden_set_is_what_the_reference_computes():
    have, now = TD.comparison_reference(), TD.comparison_reference(recompute=True)
    assert have["volumes"].tobytes() == now["volumes"].tobytes()
    assert have["max_distances"].tobytes() == now["max_distances"].tobytes()
    assert np.abs(have["ref"] - now["ref"]).max() <= 1e-9 and have["expect"] == now["expect"]


def test_the_binding_rejects_wrong_argument_shapes():
    from d3d12renderer_amd import capi
    w = capi.World.__new__(capi.World)   # (no handle: the shapes are checked before the library is called)
    vols = R.make_volumes(1, 1, (-1, 0, -1), (1, 2, 1))
    for fn in (w.terrain_distance, w.debug_terrain_distance_exhaustive):
        with pytest.raises(ValueError):
            fn(vols, np.zeros(len(vols) + 1, np.float32))
        with pytest.raises(ValueError):
            fn(vols, np.zeros((len(vols), 1), np.float32))
        with pytest.raises(ValueError):
            fn(vols, None, merge_into=np.zeros(len(vols) - 1, capi.distance_hit_dtype))
        with pytest.raises(ValueError):
            fn(vols, None, merge_into=np.zeros(len(vols), capi.sweep_hit_dtype))
        with pytest.raises(ValueError):
            fn(vols, None, merge_into=np.zeros((1, len(vols)), capi.distance_hit_dtype))
