"""The matrix of tests/sweep_terrain_matrix.py checked without a GPU, from the float64 reference alone: every family holds the volume types it
names, every decision the GPU test asserts is at least 4 delta from flipping by the reference on the rounded numbers, a family drops at most one
generated case in eight and keeps every volume type, the wide family's footprints span more than 64 blocks across the travel with the touch in the
second pass of 64, the lattice straddles every kind of line over solid ground, and the reference with its map-by-name extension and its ordered
pair casts still equals closed forms on the floor and the offset map."""
import collections

import numpy as np
import pytest

import overlap_ref as R
import raycast_terrain_matrix as RT
import sweep_matrix as SM
import sweep_ref as S
import sweep_terrain_matrix as M
import sweep_terrain_ref as ST


@pytest.mark.parametrize("name", M.FAMILIES)
def test_family_is_a_valid_yardstick(name):
    cases, kept = M.family(name), M.kept(name)
    per_type = collections.Counter(c["vt"] for c in kept)
    margins = [c["clearance"] / M.delta(c) for c in kept if c["expect"] != "invalid" and not c.get("on_surface")]    # (on_surface: closed form, below)
    said = collections.Counter(c["expect"] for c in kept)
    print(f"{name}: {len(cases)} generated, {len(kept)} kept ({dict(said)}), per type {[per_type[t] for t in M.FAMILY_TYPES.get(name, M.SIX)]}, "
          f"smallest clearance {min(margins, default=np.inf):.2f} delta, scales up to {max(c['scale'] for c in kept):.4g}")
    for c in cases:
        if not c["kept"]:
            print(f"  dropped: {c['tag']} on {c['map']}: meant as {c['expect']}, the reference: {'a miss' if c['ref'] is None else 'initial' if c['ref'][3] else 'a hit'}, "
                  f"{c['clearance'] / M.delta(c):.2f} delta clear")
    assert set(per_type) >= set(M.FAMILY_TYPES.get(name, M.SIX)), per_type
    assert len(cases) - len(kept) <= len(cases) // 8, (len(cases), len(kept))
    assert all(m >= 4.0 for m in margins), min(margins)
    for c in kept:
        if c["expect"] == "invalid":
            continue
        ref = c["ref"]
        assert (ref is None) == (c["expect"] == "miss") and (ref is None or bool(ref[3]) == (c["expect"] == "initial")), c["tag"]
        assert c["scale"] == ST.scale_of(c["conv"], c["d"]) and c["volume"]["type"][0] in range(6)
        if c.get("on_surface"):    # closed form: the lowest point lies on the floor map's plane exactly; the reference finds the gap 0
            assert ST.min_gap(c["map"], c["conv"], 1e-3) == 0.0, c["tag"]
    if name in ("generic", "features", "far"):
        assert {c["map"] for c in kept} == set(M.HILLS)
    if name == "features":
        assert {c["feature"] for c in kept} == set(M.FEATURES) and sum(c["tag"].startswith("point_") for c in kept) >= 24
    if name == "limits":
        assert said["hit"] >= 12 and said["miss"] >= 12
    if name == "initial":
        assert said["initial"] >= 24 and said["hit"] >= 12 and said["miss"] >= 6
    if name == "ordering":
        assert sum(c["collider_wins"] for c in kept) >= 4 and sum(not c["collider_wins"] for c in kept) >= 4


def test_the_wide_family_runs_the_second_pass_over_the_blocks():
    """By the kernel's own footprint formula every cast spans more than 64 blocks across the travel; the reference's touch of the `far` casts lies 64
    blocks or more from the footprint's first block (the second pass of the walk over the blocks of a row), that of the partners in the first 64."""
    hm = ST.wide_map()
    cell = hm["chunk_size"] / 128.0
    for c in M.kept("wide"):
        lo, hi = M.footprint_blocks(c)
        w = 2 if abs(c["disp"][0]) >= abs(c["disp"][2]) else 0
        block = int((c["ref"][2][w] - hm["min_corner"][w]) / cell) >> 3
        print(f"{c['tag']}: blocks {lo} to {hi} across the travel, the touch in block {block}")
        assert hi - lo >= 64, (c["tag"], lo, hi)
        assert (block - lo >= 64) == c["second_pass"], (c["tag"], lo, block)
    assert sum(c["second_pass"] for c in M.kept("wide")) >= 8 and sum(not c["second_pass"] for c in M.kept("wide")) >= 3
    # zero horizontal travel, and |d.x| = |d.z|
    assert any(c["disp"][0] == 0 and c["disp"][2] == 0 for c in M.kept("wide")) and any(c["disp"][0] == c["disp"][2] != 0 for c in M.kept("wide"))


def test_the_axes_family_holds_its_directions():
    d = np.stack([c["disp"] for c in M.kept("axes")])
    for axis in range(3):
        others = [a for a in range(3) if a != axis]
        for sign in (-1, 1):
            assert ((np.sign(d[:, axis]) == sign) & (d[:, others] == 0).all(axis=1)).any(), (axis, sign)
    assert ((d[:, 0] == 0) & (d[:, 2] != 0) & (d[:, 1] != 0)).any() and ((d[:, 2] == 0) & (d[:, 0] != 0) & (d[:, 1] != 0)).any()
    ties = {(np.sign(x), np.sign(z)) for x, _, z in d if x != 0 and abs(x) == abs(z)}
    assert len(ties) == 4, ties


@pytest.mark.parametrize("mapname", M.LATTICE_MAPS)
def test_the_lattice_straddles_every_line_over_solid_ground(mapname):
    xs, zs, h, kinds = M.lattice(mapname)
    m = M.the_map(mapname)
    count = collections.Counter(kinds)
    print(f"lattice on {mapname}: {len(xs)} casts, {dict(count)}")
    assert 2000 <= len(xs) <= 9000 and np.isfinite(h).all()
    want = {"vertex", "xline", "zline", "diagonal", "block", "border"} | ({"seam", "chunk_vertex"} if mapname != "floor" else set())
    assert set(count) == want
    # on the lines themselves and one and two float32 steps to either side
    u = (xs.astype(np.float64) - m.x0) / m.s
    on = np.flatnonzero((np.array(kinds) == "vertex") & (u == np.round(u)))
    assert len(on) >= 40
    x = xs[on[0]]
    assert {np.float32(v) for v in xs[np.array(kinds) == "vertex"] if abs(v - x) <= 3 * abs(np.spacing(x))} >= {M._ulps(x, k) for k in (-2, -1, 0, 1, 2)}


def test_the_reference_equals_closed_forms_on_the_floor_and_the_offset_map():
    """A sphere straight down onto the floor map (y = 2 exactly) to 1e-7; the offset map is the rolling map moved: the same casts moved with it give
    the same times to 1e-7."""
    ball = S.convex(R.world_shape(R.SPHERE, np.array([0, 0, 0, 0.5]), (3.3, 5.0, 4.7), (0, 0, 0, 1)))
    t, n, p, initial = ST.cast("floor", ball, (0.0, -4.0, 0.0))
    assert not initial and abs(t - (5.0 - 0.5 - RT.FLOOR_Y) / 4.0) <= 1e-7 and np.allclose(n, (0, 1, 0), atol=1e-7) and abs(p[1] - RT.FLOOR_Y) <= 1e-7
    t, n, p, initial = ST.cast("floor", ball, (0.3, -4.0, 0.2))
    assert not initial and abs(t - (5.0 - 0.5 - RT.FLOOR_Y) / 4.0) <= 1e-7
    assert ST.cast("floor", ball, (0.0, -2.4, 0.0)) is None and ST.cast("floor", S.moved(ball, (0, -4.0, 0)), (0.0, -2.0, 0.0)) is None
    shift = np.asarray(RT.OFFSET_CORNER, np.float64) - M.the_map("rolling").corner
    worst = 0.0
    for c in [c for c in M.kept("generic") if c["map"] == "rolling"][:8]:
        moved = ST.cast("offset", S.moved(c["conv"], shift), c["d"])
        assert (moved is None) == (c["ref"] is None)
        if moved is not None:
            worst = max(worst, abs(moved[0] - c["ref"][0]))
            assert abs(moved[0] - c["ref"][0]) <= 1e-7 and np.allclose(moved[1], c["ref"][1], atol=1e-6)
    print(f"offset map against the rolling map moved: largest |dt| {worst:.2e}")
