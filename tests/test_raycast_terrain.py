"""The terrain ray-cast matrix (tests/raycast_terrain_matrix.py) checked from the float64 reference alone, no GPU: the robustness filter keeps
enough of every family, the families hold what their recipes call for, the closed forms of the flat and tilted maps and of vertical rays agree
with the reference, and the set is not vacuous: a float32 restatement of an inclusion test of the hit point within 1e-4 of a cell, every
triangle computing its own t and its own point, loses kept cases far from the origin."""
from collections import Counter

import numpy as np

import raycast_terrain_matrix as M
import sweep_terrain_ref as ST


def test_filter_keeps_enough():
    total = 0
    for name in M.FAMILIES:
        cases = M.family(name)
        kept = M.kept(name)
        total += len(cases)
        print(f"{name}: {len(cases)} generated, {len(kept)} kept ({sum(c['t'] is not None for c in kept)} hits, {sum(c['t'] is None for c in kept)} misses)")
        assert len(kept) >= (4 if name in ("ordering", "invalid") else 16), name
        assert 4 * (len(cases) - len(kept)) <= len(cases), name
    assert total <= 800


def test_families_hold_hits_and_misses():
    hits_only = ("far", "ordering")   # their recipes aim at the surface; a miss is not part of them
    for name in M.FAMILIES:
        kept = M.kept(name)
        hits, misses = [c for c in kept if c["t"] is not None], [c for c in kept if c["t"] is None]
        if name == "invalid":
            assert not hits
            continue
        assert hits and (misses or name in hits_only), name
    tags = lambda name, hit: Counter(c["tag"].rstrip("0123456789") for c in M.kept(name) if (c["t"] is not None) == hit)   # noqa: E731
    down, up = tags("axes", True), tags("axes", False)
    assert down["down"] >= 12 and up["up"] >= 2 and sum(v for k, v in down.items() if k.startswith("level")) >= 4 and down["edge_flat"] + down["edge_rolling"] >= 8
    assert sum(v for k, v in down.items() if k.startswith("diag")) >= 2
    below = M.kept("below")
    assert sum(c["tag"].startswith("up") and c["t"] is not None for c in below) >= 8 and sum(c["tag"].startswith("down") and c["t"] is None for c in below) >= 8
    on = [c for c in below if c.get("on_surface")]
    assert len(on) >= 8 and all(c["t"] == 0 for c in on) and sum(c["d"][1] < 0 for c in on) >= 3 and sum(c["d"][1] > 0 for c in on) >= 3
    assert len(M.family("below")) == len(below)   # nothing generated that the filter cannot keep
    out = tags("outside", True)
    for what in ("side-x", "side+x", "side-z", "side+z", "corner--", "corner-+", "corner++", "hole+x", "hole-z"):
        assert out[what] >= 2, what
    miss = tags("outside", False)
    for what in ("over", "away", "beside-x", "beside+z", "hole_through"):
        assert miss[what] >= 2, what
    graze = M.kept("grazing")
    assert all(c["path"] > 200 * M.the_map("rolling").s and abs(c["d"][1]) < 3e-3 for c in graze)
    assert sum(c["t"] is None for c in graze) >= 12 and sum(c["t"] is not None for c in graze) >= 12   # clear of the ridge, and into it
    lim = Counter((c["tag"].rsplit("_", 1)[1], c["t"] is not None) for c in M.kept("limits"))
    assert lim["short", False] >= 4 and lim["reach", True] >= 4 and lim["zero", False] >= 4 and lim["inf", True] >= 4
    order = M.kept("ordering")
    assert sum(c["sphere_wins"] for c in order) >= 2 and sum(not c["sphere_wins"] for c in order) >= 2
    lengths = {round(float(np.log10(np.linalg.norm(c["d"]))), 1) for c in M.kept("direction_length") if c["t"] is not None}
    assert len(lengths) == len(M.LENGTHS)
    for c in M.kept("far"):
        assert np.linalg.norm(c["o"] - c["point"]) > 0.9 * 1e2
    for c in M.kept("offset"):
        assert np.abs(c["o"]).max() > 2000 and (c["t"] is None or c["t"] < 30)


def test_features_reach_every_spot():
    for name, least in (("features", 8), ("offset", 6), ("far", 8)):
        spots = Counter(c["feature"] for c in M.kept(name) if M.on_target(c))
        for kind in M.FEATURE_KINDS:
            assert spots[kind] >= least, (name, kind, spots)
    sides = Counter((c["feature"], c["t"] is not None) for c in M.kept("features") if c.get("feature") in ("border", "rim"))
    assert sides["border", True] >= 6 and sides["border", False] >= 6 and sides["rim", True] >= 3 and sides["rim", False] >= 3


def test_closed_forms():
    """Flat: the plane y = FLAT_Y; tilted: y = TILT_SLOPE x; a vertical ray: the height of the triangle under it.  To 1e-12."""
    seen = Counter()
    for c in M.kept("generic") + M.kept("axes") + M.kept("limits"):
        o, d, m = c["o"], c["d"], M.the_map(c["map"])
        if c["map"] == "flat":
            t = (ST.FLAT_Y - o[1]) / d[1]
        elif c["map"] == "tilted":
            t = (ST.TILT_SLOPE * o[0] - o[1]) / (d[1] - ST.TILT_SLOPE * d[0])
        elif d[0] == 0 and d[2] == 0 and d[1] < 0:
            t = (m.height(o[0], o[2]) - o[1]) / d[1]
        else:
            continue
        p = o + t * d
        inside = m.x0 <= p[0] <= m.x0 + m.size and m.z0 <= p[2] <= m.z0 + m.size
        if 0 <= t <= c["max_t"] and inside:
            assert c["t"] is not None and abs(c["t"] - t) <= 1e-12 * max(1.0, t), (c["tag"], c["t"], t)
        else:
            assert c["t"] is None, c["tag"]
        seen[c["map"]] += 1
    assert seen["flat"] >= 8 and seen["tilted"] >= 8 and seen["rolling"] >= 12, seen


def _inclusion_in_float32(m, o, d):
    """Whether a test of each triangle on its own finds the ray, all in float32: t from the triangle's plane, the point o + t d, the point's cell
    coordinates u, v within e = 1e-4 of the triangle.  Every triangle of every cell under the ray's way through the map's heights is tried."""
    f = np.float32
    o, d, s, e = o.astype(f), d.astype(f), f(m.s), f(1e-4)
    o64, d64 = o.astype(np.float64), d.astype(np.float64)
    ts = sorted(((m.ymax + 0.5 - o64[1]) / d64[1], (m.ymin - 0.5 - o64[1]) / d64[1]))
    ends = np.array([o64 + t * d64 for t in ts])
    gx0, gz0 = (np.floor((ends[:, 0].min() - m.x0) / m.s) - 2, np.floor((ends[:, 2].min() - m.z0) / m.s) - 2)
    gx1, gz1 = (np.floor((ends[:, 0].max() - m.x0) / m.s) + 2, np.floor((ends[:, 2].max() - m.z0) / m.s) + 2)
    gz, gx = np.meshgrid(np.arange(max(gz0, 0), min(gz1, m.n - 1) + 1, dtype=int), np.arange(max(gx0, 0), min(gx1, m.n - 1) + 1, dtype=int), indexing="ij")
    gz, gx = gz[m.solid[gz, gx]], gx[m.solid[gz, gx]]

    def vertex(ix, iz):
        return np.stack([(ix * m.s + m.x0).astype(f), m.H[iz, ix].astype(f), (iz * m.s + m.z0).astype(f)], axis=-1)
    a, b, c, dd = vertex(gx, gz), vertex(gx, gz + 1), vertex(gx + 1, gz), vertex(gx + 1, gz + 1)
    found = False
    for tri, (p0, n) in enumerate(((a, np.cross(b - a, c - a)), (c, np.cross(b - c, dd - c)))):
        n = n.astype(f)
        dn = (n * d).sum(axis=1, dtype=f)
        with np.errstate(divide="ignore", invalid="ignore"):
            t = ((p0 - o) * n).sum(axis=1, dtype=f) / dn
            p = o + t[:, None] * d
            u, v = (p[:, 0] - a[:, 0]) / s, (p[:, 2] - a[:, 2]) / s
            ok = (u >= -e) & (v >= -e) & (u + v <= f(1) + e) if tri == 0 else (u <= f(1) + e) & (v <= f(1) + e) & (u + v >= f(1) - e)
        found = found or bool((ok & (dn != 0) & (t >= 0)).any())
    return found


def test_the_set_is_not_vacuous():
    """A per-triangle inclusion test in float32 finds some kept `far` or `offset` hit in neither triangle of any cell: the rounding of o + t d at
    coordinates of thousands is many times 1e-4 of a cell, and the two triangles of a shared edge each find their own point just outside."""
    lost = Counter()
    for name in ("far", "offset"):
        for c in M.kept(name):
            if c["t"] is not None and c["d"][1] < 0 and not _inclusion_in_float32(M.the_map(c["map"]), c["o32"], c["d32"]):
                lost[name] += 1
    print(f"a float32 per-triangle inclusion test loses {dict(lost)} kept hits of far / offset")
    assert sum(lost.values()) >= 1
    # ... and none of the rays near the origin that are not aimed at an edge
    for c in M.kept("generic"):
        if c["t"] is not None and c["map"] == "rolling":
            assert _inclusion_in_float32(M.the_map("rolling"), c["o32"], c["d32"]), c["tag"]
