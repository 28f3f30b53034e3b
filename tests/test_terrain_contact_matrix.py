"""The terrain contact matrix (tests/terrain_contact_matrix.py) without a GPU: the oracle against the reference's own heightmapCollision on every case,
one world per case; the matrix's coverage on the oracle's output; and the lowest-point contact of cylinders and hulls, which the reference cannot
vouch for, against float64."""
import numpy as np
import pytest

import terrain_contact_matrix as M
import terrain_contact_ref as T
from d3d12renderer_amd import capi

needs_reference = pytest.mark.skipif(not __import__("oracle").reference_available(), reason="neither /root/reference nor a prebuilt oracle/_ref/libref.so")


def _who(c):
    return f"{c['family']} {c['map']} {c['tag']}"


def _one_step(world_factory, c):
    """The terrain contacts (point, depth, normal in list order) of one step of a world that holds the case's map and its volume as a body."""
    sc = T.terrain_scene(M.the_map(c["map"]), *T.volume_bodies(c["volume"]))
    w = sc.populate(world_factory())
    w.step_fixed(sc.settings(), sc.dt, 1)
    con = w.contacts()
    w.close()
    out = np.zeros(len(con), capi.terrain_contact_dtype)
    out["point"] = con["point"]; out["depth"] = con["penetration_depth"]; out["normal"] = con["normal"]
    return out


# ---- 1. the yardstick itself
@needs_reference
@pytest.mark.parametrize("name", M.FAMILIES)
def test_reference_equals_oracle(oracle_mod, name):
    """Points, depths and normals of the reference's own step and of the oracle's, byte for byte and in order, for every case but the cylinder and hull
    volumes (undefined behaviour in the reference) and the cases to which the oracle gives 255 contacts (the reference's uint8 count wraps there)."""
    make_oracle = lambda: oracle_mod.create_world(oracle_mod.ORDER_REFERENCE)   # noqa: E731
    differ, lowest_only, capped, compared = [], 0, 0, 0
    for c in M.family(oracle_mod, name):
        if c["vt"] in M.LOWEST_ONLY:
            lowest_only += 1
            continue
        o = _one_step(make_oracle, c)
        if len(o) == M.CAP:
            capped += 1
            continue
        r = _one_step(oracle_mod.create_reference_world, c)
        compared += 1
        if r.tobytes() != o.tobytes():
            differ.append(f"{_who(c)}: the reference has {len(r)} contacts, the oracle {len(o)}")
    print(f"{name}: {compared} cases compared, {len(differ)} differ; left out: {lowest_only} cylinder and hull volumes, {capped} cases of {M.CAP} contacts")
    assert capped == 0 or name == "windows", f"{name}: {capped} cases at the cap"
    assert compared > 0
    assert not differ, f"{len(differ)} of {compared} cases differ:\n" + "\n".join(differ[:30])


# ---- 2. the cap
def _windows(c, box):
    return [n for _, _, n in T.chunk_windows(M.the_map(c["map"]), box)]


@pytest.mark.parametrize("name", M.FAMILIES)
def test_the_cap(oracle_mod, name):
    """On the oracle's output: every type the family applies to has at least 3 cases with contacts and 3 without (many_chunks and size: 1), and the
    family reaches the windows and the counts its text names, measured by chunk_windows on the oracle's own AABBs."""
    res = M.results(oracle_mod, name)
    least = 1 if name in M.LOOSE else M.MIN_WITH
    table = {t: [0, 0] for t in M.family_types(name)}
    for c, recs, box in res:
        assert c["vt"] in table, _who(c)
        table[c["vt"]][0 if len(recs) else 1] += 1
        assert len(recs) <= M.CAP and (c["vt"] not in M.LOWEST_ONLY or len(recs) <= 1), _who(c)
    print(f"{name}: {len(res)} cases, {sum(len(r) > 0 for _, r, _ in res)} with contacts, {sum(len(r) == 0 for _, r, _ in res)} without; per type (with, without) "
          f"{ {M.NAMES[t]: tuple(v) for t, v in table.items()} }")
    for t, (hits, misses) in table.items():
        assert hits >= least and misses >= least, f"{name} {M.NAMES[t]}: {hits} with contacts, {misses} without"
    if name == "rim":
        largest = {}
        for c, recs, box in res:
            if c["place"] != "straddle":
                largest.setdefault(c["spot"], []).append(max(_windows(c, box), default=0))
        print("rim: the windows of the volumes outside the map:", {k: sorted(set(v)) for k, v in largest.items()})
        for spot in ("x_low", "z_low"):
            assert max(largest[spot]) >= 128 and max(largest[spot]) % 128 == 0, (spot, largest[spot])
        assert max(largest["low_low"]) == 128 * 128
        for spot in ("x_high", "z_high"):
            assert min(largest[spot]) == 0, (spot, largest[spot])
    if name == "windows":
        by_tag = {c["tag"]: (c, recs, box) for c, recs, box in res}
        for c, recs, box in res:
            if "cells" in c:
                assert _windows(c, box) == c["cells"], (_who(c), _windows(c, box))
            if "count" in c:
                assert len(recs) == c["count"], (_who(c), len(recs))
        # more than the cap: two boxes inside the large one's bounds, side by side, have more than 255 triangle contacts between them
        big = by_tag["over_cap"][2]
        witness = [by_tag[f"over_cap_witness{j}"] for j in range(2)]
        for _, recs, box in witness:
            assert len(recs) < M.CAP and (box[:3] >= big[:3]).all() and (box[3:] <= big[3:]).all()
        assert witness[0][2][3] < witness[1][2][0] and sum(len(r) - 1 for _, r, _ in witness) > M.CAP
        assert max(_windows(*by_tag["over_cap"][::2])) > 2000
    if name == "seam_exact":
        for c, recs, box in res:
            if c["twin"] == 0:      # the oracle's bound is the line itself
                k = (0 if c["axis"] == "x" else 2) + (0 if c["which"] == "min" else 3)
                assert float(box[k]) == c["line"], (_who(c), box)
        # the reference's quirk: a box whose upper bound is the seam gets no cell of the chunk it lies in and the first column of the next one
        quirk = {c["tag"]: T.chunk_windows(M.the_map("exact"), box) for c, recs, box in res if c["tag"] in ("max_x_seam_AABB", "max_z_seam_AABB")}
        assert quirk["max_x_seam_AABB"][0][2] == 0 and quirk["max_x_seam_AABB"][1][:2] == (1, 0) and quirk["max_x_seam_AABB"][1][2] > 0, quirk
        assert quirk["max_z_seam_AABB"][0][2] == 0 and quirk["max_z_seam_AABB"][1][:2] == (0, 1) and quirk["max_z_seam_AABB"][1][2] > 0, quirk
    if name == "many_chunks":
        for cpd in (256, 257):
            n = [len(r) for c, r, _ in res if c["map"] == f"many{cpd}"]
            assert min(k for k in n if k) <= M.STASH < max(n), (cpd, sorted(set(n)))
            assert M.the_map(f"many{cpd}")["chunks_per_dim"] == cpd and len(M.the_map(f"many{cpd}")["chunks"]) == 4
    if name == "maps":
        three = [T.chunk_windows(M.the_map("wide"), box) for c, recs, box in res if c["tag"].startswith("wide_three_chunks")]
        assert len(three) == 2 and all(len(w) == 3 and min(n for _, _, n in w) > 0 for w in three), three


def test_the_shared_windows_are_equal_on_both_maps(oracle_mod):
    """The small windows in chunk (255, 255), which the maps of 256 and of 257 chunks per dimension share: the oracle gives both the same bytes."""
    tags, vols, (o256, r256, b256), (o257, r257, _) = M.shared_expected(oracle_mod)
    n = np.diff(o256.astype(np.int64))
    print(f"shared windows: {len(tags)} volumes, counts {sorted(set(n.tolist()))}")
    assert len(tags) >= 8 and (n > 0).sum() >= 5 and n.max() <= M.STASH
    assert all(T.largest_window(M.the_map("many256"), b) <= 64 for b in b256)
    assert o256.tobytes() == o257.tobytes() and r256.tobytes() == r257.tobytes()


# ---- 3. cylinders and hulls: the lowest point under the bilinear surface, against float64
def test_lowest_point_contacts_against_float64(oracle_mod):
    """The single contact of a cylinder or hull volume: normal (0, -1, 0) exactly, the point the float64 support point along -y (the lowest vertex of
    the transformed mesh), the depth the float64 bilinear height over the point minus its y, within M.BOUNDS per unit of scale; and the oracle
    reports one exactly when float64 finds the lowest point under the surface (an undecided case: within the depth's bound of it)."""
    worst = {"point": (0.0, ""), "depth": (0.0, "")}
    seen = undecided = 0
    for name in M.FAMILIES:
        for c, recs, _ in M.results(oracle_mod, name):
            if c["vt"] not in M.LOWEST_ONLY:
                continue
            hm, v = M.the_map(c["map"]), c["volume"][0]
            low, unique = M.lowest_point(hm, v)
            h = M.height64(hm, low[0], low[2])
            scale = max(1.0, float(np.abs(low).max()))
            if len(recs) == 0:
                if h is not None and low[1] < h:
                    assert h - low[1] <= M.BOUNDS["depth"] * scale or not unique, f"{_who(c)}: no contact, the lowest point lies {h - low[1]:.3g} under the surface"
                    undecided += 1
                continue
            assert len(recs) == 1 and recs["normal"][0].tobytes() == np.array((0.0, -1.0, 0.0), np.float32).tobytes(), _who(c)
            p = recs["point"][0].astype(np.float64)
            if unique:
                e = float(np.abs(p - low).max()) / scale
            else:       # an upright cylinder: any point of the lower cap, at the cap's height
                r = float(v["shape"][6])
                e = max(abs(p[1] - low[1]), max(np.hypot(p[0] - low[0], p[2] - low[2]) - r, 0.0)) / scale
            if e > worst["point"][0]:
                worst["point"] = (e, _who(c))
            h_at = M.height64(hm, p[0], p[2])
            assert h_at is not None, _who(c)
            e = abs(float(recs["depth"][0]) - (h_at - p[1])) / scale
            if e > worst["depth"][0]:
                worst["depth"] = (e, _who(c))
            seen += 1
    print(f"lowest-point contacts: {seen} cases, {undecided} undecided; largest error per unit of scale: point {worst['point'][0]:.3g} ({worst['point'][1]}), "
          f"depth {worst['depth'][0]:.3g} ({worst['depth'][1]}); bounds {M.BOUNDS}")
    assert seen >= 200
    for k in ("point", "depth"):
        assert worst[k][0] <= M.BOUNDS[k], (k, worst[k])
