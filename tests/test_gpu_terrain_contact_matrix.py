"""The terrain contact matrix (tests/terrain_contact_matrix.py) on the GPU, bit for bit against the oracle, which tests/test_terrain_contact_matrix.py
holds to the reference's own heightmapCollision on the same cases.

Query (mi_world_terrain_contacts, the pipeline of csrc/heightmap.hpp through HmQueryOut): per map one world and one call over all of the map's cases,
an odd batch, and once more with the batch reversed, so that the volumes of the large-window instance and of the plain one share groups of 64 in
another mix.  Step (the same pipeline through HmOut): the same volumes as gravity-free dynamic bodies, one step on the GPU and on the oracle in
canonical order: counts, the terrain contacts and the poses (a NaN pose, which the massless body of a degenerate volume gets on both sides, equals a
NaN; where the oracle, like the reference, hands that NaN on through the terrain's static body and the library does not, a stated deviation, the
other bodies are held to the oracle's world with the massless ones parked off the map).  Both instances of the WRITE pass: the maps of 256 and of 257 chunks per dimension (above 256 the stash id cannot hold the chunk, and the
wave-per-collider pass writes every collider) give the same bytes for the same small windows in the chunk they share."""
from dataclasses import replace

import numpy as np
import pytest

import contact_matrix as CM
import terrain_contact_matrix as M
import terrain_contact_ref as T

pytestmark = pytest.mark.gpu

MAP_NAMES = ("rolling", "offset", "coarse", "exact", "fine", "flat", "tilted", "floor", "plateau", "ripple", "wide", "many256", "many257")


def _query_world(mi, mapname):
    return T.terrain_scene(M.the_map(mapname)).populate(mi.create_world(0))


def test_every_map_of_the_matrix_is_run(oracle_mod):
    assert set(M.by_map(oracle_mod)) == set(MAP_NAMES)


# ---- the query
@pytest.mark.parametrize("name", MAP_NAMES)
def test_query_matrix_matches_oracle(mi_lib, oracle_mod, name):
    cases, vols, want_offsets, want_recs, _ = M.expected(oracle_mod, name)
    n = len(vols)
    assert n % 2 == 1
    w = _query_world(mi_lib, name)
    offsets, recs = w.terrain_contacts(vols)
    back_offsets, back_recs = w.terrain_contacts(vols[::-1])
    w.close()
    print(f"{name}: {n} volumes, {len(recs)} records, oracle {len(want_recs)}")
    problems = T.differences(offsets, recs, want_offsets, want_recs)
    assert not problems, "\n".join(problems) + "\nfirst cases: " + ", ".join(c["tag"] for c in cases[:3])
    # reversed: volume v of the batch is case n - 1 - v; its records are the same bytes under that index
    sizes = np.diff(want_offsets.astype(np.int64))[::-1]
    rev_offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
    rev_recs = np.concatenate([want_recs[int(want_offsets[i]):int(want_offsets[i + 1])] for i in range(n - 1, -1, -1)]) if len(want_recs) else want_recs.copy()
    rev_recs["volume"] = n - 1 - rev_recs["volume"]
    problems = T.differences(back_offsets, back_recs, rev_offsets, rev_recs)
    assert not problems, "reversed batch: " + "\n".join(problems)


# ---- the step
@pytest.mark.parametrize("name", MAP_NAMES)
def test_step_matrix_matches_oracle(mi_lib, oracle_mod, name):
    cases, vols, _, want_recs, _ = M.expected(oracle_mod, name)
    sc = M.step_scene(name, vols)
    o = sc.populate(oracle_mod.create_world(oracle_mod.ORDER_CANONICAL))
    o.step_fixed(sc.settings(), sc.dt, 1)
    counts, want_xf = o.counts(), tuple(np.array(a) for a in o.physics_transforms())
    o.close()
    g = sc.populate(mi_lib.create_world(0))
    g.step_fixed(sc.settings(), sc.dt, 1)
    got_counts, got_xf, c = g.counts(), tuple(np.array(a) for a in g.physics_transforms()), g.contacts()
    g.close()
    poses, got_poses = CM.pose_bits(want_xf), CM.pose_bits(got_xf)
    assert got_counts == counts, name
    c = c[c["collider_b"] == T.TERRAIN]
    step = np.zeros(len(c), T.capi.terrain_contact_dtype)
    step["point"] = c["point"]; step["depth"] = c["penetration_depth"]; step["normal"] = c["normal"]; step["volume"] = len(vols) - 1 - c["collider_a"]
    print(f"{name}: {len(vols)} bodies, {len(step)} terrain contacts, {counts['num_contacts']} contacts in all")
    assert len(step) == len(want_recs)
    assert sorted(r.tobytes() for r in step) == sorted(r.tobytes() for r in want_recs)
    if got_poses == poses:
        return
    # A stated deviation (include/mi_physics.h, mi_heightmap_create): in the reference a NaN impulse enters the velocity of the
    # static body that all terrain contacts share (NaN x its zero inverse mass), and every body that touches the terrain leaves the step with a NaN
    # pose; the library keeps the terrain at rest, and the NaN stays with the massless body it came from.  So: a body the GPU gives a NaN pose
    # has one in the oracle's world too, and alone in a world of its own (it is a source, not a victim); and with exactly those bodies parked
    # off the map the oracle has no NaN left and every other pose equals the GPU's, bit for bit.
    nan = np.isnan(got_xf[0]).any(axis=1) | np.isnan(got_xf[1]).any(axis=1)
    assert nan.any() and (np.isnan(want_xf[0]).any(axis=1) | np.isnan(want_xf[1]).any(axis=1))[nan].all(), name
    print(f"{name}: {int(nan.sum())} bodies with a NaN pose on the GPU: {[cases[i]['tag'] for i in np.flatnonzero(nan)]}")
    for i in np.flatnonzero(nan):
        alone = M.step_scene(name, vols[i:i + 1])
        o = alone.populate(oracle_mod.create_world(oracle_mod.ORDER_CANONICAL))
        o.step_fixed(alone.settings(), alone.dt, 1)
        assert np.isnan(o.physics_transforms()[0]).any(), f"{cases[i]['tag']}: a NaN pose on the GPU, a finite one alone in the oracle"
        o.close()
    parked = sc.entities.copy()
    parked["position"][nan] = (500.0, 500.0, 500.0)
    o = replace(sc, entities=parked).populate(oracle_mod.create_world(oracle_mod.ORDER_CANONICAL))
    o.step_fixed(sc.settings(), sc.dt, 1)
    clean = o.physics_transforms()
    o.close()
    assert not np.isnan(clean[0][~nan]).any() and not np.isnan(clean[1][~nan]).any(), name
    for got, want in zip(got_xf, clean):
        assert np.ascontiguousarray(got[~nan]).tobytes() == np.ascontiguousarray(want[~nan]).tobytes(), name


# ---- both instances of the WRITE pass
def test_small_windows_are_equal_at_256_and_257_chunks(mi_lib, oracle_mod):
    tags, vols, (o256, r256, _), (o257, r257, _) = M.shared_expected(oracle_mod)
    assert len(vols) % 2 == 1 or len(vols) > 8
    assert o256.tobytes() == o257.tobytes() and r256.tobytes() == r257.tobytes(), "the oracle's two maps differ"
    got = {}
    for name in ("many256", "many257"):
        w = _query_world(mi_lib, name)
        got[name] = w.terrain_contacts(vols)
        w.close()
    for name, (offsets, recs) in got.items():
        problems = T.differences(offsets, recs, o256, r256)
        assert not problems, f"{name}: " + "\n".join(problems)
    assert got["many256"][1].tobytes() == got["many257"][1].tobytes() and len(r256) > 50
