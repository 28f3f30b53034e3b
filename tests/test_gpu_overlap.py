"""Volume-overlap scene queries on the GPU (mi_world_overlap, mi_world_overlap_device_async, mi_debug_overlap_exhaustive): against the
reference's own trigger path (shrunk and grown volumes in oracle worlds), against the numpy gaps of tests/overlap_ref.py, the
accelerated grid walk against the exhaustive scan byte for byte, the capacity protocol, the device variant, the cache's invalidation,
that queries change nothing a step computes, and the pair-level matrix of tests/overlap_matrix.py: every decision against a verified
float64 certificate, the zero-displacement shape cast, and the same cases as triggers in a step (which keep the reference's bits)."""
import ctypes as C

import numpy as np
import pytest

import overlap_exact as E
import overlap_matrix as OM
import overlap_ref as R
import query_helpers as Q

pytestmark = pytest.mark.gpu

RIGID, ALL = 1, 31
SORT_BOUND = 1024   # kOvSortMax: the longest segment a wave sorts in LDS


def _accel_equals_exhaustive(w, vols, include, ranges=None, what=""):
    return Q.accel_equals_exhaustive(w.overlap, w.debug_overlap_exhaustive, Q.check_csr, vols, include, ranges, what)


# ---- 1. against the reference's trigger path
@pytest.mark.parametrize("name", ["shape_zoo", "zones"])
@pytest.mark.parametrize("settled", [False, True])
def test_sandwiched_by_the_reference_trigger_path(mi_lib, oracle_mod, name, settled):
    """shrunk-oracle <= query <= grown-oracle per volume, as entity sets, with no budget: wherever the reference's answer does not depend
    on a relative 1e-3 of the volume's size, the query gives exactly it - except where a VERIFIED float64 certificate (tests/overlap_exact.py)
    contradicts the reference: there the query must give the certificate's answer, and the pair must be of a class the header names (a
    cylinder or a hull in the pair, or a capsule against a box)."""
    sc = R.query_scene(name)
    w = Q.world(mi_lib, sc, 300 if settled else 0)
    vols = R.volume_set(name, settled)
    ents = Q.bodies(sc)
    states = (ents, w.get_body_states(ents)) if settled else None
    shrunk, grown, (subset, both, ambiguous) = R.oracle_sandwich(oracle_mod, sc, vols, states)
    offsets, hits = w.overlap(vols, include=RIGID)
    Q.check_csr(offsets, hits, len(vols))
    assert (hits["object_type"] == 0).all()
    got = R.entity_sets(offsets, hits, len(vols))
    print(f"{name} settled={settled}: {sum(map(len, shrunk))} shrunk / {sum(map(len, got))} query / {sum(map(len, grown))} grown; both non-empty {both:.0%}, ambiguous {ambiguous:.2%}")
    assert subset and sum(map(len, shrunk)) > 100
    assert both > 0.5 and ambiguous <= 0.02   # the yardstick's own validity for THIS set (a condition on the inputs: seeds and boxes in overlap_ref)
    # where the query leaves the sandwich: the certificates of the volume against every collider of the entity, at the poses the query read
    shapes = R.scene_world_shapes(sc, *w.physics_transforms())
    nc = len(sc.colliders)
    of_entity = {}
    for k, (ent, obj, ws) in enumerate(shapes):
        c = sc.colliders[nc - 1 - k]
        of_entity.setdefault(ent, []).append(E.with_hull(ws, sc.hulls[int(c["hull_geometry"])] if ws[0] == R.HULL else None))
    contradicted, undecided = [], []

    def certificate_overrules(v, ent, query_reports):
        vs = E.with_hull(R.volume_world_shape(vols[v]), sc.hulls[int(vols[v]["hull_geometry"])] if int(vols[v]["type"]) == R.HULL else None)
        verdicts = [(cs[0], *E.certify(vs, cs)) for cs in of_entity[ent]]
        overlapping = any(d is True for _, d, _ in verdicts)
        decided = overlapping or all(d is False for _, d, _ in verdicts)
        if not decided or overlapping != query_reports:
            undecided.append((v, ent, "no certificate verified" if not decided else "the certificate sides with the reference"))
            return False    # no certificate against the reference here (or one against the query): the sandwich stands
        quirk = [t for t, d, _ in verdicts if (d is True) == overlapping and ({R.CYLINDER, R.HULL} & {t, vs[0]} or {t, vs[0]} in ({R.CAPSULE, R.AABB}, {R.CAPSULE, R.OBB}))]
        assert quirk, f"volume {v} (type {vs[0]}) and entity {ent}: the certificate contradicts the reference on a pair of no class the header names: {verdicts}"
        contradicted.append((v, ent, "overlapping" if overlapping else "apart", min(c for _, d, c in verdicts if (d is True) == overlapping)))
        return True

    missing = [(v, sorted(e for e in shrunk[v] - got[v] if not certificate_overrules(v, e, False))) for v in range(len(vols)) if not shrunk[v] <= got[v]]
    extra = [(v, sorted(e for e in got[v] - grown[v] if not certificate_overrules(v, e, True))) for v in range(len(vols)) if not got[v] <= grown[v]]
    missing, extra = [m for m in missing if m[1]], [x for x in extra if x[1]]
    print(f"{name} settled={settled}: {len(contradicted)} (volume, entity) pairs where a verified certificate contradicts the reference and the query follows the certificate: {contradicted[:8]}; "
          f"{len(undecided)} pairs outside the sandwich that no certificate excuses (they fail below): {undecided[:8]}")
    assert not missing, f"the reference reports these even for the shrunk volume (volume, entities; types {[int(vols['type'][v]) for v, _ in missing[:6]]}): {missing[:6]}"
    assert not extra, f"the reference reports none of these even for the grown volume (volume, entities; types {[int(vols['type'][v]) for v, _ in extra[:6]]}): {extra[:6]}"
    w.close()


# ---- 2. against the numpy reference
@pytest.mark.parametrize("name", ["shape_zoo", "zones"])
def test_closed_form_pairs_match_numpy_gaps(mi_lib, name):
    sc = R.query_scene(name)
    w = Q.world(mi_lib, sc, 40)
    vols = np.concatenate([R.volume_set(name, False, per_type=24), R.volume_set(name, True, per_type=8)])
    offsets, hits = w.overlap(vols, include=ALL)
    Q.check_csr(offsets, hits, len(vols))
    shapes = R.scene_world_shapes(sc, *w.physics_transforms())
    compared = skipped = overlapping = 0
    wrong = []
    for v in range(len(vols)):
        reported = set(int(k) for k in hits["collider"][offsets[v]:offsets[v + 1]])
        vs = R.volume_world_shape(vols[v])
        for k, (ent, obj, ks) in enumerate(shapes):
            gap = R.signed_gap(vs, ks)
            if gap is None:
                continue
            if abs(gap) <= 1e-4:
                skipped += 1
                continue
            compared += 1
            overlapping += gap < 0
            if (k in reported) != (gap < 0):
                wrong.append((v, k, float(gap)))
    for rec in hits[:: max(1, len(hits) // 64)]:   # the records' other columns
        ent, obj, _ = shapes[int(rec["collider"])]
        assert rec["entity"] == ent and rec["object_type"] == obj
    print(f"{name}: {compared} pairs compared ({overlapping} overlapping), {skipped} within 1e-4 not compared")
    assert not wrong, f"(volume, collider, gap): {wrong[:8]}"
    assert overlapping > 200 and skipped < 0.01 * (compared + skipped)
    if name == "zones":   # statics, triggers and force fields are reported under include = ALL
        assert {1, 2, 3} <= set(int(t) for t in hits["object_type"])
    w.close()


# ---- 3. accelerated equals exhaustive
def test_accelerated_equals_exhaustive(mi_lib):
    from d3d12renderer_amd import capi, scenes
    rng = np.random.default_rng(15)
    cases = [(R.query_scene("shape_zoo"), 30, (-7, -1, -7), (7, 8, 7), True),
             (scenes.obb_pile(128, 4, 128), 60, (-100, -1, -100), (100, 8, 100), False),
             (scenes.terrain_field(), 30, (-18, -1, -18), (18, 10, 18), False)]
    for sc, steps, lo, hi, hull_ok in cases:
        w = Q.world(mi_lib, sc, steps)
        vols, n_bad = Q.edge_volumes(rng, lo, hi, hull_ok, (40, 8, 4), 16, 0)
        offsets, hits = _accel_equals_exhaustive(w, vols, ALL, what=sc.name)
        counts = np.diff(offsets.astype(np.int64))
        assert (counts[-n_bad:] == 0).all(), f"{sc.name}: an invalid volume reported something"
        assert (counts == 0).any() and (counts > 0).any() and counts.max() > 0.5 * len(sc.colliders), sc.name   # (the giant sphere)
        if len(sc.colliders) > 10000:
            assert (counts > SORT_BOUND).any(), sc.name
        n_ent = len(sc.entities)
        lo_e = rng.integers(0, n_ent, len(vols)).astype(np.uint32)
        ranges = np.stack([lo_e, np.minimum(lo_e + rng.integers(1, max(2, n_ent // 4), len(vols)), n_ent)], axis=1).astype(np.uint32)
        ranges[::5] = (0, 0xFFFFFFFF)
        ro, rh = _accel_equals_exhaustive(w, vols, ALL, ranges, what=f"{sc.name} ranges")
        per_hit = ranges[rh["volume"]]
        assert ((rh["entity"] >= per_hit[:, 0]) & (rh["entity"] < per_hit[:, 1])).all(), sc.name
        sub = vols[:: max(1, len(vols) // 96)]
        for include in range(32):
            mo, mh = _accel_equals_exhaustive(w, sub, include, what=f"{sc.name} include {include}")
            flags = np.array([2 ** 0, 2 ** 1, 2 ** 4, 2 ** 3])[mh["object_type"]] if len(mh) else np.zeros(0, int)
            assert ((flags & include) != 0).all(), (sc.name, include)
            if include in (0, 4):   # nothing selected; the terrain is accepted and ignored
                assert len(mh) == 0
        w.close()
    # segments beyond the LDS sort bound out of a walk over few cells
    sc = Q.dense_cluster()
    w = Q.world(mi_lib, sc)
    vols = np.concatenate([capi.box_volume((0.5, 1.0, 0.5), (0.6, 0.6, 0.6)), capi.sphere_volume((0.5, 1.0, 0.5), 0.45), capi.sphere_volume((0.2, 0.8, 0.3), 0.3),
                           capi.box_volume((0.5, 1.0, 0.5), (0.7, 0.7, 0.7), rotation=(0.0, 0.38268343, 0.0, 0.92387953)), capi.sphere_volume((12.0, 1.0, 0.0), 0.2),
                           R.make_volumes(5, 6, (0, 0.5, 0), (1, 1.5, 1), 0.05, 0.5)])
    offsets, hits = _accel_equals_exhaustive(w, vols, ALL, what="dense cluster")
    counts = np.diff(offsets.astype(np.int64))
    assert counts[0] == 3000 and counts[1] > SORT_BOUND and 0 < counts[2] <= SORT_BOUND and counts[4] == 1, counts[:5]
    w.close()


# ---- 4. capacity protocol
def test_capacity_protocol(mi_lib):
    from d3d12renderer_amd import capi
    import torch
    sc = R.query_scene("shape_zoo")
    w = Q.world(mi_lib, sc, 20)
    vols = R.volume_set("shape_zoo", False)
    offsets, hits = w.overlap(vols, include=ALL)
    total = len(hits)
    assert total > 50
    rc, o, h, t = w.overlap_raw(vols, ALL, None, 0)                       # count only
    assert rc == 0 and t == total and o.tobytes() == offsets.tobytes()
    rc, o, h, t = w.overlap_raw(vols, ALL, None, total)                   # exact capacity
    assert rc == 0 and t == total and o.tobytes() == offsets.tobytes() and h.tobytes() == hits.tobytes()
    for name in ("world_overlap", "debug_overlap_exhaustive"):
        for cap in (total - 1, total // 2, 1):                            # short: the prefix, full offsets and total
            rc, o, h, t = w.overlap_raw(vols, ALL, None, cap, name=name)
            assert rc == capi.MI_ERR_CAPACITY == -5 and t == total and o.tobytes() == offsets.tobytes(), (name, cap)
            assert h.tobytes() == hits[:cap].tobytes(), (name, cap)
    # the device variant writes nothing at or past `capacity`
    vols_d = torch.tensor(np.frombuffer(vols.tobytes(), np.uint8).copy(), device="cuda")
    off_d = torch.zeros(len(vols) + 1, dtype=torch.int32, device="cuda"); tot_d = torch.zeros(1, dtype=torch.int32, device="cuda")
    for cap in (total // 3, total - 1, total, 0):
        buf = torch.full(((cap + 64) * 16,), 0xAB, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        w.overlap_device_async(len(vols), vols_d.data_ptr(), off_d.data_ptr(), buf.data_ptr(), cap, tot_d.data_ptr(), include=ALL)
        w.overlap(vols[:1], include=0)   # (a blocking call: synchronises the world's stream)
        out = buf.cpu().numpy()
        assert (out[cap * 16:] == 0xAB).all(), cap
        assert out[: cap * 16].tobytes() == hits[:cap].tobytes(), cap
        assert int(tot_d.cpu()[0]) == total and off_d.cpu().numpy().view(np.uint32).tobytes() == offsets.tobytes(), cap
    w.close()


# ---- 5. device variant
def test_device_variant_equals_host_variant(mi_lib):
    import torch
    sc = R.query_scene("shape_zoo")
    w = Q.world(mi_lib, sc, 10)
    rng = np.random.default_rng(4)
    vols = np.concatenate([R.volume_set("shape_zoo", False), R.volume_set("shape_zoo", True)])
    cap = 16384
    vols_d = torch.tensor(np.frombuffer(vols.tobytes(), np.uint8).copy(), device="cuda")
    off_d = torch.zeros(len(vols) + 1, dtype=torch.int32, device="cuda"); tot_d = torch.zeros(1, dtype=torch.int32, device="cuda")
    hits_d = torch.zeros(cap * 16, dtype=torch.uint8, device="cuda")
    lo_e = rng.integers(0, len(sc.entities), len(vols)).astype(np.uint32)
    ranges = np.stack([lo_e, lo_e + 60], axis=1).astype(np.uint32)
    ranges_d = torch.tensor(ranges.view(np.int32), device="cuda")
    torch.cuda.synchronize()

    def device_result():
        total = int(tot_d.cpu()[0])
        return off_d.cpu().numpy().view(np.uint32).tobytes(), hits_d.cpu().numpy()[: total * 16].tobytes()

    previous = None
    for _ in range(2):
        w.step_fixed(sc.settings(), sc.dt, 1)
        w.overlap_device_async(len(vols), vols_d.data_ptr(), off_d.data_ptr(), hits_d.data_ptr(), cap, tot_d.data_ptr(), include=ALL)   # right behind the step
        offsets, hits = w.overlap(vols, include=ALL)                                                                                # (synchronises that stream)
        dev = device_result()
        assert len(hits) <= cap and dev == (offsets.tobytes(), hits.tobytes())
        assert previous is None or dev != previous
        previous = dev
        w.overlap_device_async(len(vols), vols_d.data_ptr(), off_d.data_ptr(), hits_d.data_ptr(), cap, tot_d.data_ptr(), include=RIGID, ranges_ptr=ranges_d.data_ptr())
        offsets, hits = w.overlap(vols, include=RIGID, entity_ranges=ranges)
        assert device_result() == (offsets.tobytes(), hits.tobytes())
        w.step_fixed(sc.settings(), sc.dt, 20)
    w.close()


# ---- 6. the cache
def test_cache_follows_every_change(mi_lib):
    from d3d12renderer_amd import capi, scenes
    import torch
    sc = scenes.shape_zoo(3, 2, 3)
    w = Q.world(mi_lib, sc, 5)
    vols = np.concatenate([R.make_volumes(9, 16, (-4, 0, -4), (4, 5, 4), 0.2, 3.0),
                           R.make_volumes(10, 2, (-45, 0, -45), (45, 6, 45), 1.0, 4.0)])
    rng = np.random.default_rng(2)
    ro = rng.uniform((-4, -1, -4), (4, 6, 4), (512, 3)).astype(np.float32)
    rd = rng.normal(size=(512, 3)); rd = (rd / np.linalg.norm(rd, axis=1, keepdims=True)).astype(np.float32)

    def check(what):
        return _accel_equals_exhaustive(w, vols, ALL, what=what)

    def around(p, r=0.5):
        o, h = w.overlap(capi.sphere_volume(p, r), include=ALL)
        return set(int(e) for e in h["entity"])

    check("start")
    w.step_fixed(sc.settings(), sc.dt, 1); check("step")
    st = w.get_body_states([3]); st[0, :3] = (40.0, 3.0, -35.0); w.set_body_states([3], st)      # host write: far from the grid the last query built
    assert around((40.0, 3.0, -35.0)) == {3}; check("set_body_states")
    body = w.entities_to_bodies([4])
    st = w.get_body_states([4]); st[0, :3] = (-30.0, 2.0, 33.0)
    ids = torch.tensor(body.astype(np.int32), device="cuda"); sd = torch.tensor(st, device="cuda")
    torch.cuda.synchronize()
    w.set_body_states_device_async(1, ids.data_ptr(), sd.data_ptr())                            # device write on the world's stream
    assert around((-30.0, 2.0, 33.0)) == {4}; check("set_body_states_device_async")
    blob = w.save_checkpoint()
    before = w.overlap(vols, include=ALL)
    w.step_fixed(sc.settings(), sc.dt, 10)
    after = check("steps")
    assert after[1].tobytes() != before[1].tobytes()
    w.load_checkpoint(blob)
    again = w.overlap(vols, include=ALL)
    assert again[0].tobytes() == before[0].tobytes() and again[1].tobytes() == before[1].tobytes(); check("load_checkpoint")
    w.destroy_entity(3)
    assert around((40.0, 3.0, -35.0)) == set(); check("destroy")
    e = w.create_entities(scenes.make_entities(1, capi.ENTITY_STATIC))
    c = scenes.make_colliders(1, capi.SPHERE); c["shape"][0, :4] = (25.0, 4.0, 25.0, 1.0)
    w.add_colliders([e], c)
    o, h = w.overlap(capi.sphere_volume((25.0, 5.2, 25.0), 0.3), include=ALL)
    assert len(h) == 1 and h["entity"][0] == e and h["object_type"][0] == 1; check("collider add")
    # rays and volumes interleaved in one pose epoch share one build
    w.step_fixed(sc.settings(), sc.dt, 1)
    for i in range(3):
        a = w.raycast(ro, rd, include=ALL); check(f"interleaved {i}")
        assert a.tobytes() == w.debug_raycast_exhaustive(ro, rd, include=ALL).tobytes()
        assert a.tobytes() == w.raycast(ro, rd, include=ALL).tobytes()
    w.close()


# ---- 7. queries change nothing
def test_queries_change_nothing(mi_lib):
    sc = R.query_scene("shape_zoo")
    a = Q.world(mi_lib, sc); b = Q.world(mi_lib, sc)
    vols = np.concatenate([R.volume_set("shape_zoo", False), R.volume_set("shape_zoo", True)])
    s = sc.settings()
    ents = Q.bodies(sc)
    for i in range(100):
        a.step_fixed(s, sc.dt, 1); b.step_fixed(s, sc.dt, 1)
        b.overlap(vols, include=ALL)
        if i % 10 == 0:
            b.debug_overlap_exhaustive(vols, include=RIGID)
    assert a.get_body_states(ents).tobytes() == b.get_body_states(ents).tobytes()
    assert a.debug_step_ahead_stats() == b.debug_step_ahead_stats()
    a.close(); b.close()


# ---- 8. the pair-level matrix: every volume type against every collider type, one collider at a time (tests/overlap_matrix.py)
def _matrix_query(mi_lib, name):
    """One world per family, one static entity with one collider per case (kept and sub-bound alike); volume i is restricted to entity i.
    The batch is made odd (never a multiple of the volumes per workgroup) by a repeat of the first volume.  Returns (world, cases, volumes,
    ranges, per case whether the query reports its collider)."""
    cases = OM.family(name)
    w = Q.world(mi_lib, OM.scene_of(cases, f"overlap matrix {name}"))
    pick = list(range(len(cases))) + ([0] if len(cases) % 2 == 0 else [])
    vols = np.concatenate([cases[i]["volume"] for i in pick])
    ranges = np.array([(i, i + 1) for i in pick], np.uint32)
    offsets, hits = _accel_equals_exhaustive(w, vols, ALL, ranges, what=f"matrix {name}")
    sizes = np.diff(offsets.astype(np.int64))
    assert (sizes <= 1).all() and (hits["entity"] == ranges[hits["volume"], 0]).all() and (hits["object_type"] == 1).all()
    assert len(pick) == len(cases) or sizes[-1] == sizes[0]
    return w, cases, vols, ranges, sizes[:len(cases)] == 1


def _who(name, i, c):
    return (f"{name}[{i}] {OM.TYPES[c['vt']]} -> {OM.TYPES[c['ct']]} {c['tag']}: {'overlapping' if c['expected'] else 'apart'} by {c['cert']:.3e} "
            f"= {c['cert'] / c['scale']:.3e} scale (scale {c['scale']:.3g})")


def _report_wrong(name, cases, got, what):
    """Prints what the family measures (the largest certificate per unit of scale of a wrong decision, over all its cases and per pair) and
    returns the wrong decisions among the KEPT cases."""
    wrong = [i for i, c in enumerate(cases) if bool(got[i]) != c["expected"]]
    rel = {i: cases[i]["cert"] / cases[i]["scale"] for i in wrong}
    per_pair = {}
    for i in wrong:
        key = (OM.TYPES[cases[i]["vt"]], OM.TYPES[cases[i]["ct"]], "overlapping" if cases[i]["expected"] else "apart")
        per_pair[key] = max(per_pair.get(key, 0.0), rel[i])
    kept = sum(OM.is_kept(c) for c in cases)
    print(f"{what} {name}: {len(cases)} certified cases ({kept} kept at the bound {OM.BOUNDS[name]:.0e}), {len(wrong)} decided wrongly; the largest certificate of a wrong "
          f"decision per unit of scale: {max(rel.values(), default=0.0):.3e}; smallest certificate of the family {min(c['cert'] / c['scale'] for c in cases):.3e}")
    for key, v in sorted(per_pair.items(), key=lambda kv: -kv[1])[:12]:
        print(f"    {key[0]} -> {key[1]}, {key[2]}: wrong up to {v:.3e} scale")
    closed = [rel[i] for i in wrong if R.signed_gap(cases[i]["vs"], cases[i]["cs"]) is not None or {cases[i]["vt"], cases[i]["ct"]} <= {R.AABB, R.OBB}]
    print(f"    the reference's closed forms (spheres, capsules, sphere-box, box-box) among them: {len(closed)}, wrong up to {max(closed, default=0.0):.3e} scale; "
          f"overlapping cases reported apart: {sum(cases[i]['expected'] for i in wrong)}")
    return [i for i in wrong if OM.is_kept(cases[i])]


@pytest.mark.parametrize("name", OM.FAMILIES)
def test_matrix_decisions(mi_lib, name):
    """The query's decision equals the verified float64 certificate's in every kept case (certificate >= 4 x the family's bound x scale); the
    sub-bound cases are decided too and only printed: they measure the resolution (overlap_matrix.MEASURED)."""
    w, cases, vols, ranges, got = _matrix_query(mi_lib, name)
    w.close()
    bad = _report_wrong(name, cases, got, "overlap")
    one_sided = OM.one_sided(name)   # (size_ratio: overlapping cases below the family's bound, held never to be reported apart)
    index = {id(c): i for i, c in enumerate(cases)}
    bad += [index[id(c)] for c in one_sided if not got[index[id(c)]]]
    print(f"{name}: {len(one_sided)} overlapping cases under the one-sided bound {OM.ONE_SIDED_BOUND:.0e}")
    assert not bad, f"{len(bad)} kept cases decided wrongly:\n" + "\n".join(_who(name, i, cases[i]) + f": the query says {'overlapping' if got[i] else 'apart'}" for i in bad[:40])


@pytest.mark.parametrize("name", OM.FAMILIES)
def test_matrix_accelerated_equals_exhaustive(mi_lib, name):
    """Every case of the family, sub-bound ones included: the grid walk and the exhaustive scan give the same bytes, with and without the
    entity ranges (without them every volume meets every collider of the family)."""
    w, cases, vols, ranges, got = _matrix_query(mi_lib, name)
    sub = vols[:: max(1, len(vols) // 64)]
    offsets, hits = _accel_equals_exhaustive(w, sub, ALL, what=f"matrix {name}, no ranges")
    assert len(hits) > 0
    w.close()


@pytest.mark.parametrize("name", OM.FAMILIES)
def test_matrix_zero_displacement_sweep_agrees(mi_lib, name):
    """mi_world_sweep with a zero displacement: its initial-overlap verdict is the overlap query's, on every kept case of the family (the
    sub-bound ones are counted and printed)."""
    w, cases, vols, ranges, got = _matrix_query(mi_lib, name)
    recs = w.sweep(vols, np.zeros((len(vols), 3), np.float32), ALL, ranges)[:len(cases)]
    w.close()
    hit = recs["entity"] != 0xFFFFFFFF
    assert (recs["flags"][hit] & 1).all() and (recs["t"][hit] == 0).all(), "a zero displacement hit something it did not start in"
    # the pair test never ran out of iterations on a kept case: "overlapping" there is a search that ended, not one that gave up
    gave_up = [i for i in range(len(cases)) if hit[i] and recs["flags"][i] & 2]
    print(f"{name}: {len(gave_up)} cases end with the sweep's unconverged flag,{sum(OM.is_kept(cases[i]) for i in gave_up)} of them kept: {[_who(name, i, cases[i]) for i in gave_up[:6]]}")
    assert not [i for i in gave_up if OM.is_kept(cases[i])]
    bad = _report_wrong(name, cases, hit, "zero-displacement sweep")
    differ = [i for i in range(len(cases)) if bool(hit[i]) != bool(got[i])]
    print(f"{name}: sweep and overlap differ on {len(differ)} cases, {sum(OM.is_kept(cases[i]) for i in differ)} of them kept")
    assert not bad, f"{len(bad)} kept cases:\n" + "\n".join(_who(name, i, cases[i]) for i in bad[:40])
    assert not [i for i in differ if OM.is_kept(cases[i])]


def test_matrix_triggers_in_the_step_keep_the_reference_bits(mi_lib, oracle_mod):
    """The cylinder_caps cases and the small cases of `size` as trigger entities over rigid bodies, one step: the step's TRIGGER_ENTER events are
    the oracle's, pair for pair: the query's corrected predicate did not reach k_overlap.  The world holds cases that the reference decides
    against their certificate, so the two predicates do differ on it."""
    cases = OM.trigger_cases()
    n = len(cases)
    sc = OM.trigger_scene(cases)
    o = sc.populate(oracle_mod.create_world(oracle_mod.ORDER_REFERENCE))
    want = OM.trigger_enters(o, sc, n)
    o.close()
    w = Q.world(mi_lib, sc)
    vols = np.concatenate([c["volume"] for c in cases])
    _, hits = w.overlap(vols, include=RIGID, entity_ranges=np.array([(i, i + 1) for i in range(n)], np.uint32))
    query = set(int(v) for v in hits["volume"])
    got = OM.trigger_enters(w, sc, n)
    w.close()
    own = {a for a, b in want if a == b}
    quirks = [i for i, c in enumerate(cases) if OM.is_kept(c) and (i in own) != c["expected"]]
    print(f"{n} cases: {len(want)} trigger events in the oracle, {len(got)} on the GPU; the reference decides {len(quirks)} kept cases against their certificate; "
          f"the query differs from the step on {len(query ^ own)} cases")
    assert got == want, f"only the GPU: {sorted(got - want)[:8]}; only the oracle: {sorted(want - got)[:8]}"
    assert len(quirks) >= 10 and all((i in query) == cases[i]["expected"] for i in quirks)


# ---- 9. errors
def test_errors(mi_lib):
    from d3d12renderer_amd import capi, scenes, sharding
    sc = scenes.shape_zoo(2, 1, 2)
    w = Q.world(mi_lib, sc)
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    vol = capi.sphere_volume((0, 1, 0), 5.0); off = np.zeros(2, np.uint32); hits = np.zeros(64, capi.overlap_hit_dtype); total = C.c_uint32(7)
    u = C.c_uint32
    for name in ("world_overlap", "debug_overlap_exhaustive"):
        f = w.L.fn(name)
        assert f(None, u(1), p(vol), u(ALL), None, p(off), p(hits), u(64), C.byref(total)) == -1
        assert f(w.h, u(1), None, u(ALL), None, p(off), p(hits), u(64), C.byref(total)) == -1
        assert f(w.h, u(1), p(vol), u(ALL), None, None, p(hits), u(64), C.byref(total)) == -1
        assert f(w.h, u(1), p(vol), u(ALL), None, p(off), None, u(64), C.byref(total)) == -1
        assert f(w.h, u(1), p(vol), u(ALL), None, p(off), p(hits), u(64), None) == -1
        assert f(w.h, u(0), None, u(ALL), None, None, None, u(0), None) == 0
        assert f(w.h, u(0), None, u(ALL), None, p(off), None, u(0), C.byref(total)) == 0 and total.value == 0 and off[0] == 0
        assert f(w.h, u(1), p(vol), u(ALL), None, p(off), p(hits), u(64), C.byref(total)) == 0 and total.value == off[1] >= 4
    d = w.L.fn("world_overlap_device_async")
    assert d(w.h, u(1), None, u(ALL), None, None, None, u(0), None) == -1
    assert d(None, u(1), None, u(ALL), None, None, None, u(0), None) == -1
    assert d(w.h, u(0), None, u(ALL), None, None, None, u(0), None) == 0
    o, h = w.overlap(np.zeros(0, capi.query_volume_dtype))
    assert len(o) == 1 and o[0] == 0 and len(h) == 0
    w.close()
    w = Q.world(mi_lib, sc)
    w.shard_enable(sharding._desc_for(sharding.tile_grid(sc, 1), 0))
    for name in ("world_overlap", "debug_overlap_exhaustive"):
        assert w.L.fn(name)(w.h, u(1), p(vol), u(ALL), None, p(off), p(hits), u(64), C.byref(total)) == -6
    w.close()
