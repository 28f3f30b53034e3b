"""The contact-manifold matrix (tests/contact_matrix.py) on the GPU, bit for bit against the oracle, which tests/test_contact_matrix.py holds to
the reference's own narrow phase on the same cases.

Query (mi_world_volume_contacts): one world per family with one static collider per item, volume i restricted to entity i; the record set and
every record's bits equal the oracle's, no tolerance, no case left out (an equal-type pair is asked in the orientation the oracle's step took,
or in both when it gave no manifold: the orientation the step did not take then expects what the oracle's narrow phase gives for it, which is
none but for ladder[1244], two cylinders 3.2e-3 deep whose GJK finds the overlap only with the volume as A); accelerated equals exhaustive.

Step (k_narrow, k_narrow_clip, the wave GJK / EPA): the unit-scale families in worlds of at most 512 cases on an 8 x 8 x 8 grid of spacing 8, the
collider static, the volume a dynamic body without gravity; one step on the GPU and on the oracle in canonical order: counts, contacts as a set
and poses, bit for bit (a NaN pose, which the massless body of a degenerate volume gets on both sides, counts as equal to a NaN).  Moving a case changes its low bits, so the coverage conditions are held on the ORACLE's output of the moved worlds."""
import numpy as np
import pytest

import contact_matrix as CM
import overlap_matrix as OM
import query_helpers as Q
from helpers import contact_set
from test_gpu_volume_contacts import RIGID_STATIC, _accel_equals_exhaustive

pytestmark = pytest.mark.gpu


# ---- the query
@pytest.mark.parametrize("name", CM.FAMILIES)
def test_query_matrix_matches_oracle(mi_lib, oracle_mod, name):
    cases, manifolds = CM.family(name), CM.oracle_manifolds(oracle_mod, name)
    items = CM.query_items(cases, manifolds, CM.oracle_orientations(oracle_mod, name))
    n = len(items)
    w = Q.world(mi_lib, OM.scene_of(items, f"contact matrix {name}"))
    pick = list(range(n)) + ([0] if n % 2 == 0 else [])     # (an odd batch: never a multiple of the volumes per workgroup)
    vols = np.concatenate([items[i]["volume"] for i in pick])
    ranges = np.array([(i, i + 1) for i in pick], np.uint32)
    offsets, recs = _accel_equals_exhaustive(w, vols, RIGID_STATIC, ranges, what=f"contact matrix {name}")   # (applies _check_result)
    w.close()
    got = {}
    for r in recs:
        got.setdefault(int(r["volume"]), []).append(r)
    problems = []
    for slot, i in enumerate(pick):
        it, mine = items[i], got.get(slot, [])
        c = cases[it["case"]]
        who = f"{name}[{it['case']}] {CM.TYPES[c['vt']]} -> {CM.TYPES[c['ct']]} {c['tag']}"
        e = it["expect"]
        if e is None:
            if mine:
                problems.append(f"{who}: {len(mine)} records, the oracle has no manifold")
            continue
        if len(mine) != 1:
            problems.append(f"{who}: {len(mine)} records, the oracle has a manifold of {len(e['points'])}")
            continue
        r = mine[0]
        k = len(e["points"])
        want_points = np.zeros((4, 4), np.float32); want_points[:k] = e["points"]
        same = (int(r["count_flags"]) == (k | (256 if e["volume_is_b"] else 0)) and int(r["entity"]) == i and int(r["collider"]) == n - 1 - i and int(r["object_type"]) == 1
                and r["normal"].tobytes() == e["normal"].tobytes() and r["points"].tobytes() == want_points.tobytes())
        if not same:
            problems.append(f"{who}: got flags {int(r['count_flags']):#x} entity {int(r['entity'])} collider {int(r['collider'])} normal {r['normal']} points "
                            f"{r['points'][:max(int(r['count_flags']) & 7, 1)]}; oracle B={e['volume_is_b']} normal {e['normal']} points {e['points']}")
    hits = sum(it["expect"] is not None for it in items)
    print(f"{name}: {len(cases)} cases, {n} items ({hits} with a manifold, {n - len(cases)} second orientations), {len(recs)} records, {len(problems)} differences")
    assert not problems, f"{len(problems)} differences:\n" + "\n".join(problems[:12])


# ---- the step
STEP_RUNS = [(name, "speculative") for name in CM.UNIT_FAMILIES] + [("features", "synchronous")]


@pytest.mark.parametrize("name,stepping", STEP_RUNS)
def test_step_matrix_matches_oracle(mi_lib, oracle_mod, monkeypatch, name, stepping):
    if stepping == "synchronous":
        monkeypatch.setenv("MI_ASYNC", "0")
    worlds, _, _ = CM.oracle_steps(oracle_mod, name)   # (holds the cap on the moved worlds)
    for sc, counts, cset, poses in worlds:
        g = sc.populate(mi_lib.create_world(0))
        g.step_fixed(sc.settings(), sc.dt, 1)
        assert g.counts() == counts, sc.name
        assert contact_set(g.contacts()) == cset, sc.name
        assert CM.pose_bits(g.physics_transforms()) == poses, sc.name
        g.close()
    print(f"{name} {stepping}: {len(worlds)} worlds, {sum(len(s.entities) // 2 for s, *_ in worlds)} cases, {sum(c['num_collisions'] for _, c, *_ in worlds)} manifolds")
