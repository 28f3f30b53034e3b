"""The yardstick of the contact-manifold scene query, from the oracle alone (no GPU): the scenes and volume sets that
tests/test_gpu_volume_contacts.py compares bit for bit cover every pair of world types, and the equal-type pairs whose orientation the
step and the query choose differently ("reversed", tests/contact_ref.py) are a small share.  Also the record layout of the binding."""
import itertools

import pytest

import contact_ref as CR
import overlap_ref as R

SCENES = ("shape_zoo", "zones")


@pytest.fixture(scope="module")
def start_state(oracle_mod):
    out = {}
    for name in SCENES:
        sc = R.query_scene(name)
        vols = CR.contact_volume_set(name, False, sc, *CR.start_poses(sc))
        out[name] = (sc, vols, CR.oracle_manifolds(oracle_mod, sc, vols))
    return out


def test_every_type_pair_is_covered(start_state):
    total = {}
    for name in SCENES:
        sc, vols, (expected, reversed_pairs, info) = start_state[name]
        print(f"{name}: {len(vols)} volumes, {len(expected)} compared manifolds, {info['reversed_manifolds']} reversed of {info['equal_type_manifolds']} of equal type, "
              f"sweep axis {info['axis']}; per type pair {sorted(info['per_pair'].items())}")
        for key, n in info["per_pair"].items():
            total[key] = total.get(key, 0) + n
    pairs = list(itertools.combinations_with_replacement(range(6), 2))
    assert len(pairs) == 21
    thin = {p: total.get(p, 0) for p in pairs if total.get(p, 0) < 10}
    assert not thin, f"world type pairs with fewer than 10 non-reversed manifolds over both scenes: {thin}"


@pytest.mark.parametrize("name", SCENES)
def test_reversed_pairs_are_a_small_share(start_state, name):
    _, _, (expected, reversed_pairs, info) = start_state[name]
    assert info["equal_type_manifolds"] > 50
    assert info["reversed_manifolds"] <= 0.25 * info["equal_type_manifolds"], info
    assert not set(expected) & reversed_pairs


def test_record_layout():
    from d3d12renderer_amd import capi
    d = capi.volume_contact_dtype
    assert d.itemsize == 96
    assert [d.fields[n][1] for n in ("entity", "collider", "object_type", "volume", "normal", "count_flags", "points")] == [0, 4, 8, 12, 16, 28, 32]
    assert d["points"].shape == (4, 4)
