"""Volume-overlap scene queries without a GPU: the ABI (header, exports, record sizes), the numpy reference the GPU tests compare
against, and the validity of the trigger yardstick (the reference's own trigger path on shrunk and grown volumes) for the very volume
sets the GPU tests use."""
import re
from pathlib import Path

import numpy as np
import pytest

import overlap_ref as R
from overlap_ref import AABB, CAPSULE, CYLINDER, HULL, OBB, SPHERE

ROOT = Path(__file__).resolve().parent.parent
OVERLAP_SYMBOLS = ("mi_world_overlap", "mi_world_overlap_device_async", "mi_debug_overlap_exhaustive")


def test_header_declares_and_library_exports_the_overlap_api(mi_lib):
    text = (ROOT / "include" / "mi_physics.h").read_text()
    declared = set(re.findall(r"MI_API\s+[\w\s\*]+?\b(mi_\w+)\s*\(", text))
    for name in OVERLAP_SYMBOLS:
        assert name in declared, name
    L = mi_lib.library()
    missing = [n for n in OVERLAP_SYMBOLS if not hasattr(L.lib, n)]
    assert not missing, missing
    from d3d12renderer_amd import capi
    assert capi.query_volume_dtype.itemsize == 96 and capi.overlap_hit_dtype.itemsize == 16
    assert capi.query_volume_dtype.fields["position"][1] == 56 and capi.query_volume_dtype.fields["rotation"][1] == 72
    assert "} mi_query_volume;" in text and "} mi_overlap_hit;" in text
    assert re.search(r"uint32_t type; uint32_t hull_geometry; float shape\[12\];\s*float position\[3\]; float pad0; float rotation\[4\]; float pad1\[2\];", text)
    assert "typedef struct mi_overlap_hit { uint32_t entity, collider, object_type, volume; } mi_overlap_hit;" in text


def test_volume_helpers():
    from d3d12renderer_amd import capi
    v = capi.sphere_volume((1, 2, 3), 0.5)[0]
    assert v["type"] == SPHERE and tuple(v["shape"][:4]) == (1, 2, 3, 0.5) and tuple(v["rotation"]) == (0, 0, 0, 1)
    v = capi.box_volume((1, 2, 3), (1, 1, 2))[0]
    assert v["type"] == AABB and tuple(v["shape"][:6]) == (0, 1, 1, 2, 3, 5)
    v = capi.box_volume((1, 2, 3), (1, 1, 2), rotation=(0, 0, 0, 1))[0]
    assert v["type"] == OBB and tuple(v["shape"][:10]) == (0, 0, 0, 1, 1, 2, 3, 1, 1, 2)
    assert capi.capsule_volume((0, 0, 0), (0, 1, 0), 0.25)[0]["type"] == CAPSULE
    assert capi.cylinder_volume((0, 0, 0), (0, 1, 0), 0.25)[0]["type"] == CYLINDER
    v = capi.hull_volume(3, position=(1, 0, 0))[0]
    assert v["type"] == HULL and v["hull_geometry"] == 3 and tuple(v["shape"][:4]) == (0, 0, 0, 1)
    assert len(np.concatenate([capi.sphere_volume((0, 0, 0), 1), capi.box_volume((0, 0, 0), (1, 1, 1))])) == 2


I = (0, 0, 0, 1)
Z90 = (0, 0, 0.5 ** 0.5, 0.5 ** 0.5)


def _gap(ta, sa, tb, sb, pa=(0, 0, 0), qa=I, pb=(0, 0, 0), qb=I):
    return R.signed_gap(R.world_shape(ta, np.asarray(sa, float), pa, qa), R.world_shape(tb, np.asarray(sb, float), pb, qb))


def test_gap_spheres_and_capsules():
    assert np.isclose(_gap(SPHERE, [0, 0, 0, 1], SPHERE, [3, 0, 0, 0.5]), 1.5)
    assert np.isclose(_gap(SPHERE, [0, 0, 0, 1], SPHERE, [1, 0, 0, 0.5]), -0.5)
    assert np.isclose(_gap(SPHERE, [0, 0, 0, 1], SPHERE, [0, 0, 0, 0.5], pb=(0, 4, 0)), 2.5)              # the pose moves it
    cap = [0, -1, 0, 0, 1, 0, 0.25]
    assert np.isclose(_gap(SPHERE, [2, 0.5, 0, 0.5], CAPSULE, cap), 1.25)                                   # beside the segment
    assert np.isclose(_gap(CAPSULE, cap, SPHERE, [0, 3, 0, 0.5]), 1.25)                                     # beyond its end; the order does not matter
    assert np.isclose(_gap(SPHERE, [2, 0, 0, 0.5], CAPSULE, cap, qb=Z90), 0.25)                             # capsule turned onto the x axis: end at x = 1
    assert np.isclose(_gap(CAPSULE, cap, CAPSULE, cap, pb=(2, 0, 0)), 1.5)                                  # parallel
    assert np.isclose(_gap(CAPSULE, cap, CAPSULE, cap, pb=(0, 0, 1), qb=Z90), 0.5)                          # crossed
    assert np.isclose(_gap(CAPSULE, cap, CAPSULE, cap, pb=(0, 3, 0)), 0.5)                                  # end to end
    assert _gap(CAPSULE, cap, CAPSULE, cap, pb=(0.1, 0, 0), qb=Z90) < 0
    assert _gap(CAPSULE, cap, CYLINDER, cap) is None and _gap(SPHERE, [0, 0, 0, 1], HULL, [0, 0, 0, 1, 0, 0, 0]) is None


def test_gap_boxes():
    box = [-1, -2, -3, 1, 2, 3]
    assert np.isclose(_gap(SPHERE, [3, 0, 0, 0.5], AABB, box), 1.5)
    assert np.isclose(_gap(SPHERE, [2, 3, 0, 0.5], AABB, box), 2 ** 0.5 - 0.5)                              # off an edge
    assert _gap(SPHERE, [0, 0, 0, 0.5], AABB, box) == -0.5                                                  # inside
    # a rotated AABB is an OBB: 90 degrees about z swaps its x and y half-extents
    assert R.world_shape(AABB, np.asarray(box, float), (0, 0, 0), Z90)[0] == OBB
    assert np.isclose(_gap(SPHERE, [3, 0, 0, 0.5], AABB, box, qb=Z90), 0.5)
    assert np.isclose(_gap(SPHERE, [3, 0, 0, 0.5], OBB, [*Z90, 0, 0, 0, 1, 2, 3]), 0.5)
    assert np.isclose(_gap(SPHERE, [3, 0, 0, 0.5], OBB, [*I, 0, 0, 0, 1, 2, 3], pb=(0.5, 0, 0)), 1.0)
    assert np.isclose(_gap(AABB, box, AABB, box, pb=(2.5, 0, 0)), 0.5)
    assert np.isclose(_gap(AABB, box, AABB, box, pb=(1.5, 1, 1)), -0.5)                                     # overlapping on every axis: the largest slab gap
    assert np.isclose(_gap(AABB, box, AABB, box, pb=(1.5, 1, 7)), 1.0)
    assert _gap(AABB, box, AABB, box, qb=Z90) is None                                                       # AABB vs OBB: no closed form here


def test_scaling_about_the_centre():
    vols = R.make_volumes(1, 2, (-1, -1, -1), (1, 1, 1))
    big = R.scale_volumes(vols, 2.0, 9)
    for v, b in zip(vols, big):
        t = int(v["type"])
        assert tuple(b["position"]) == tuple(v["position"]) and tuple(b["rotation"]) == tuple(v["rotation"])
        if t == SPHERE:
            assert np.allclose(b["shape"][:3], v["shape"][:3]) and np.isclose(b["shape"][3], 2 * v["shape"][3])
        elif t in (CAPSULE, CYLINDER):
            assert np.allclose(b["shape"][:3] + b["shape"][3:6], v["shape"][:3] + v["shape"][3:6], atol=1e-6)
            assert np.allclose(b["shape"][3:6] - b["shape"][:3], 2 * (v["shape"][3:6] - v["shape"][:3]), atol=1e-6) and np.isclose(b["shape"][6], 2 * v["shape"][6])
        elif t == AABB:
            assert np.allclose(b["shape"][3:6] - b["shape"][:3], 2 * (v["shape"][3:6] - v["shape"][:3]), atol=1e-6)
        elif t == OBB:
            assert np.allclose(b["shape"][7:10], 2 * v["shape"][7:10]) and np.allclose(b["shape"][:7], v["shape"][:7])
        else:
            assert b["hull_geometry"] == 9
    assert sorted(set(int(t) for t in vols["type"])) == [0, 1, 2, 3, 4, 5]


@pytest.mark.parametrize("name", ["shape_zoo", "zones"])
@pytest.mark.parametrize("settled", [False, True])
def test_trigger_yardstick_is_valid_for_the_gpu_tests_volumes(oracle_mod, name, settled):
    """The reference's trigger path on the volumes shrunk and grown by a relative 1e-3, for the four volume sets the GPU test uses (the
    settled ones at the poses the oracle reaches after the GPU test's 300 steps, in the GPU's order; the GPU test asserts the same three
    conditions again at the poses it reaches): shrunk within grown, both non-empty for most volumes, at most 2 % of the grown overlaps
    ambiguous.  A condition on the inputs, met by the choice of seeds, boxes and sizes in overlap_ref.volume_set."""
    from d3d12renderer_amd import capi
    sc = R.query_scene(name)
    vols = R.volume_set(name, settled)
    states = None
    if settled:
        w = sc.populate(oracle_mod.create_world(oracle_mod.ORDER_CANONICAL))
        w.step_fixed(sc.settings(), sc.dt, 300)
        ents = np.flatnonzero((sc.entities["kind"] == capi.ENTITY_DYNAMIC) | (sc.entities["kind"] == capi.ENTITY_KINEMATIC)).astype(np.uint32)
        states = (ents, w.get_body_states(ents))
        w.close()
    shrunk, grown, (subset, both, ambiguous) = R.oracle_sandwich(oracle_mod, sc, vols, states)
    print(f"{name} settled={settled}: {sum(map(len, shrunk))} shrunk / {sum(map(len, grown))} grown overlaps, both non-empty for {both:.0%} of {len(vols)} volumes, ambiguous {ambiguous:.2%}")
    assert subset
    assert both > 0.5
    assert ambiguous <= 0.02
    for t in range(6):   # every volume type takes part
        assert any(grown[i] for i in range(len(vols)) if int(vols["type"][i]) == t), t
