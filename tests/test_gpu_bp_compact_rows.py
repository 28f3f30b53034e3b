"""The grid pass of the broad phase walks 16-byte compact rows (the box quantised to 16 bits per bound on a frame around the step's grid: csrc/bp_quant.hpp) and
puts what passes to the exact test.  The quantised test may only ever let too much through, so the pair set, every count and the trajectory stay what the CPU oracle
computes.  Scenes that sit where a quantised test could go wrong: faces that coincide exactly and lie off the quantisation lattice, boxes beyond the frame's clamped
ends, a frame so coarse that a quantum is larger than a box, and a heap in which one collider's candidates exceed a 64-candidate window and every staging tier."""
import numpy as np
import pytest

from d3d12renderer_amd import capi, scenes
from helpers import _same_counts, contact_set

pytestmark = pytest.mark.gpu


def _boxes(pos, half, rot=None, seed=11):
    n = len(pos)
    e = scenes.make_entities(n)
    e["position"] = np.asarray(pos, np.float32)
    if rot is not None:
        e["rotation"] = rot
    c = scenes.make_colliders(n, capi.AABB)
    h = np.broadcast_to(np.asarray(half, np.float32), (n, 3))
    c["shape"][:, 0:3] = -h
    c["shape"][:, 3:6] = h
    return e, c


def _scene(name, parts, iterations=10):
    ents = np.concatenate([p[0] for p in parts]); cols = np.concatenate([p[1] for p in parts])
    return scenes.Scene(name, ents, np.arange(len(ents), dtype=np.uint32), cols, iterations)


def touching_block(with_large=False):
    """6 x 6 x 6 unit AABB colliders whose neighbouring faces coincide exactly in fp32 (lattice step 1 = the box size; the translation keeps every coordinate inside
    one binade, so centre +- 0.5 is exact), far from the origin so that no face falls on a quantisation step."""
    ix, iy, iz = np.meshgrid(np.arange(6), np.arange(6), np.arange(6), indexing="ij")
    base = np.asarray([3000.37, 50.1, -7000.73], np.float32)
    pos = np.stack([ix.ravel(), iy.ravel(), iz.ravel()], axis=1).astype(np.float32) + base
    parts = [_boxes(pos, 0.5)]
    if with_large:   # one much larger static box under the block: a "large" collider beside the grid's small ones
        ge, gc = scenes._ground(200.0)
        ge["position"][0] = (base[0], base[1] - 0.5, base[2])
        parts.append((ge, gc))
    return _scene("touching_block", parts)


def coarse_frame():
    """Two clusters of 64 rotated boxes 1e5 m apart: the grid's long axis is quantised in steps of about 1.5 m, more than a box."""
    parts = []
    for k, cx in enumerate((-5.0e4, 5.0e4)):
        pos = scenes._lattice(4, 4, 4, 0.9, 5.0, 21 + k, 0.05) + np.asarray([cx, 0.0, 0.0], np.float32)
        h = np.stack([scenes.uniform(31 + k, 30 + a, 64, 0.3, 0.6) for a in range(3)], axis=1)
        parts.append(_boxes(pos, h, rot=scenes.random_unit_quaternions(41 + k, 20, 64)))
    return _scene("coarse_frame", parts)


def dense_heap():
    """96 unit boxes whose centres lie within 1 cm: every one of the 4 560 pairs overlaps."""
    pos = np.stack([scenes.uniform(51, a, 96, -0.005, 0.005) for a in range(3)], axis=1) + np.asarray([10.0, 20.0, -30.0], np.float32)
    return _scene("dense_heap", [_boxes(pos, 0.5)], iterations=4)


def _against_oracle(mi_lib, oracle_mod, sc, steps, between=None):
    g = sc.populate(mi_lib.create_world(0)); o = sc.populate(oracle_mod.create_world(oracle_mod.ORDER_CANONICAL))
    s = sc.settings(); ids = np.arange(sc.num_bodies, dtype=np.uint32)
    overlaps = []
    for i in range(steps):
        if between is not None and i:
            between(i, g, o, ids)
        g.step_fixed(s, sc.dt, 1); o.step_fixed(s, sc.dt, 1)
        cc, co = g.counts(), o.counts()
        print(f"step {i}: gpu {cc}  oracle {co}")
        _same_counts(cc, co, i, o.aabbs(), co["sorting_axis"])     # bodies, colliders, manifolds, contacts bit-exact; overlaps = the closed-interval census of the AABBs
        assert cc["sorting_axis"] == co["sorting_axis"], f"step {i}"
        assert contact_set(g.contacts()) == contact_set(o.contacts()), f"step {i}: contact lists"
        assert g.get_body_states(ids).tobytes() == o.get_body_states(ids).tobytes(), f"step {i}: body states"
        overlaps.append(cc["num_broadphase_overlaps"])
    return overlaps


# closed-interval overlaps inside a 6^3 lattice of touching unit boxes: ordered neighbour pairs per axis 6 + 2 * 5 = 16, so (16^3 - 216) / 2 unordered pairs
TOUCHING_PAIRS = (16 ** 3 - 216) // 2


def test_touching_faces_off_the_lattice(mi_lib, oracle_mod):
    ov = _against_oracle(mi_lib, oracle_mod, touching_block(), 2)
    assert ov[0] == TOUCHING_PAIRS      # the faces do coincide: every face, edge and corner neighbour is found, none is lost to the rounding of a bound


def test_touching_faces_beyond_the_frames_clamped_end(mi_lib, oracle_mod):
    """Steps after the first use the grid — and with it the frame — prepared at the end of the previous step.  The block is moved by 4.3 m along x between the steps:
    part of it then lies beyond the frame's upper end, where minima and maxima both clamp to 65535; then back by 9.1 m, beyond the lower end, where both clamp to 0."""
    def shift(i, g, o, ids):
        st = o.get_body_states(ids)
        assert st.tobytes() == g.get_body_states(ids).tobytes()
        st[:, 0] += np.float32(4.3) if i == 1 else np.float32(-9.1)
        g.set_body_states(ids, st); o.set_body_states(ids, st)
    ov = _against_oracle(mi_lib, oracle_mod, touching_block(with_large=True), 3, between=shift)
    assert ov[0] == TOUCHING_PAIRS + 36     # + the bottom layer on the large box


def test_frame_coarser_than_a_box(mi_lib, oracle_mod):
    ov = _against_oracle(mi_lib, oracle_mod, coarse_frame(), 3)
    assert min(ov) > 100


def test_dense_heap_exceeds_a_window_and_every_staging_tier(mi_lib, oracle_mod):
    ov = _against_oracle(mi_lib, oracle_mod, dense_heap(), 2)
    assert ov[0] == 96 * 95 // 2 == 4560
