"""Free steps that follow caller-ordered ones (mi_debug_set_solve_order, optionally through mi_debug_set_solve_dataflow), the product against the
oracle's canonical schedule.  An ordered step solves in the caller's order, but it also writes the colour history the next FREE step trusts
(k_emit_manifolds keeps every colour it finds there): include/mi_physics.h fixes what that history holds — the overflow colour for every manifold of
the ordered step.  The replay tests order every step, so they never read that history back; these tests mix the two kinds of step and check, every
step, counts, contact sets and body states bit for bit, and after every free step the schedule itself: no shared dynamic body within a colour below 64,
and the oracle's colour for every manifold."""
import re

import numpy as np
import pytest

from d3d12renderer_amd import capi, scenes
from helpers import assert_schedule_valid, contact_set, make_order, manifold_colors, manifold_order, next_manifolds

pytestmark = pytest.mark.gpu

# the scenes of the dataflow replay (tests/test_gpu_reference_direct.py) + the joint zoo (joints force the one-lane kernel); (make, free steps before the first order)
SCENES = {
    "spheres": (lambda: scenes.sphere_drop(6), 75),
    "mixed stack": (lambda: scenes.mixed_stack(6, 4, 6), 60),
    "box pile": (lambda: scenes.obb_pile(5, 3, 5, spacing=1.0), 60),
    "box pile, 256 boxes": (lambda: scenes.obb_pile(8, 4, 8, spacing=1.0), 60),
    "shape zoo": (lambda: scenes.shape_zoo(), 60),
    "aligned boxes": (scenes.EDGE_CASES["aligned boxes"], 40),
    "parallel capsules": (scenes.EDGE_CASES["parallel capsules and cylinders"], 40),
    "joint zoo": (lambda: scenes.joint_zoo(copies=2), 110),
}
# F = free step, O = ordered step (the ordered steps take "new manifolds first" and seeded random orders in turn)
PATTERNS = {
    "free, ordered, free": "FFOFFFFF",
    "ordered run, then free": "OOOOFFFFF",
    "alternating": "OFOFOFOFOF",
}


class Run:
    """A product world, the oracle and a twin product world that is never ordered, stepped together."""

    def __init__(self, mi_lib, oracle_mod, sc, dataflow, events=False, seed=11, schedule=True):
        self.sc, self.om = sc, oracle_mod
        self.g = sc.populate(mi_lib.create_world(0))
        self.o = sc.populate(oracle_mod.create_world(oracle_mod.ORDER_CANONICAL))
        self.twin = sc.populate(mi_lib.create_world(0))
        self.s = sc.settings()
        self.ids = np.arange(sc.num_bodies, dtype=np.uint32)
        self.events, self.schedule = events, schedule
        if dataflow:
            self.g.debug_set_solve_dataflow(True)
        if events:
            self.g.enable_events(True); self.o.enable_events(True)
        self.rng = np.random.default_rng(seed)
        self.step_no = 0
        self.ordered = 0
        self.levelled = 0
        self.last_ordered = False
        self.num_events = 0

    def same(self, tag, ordered):
        cg, co = self.g.counts(), self.o.counts()
        if ordered:   # (num_colors: the product reports the colours the order ran in, the oracle 65)
            cg.pop("num_colors"); co.pop("num_colors")
        assert cg == co, f"{tag}: counts {cg} != oracle {co}"
        assert contact_set(self.g.contacts()) == contact_set(self.o.contacts()), f"{tag}: contact sets differ"
        assert self.g.get_body_states(self.ids).tobytes() == self.o.get_body_states(self.ids).tobytes(), f"{tag}: body states differ from the oracle's"
        if self.events:
            eg, eo = self.g.poll_events(), self.o.poll_events()
            assert eg.tobytes() == eo.tobytes(), f"{tag}: events ({len(eg)} / oracle {len(eo)})"
            self.num_events += len(eg)

    def free(self, tag):
        retries = self.g.step_mode_stats()[2]
        self.g.step_fixed(self.s, self.sc.dt, 1); self.o.step_fixed(self.s, self.sc.dt, 1); self.twin.step_fixed(self.s, self.sc.dt, 1)
        self.step_no += 1
        tag = f"{tag}, step {self.step_no} (free{', after an ordered one' if self.last_ordered else ''})"
        self.same(tag, False)
        if self.schedule:
            assert_schedule_valid(self.g, self.o, tag=f"{tag}: ")
        assert self.g.solver_kind() == self.twin.solver_kind(), f"{tag}: solver kind {self.g.solver_kind()}, a world never ordered runs {self.twin.solver_kind()}"
        if self.last_ordered:
            assert self.g.step_mode_stats()[2] == retries, f"{tag}: the step was re-run (synchronous retries {retries} -> {self.g.step_mode_stats()[2]})"
        self.last_ordered = False

    def order(self, tag, kind=None, dataflow=False):
        kind = kind or ("new first" if self.ordered % 2 == 0 else "random")
        pairs = make_order(next_manifolds(self.sc, self.om, self.o), manifold_order(self.o.contacts()), self.rng, kind)
        self.g.debug_set_solve_order(pairs); self.o.debug_set_solve_order(pairs)
        self.g.step_fixed(self.s, self.sc.dt, 1); self.o.step_fixed(self.s, self.sc.dt, 1); self.twin.step_fixed(self.s, self.sc.dt, 1)
        self.step_no += 1; self.ordered += 1
        self.same(f"{tag}, step {self.step_no} (ordered, {kind}, {len(pairs)} manifolds)", True)
        if dataflow and self.g.debug_solve_order_depth() > 0:
            self.levelled += 1
        self.last_ordered = True
        return pairs

    def warm(self, n, tag):
        for _ in range(n):
            self.free(tag)


@pytest.mark.parametrize("dataflow", [False, True], ids=["one lane", "dataflow"])
@pytest.mark.parametrize("pattern", list(PATTERNS))
@pytest.mark.parametrize("name", list(SCENES))
def test_gpu_free_steps_after_ordered_steps_match_the_oracle(mi_lib, oracle_mod, name, pattern, dataflow):
    make, warm = SCENES[name]
    r = Run(mi_lib, oracle_mod, make(), dataflow)
    tag = f"{name}, {pattern}, {'dataflow' if dataflow else 'one lane'}"
    r.warm(warm, tag)
    assert r.o.counts()["num_collisions"] > 0, f"{tag}: no contact before the first order"
    for c in PATTERNS[pattern]:
        if c == "O":
            r.order(tag, dataflow=dataflow)
        else:
            r.free(tag)
    if dataflow and name != "joint zoo":
        assert r.levelled > 0, f"{tag}: no ordered step went through the production solver"
    if name == "joint zoo":
        assert r.levelled == 0 and r.g.debug_solve_order_depth() == 0


@pytest.mark.parametrize("dataflow", [False, True], ids=["one lane", "dataflow"])
def test_gpu_events_across_ordered_steps_match_the_oracle(mi_lib, oracle_mod, dataflow):
    """Collision begin / end events read the same history table: polled after every step, they must be the oracle's byte for byte."""
    r = Run(mi_lib, oracle_mod, scenes.mixed_stack(6, 4, 6), dataflow, events=True)
    r.warm(50, "events")
    for c in "OOFFOFOFFFOOOFFF":
        r.order("events", dataflow=dataflow) if c == "O" else r.free("events")
    assert r.num_events > 50
    if dataflow:
        assert r.levelled > 0


@pytest.mark.parametrize("dataflow", [False, True], ids=["one lane", "dataflow"])
def test_gpu_checkpoint_right_after_an_ordered_step(mi_lib, oracle_mod, dataflow):
    """A checkpoint saved right after an ordered step carries the history that step left: a fresh product world and an oracle world loaded from
    it continue freely exactly like the original."""
    sc = scenes.obb_pile(5, 3, 5, spacing=1.0)
    r = Run(mi_lib, oracle_mod, sc, dataflow)
    r.warm(60, "checkpoint")
    r.order("checkpoint", dataflow=dataflow); r.order("checkpoint", dataflow=dataflow)
    blob = r.g.save_checkpoint()
    g2 = sc.populate(mi_lib.create_world(0)); g2.load_checkpoint(blob)
    o2 = sc.populate(oracle_mod.create_world(oracle_mod.ORDER_CANONICAL)); o2.load_checkpoint(blob)
    for k in range(8):
        r.free("checkpoint")
        g2.step_fixed(r.s, sc.dt, 1); o2.step_fixed(r.s, sc.dt, 1)
        tag = f"checkpoint: free step {k + 1} after loading"
        for w, who in ((g2, "reloaded product"), (o2, "reloaded oracle")):
            assert w.counts() == r.g.counts(), f"{tag}: {who} counts"
            assert contact_set(w.contacts()) == contact_set(r.g.contacts()), f"{tag}: {who} contacts"
            assert w.get_body_states(r.ids).tobytes() == r.g.get_body_states(r.ids).tobytes(), f"{tag}: {who} body states"
        assert_schedule_valid(g2, o2, tag=f"{tag}: ")
        assert np.array_equal(manifold_colors(g2)[2], manifold_colors(r.g)[2]), f"{tag}: colours"
    if dataflow:
        assert r.levelled > 0


def test_gpu_no_ordered_step_with_heightmap_terrain(mi_lib, oracle_mod):
    """mi_debug_set_solve_order refuses a world with terrain (MI_ERR_UNSUPPORTED = -6), and the world steps on as if it had never been asked."""
    sc = scenes.terrain_field(6, 2, 6)
    # (no schedule check: the product's colour getter lists terrain manifolds otherwise than num_collisions counts them)
    r = Run(mi_lib, oracle_mod, sc, dataflow=True, schedule=False)
    r.warm(130, "terrain")
    pairs = manifold_order(r.o.contacts())
    assert len(pairs) > 0
    with pytest.raises(capi.PhysicsError, match=re.escape("status -6")):
        r.g.debug_set_solve_order(pairs)
    r.warm(5, "terrain, after the refused order")


@pytest.mark.parametrize("dataflow", [False, True], ids=["one lane", "dataflow"])
@pytest.mark.parametrize("bad", ["one too few", "one too many"])
def test_gpu_rejected_order_leaves_the_world_as_it_was(mi_lib, oracle_mod, bad, dataflow):
    """A list that does not name the step's manifolds exactly fails the step (MI_ERR_INVALID_ARGUMENT = -1) and changes nothing: same body states, and the
    next free steps are those of a twin world that never got the list.  (The oracle finishes such a step before it reports the error: not the
    reference here.)"""
    sc = scenes.obb_pile(5, 3, 5, spacing=1.0)
    r = Run(mi_lib, oracle_mod, sc, dataflow)
    r.warm(60, "rejected")
    pairs = next_manifolds(sc, oracle_mod, r.o)
    if bad == "one too few":
        pairs = pairs[:-1]
    else:
        listed = {(int(a), int(b)) for a, b in pairs} | {(int(b), int(a)) for a, b in pairs}
        nc = r.g.counts()["num_colliders"]
        extra = next((a, b) for a in range(nc) for b in range(nc - 1, a, -1) if (a, b) not in listed)
        pairs = np.concatenate([pairs, np.asarray([extra], np.uint32)])
    before = r.g.get_body_states(r.ids).tobytes()
    with pytest.raises(capi.PhysicsError, match=re.escape("status -1")):
        r.g.debug_set_solve_order(pairs)
        r.g.step_fixed(r.s, sc.dt, 1)
    assert r.g.get_body_states(r.ids).tobytes() == before, "the rejected step changed the body states"
    for k in range(4):
        r.g.step_fixed(r.s, sc.dt, 1); r.twin.step_fixed(r.s, sc.dt, 1)
        tag = f"rejected ({bad}): free step {k + 1} after it"
        assert r.g.counts() == r.twin.counts(), tag
        assert contact_set(r.g.contacts()) == contact_set(r.twin.contacts()), tag
        assert r.g.get_body_states(r.ids).tobytes() == r.twin.get_body_states(r.ids).tobytes(), tag
        assert np.array_equal(assert_schedule_valid(r.g, tag=f"{tag}: "), manifold_colors(r.twin)[2]), f"{tag}: colours"
        assert r.g.solver_kind() == r.twin.solver_kind(), tag
