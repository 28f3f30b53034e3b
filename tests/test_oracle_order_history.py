"""The colour history after a caller-ordered step (mi_debug_set_solve_order, include/mi_physics.h), the oracle's side of the contract: every
manifold of an ordered step enters the history with the overflow colour 64, so the next free step colours every manifold afresh — greedy in
descending pair priority.  The free step after an ordered one must therefore (a) give no two manifolds of one colour below 64 a shared dynamic
body and (b) colour exactly as that rule says.  The GPU suite (tests/test_gpu_order_transitions.py) holds the product to the oracle."""
import numpy as np
import pytest

from d3d12renderer_amd import scenes
from helpers import assert_schedule_valid, dynamic_bodies, greedy_colors, make_order, manifold_colors, manifold_order, next_manifolds

SCENES = {
    "box pile": (lambda: scenes.obb_pile(5, 3, 5, spacing=1.0), 60),
    "mixed stack": (lambda: scenes.mixed_stack(6, 4, 6), 60),
    "joint zoo": (lambda: scenes.joint_zoo(copies=2), 110),
}


@pytest.mark.parametrize("kind", ["new first", "random"])
@pytest.mark.parametrize("ordered_steps", [1, 3])
@pytest.mark.parametrize("name", list(SCENES))
def test_oracle_free_step_after_an_ordered_one_recolours_everything(oracle_mod, name, ordered_steps, kind):
    make, warm = SCENES[name]
    sc = make()
    o = sc.populate(oracle_mod.create_world(oracle_mod.ORDER_CANONICAL))
    s = sc.settings()
    o.step_fixed(s, sc.dt, warm)
    rng = np.random.default_rng(7)
    for _ in range(ordered_steps):
        prev = manifold_order(o.contacts())
        pairs = next_manifolds(sc, oracle_mod, o)
        o.debug_set_solve_order(make_order(pairs, prev, rng, kind))
        o.step_fixed(s, sc.dt, 1)
        assert o.counts()["num_collisions"] == len(pairs)
    o.step_fixed(s, sc.dt, 1)                    # free
    pairs, heads, colors = manifold_colors(o)
    assert len(pairs) > 12, "not a scene in contact"
    assert_schedule_valid(o, tag=f"{name}: ")
    want = greedy_colors(pairs, heads, dynamic_bodies(o))
    assert np.array_equal(colors, want), f"{name}: {int((colors != want).sum())} of {len(pairs)} colours are not the fresh greedy colouring"
    # and a second free step keeps them (the ordinary history)
    o.step_fixed(s, sc.dt, 1)
    assert_schedule_valid(o, tag=f"{name}, second free step: ")


def test_oracle_history_survives_free_steps(oracle_mod):
    """Control: without an ordered step the history keeps colours, so a settled pile is NOT coloured afresh — the test above can tell the two apart."""
    sc = scenes.obb_pile(5, 3, 5, spacing=1.0)
    o = sc.populate(oracle_mod.create_world(oracle_mod.ORDER_CANONICAL))
    o.step_fixed(sc.settings(), sc.dt, 62)
    pairs, heads, colors = manifold_colors(o)
    assert_schedule_valid(o)
    assert not np.array_equal(colors, greedy_colors(pairs, heads, dynamic_bodies(o)))
