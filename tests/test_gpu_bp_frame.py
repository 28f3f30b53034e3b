"""The broad phase's set-up passes (k_bp_prepare: world colliders, classification, centre statistics, bounds of the small centres, cell keys and arrival ranks;
k_bp_scatter_sorted: the cell-sorted rows and the compact rows on the grid's quantisation frame) produce integers and exactly the same floats whatever way their
reductions, their atomics and the frame are arranged: a 4 096-box pile and the all-shapes zoo, 30 steps each, against the oracle as tests/test_gpu_parity.py
does it — every body bit, every count — and without a synchronous re-run."""
import pytest

from d3d12renderer_amd import scenes

pytestmark = pytest.mark.gpu
STEPS = 30


@pytest.fixture(scope="module")
def oracle_runs(oracle_mod):
    """The oracle's 30 steps of both scenes, computed once: counts after every step, body state at the end."""
    out = {}
    for name, make in SCENES.items():
        sc = make()
        o = sc.populate(oracle_mod.create_world(oracle_mod.ORDER_CANONICAL))
        s = sc.settings()
        counts = []
        for _ in range(STEPS):
            o.step_fixed(s, sc.dt, 1)
            counts.append(o.counts())
        out[name] = (counts, [a.tobytes() for a in o.physics_transforms() + o.velocities()])
    return out


SCENES = {
    "pile of 4096 boxes": lambda: scenes.obb_pile(16, 16, 16, spacing=1.05),
    "all-shapes zoo": lambda: scenes.shape_zoo(8, 5, 8),
}


@pytest.mark.parametrize("name", sorted(SCENES))
def test_broad_phase_setup_keeps_every_bit(mi_lib, oracle_runs, name):
    sc = SCENES[name]()
    g = sc.populate(mi_lib.create_world(0))
    s = sc.settings()
    want_counts, want_state = oracle_runs[name]
    for i in range(STEPS):
        g.step_fixed(s, sc.dt, 1)
        assert g.counts() == want_counts[i], f"step {i}"      # overlaps, manifolds, contacts, colours, sweep axis
    got = [a.tobytes() for a in g.physics_transforms() + g.velocities()]
    assert got == want_state, "positions, rotations, linear and angular velocities, bit for bit"
    assert want_counts[-1]["num_broadphase_overlaps"] > 0
    # what the library gave on these scenes before the passes were rearranged: the first step synchronous, every other one speculative, no re-run
    steps, speculative, reruns = g.step_mode_stats()
    assert (steps, speculative, reruns) == (STEPS, STEPS - 1, 0)
