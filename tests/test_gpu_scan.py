"""k_exclusive_scan (csrc/kernels_scan.hpp), the step's device-wide exclusive prefix sum, through mi_debug_exclusive_scan: the production kernel on the world's stream
and through the step's own scan sites, against a numpy prefix sum — exactly.  Sizes around a wave, around one tile, a few tiles with a ragged end, and 70 tiles + 5, where the
look-back of the last tiles reaches past 64 predecessors.  The 64-bit variant carries two independent 32-bit sums side by side (the narrow phase's packed
(manifold flag, contact count)); every total here ends at 2^32 - 1, the most the contract allows, so no carry crosses between the halves and every bit of a half is used."""
import re
from pathlib import Path
import numpy as np
import pytest

from d3d12renderer_amd import scenes

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
TOP = (1 << 32) - 1


def tile_items(width):
    """Items of one workgroup's tile: 256 threads x the items per lane kernels_scan.hpp is built with."""
    src = (ROOT / "d3d12renderer_amd" / "csrc" / "kernels_scan.hpp").read_text()
    return 256 * int(re.search(rf"kScanItems{width} = (\d+)", src).group(1))


def sizes(width):
    t = tile_items(width)
    return [0, 1, 63, 64, 65, t - 1, t, t + 1, 3 * t + 17, 70 * t + 5]


def halves(rng, n):
    """n values whose sum is exactly 2^32 - 1; the first one takes what the random ones leave, so the prefix sums are large from the second item on."""
    if n == 0:
        return np.zeros(0, np.uint64)
    v = rng.integers(0, TOP // n + 1, n, dtype=np.uint64)
    v[0] = 0
    v[0] = TOP - int(v.sum())
    return v


def make_input(rng, width, n):
    lo = halves(rng, n)
    if width == 32:
        return lo.astype(np.uint32)
    return (halves(rng, n) << np.uint64(32)) | lo


def exclusive(a):
    """The reference: an exclusive prefix sum per 32-bit half, in 64-bit arithmetic."""
    def ex(v):
        c = np.cumsum(v, dtype=np.uint64)
        assert c.size == 0 or int(c[-1]) <= TOP
        return np.concatenate([np.zeros(1, np.uint64), c[:-1]]) if c.size else c
    if a.dtype == np.uint32:
        return ex(a.astype(np.uint64)).astype(np.uint32)
    return (ex(a >> np.uint64(32)) << np.uint64(32)) | ex(a & np.uint64(TOP))


@pytest.fixture(scope="module")
def cases():
    """Inputs and their reference sums, computed once and left unchanged."""
    rng = np.random.default_rng(20)
    out = {}
    for width in (32, 64):
        for n in sizes(width):
            a = make_input(rng, width, n)
            a.setflags(write=False)
            out[width, n] = (a, exclusive(a))
    return out


@pytest.mark.parametrize("width", [32, 64])
def test_scan_equals_numpy_prefix_sum_on_one_world(mi_lib, cases, width):
    """Every size, one call after the other on ONE world (so every launch finds the ticket base, the generation and the records of the launches before it, larger and
    smaller), then the sizes again in reverse with zero_input = 1, which must leave the input cleared."""
    w = mi_lib.create_world(0)
    for n in sizes(width):
        a, want = cases[width, n]
        got, left = w.debug_exclusive_scan(a)
        assert got.dtype == a.dtype and got.tobytes() == want.tobytes(), f"n = {n}"
        assert left.tobytes() == a.tobytes(), f"n = {n}: zero_input = 0 leaves the input alone"
    for n in reversed(sizes(width)):
        a, want = cases[width, n]
        got, left = w.debug_exclusive_scan(a, zero_input=True)
        assert got.tobytes() == want.tobytes(), f"n = {n}, zero_input"
        assert not left.any(), f"n = {n}: input not cleared"


def test_scan_behind_the_steps_own_scans(mi_lib, cases):
    """40 steps of a box pile leave their records, tickets and generations in the cell histogram's and the pair scan's sites; a call through the same sites
    afterwards is still exact, and the steps after it still run (speculatively, without a synchronous re-run because of it)."""
    sc = scenes.obb_pile(12, 5, 12, spacing=1.05)
    w = sc.populate(mi_lib.create_world(0))
    s = sc.settings()
    w.step_fixed(s, sc.dt, 40)
    retries = w.step_mode_stats()[2]
    for width in (32, 64):
        n = sizes(width)[-2]
        a, want = cases[width, n]
        got, _ = w.debug_exclusive_scan(a)
        assert got.tobytes() == want.tobytes(), f"width {width}"
    before = w.counts()
    w.step_fixed(s, sc.dt, 5)
    assert w.counts()["num_contacts"] > 0 and before["num_contacts"] > 0
    assert w.step_mode_stats()[2] == retries
    pile = sc.populate(mi_lib.create_world(0))
    pile.step_fixed(s, sc.dt, 45)
    assert pile.physics_transforms()[0].tobytes() == w.physics_transforms()[0].tobytes() and pile.counts() == w.counts()
