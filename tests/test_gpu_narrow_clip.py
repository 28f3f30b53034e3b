"""The box narrow phase (k_narrow: SAT + class-staged hit queues; k_narrow_clip: face clipping / edge contacts) on scenes built to reach every
class of box pair and every state of the queues, against the CPU oracle in canonical order: counts, contacts as a set and poses, bit for bit.

Scene 1, `box_pair_zoo`: 602 isolated two-box pairs (7 families x 86; 602 = 2 x 256 + 90: three k_narrow workgroups, the last one partial), 6 m apart, no
gravity, the first box of a pair static.  The families, in creation order:
  face_a / face_b   a small box resting on (face_a) or under (face_b) a larger one, random yaw, tilted about a random horizontal axis by 0.2 - 4 degrees: the larger
                    tilts lift one or two vertices of the incident face out of the reference face (dropped: swap-and-pop), so these give 4, 3 and 2 contacts;
                    half of the pairs are created small box first, half large box first, so the reference face is A's in some and B's in the others
  aligned           two OBB colliders with the SAME quaternion (the SAT's "parallel" branch: no edge axes), overlapping by part of a face
  corner            a cube standing on a corner in the face of a flat box: three of the four incident vertices have negative depth
  aabb_obb          a static AABB collider (identity pose: it stays an AABB, the pair is of the other box bucket) under a yawed and tilted box
  edge              edge over edge: the lower cube turned 45 degrees about x, the upper one 45 degrees about z and about 35 degrees about y
  separated         two cubes yawed 45 degrees whose AABBs overlap while their faces are 0.05 m apart: the SAT misses, the queues hold fewer hits than pairs
The coverage conditions are checked on the ORACLE's output (they hold for any implementation that matches it).  Which 256 pairs share a k_narrow workgroup is not
reported by anything; the pairs of a family are created one after the other on consecutive grid positions, and the test holds the conditions "a workgroup of one
class" / "a workgroup of both classes" against chunks of 256 pairs in creation order, forwards and backwards.

Scene 2, `full_lattice`: 8 x 8 x 8 OBBs of half-extent 0.5 at spacing 0.7, those of odd parity turned by 6 - 15 degrees about a random axis (their AABBs stay
under 0.7, so the second neighbours stay out of the pair list; every cube contains the sphere of radius 0.5 and the aligned ones reach into it): each of the
5 068 AABB-overlapping pairs (26-neighbourhood) intersects, about 300 of them by an edge.  In the synchronous first step every queue region (20 workgroups over
16 queues: 512 slots, filled by two workgroups in queues 0-3) is filled to capacity, the face run and the edge run of a region meet, and the last k_narrow
workgroup is partial (5 068 = 19 x 256 + 204)."""
import numpy as np
import pytest

from d3d12renderer_amd import scenes, capi
from helpers import contact_set

pytestmark = pytest.mark.gpu

FAMILIES = ("face_a", "face_b", "aligned", "corner", "aabb_obb", "edge", "separated")
PER_FAMILY = 86
EDGE_CLASS = {"edge"}
MISS = {"separated"}


def _q(axis, deg):
    return scenes.q_axis_angle(axis, np.deg2rad(deg))


def box_pair_zoo(seed=41):
    rng = np.random.default_rng(seed)
    n_pairs = PER_FAMILY * len(FAMILIES)
    e = scenes.make_entities(2 * n_pairs)
    e["gravity_factor"] = 0.0
    c = scenes.make_colliders(2 * n_pairs, capi.AABB)
    family = []
    cols = 25

    def put(i, pos, rot, half, static=False):
        e["position"][i] = pos
        e["rotation"][i] = rot
        if static:
            e["kind"][i] = capi.ENTITY_STATIC
        c["shape"][i, 0:3] = -np.asarray(half, np.float32)
        c["shape"][i, 3:6] = half

    def put_obb(i, pos, lrot, half, static=False):   # an OBB collider on an entity with the identity rotation: world rotation = lrot, bit for bit
        e["position"][i] = pos
        if static:
            e["kind"][i] = capi.ENTITY_STATIC
        c["type"][i] = capi.OBB
        c["shape"][i, 0:4] = lrot
        c["shape"][i, 4:7] = 0.0
        c["shape"][i, 7:10] = half

    ident = np.array([0, 0, 0, 1], np.float32)
    for p in range(n_pairs):
        fam = FAMILIES[p // PER_FAMILY]
        family.append(fam)
        base = np.array([6.0 * (p % cols), 0.0, 6.0 * (p // cols)])
        i0, i1 = 2 * p, 2 * p + 1
        yaw0, yaw1 = rng.uniform(0, 360, 2)
        if fam in ("face_a", "face_b"):
            big = np.array([1.0, 0.5, 1.0]) * rng.uniform(0.9, 1.1); small = rng.uniform(0.3, 0.45, 3)
            tilt = (0.2, 1.5, 2.5, 4.0)[p % 4]
            tq = _q((np.cos(np.deg2rad(yaw1)), 0.0, np.sin(np.deg2rad(yaw1))), tilt)
            off = np.array([rng.uniform(-0.3, 0.3), 0.0, rng.uniform(-0.3, 0.3)])
            gap = big[1] + small[1] - 0.012
            big_rot = _q((0, 1, 0), yaw0); small_rot = scenes.q_mul(tq, _q((0, 1, 0), rng.uniform(0, 360)))
            up = 1.0 if fam == "face_a" else -1.0     # the small box above / below
            if p % 2 == 0:
                put(i0, base, big_rot, big, static=True); put(i1, base + off + (0, up * gap, 0), small_rot, small)
            else:
                put(i0, base + off + (0, up * gap, 0), small_rot, small, static=True); put(i1, base, big_rot, big)
        elif fam == "aligned":
            rot = np.asarray(_q((0, 1, 0), yaw0), np.float32)
            h0 = rng.uniform(0.4, 0.6, 3); h1 = rng.uniform(0.3, 0.5, 3)
            off = scenes.q_rot(rot, np.array([rng.uniform(-0.5, 0.5), h0[1] + h1[1] - 0.02, rng.uniform(-0.5, 0.5)], np.float32))
            put_obb(i0, base, rot, h0, static=True); put_obb(i1, base + off, rot, h1)
        elif fam == "corner":
            flat = np.array([1.0, 0.3, 1.0])
            rot = scenes.q_mul(_q((0, 1, 0), yaw1), scenes.q_mul(_q((1, 0, 0), 35.2644), _q((0, 0, 1), 45.0)))
            put(i0, base, _q((0, 1, 0), yaw0), flat, static=True)
            put(i1, base + (rng.uniform(-0.3, 0.3), 0.3 + 0.5 * np.sqrt(3.0) - 0.03, rng.uniform(-0.3, 0.3)), rot, (0.5, 0.5, 0.5))
        elif fam == "aabb_obb":
            h0 = np.array([1.0, 0.5, 1.0]); h1 = rng.uniform(0.3, 0.45, 3)
            tq = _q((np.cos(np.deg2rad(yaw0)), 0.0, np.sin(np.deg2rad(yaw0))), (0.2, 2.0)[p % 2])
            put(i0, base, ident, h0, static=True)
            put(i1, base + (rng.uniform(-0.7, 0.7), h0[1] + h1[1] - 0.012, rng.uniform(-0.7, 0.7)), scenes.q_mul(tq, _q((0, 1, 0), yaw1)), h1)
        elif fam == "edge":
            lower = _q((1, 0, 0), 45.0)
            upper = scenes.q_mul(_q((0, 1, 0), 35.0 + rng.uniform(-10, 10)), _q((0, 0, 1), 45.0))
            put(i0, base, lower, (0.5, 0.5, 0.5), static=True)
            put(i1, base + (rng.uniform(-0.1, 0.1), np.sqrt(2.0) - 0.03, rng.uniform(-0.1, 0.1)), upper, (0.5, 0.5, 0.5))
        else:   # separated
            rot = _q((0, 1, 0), 45.0)
            d = 1.05 / np.sqrt(2.0)
            put(i0, base, rot, (0.5, 0.5, 0.5), static=True); put(i1, base + (d, rng.uniform(-0.2, 0.2), d), rot, (0.5, 0.5, 0.5))
    sc = scenes.Scene("box_pair_zoo", e, np.arange(2 * n_pairs, dtype=np.uint32), c, 10)
    return sc, family


def full_lattice(n=8, seed=43):
    rng = np.random.default_rng(seed)
    nb = n ** 3
    e = scenes.make_entities(nb)
    e["gravity_factor"] = 0.0
    ix, iy, iz = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    e["position"] = np.stack([ix.ravel(), iy.ravel(), iz.ravel()], axis=1).astype(np.float32) * np.float32(0.7)
    c = scenes.make_colliders(nb, capi.OBB)
    c["shape"][:, 0:4] = (0, 0, 0, 1)
    c["shape"][:, 7:10] = 0.5
    for k in np.flatnonzero((ix + iy + iz).ravel() % 2 == 1):
        axis = rng.normal(size=3); axis /= np.linalg.norm(axis)
        c["shape"][k, 0:4] = scenes.q_axis_angle(axis, np.deg2rad(rng.uniform(6.0, 15.0)))
    return scenes.Scene("full_lattice", e, np.arange(nb, dtype=np.uint32), c, 4)


def manifold_sizes(contacts):
    """{(collider_a, collider_b): contacts in the manifold} of a contact list."""
    out = {}
    for k in contacts:
        key = (int(k["collider_a"]), int(k["collider_b"]))
        out[key] = out.get(key, 0) + 1
    return out


@pytest.fixture(scope="module")
def zoo_reference(oracle_mod):
    """The zoo, its family labels and the oracle's three steps (counts, contact set, contact list), computed once; and the coverage conditions, held here."""
    sc, family = box_pair_zoo()
    o = sc.populate(oracle_mod.create_world(oracle_mod.ORDER_CANONICAL))
    s = sc.settings()
    steps = []
    for _ in range(3):
        o.step_fixed(s, sc.dt, 1)
        con = o.contacts()
        steps.append((o.counts(), contact_set(con), con))
    poses = tuple(a.tobytes() for a in o.physics_transforms())
    n_pairs = len(family)
    assert n_pairs % 256 != 0 and n_pairs > 2 * 256
    counts, _, con = steps[0]
    assert counts["num_broadphase_overlaps"] == n_pairs, "every pair overlaps in its AABBs and no pair touches another"
    nc = 2 * n_pairs
    sizes = manifold_sizes(con)
    per_family = {f: [] for f in FAMILIES}
    for (a, b), k in sizes.items():    # world collider index = nc - 1 - creation index; a pair's colliders are creations 2p and 2p + 1
        pa, pb = (nc - 1 - a) // 2, (nc - 1 - b) // 2
        assert pa == pb, "a manifold between two pairs"
        per_family[family[pa]].append(k)
    total = len(sizes)
    assert total == counts["num_collisions"]
    for k in (1, 2, 3, 4):
        share = sum(v.count(k) for v in per_family.values()) / total
        assert share >= 0.05, f"manifolds with {k} contacts: {share:.3f} of all"
    for f in FAMILIES:
        if f in MISS:
            assert not per_family[f], "the separated pairs must miss"
        else:
            assert len(per_family[f]) >= 40, (f, len(per_family[f]))
    assert set(per_family["edge"]) == {1} and len(per_family["edge"]) == PER_FAMILY
    assert counts["num_collisions"] < counts["num_broadphase_overlaps"]
    cls = ["miss" if f in MISS else "edge" if f in EDGE_CLASS else "face" for f in family]
    for order in (cls, cls[::-1]):
        chunks = [set(order[i:i + 256]) - {"miss"} for i in range(0, n_pairs, 256)]
        assert any(len(ch) == 1 for ch in chunks) and any(len(ch) == 2 for ch in chunks), chunks
    return sc, steps, poses


@pytest.mark.parametrize("stepping", ["speculative", "synchronous"])
def test_gpu_every_class_of_box_pair_matches_oracle(mi_lib, zoo_reference, monkeypatch, stepping):
    if stepping == "synchronous":
        monkeypatch.setenv("MI_ASYNC", "0")
    sc, steps, poses = zoo_reference
    g = sc.populate(mi_lib.create_world(0))
    s = sc.settings()
    for i, (counts, cset, _) in enumerate(steps):
        g.step_fixed(s, sc.dt, 1)
        assert g.counts() == counts, f"step {i}"
        assert contact_set(g.contacts()) == cset, f"step {i}"
    pg, qg = g.physics_transforms()
    assert (pg.tobytes(), qg.tobytes()) == poses


def test_gpu_full_box_queues_match_oracle(mi_lib, oracle_mod):
    sc = full_lattice()
    o = sc.populate(oracle_mod.create_world(oracle_mod.ORDER_CANONICAL))
    g = sc.populate(mi_lib.create_world(0))
    s = sc.settings()
    o.step_fixed(s, sc.dt, 1); g.step_fixed(s, sc.dt, 1)
    co = o.counts()
    assert co["num_collisions"] == co["num_broadphase_overlaps"] and 4500 < co["num_collisions"] < 5500 and co["num_collisions"] % 256 != 0
    sizes = list(manifold_sizes(o.contacts()).values())
    assert sizes.count(1) >= 16 and sizes.count(4) >= 16, "face hits and edge hits in the queues"
    assert g.counts() == co
    assert contact_set(g.contacts()) == contact_set(o.contacts())
    pg, qg = g.physics_transforms(); po, qo = o.physics_transforms()
    assert pg.tobytes() == po.tobytes() and qg.tobytes() == qo.tobytes()
