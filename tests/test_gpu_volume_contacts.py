"""Contact-manifold scene queries on the GPU (mi_world_volume_contacts, ..._device_async, ..._reserve, mi_debug_volume_contacts_exhaustive):
bit for bit against the reference's narrow phase (tests/contact_ref.py: the volumes as rigid bodies of an oracle world, one step), the
accelerated candidates against the exhaustive ones byte for byte, the capacity protocol, the device variant with and without enough
staging, that queries change nothing a step computes and follow every pose change, overlaps, contacts and rays interleaved on one world
(they share the blocking variants' staging), and the sharded world's refusal."""
import ctypes as C

import numpy as np
import pytest

import contact_ref as CR
import overlap_ref as R
import query_helpers as Q

pytestmark = pytest.mark.gpu

RIGID_STATIC, ALL = 3, 31
ERR_CAPACITY, ERR_UNSUPPORTED = -5, -6


def _check_result(offsets, recs, count, what=""):
    """The CSR checks, and of the records: counts 1..4, no flag bits but the volume-was-B one, rows past the count all zero."""
    Q.check_csr(offsets, recs, count, what)
    n = recs["count_flags"] & 7
    assert ((n >= 1) & (n <= 4)).all() and ((recs["count_flags"] & ~np.uint32(0x107)) == 0).all(), what
    unused = np.arange(4)[None, :] >= n[:, None]
    assert (recs["points"].view(np.uint32)[unused] == 0).all(), f"{what}: a row past the contact count is not zero"


def _accel_equals_exhaustive(w, vols, include, ranges=None, what=""):
    return Q.accel_equals_exhaustive(w.volume_contacts, w.debug_volume_contacts_exhaustive, _check_result, vols, include, ranges, what)


# ---- 1. against the reference's narrow phase
@pytest.mark.parametrize("name", ["shape_zoo", "zones"])
@pytest.mark.parametrize("settled", [False, True])
def test_bit_equal_to_the_reference_narrow_phase(mi_lib, oracle_mod, name, settled):
    """The non-reversed (volume, collider) records are exactly the oracle's manifolds, with its bits in the normal, the contact count, every
    point and every depth, the right entity, object type and volume-was-B flag.  No tolerance."""
    sc = R.query_scene(name)
    w = Q.world(mi_lib, sc, 300 if settled else 0)
    ents = Q.bodies(sc)
    states = (ents, w.get_body_states(ents)) if settled else None
    vols = CR.contact_volume_set(name, settled, sc, *w.physics_transforms())
    expected, reversed_pairs, info = CR.oracle_manifolds(oracle_mod, sc, vols, states)
    offsets, recs = w.volume_contacts(vols, include=RIGID_STATIC)
    _check_result(offsets, recs, len(vols), name)
    print(f"{name} settled={settled}: {len(vols)} volumes, {len(recs)} records, {len(expected)} oracle manifolds compared, {info['reversed_manifolds']} reversed; "
          f"per type pair {sorted(info['per_pair'].items())}")
    assert len(expected) > 300
    problems = CR.compare_with_oracle(offsets, recs, expected, reversed_pairs)
    assert not problems, f"{len(problems)} differences:\n" + "\n".join(problems[:12])
    w.close()


# ---- 2. accelerated equals exhaustive
def test_accelerated_equals_exhaustive(mi_lib):
    from d3d12renderer_amd import capi
    rng = np.random.default_rng(15)
    cases = [(R.query_scene("shape_zoo"), 30, (-7, -1, -7), (7, 8, 7)), (R.query_scene("zones"), 30, (-6, -1, -6), (8, 7, 6))]
    for sc, steps, lo, hi in cases:
        w = Q.world(mi_lib, sc, steps)
        vols, n_bad = Q.edge_volumes(rng, lo, hi, True, (24, 6, 2), 8, 4)
        offsets, recs = _accel_equals_exhaustive(w, vols, ALL, what=sc.name)
        counts = np.diff(offsets.astype(np.int64))
        assert (counts[-n_bad:] == 0).all(), f"{sc.name}: an invalid volume reported something"
        assert (counts == 0).any() and counts.max() >= 10, sc.name   # (the giant volumes)
        assert {0, 1} <= set(int(t) for t in recs["object_type"]) and (recs["count_flags"] & 256).any() and not (recs["count_flags"] & 256).all(), sc.name
        if sc.name.startswith("zones"):
            assert {2, 3} <= set(int(t) for t in recs["object_type"]), "triggers and force fields are reported under every include flag"
        n_ent = len(sc.entities)
        lo_e = rng.integers(0, n_ent, len(vols)).astype(np.uint32)
        ranges = np.stack([lo_e, np.minimum(lo_e + rng.integers(1, max(2, n_ent // 4), len(vols)), n_ent)], axis=1).astype(np.uint32)
        ranges[::5] = (0, 0xFFFFFFFF)
        ro, rr = _accel_equals_exhaustive(w, vols, ALL, ranges, what=f"{sc.name} ranges")
        per = ranges[rr["volume"]]
        assert len(rr) and ((rr["entity"] >= per[:, 0]) & (rr["entity"] < per[:, 1])).all(), sc.name
        for include in (0, 1, 2, 4, 8, 16, 24):
            mo, mr = _accel_equals_exhaustive(w, vols[::3], include, what=f"{sc.name} include {include}")
            flags = np.array([1, 2, 16, 8])[mr["object_type"]] if len(mr) else np.zeros(0, int)
            assert ((flags & include) != 0).all(), (sc.name, include)
            if include in (0, 4):   # nothing selected; the terrain flag is accepted and ignored
                assert len(mr) == 0
        w.close()
    # candidate segments beyond the LDS sort bound of the ordered write, out of a walk over few cells
    sc = Q.dense_cluster()
    w = Q.world(mi_lib, sc)
    vols = np.concatenate([capi.box_volume((0.5, 1.0, 0.5), (0.6, 0.6, 0.6)), capi.sphere_volume((0.5, 1.0, 0.5), 0.45), capi.sphere_volume((0.2, 0.8, 0.3), 0.3),
                           capi.box_volume((0.5, 1.0, 0.5), (0.7, 0.7, 0.7), rotation=(0.0, 0.38268343, 0.0, 0.92387953)), capi.sphere_volume((12.0, 1.0, 0.0), 0.2),
                           R.make_volumes(5, 6, (0, 0.5, 0), (1, 1.5, 1), 0.05, 0.5)])
    offsets, recs = _accel_equals_exhaustive(w, vols, ALL, what="dense cluster")
    counts = np.diff(offsets.astype(np.int64))
    assert counts[0] == 3000 and counts[1] > 1024 and 0 < counts[2] <= 1024 and counts[4] == 1, counts[:5]
    w.close()


# ---- 3. capacity protocol
def test_capacity_protocol(mi_lib):
    sc = R.query_scene("shape_zoo")
    w = Q.world(mi_lib, sc, 20)
    vols = CR.contact_volume_set("shape_zoo", False, sc, *CR.start_poses(sc), per_type=16)
    offsets, recs = w.volume_contacts(vols, include=ALL)
    total = len(recs)
    assert total > 50
    for name in ("world_volume_contacts", "debug_volume_contacts_exhaustive"):
        rc, o, r, t = w.volume_contacts_raw(vols, ALL, None, 0, name=name)                # count only
        assert rc == 0 and t == total and o.tobytes() == offsets.tobytes(), name
        rc, o, r, t = w.volume_contacts_raw(vols, ALL, None, total, name=name)            # exact capacity
        assert rc == 0 and t == total and o.tobytes() == offsets.tobytes() and r.tobytes() == recs.tobytes(), name
        slack = 3                                                                          # records of sentinel bytes behind the capacity the call is given
        for cap in (total - 1, total // 2, 1):
            v = np.ascontiguousarray(vols); off = np.zeros(len(v) + 1, np.uint32); tot = C.c_uint32(0)
            buf = np.full((cap + slack) * 96, 0xAB, np.uint8)
            rc = w.L.fn(name)(w.h, C.c_uint32(len(v)), v.ctypes.data_as(C.c_void_p), C.c_uint32(ALL), None, off.ctypes.data_as(C.c_void_p), buf.ctypes.data_as(C.c_void_p),
                              C.c_uint32(cap), C.byref(tot))
            assert rc == ERR_CAPACITY and tot.value == total and off.tobytes() == offsets.tobytes(), (name, cap)
            assert buf[: cap * 96].tobytes() == recs[:cap].tobytes(), (name, cap)
            assert (buf[cap * 96:] == 0xAB).all(), (name, cap)
    w.close()


# ---- 4. device variant
class _Guarded:
    """A device buffer of `nbytes` between two runs of sentinel bytes."""
    PAD = 4096

    def __init__(self, nbytes, torch):
        self.n = nbytes
        self.t = torch.full((nbytes + 2 * self.PAD,), 0xAB, dtype=torch.uint8, device="cuda")
        self.ptr = self.t.data_ptr() + self.PAD
        assert self.ptr % 16 == 0

    def bytes(self):
        return self.t.cpu().numpy()[self.PAD:self.PAD + self.n]

    def intact(self):
        a = self.t.cpu().numpy()
        return bool((a[:self.PAD] == 0xAB).all() and (a[self.PAD + self.n:] == 0xAB).all())


def test_device_variant(mi_lib):
    import torch
    sc = R.query_scene("shape_zoo")
    vols = CR.contact_volume_set("shape_zoo", False, sc, *CR.start_poses(sc), per_type=16)
    ref = Q.world(mi_lib, sc, 10)
    offsets, recs = ref.volume_contacts(vols, include=ALL)
    total = len(recs)
    ref.close()
    assert total > 50
    w = Q.world(mi_lib, sc, 10)
    cap = total + 8
    vols_d = torch.tensor(np.frombuffer(vols.tobytes(), np.uint8).copy(), device="cuda")

    def run(capacity):
        off = _Guarded(4 * (len(vols) + 1), torch); out = _Guarded(96 * capacity, torch); tot = _Guarded(8, torch)
        torch.cuda.synchronize()
        rc = w.volume_contacts_device_async(len(vols), vols_d.data_ptr(), off.ptr, out.ptr, capacity, tot.ptr, include=ALL)
        w.overlap(vols[:1], include=0)   # (a blocking call: synchronises the world's stream)
        assert off.intact() and out.intact() and tot.intact() and (vols_d.cpu().numpy().tobytes() == vols.tobytes())
        return rc, off.bytes().view(np.uint32), out.bytes(), tot.bytes().view(np.uint32)

    rc, o, r, t = run(cap)                                                  # nothing reserved: refused, nothing written
    assert rc == ERR_CAPACITY and (o.view(np.uint8) == 0xAB).all() and (r == 0xAB).all() and (t.view(np.uint8) == 0xAB).all()
    w.volume_contacts_reserve(1 << 16)                                      # ample
    rc, o, r, t = run(cap)
    assert rc == 0 and int(t[0]) == total and int(t[1]) >= int(t[0]) and int(t[1]) < (1 << 16)
    assert o.tobytes() == offsets.tobytes() and r[: 96 * total].tobytes() == recs.tobytes() and (r[96 * total:] == 0xAB).all()
    candidates = int(t[1])
    rc, o, r, t = run(total // 2)                                           # short capacity: the prefix, full offsets and totals
    assert rc == 0 and int(t[0]) == total and int(t[1]) == candidates and o.tobytes() == offsets.tobytes() and r.tobytes() == recs[: total // 2].tobytes()
    w.close()
    # a reservation below the candidates: the first reserved candidates are evaluated, totals[1] still tells the full number
    w = Q.world(mi_lib, sc, 10)
    reserved = candidates // 2
    w.volume_contacts_reserve(reserved)
    rc, o, r, t = run(cap)
    n = int(t[0])
    assert rc == 0 and int(t[1]) == candidates and 0 < n < total
    assert (np.diff(o.astype(np.int64)) >= 0).all() and o[0] == 0 and o[-1] == n and (o <= offsets).all()
    assert r[: 96 * n].tobytes() == recs[:n].tobytes() and (r[96 * n:] == 0xAB).all()
    w.close()


# ---- 5. read-only, and the cache follows the poses
def test_queries_change_nothing_and_follow_the_poses(mi_lib):
    from d3d12renderer_amd import capi
    sc = R.query_scene("shape_zoo")
    a = Q.world(mi_lib, sc); b = Q.world(mi_lib, sc)
    vols = CR.contact_volume_set("shape_zoo", False, sc, *CR.start_poses(sc), per_type=8)
    s = sc.settings()
    ents = Q.bodies(sc)
    previous = None
    for i in range(40):
        a.step_fixed(s, sc.dt, 1); b.step_fixed(s, sc.dt, 1)
        if i % 8 == 0:
            got = _accel_equals_exhaustive(b, vols, ALL, what=f"after step {i + 1}")   # (the exhaustive call reads the poses itself)
            assert previous is None or got[1].tobytes() != previous
            previous = got[1].tobytes()
        else:
            b.volume_contacts(vols, include=ALL)
    assert a.get_body_states(ents).tobytes() == b.get_body_states(ents).tobytes()
    assert a.debug_step_ahead_stats() == b.debug_step_ahead_stats()
    st = b.get_body_states([3]); st[0, :3] = (40.0, 3.0, -35.0); b.set_body_states([3], st)   # far from the grid the last query built
    o, r = _accel_equals_exhaustive(b, np.concatenate([capi.sphere_volume((40.0, 3.0, -35.0), 0.3), vols]), ALL, what="set_body_states")
    assert o[1] == 1 and r["entity"][0] == 3
    # the kernel times of the bench tool: nothing unless stage timing is on
    assert b.debug_volume_contacts_times() == (0.0, 0.0, 0.0)
    b.set_stage_timing(1)
    b.volume_contacts(vols, include=ALL)
    prim, gjk, whole = b.debug_volume_contacts_times()
    assert prim > 0 and gjk > 0 and whole >= prim + gjk
    b.set_stage_timing(0)
    a.close(); b.close()


# ---- 6. one world, every family: the blocking variants share their staging
def test_families_interleaved_on_one_world(mi_lib):
    """Overlaps, contacts and rays in turn on one world, with growing and shrinking volume counts and a call without entity ranges behind one
    with them: a repeated call returns the bytes of its first occurrence, and every call the bytes a fresh world gives for it alone."""
    sc = R.query_scene("shape_zoo")
    full = R.volume_set("shape_zoo", False); small = full[:8]
    assert len(full) == 96
    rng = np.random.default_rng(23)
    o = rng.uniform((-7, -1, -7), (7, 8, 7), (64, 3)).astype(np.float32)
    d = rng.normal(size=(64, 3)); d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    half = len(sc.entities) // 2
    ray_ranges = np.stack([np.zeros(64), np.full(64, half)], axis=1).astype(np.uint32); ray_ranges[::2] += half
    vol_ranges = np.stack([np.zeros(96), np.full(96, half)], axis=1).astype(np.uint32); vol_ranges[1::2] += half
    calls = {"overlap small": lambda w: w.overlap(small, include=ALL),
             "contacts full": lambda w: w.volume_contacts(full, include=ALL),
             "rays ranged": lambda w: (w.raycast(o, d, include=ALL, entity_ranges=ray_ranges),),
             "contacts small": lambda w: w.volume_contacts(small, include=ALL),
             "overlap full ranged": lambda w: w.overlap(full, include=ALL, entity_ranges=vol_ranges)}
    order = ["overlap small", "contacts full", "overlap small", "rays ranged", "contacts small", "overlap full ranged", "contacts full"]

    def run(w, name):
        return tuple(a.tobytes() for a in calls[name](w))

    alone = {}
    for name in calls:
        w = Q.world(mi_lib, sc, 10)
        alone[name] = run(w, name)
        w.close()
    assert len(alone["contacts full"][1]) > 0 and len(alone["overlap full ranged"][1]) > 0, "the full sets report nothing"
    w = Q.world(mi_lib, sc, 10)
    first = {}
    for i, name in enumerate(order):
        got = run(w, name)
        assert got == first.setdefault(name, got), f"call {i} ({name}) differs from its first occurrence"
        assert got == alone[name], f"call {i} ({name}) differs from the same call on a fresh world"
    w.close()


# ---- 7. errors
def test_errors_and_sharded_world(mi_lib):
    from d3d12renderer_amd import capi, scenes, sharding
    sc = scenes.shape_zoo(2, 1, 2)
    w = Q.world(mi_lib, sc)
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    vol = capi.sphere_volume((0, 1, 0), 5.0); off = np.zeros(2, np.uint32); recs = np.zeros(64, capi.volume_contact_dtype); total = C.c_uint32(7)
    u = C.c_uint32
    for name in ("world_volume_contacts", "debug_volume_contacts_exhaustive"):
        f = w.L.fn(name)
        assert f(None, u(1), p(vol), u(ALL), None, p(off), p(recs), u(64), C.byref(total)) == -1
        assert f(w.h, u(1), None, u(ALL), None, p(off), p(recs), u(64), C.byref(total)) == -1
        assert f(w.h, u(1), p(vol), u(ALL), None, p(off), None, u(64), C.byref(total)) == -1
        assert f(w.h, u(0), None, u(ALL), None, p(off), None, u(0), C.byref(total)) == 0 and total.value == 0 and off[0] == 0
        assert f(w.h, u(1), p(vol), u(ALL), None, p(off), p(recs), u(64), C.byref(total)) == 0 and total.value == off[1] >= 4
    o, r = w.volume_contacts(np.zeros(0, capi.query_volume_dtype))
    assert len(o) == 1 and o[0] == 0 and len(r) == 0
    w.close()
    w = Q.world(mi_lib, sc)
    w.shard_enable(sharding._desc_for(sharding.tile_grid(sc, 1), 0))
    for name in ("world_volume_contacts", "debug_volume_contacts_exhaustive"):
        assert w.L.fn(name)(w.h, u(1), p(vol), u(ALL), None, p(off), p(recs), u(64), C.byref(total)) == ERR_UNSUPPORTED
    assert w.L.fn("world_volume_contacts_reserve")(w.h, u(64)) == ERR_UNSUPPORTED
    assert w.L.fn("world_volume_contacts_device_async")(w.h, u(1), p(vol), u(ALL), None, p(off), p(recs), u(64), p(off)) == ERR_UNSUPPORTED
    w.close()
