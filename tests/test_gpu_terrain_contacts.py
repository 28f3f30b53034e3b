"""Terrain contact scene queries on the GPU (mi_world_terrain_contacts, ..._device_async): bit for bit and in order against the reference's
heightmapCollision (tests/terrain_contact_ref.py: the volumes as rigid bodies of an oracle world, one step) on two maps, against the step's
own terrain contacts, tiled past the point where a wave of the flag-scanning passes takes several groups of 64 volumes, the capacity
protocol, the device variant between guard bands, that queries change nothing a step computes and follow heightmap edits, all four query
families interleaved on one world, and the error returns."""
import ctypes as C
from dataclasses import replace

import numpy as np
import pytest

import query_helpers as Q
import terrain_contact_ref as T

pytestmark = pytest.mark.gpu

ERR_CAPACITY, ERR_UNSUPPORTED = -5, -6
REC = 32


def _world(mi, hm, bodies=None):
    sc = T.terrain_scene(hm, *(bodies or ()))
    return sc, sc.populate(mi.create_world(0))


def _check_csr(offsets, recs, count):
    assert len(offsets) == count + 1 and offsets[0] == 0 and offsets[-1] == len(recs)
    sizes = np.diff(offsets.astype(np.int64))
    assert (sizes >= 0).all() and sizes.max(initial=0) <= 255
    assert np.array_equal(recs["volume"], np.repeat(np.arange(count, dtype=np.uint32), sizes))


@pytest.fixture(scope="module")
def results(mi_lib):
    """The blocking call's (offsets, records) of both volume sets on a fresh world: computed once, read-only."""
    out = {}
    for name in T.MAPS:
        hm, vols, _ = T.volume_set(name)
        _, w = _world(mi_lib, hm)
        o, r = w.terrain_contacts(vols)
        w.close()
        r = r.copy(); o.setflags(write=False); r.setflags(write=False)
        out[name] = (o, r)
    return out


# ---- 1. against the reference
@pytest.mark.parametrize("name", list(T.MAPS))
def test_bit_equal_to_the_reference(results, oracle_mod, name):
    """Per-volume counts, order and every byte of point, depth and normal are the oracle's.  No tolerance, nothing sorted."""
    hm, vols, _ = T.volume_set(name)
    want_offsets, want_recs, _ = T.expected(oracle_mod, name)
    offsets, recs = results[name]
    _check_csr(offsets, recs, len(vols))
    print(f"{name}: {len(vols)} volumes, {len(recs)} records, oracle {len(want_recs)}")
    assert len(want_recs) > 1000
    problems = T.differences(offsets, recs, want_offsets, want_recs)
    assert not problems, "\n".join(problems)


# ---- 2. the query equals the step
@pytest.mark.parametrize("name", list(T.MAPS))
def test_the_query_equals_the_step(mi_lib, results, name):
    """The same volumes as dynamic bodies of a GPU world, one step: the terrain contacts of mi_world_get_contacts are the query's records as
    multisets of (volume, bytes)."""
    hm, vols, _ = T.volume_set(name)
    sc, w = _world(mi_lib, hm, T.volume_bodies(vols))
    w.step_fixed(sc.settings(), sc.dt, 1)
    c = w.contacts()
    w.close()
    c = c[c["collider_b"] == T.TERRAIN]
    step = np.zeros(len(c), T.capi.terrain_contact_dtype)
    step["point"] = c["point"]; step["depth"] = c["penetration_depth"]; step["normal"] = c["normal"]; step["volume"] = len(vols) - 1 - c["collider_a"]
    _, recs = results[name]
    assert len(step) == len(recs) > 1000
    assert sorted(r.tobytes() for r in step) == sorted(r.tobytes() for r in recs)


# ---- 3. the flag-scanning passes stride
def test_tiled_past_one_group_per_wave(mi_lib, results):
    hm, vols, _ = T.volume_set("coarse")
    small_o, small_r = results["coarse"]
    n = len(vols); per = len(small_r)
    tiles = 131072 // n + 2
    assert tiles * n > 131072
    _, w = _world(mi_lib, hm)
    rc, o, r, total = w.terrain_contacts_raw(np.tile(vols, tiles), tiles * per)
    assert rc == 0 and total == tiles * per
    shifted = (small_o[:-1].astype(np.int64)[None, :] + per * np.arange(tiles)[:, None]).ravel()
    assert np.array_equal(o[:-1], shifted) and o[-1] == total
    r = r.reshape(tiles, per)
    for field in ("point", "depth", "normal"):
        assert (r[field].view(np.uint32) == small_r[field].view(np.uint32)[None]).all(), field
    assert np.array_equal(r["volume"], small_r["volume"][None, :] + (n * np.arange(tiles, dtype=np.uint32))[:, None])
    for count in (0, 1, 5, 65):
        o, r = w.terrain_contacts(vols[:count])
        assert o.tobytes() == small_o[:count + 1].tobytes() and r.tobytes() == small_r[:int(small_o[count])].tobytes(), count
    w.close()


# ---- 4. capacity protocol
def test_capacity_protocol(mi_lib, results):
    hm, vols, _ = T.volume_set("fine")
    offsets, recs = results["fine"]
    total = len(recs)
    _, w = _world(mi_lib, hm)
    rc, o, r, t = w.terrain_contacts_raw(vols, 0)                      # count only
    assert rc == 0 and t == total and o.tobytes() == offsets.tobytes()
    rc, o, r, t = w.terrain_contacts_raw(vols, total)                  # exact capacity
    assert rc == 0 and t == total and o.tobytes() == offsets.tobytes() and r.tobytes() == recs.tobytes()
    sizes = np.diff(offsets.astype(np.int64))
    v = int(np.flatnonzero(sizes >= 3)[0])
    inside = int(offsets[v]) + 1                                        # a cut inside a volume's segment
    assert offsets[v] < inside < offsets[v + 1]
    slack = 3                                                           # records of sentinel bytes behind the capacity the call is given
    f = w.L.fn("world_terrain_contacts")
    for cap in (total - 1, total // 2, 1, inside):
        vv = np.ascontiguousarray(vols); off = np.zeros(len(vv) + 1, np.uint32); tot = C.c_uint32(0)
        buf = np.full((cap + slack) * REC, 0xAB, np.uint8)
        rc = f(w.h, C.c_uint32(len(vv)), vv.ctypes.data_as(C.c_void_p), off.ctypes.data_as(C.c_void_p), buf.ctypes.data_as(C.c_void_p), C.c_uint32(cap), C.byref(tot))
        assert rc == ERR_CAPACITY and tot.value == total and off.tobytes() == offsets.tobytes(), cap
        assert buf[: cap * REC].tobytes() == recs[:cap].tobytes(), cap
        assert (buf[cap * REC:] == 0xAB).all(), cap
    w.close()


# ---- 5. device variant
class _Guarded:
    """A device buffer of `nbytes` between two runs of sentinel bytes."""
    PAD = 4096

    def __init__(self, nbytes, torch, init=None):
        self.n = nbytes
        self.t = torch.full((nbytes + 2 * self.PAD,), 0xAB, dtype=torch.uint8, device="cuda")
        if init is not None:
            self.t[self.PAD:self.PAD + nbytes] = torch.tensor(np.frombuffer(init, np.uint8).copy(), device="cuda")
        self.ptr = self.t.data_ptr() + self.PAD
        assert self.ptr % 16 == 0

    def bytes(self):
        return self.t.cpu().numpy()[self.PAD:self.PAD + self.n]

    def intact(self):
        a = self.t.cpu().numpy()
        return bool((a[:self.PAD] == 0xAB).all() and (a[self.PAD + self.n:] == 0xAB).all())


def test_device_variant(mi_lib, results):
    import torch
    hm, vols, _ = T.volume_set("fine")
    offsets, recs = results["fine"]
    total = len(recs)
    _, w = _world(mi_lib, hm)

    def run(capacity):
        vd = _Guarded(96 * len(vols), torch, vols.tobytes())
        off = _Guarded(4 * (len(vols) + 1), torch); out = _Guarded(REC * capacity, torch); tot = _Guarded(4, torch)
        torch.cuda.synchronize()
        w.terrain_contacts_device_async(len(vols), vd.ptr, off.ptr, out.ptr, capacity, tot.ptr)
        w.overlap(vols[:1], include=0)   # (a blocking call: synchronises the world's stream)
        assert off.intact() and out.intact() and tot.intact() and vd.intact() and vd.bytes().tobytes() == vols.tobytes()
        return off.bytes().view(np.uint32), out.bytes(), int(tot.bytes().view(np.uint32)[0])

    o, r, t = run(total + 8)                                             # ample
    assert t == total and o.tobytes() == offsets.tobytes() and r[: REC * total].tobytes() == recs.tobytes() and (r[REC * total:] == 0xAB).all()
    o, r, t = run(total // 2)                                            # short: the prefix, the full offsets and the full total
    assert t == total and o.tobytes() == offsets.tobytes() and r.tobytes() == recs[: total // 2].tobytes()
    w.close()


# ---- 6. read-only, and current
def test_queries_change_nothing_and_follow_heightmap_edits(mi_lib):
    from d3d12renderer_amd import scenes
    sc = scenes.terrain_field(4, 1, 4)
    vols = T.volume_set("coarse")[1][::4]
    a = Q.world(mi_lib, sc); b = Q.world(mi_lib, sc)
    s = sc.settings(); ents = Q.bodies(sc)
    seen = 0
    for i in range(40):
        a.step_fixed(s, sc.dt, 1); b.step_fixed(s, sc.dt, 1)
        seen += len(b.terrain_contacts(vols)[1])
    assert seen > 0
    assert a.get_body_states(ents).tobytes() == b.get_body_states(ents).tobytes()
    assert a.debug_step_ahead_stats() == b.debug_step_ahead_stats()
    a.close()
    before = b.terrain_contacts(vols)
    # another amplitude
    hm = dict(sc.heightmap); hm["amplitude"] = 5.0
    b.update_heightmap(hm["min_corner"], hm["amplitude"])
    got = b.terrain_contacts(vols)
    fresh = Q.world(mi_lib, replace(sc, heightmap=hm))
    want = fresh.terrain_contacts(vols)
    fresh.close()
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes() and got[1].tobytes() != before[1].tobytes()
    # other heights in one chunk
    chunks = dict(hm["chunks"]); chunks[(0, 1)] = np.ascontiguousarray((chunks[(0, 1)].astype(np.int64) * 7 // 8 + 3000).astype(np.uint16))
    hm2 = dict(hm); hm2["chunks"] = chunks
    b.set_chunk_heights(0, 1, chunks[(0, 1)])
    got2 = b.terrain_contacts(vols)
    fresh = Q.world(mi_lib, replace(sc, heightmap=hm2))
    want2 = fresh.terrain_contacts(vols)
    fresh.close()
    assert got2[0].tobytes() == want2[0].tobytes() and got2[1].tobytes() == want2[1].tobytes() and got2[1].tobytes() != got[1].tobytes()
    b.close()


# ---- 7. one world, every family
def test_families_interleaved_on_one_world(mi_lib):
    from d3d12renderer_amd import scenes
    sc = scenes.terrain_field(4, 1, 4)
    full = T.volume_set("coarse")[1][::2][:96]; small = full[:8]
    full = full[~T.is_invalid(full)]
    rng = np.random.default_rng(23)
    o = rng.uniform((-7, 3, -7), (7, 9, 7), (64, 3)).astype(np.float32)
    d = rng.normal(size=(64, 3)); d[:, 1] = -np.abs(d[:, 1]) - 0.5; d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    calls = {"overlap small": lambda w: w.overlap(small, include=31),
             "terrain full": lambda w: w.terrain_contacts(full),
             "contacts full": lambda w: w.volume_contacts(full, include=31),
             "rays": lambda w: (w.raycast(o, d, include=31),),
             "terrain small": lambda w: w.terrain_contacts(small),
             "overlap full": lambda w: w.overlap(full, include=31)}
    order = ["overlap small", "terrain full", "contacts full", "terrain small", "rays", "terrain full", "overlap full", "terrain small", "contacts full", "terrain full"]

    def run(w, name):
        return tuple(a.tobytes() for a in calls[name](w))

    alone = {}
    for name in calls:
        w = Q.world(mi_lib, sc, 10)
        alone[name] = run(w, name)
        w.close()
    assert len(alone["terrain full"][1]) > 0 and len(alone["terrain small"][1]) > 0, "the terrain sets report nothing"
    w = Q.world(mi_lib, sc, 10)
    first = {}
    for i, name in enumerate(order):
        got = run(w, name)
        assert got == first.setdefault(name, got), f"call {i} ({name}) differs from its first occurrence"
        assert got == alone[name], f"call {i} ({name}) differs from the same call on a fresh world"
    w.close()


# ---- 8. errors
def test_errors_no_heightmap_and_sharded_world(mi_lib):
    from d3d12renderer_amd import capi, scenes, sharding
    hm, vols, _ = T.volume_set("coarse")
    _, w = _world(mi_lib, hm)
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    u = C.c_uint32
    vol = np.ascontiguousarray(vols[:1]); off = np.zeros(2, np.uint32); recs = np.zeros(300, capi.terrain_contact_dtype); total = C.c_uint32(7)
    f = w.L.fn("world_terrain_contacts"); g = w.L.fn("world_terrain_contacts_device_async")
    assert f(None, u(1), p(vol), p(off), p(recs), u(300), C.byref(total)) == -1
    assert f(w.h, u(1), None, p(off), p(recs), u(300), C.byref(total)) == -1
    assert f(w.h, u(1), p(vol), None, p(recs), u(300), C.byref(total)) == -1
    assert f(w.h, u(1), p(vol), p(off), None, u(300), C.byref(total)) == -1
    assert f(w.h, u(1), p(vol), p(off), p(recs), u(300), None) == -1
    assert g(None, u(1), p(vol), p(off), p(recs), u(300), p(off)) == -1
    assert g(w.h, u(1), None, p(off), p(recs), u(300), p(off)) == -1
    assert g(w.h, u(1), p(vol), p(off), p(recs), u(300), None) == -1
    off[0] = 9
    assert f(w.h, u(0), None, p(off), None, u(0), C.byref(total)) == 0 and total.value == 0 and off[0] == 0
    assert f(w.h, u(1), p(vol), p(off), p(recs), u(300), C.byref(total)) == 0 and total.value == off[1]
    o, r = w.terrain_contacts(np.zeros(0, capi.query_volume_dtype))
    assert len(o) == 1 and o[0] == 0 and len(r) == 0
    w.close()
    # a world without a heightmap: all-zero offsets, MI_OK
    sc = scenes.shape_zoo(2, 1, 2)
    w = Q.world(mi_lib, sc)
    rc, o, r, t = w.terrain_contacts_raw(vols[:32], 64, fill=0xAB)
    assert rc == 0 and t == 0 and not o.any() and (r.view(np.uint8) == 0xAB).all()
    w.close()
    # a sharded world: refused by both entry points
    w = Q.world(mi_lib, sc)
    w.shard_enable(sharding._desc_for(sharding.tile_grid(sc, 1), 0))
    assert w.L.fn("world_terrain_contacts")(w.h, u(1), p(vol), p(off), p(recs), u(300), C.byref(total)) == ERR_UNSUPPORTED
    assert w.L.fn("world_terrain_contacts_device_async")(w.h, u(1), p(vol), p(off), p(recs), u(300), p(off)) == ERR_UNSUPPORTED
    w.close()
