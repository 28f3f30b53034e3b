"""Contact-manifold scene queries on the device (mi_world_volume_contacts*): volumes/s and manifolds/s per scene, the ratio to the
exhaustive call on the same volumes, and the share of the time spent in the GJK kernel.  Prints one JSON line.

    python tools/bench_volume_contacts.py [--settle 30] [--reps 10] [--volumes 16384]

Scenes: cfg3 (262 144 OBBs on the ground, settled) and a shape zoo of 9 216 bodies of all six collider types.  Volumes: all six types
in equal parts (no hulls where the scene has no hull geometry), sizes 0.3 .. 1.5, placed where the bodies are.  Device times of the
device call come from HIP events on the world's stream (torch.cuda.ExternalStream).  The kernel times come from the library's own event
pairs (mi_debug_volume_contacts_times, under set_stage_timing) in one extra call that is not part of the throughput figure.  The
exhaustive ratio compares the two blocking count-only calls on (at most) 256 of the volumes, so that their copies are alike."""
import argparse
import json

import numpy as np

from query_bench_common import settled_world, stream_timer

RESERVE = 1 << 20    # candidates (about 150 MiB of staging); `truncated` says when a workload found more
CAPACITY = 1 << 19   # records (48 MiB)


def mixed_volumes(n, lo, hi, rng, hulls):
    from d3d12renderer_amd import capi
    v = np.zeros(n, dtype=capi.query_volume_dtype)
    types = np.arange(n) % (6 if hulls else 5)
    q = rng.normal(size=(n, 4)); q /= np.linalg.norm(q, axis=1, keepdims=True)
    s = np.exp(rng.uniform(np.log(0.3), np.log(1.5), n))
    v["type"] = types
    v["position"] = rng.uniform(lo, hi, (n, 3))
    v["rotation"] = q
    v["rotation"][(types == capi.AABB) & (np.arange(n) % 12 < 6)] = (0, 0, 0, 1)   # every second AABB stays one; the others become OBBs
    sh = np.zeros((n, 12), np.float32)
    m = types == capi.SPHERE; sh[m, 3] = s[m]
    m = (types == capi.CAPSULE) | (types == capi.CYLINDER); sh[m, 1] = -s[m]; sh[m, 4] = s[m]; sh[m, 6] = 0.5 * s[m]
    m = types == capi.AABB; h = rng.uniform(0.4, 1.0, (n, 3)) * s[:, None]; sh[m, :3] = -h[m]; sh[m, 3:6] = h[m]
    m = types == capi.OBB; sh[m, 3] = 1.0; sh[m, 7:10] = h[m]
    m = types == capi.HULL; sh[m, 3] = 1.0
    v["shape"] = sh
    return v


def measure(mi, sc, settle, reps, n, lo, hi):
    import torch
    from d3d12renderer_amd import capi
    w, _, st = settled_world(mi, sc, settle)
    timed = stream_timer(st, reps)
    rng = np.random.default_rng(1)

    host = mixed_volumes(n, lo, hi, rng, bool(sc.hulls))
    vols = torch.tensor(np.frombuffer(host.tobytes(), np.uint8).copy(), device="cuda")
    offs = torch.zeros(n + 1, dtype=torch.int32, device="cuda")
    recs = torch.zeros(CAPACITY * 96, dtype=torch.uint8, device="cuda")
    totals = torch.zeros(2, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    w.volume_contacts_reserve(RESERVE)
    run = lambda: w.volume_contacts_device_async(n, vols.data_ptr(), offs.data_ptr(), recs.data_ptr(), CAPACITY, totals.data_ptr(), include=capi.QUERY_ALL)   # noqa: E731
    run()
    torch.cuda.synchronize()
    ms = timed(run)
    manifolds, candidates = (int(x) for x in totals.cpu())
    out = {"volumes": n, "ms": round(ms, 4), "volumes_per_s": round(n / ms * 1e3), "manifolds": manifolds, "manifolds_per_s": round(manifolds / ms * 1e3),
           "candidates": candidates, "truncated": candidates > RESERVE or manifolds > CAPACITY}
    w.set_stage_timing(1)
    run()
    prim_ms, gjk_ms, narrow_ms = w.debug_volume_contacts_times()
    w.set_stage_timing(0)
    out.update({"primitive_box_kernel_ms": round(prim_ms, 4), "gjk_kernel_ms": round(gjk_ms, 4), "narrow_and_compaction_ms": round(narrow_ms, 4),
                "gjk_share_of_narrow_and_compaction": round(gjk_ms / narrow_ms, 3) if narrow_ms else None, "gjk_share_of_call": round(gjk_ms / ms, 3)})
    sub = host[:256]
    w.volume_contacts_raw(sub, capi.QUERY_ALL, None, 0, name="debug_volume_contacts_exhaustive")
    ex_ms = timed(lambda: w.volume_contacts_raw(sub, capi.QUERY_ALL, None, 0, name="debug_volume_contacts_exhaustive"), 3)
    grid_ms = timed(lambda: w.volume_contacts_raw(sub, capi.QUERY_ALL, None, 0), 3)
    out.update({"exhaustive_ms_per_volume": round(ex_ms / len(sub), 5), "grid_same_volumes_ms_per_volume": round(grid_ms / len(sub), 5),
                "speedup_same_volumes": round(ex_ms / grid_ms, 1), "speedup_per_volume_in_batch": round((ex_ms / len(sub)) / (ms / n), 1)})
    w.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--settle", type=int, default=30)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--volumes", type=int, default=16384)
    a = ap.parse_args()
    import torch
    torch.cuda.init()
    import d3d12renderer_amd as mi
    from d3d12renderer_amd import scenes
    res = {"tool": "bench_volume_contacts", "device": torch.cuda.get_device_name(0), "settle_steps": a.settle}
    res["cfg3_262144"] = measure(mi, scenes.obb_pile(), a.settle, a.reps, a.volumes, (-96.0, 0.0, -96.0), (96.0, 12.0, 96.0))
    res["shape_zoo_9216"] = measure(mi, scenes.shape_zoo(48, 4, 48), a.settle, a.reps, a.volumes, (-38.0, 0.0, -38.0), (38.0, 7.0, 38.0))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
