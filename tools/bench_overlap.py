"""Volume-overlap scene queries on the device: volumes/s and records/s per workload, the exhaustive scan as the baseline, the
query-structure rebuild (shared with the ray casts), and what a batch between steps costs the stepping.  Prints one JSON line.

    python tools/bench_overlap.py [--settle 30] [--reps 10]

Scenes: cfg3 (262 144 OBBs on the ground, settled) and the 65 536-body terrain scene (scenes.terrain_big).  Workloads: small spheres
(about one grid cell), medium boxes (about 4 x 4 x 4 cells), a few large spheres (they stride over all colliders).  Device times come
from HIP events on the world's stream (torch.cuda.ExternalStream), the exhaustive scan's included (its volumes' copies too); the
steps/s figures are host wall time.  `count_pass_share` = the blocking count-only call over the blocking full call on the same
volumes: how much of a query is the first of the two passes that both run the predicate."""
import argparse
import json
import time

import numpy as np

from query_bench_common import settled_world, stream_timer

CAPACITY = 1 << 22   # records (64 MiB); `truncated` says when a workload needed more


def volumes_for(kind, n, lo, hi, rng):
    from d3d12renderer_amd import capi
    v = np.zeros(n, dtype=capi.query_volume_dtype)
    v["rotation"][:, 3] = 1.0
    c = rng.uniform(lo, hi, (n, 3)).astype(np.float32)
    if kind == "small_spheres":
        v["type"] = capi.SPHERE; v["shape"][:, :3] = c; v["shape"][:, 3] = 0.5
    elif kind == "medium_boxes":
        v["type"] = capi.AABB; v["shape"][:, :3] = c - 2.0; v["shape"][:, 3:6] = c + 2.0
    else:
        v["type"] = capi.SPHERE; v["shape"][:, :3] = c; v["shape"][:, 3] = 30.0
    return v


def measure(mi, sc, settle, reps, lo, hi):
    import torch
    from d3d12renderer_amd import capi
    w, s, st = settled_world(mi, sc, settle)
    timed = stream_timer(st, reps)
    rng = np.random.default_rng(1)

    hits = torch.zeros(CAPACITY * 16, dtype=torch.uint8, device="cuda")
    total = torch.zeros(1, dtype=torch.int32, device="cuda")
    out = {}
    bufs = {}
    for kind, n in (("small_spheres", 65536), ("medium_boxes", 16384), ("large_spheres", 64)):
        host = volumes_for(kind, n, lo, hi, rng)
        vols = torch.tensor(np.frombuffer(host.tobytes(), np.uint8).copy(), device="cuda")
        offs = torch.zeros(n + 1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        run = lambda: w.overlap_device_async(n, vols.data_ptr(), offs.data_ptr(), hits.data_ptr(), CAPACITY, total.data_ptr(), include=capi.QUERY_ALL)   # noqa: E731
        run()
        torch.cuda.synchronize()
        ms = timed(run)
        records = int(total.cpu()[0])
        out[kind] = {"volumes": n, "ms": round(ms, 4), "volumes_per_s": round(n / ms * 1e3), "records": records, "records_per_s": round(records / ms * 1e3),
                     "truncated": records > CAPACITY}
        # the exhaustive scan on (at most) 256 of them, and the grid on the same ones; both blocking calls, count-only, so that the copies are alike
        sub = host[:256]
        w.overlap_raw(sub, capi.QUERY_ALL, None, 0, name="debug_overlap_exhaustive")
        ex_ms = timed(lambda: w.overlap_raw(sub, capi.QUERY_ALL, None, 0, name="debug_overlap_exhaustive"), 3)
        grid_ms = timed(lambda: w.overlap_raw(sub, capi.QUERY_ALL, None, 0), 3)
        out[kind]["exhaustive_ms_per_volume"] = round(ex_ms / len(sub), 5)
        out[kind]["grid_same_volumes_ms_per_volume"] = round(grid_ms / len(sub), 5)
        out[kind]["speedup_same_volumes"] = round(ex_ms / grid_ms, 1)
        out[kind]["speedup_per_volume_in_batch"] = round((ex_ms / len(sub)) / (ms / n), 1)
        # count pass against both passes (blocking calls on up to 4096 volumes, capacity for everything)
        part = host[:4096]
        full_ms = timed(lambda: w.overlap_raw(part, capi.QUERY_ALL, None, CAPACITY // 4), 3)
        count_ms = timed(lambda: w.overlap_raw(part, capi.QUERY_ALL, None, 0), 3)
        out[kind]["count_pass_share"] = round(count_ms / full_ms, 3)
        bufs[kind] = (n, vols, offs)
    # rebuild: a one-volume query with and without a new pose epoch (a body state written back unchanged bumps it)
    n1, vols, offs = bufs["small_spheres"]
    body = torch.tensor(w.entities_to_bodies([0]).astype(np.int32), device="cuda")
    state = torch.tensor(w.get_body_states([0]), device="cuda")
    torch.cuda.synchronize()
    one = lambda: w.overlap_device_async(1, vols.data_ptr(), offs.data_ptr(), hits.data_ptr(), CAPACITY, total.data_ptr(), include=capi.QUERY_ALL)   # noqa: E731
    plain = timed(one)
    w.set_body_states_device_async(1, body.data_ptr(), state.data_ptr())
    torch.cuda.synchronize()

    def rebuilt():
        w.set_body_states_device_async(1, body.data_ptr(), state.data_ptr())
        one()
    with_rebuild = timed(rebuilt)
    write_only = timed(lambda: w.set_body_states_device_async(1, body.data_ptr(), state.data_ptr()))
    out["one_volume_query_ms"] = round(plain, 4)
    out["rebuild_ms"] = round(with_rebuild - plain - write_only, 4)
    # stepping with one batch of 16 384 medium boxes between steps
    n, vols, offs = bufs["medium_boxes"]
    k = 50
    w.step_fixed(s, sc.dt, 5)
    t0 = time.perf_counter(); w.step_fixed(s, sc.dt, k); torch.cuda.synchronize(); plain_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    for _ in range(k):
        w.step_fixed(s, sc.dt, 1)
        w.overlap_device_async(n, vols.data_ptr(), offs.data_ptr(), hits.data_ptr(), CAPACITY, total.data_ptr(), include=capi.QUERY_ALL)
    torch.cuda.synchronize(); batch_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    for _ in range(k):
        w.step_fixed(s, sc.dt, 1)
    torch.cuda.synchronize(); single_s = time.perf_counter() - t0
    out["steps_per_s"] = round(k / single_s, 1)
    out["steps_per_s_fixed_n"] = round(k / plain_s, 1)
    out["steps_per_s_with_batch"] = round(k / batch_s, 1)
    out["batch_cost_ms_per_step"] = round((batch_s - single_s) / k * 1e3, 4)
    w.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--settle", type=int, default=30)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    import torch
    torch.cuda.init()
    import d3d12renderer_amd as mi
    from d3d12renderer_amd import scenes
    res = {"tool": "bench_overlap", "device": torch.cuda.get_device_name(0), "settle_steps": a.settle}
    res["cfg3_262144"] = measure(mi, scenes.obb_pile(), a.settle, a.reps, (-96.0, 0.0, -96.0), (96.0, 12.0, 96.0))
    res["terrain_65536"] = measure(mi, scenes.terrain_big(), a.settle, a.reps, (-80.0, 0.0, -80.0), (80.0, 12.0, 80.0))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
