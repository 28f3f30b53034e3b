"""Distance scene queries on the device: queries/s of the accelerated path (the shell walk) and of the exhaustive scan, on the settled headline
pile and on the shape zoo, for three largest distances.  Prints one JSON line and writes it to profiles/distance_first_bench.json.

    python tools/bench_distance.py [--settle 30] [--reps 10] [--queries 16384] [--out profiles/distance_first_bench.json]

Scenes: cfg3 (262 144 OBBs on the ground, settled) and shape_zoo (every collider type).  Volumes: spheres of radius 0.25 and unit boxes at random
places in a slab from the ground to a few units above the bodies, so some touch the bodies and some hang clear of them.  Largest distances: one
grid cell size, sixteen, and +inf (the cell size is read off the scene: the mean collider extent, as the grid build takes it).  Device times
come from HIP events on the world's stream (torch.cuda.ExternalStream); the exhaustive scan (a full pair test per collider: nothing is skipped) runs on 64 of the volumes through its blocking
call (its copies included), beside the accelerated path on the same 64, as in tools/bench_sweep.py.  Not part of bench.py; no threshold is
derived from it."""
import argparse
import json
from pathlib import Path

import numpy as np

from query_bench_common import settled_world, stream_timer


def volumes_for(kind, n, lo, hi, rng):
    from d3d12renderer_amd import capi
    v = np.zeros(n, dtype=capi.query_volume_dtype)
    v["rotation"][:, 3] = 1.0
    c = rng.uniform(lo, hi, (n, 3)).astype(np.float32)
    if kind == "sphere":
        v["type"] = capi.SPHERE; v["shape"][:, :3] = c; v["shape"][:, 3] = 0.25
    else:
        v["type"] = capi.AABB; v["shape"][:, :3] = c - 0.5; v["shape"][:, 3:6] = c + 0.5
    return v


def measure(mi, sc, settle, reps, n, lo, hi):
    import torch
    from d3d12renderer_amd import capi
    w, s, st = settled_world(mi, sc, settle)
    timed = stream_timer(st, reps)
    rng = np.random.default_rng(1)
    shapes = np.asarray(sc.colliders["shape"], np.float64); types = np.asarray(sc.colliders["type"])
    extent = np.where(types == capi.OBB, 2.0 * np.abs(shapes[:, 7:10]).max(axis=1), np.where(types == capi.SPHERE, 2.0 * shapes[:, 3], np.abs(shapes[:, 3:6] - shapes[:, 0:3]).max(axis=1)))
    cell = float(np.mean(extent[(extent < 10.0) & (extent > 0.0)]))   # (without the ground)
    top = float(w.physics_transforms()[0][:, 1].max()) + 3.0          # the slab ends 3 above the highest entity
    lo, hi = (lo[0], 0.3, lo[2]), (hi[0], top, hi[2])
    out = {"queries": n, "colliders": int(len(sc.colliders)), "cell_size": round(cell, 4), "slab_top": round(top, 2)}
    hits = torch.zeros(n * 64, dtype=torch.uint8, device="cuda")
    for kind in ("sphere", "box"):
        host = volumes_for(kind, n, lo, hi, rng)
        vols = torch.tensor(np.frombuffer(host.tobytes(), np.uint8).copy(), device="cuda")
        for label, max_d in (("1_cell", cell), ("16_cells", 16.0 * cell), ("inf", np.inf)):
            limits = np.full(n, max_d, np.float32)
            limits_d = torch.tensor(limits, device="cuda")
            torch.cuda.synchronize()
            run = lambda: w.distance_device_async(n, vols.data_ptr(), hits.data_ptr(), max_distances_ptr=limits_d.data_ptr(), include=capi.QUERY_ALL)   # noqa: E731
            run()
            torch.cuda.synchronize()
            ms = timed(run)
            rec = np.frombuffer(hits.cpu().numpy().tobytes(), dtype=capi.distance_hit_dtype)
            sub, sub_l = host[:64], limits[:64]
            w.debug_distance_exhaustive(sub, sub_l, capi.QUERY_ALL)
            ex_ms = timed(lambda: w.debug_distance_exhaustive(sub, sub_l, capi.QUERY_ALL), 3)
            grid_ms = timed(lambda: w.distance(sub, sub_l, capi.QUERY_ALL), 3)
            found = rec["entity"] != capi.RAY_MISS
            out[f"{kind}_{label}"] = {
                "max_distance": None if np.isinf(max_d) else round(float(max_d), 4), "ms": round(ms, 4), "queries_per_s": round(n / ms * 1e3),
                "found_share": round(float(found.mean()), 3), "overlap_share": round(float(((rec["flags"] & 1) != 0).mean()), 3),
                "unconverged": int(((rec["flags"] & 2) != 0).sum()), "mean_distance": round(float(rec["distance"][found].mean()), 4) if found.any() else None,
                "exhaustive_queries_per_s": round(len(sub) / ex_ms * 1e3), "accelerated_same_queries_per_s": round(len(sub) / grid_ms * 1e3),
                "speedup_same_queries": round(ex_ms / grid_ms, 1)}
    w.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--settle", type=int, default=30)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--queries", type=int, default=16384)
    ap.add_argument("--out", default=str(Path(__file__).resolve().parent.parent / "profiles" / "distance_first_bench.json"))
    a = ap.parse_args()
    import torch
    torch.cuda.init()
    import d3d12renderer_amd as mi
    from d3d12renderer_amd import scenes
    res = {"tool": "bench_distance", "device": torch.cuda.get_device_name(0), "settle_steps": a.settle}
    res["cfg3_262144"] = measure(mi, scenes.obb_pile(), a.settle, a.reps, a.queries, (-96.0, 0.0, -96.0), (96.0, 0.0, 96.0))
    res["shape_zoo"] = measure(mi, scenes.shape_zoo(), a.settle, a.reps, a.queries, (-6.0, 0.0, -6.0), (6.0, 0.0, 6.0))
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
