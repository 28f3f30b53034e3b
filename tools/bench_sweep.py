"""Shape-cast scene queries on the device: casts/s of the accelerated path and of the exhaustive scan on the headline pile, for two
shapes and two cast lengths.  Prints one JSON line.

    python tools/bench_sweep.py [--settle 30] [--reps 10] [--casts 16384]

Scene: cfg3 (262 144 OBBs on the ground, settled).  Shapes: a capsule of radius 0.5 and a unit box.  Cast lengths: one and sixteen grid
cell sizes (the cell size is read off the pile: the mean collider extent, as the grid build takes it), from above the pile in random
downward directions.  The accelerated path visits the cells under the cast's swept AABB, so the sixteen-cell casts show what a cell walk along
the cast would save.  Device times come from HIP events on the world's stream (torch.cuda.ExternalStream); the exhaustive scan runs on
256 of the casts through its blocking call (its copies included), as in tools/bench_overlap.py."""
import argparse
import json

import numpy as np

from query_bench_common import settled_world, stream_timer


def casts_for(kind, n, lo, hi, length, rng):
    from d3d12renderer_amd import capi
    v = np.zeros(n, dtype=capi.query_volume_dtype)
    v["rotation"][:, 3] = 1.0
    c = rng.uniform(lo, hi, (n, 3)).astype(np.float32)
    if kind == "capsule":
        v["type"] = capi.CAPSULE; v["shape"][:, :3] = c - (0, 0.5, 0); v["shape"][:, 3:6] = c + (0, 0.5, 0); v["shape"][:, 6] = 0.5
    else:
        v["type"] = capi.AABB; v["shape"][:, :3] = c - 0.5; v["shape"][:, 3:6] = c + 0.5
    u = rng.normal(size=(n, 3)); u[:, 1] = -np.abs(u[:, 1])   # downwards: from above the pile into it
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    d = np.zeros((n, 4), np.float32); d[:, :3] = u * length
    return v, d


def measure(mi, sc, settle, reps, n, lo, hi):
    import torch
    from d3d12renderer_amd import capi
    w, s, st = settled_world(mi, sc, settle)
    timed = stream_timer(st, reps)
    rng = np.random.default_rng(1)
    shapes = np.asarray(sc.colliders["shape"], np.float64); types = np.asarray(sc.colliders["type"])
    extent = np.where(types == capi.OBB, 2.0 * np.abs(shapes[:, 7:10]).max(axis=1), (shapes[:, 3:6] - shapes[:, 0:3]).max(axis=1))   # cfg3 holds AABB and OBB colliders
    cell = float(np.mean(extent[extent < 10.0]))   # (without the ground)
    top = float(np.asarray(sc.entities["position"])[:, 1].max()) + 2.0   # the casts start clear of the pile, between 2 and 4 above its highest body centre
    lo, hi = (lo[0], top, lo[2]), (hi[0], top + 2.0, hi[2])
    out = {"casts": n, "cell_size": round(cell, 4), "start_height": round(top, 2)}
    hits = torch.zeros(n * 48, dtype=torch.uint8, device="cuda")
    for kind in ("capsule", "box"):
        for cells in (1, 16):
            host, disp = casts_for(kind, n, lo, hi, cells * cell, rng)
            vols = torch.tensor(np.frombuffer(host.tobytes(), np.uint8).copy(), device="cuda")
            disp_d = torch.tensor(disp, device="cuda")
            torch.cuda.synchronize()
            run = lambda: w.sweep_device_async(n, vols.data_ptr(), disp_d.data_ptr(), hits.data_ptr(), include=capi.QUERY_ALL)   # noqa: E731
            run()
            torch.cuda.synchronize()
            ms = timed(run)
            rec = np.frombuffer(hits.cpu().numpy().tobytes(), dtype=capi.sweep_hit_dtype)
            sub, sub_d = host[:256], disp[:256, :3]
            w.debug_sweep_exhaustive(sub, sub_d, capi.QUERY_ALL)
            ex_ms = timed(lambda: w.debug_sweep_exhaustive(sub, sub_d, capi.QUERY_ALL), 3)
            grid_ms = timed(lambda: w.sweep(sub, sub_d, capi.QUERY_ALL), 3)
            out[f"{kind}_{cells}_cells"] = {
                "length": round(cells * cell, 4), "ms": round(ms, 4), "casts_per_s": round(n / ms * 1e3),
                "hit_share": round(float((rec["entity"] != capi.RAY_MISS).mean()), 3), "initial_overlap_share": round(float(((rec["flags"] & 1) != 0).mean()), 3),
                "unconverged": int(((rec["flags"] & 2) != 0).sum()),
                "exhaustive_casts_per_s": round(len(sub) / ex_ms * 1e3), "accelerated_same_casts_per_s": round(len(sub) / grid_ms * 1e3),
                "speedup_same_casts": round(ex_ms / grid_ms, 1)}
    w.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--settle", type=int, default=30)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--casts", type=int, default=16384)
    a = ap.parse_args()
    import torch
    torch.cuda.init()
    import d3d12renderer_amd as mi
    from d3d12renderer_amd import scenes
    res = {"tool": "bench_sweep", "device": torch.cuda.get_device_name(0), "settle_steps": a.settle}
    res["cfg3_262144"] = measure(mi, scenes.obb_pile(), a.settle, a.reps, a.casts, (-96.0, 0.0, -96.0), (96.0, 0.0, 96.0))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
