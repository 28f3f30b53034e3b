"""Shape casts against the heightmap terrain on the device: casts/s of the accelerated path with the terrain alone (include = 4) and with
bodies, static colliders and the terrain (include = 7), and of the exhaustive scan, for ground probes and for long level casts.  Prints one
JSON line.

    python tools/bench_sweep_terrain.py [--settle 120] [--reps 10] [--casts 16384]

Scene: terrain_big (65 536 mixed bodies on a 4 x 4-chunk heightmap of 160 m, cells of 31 cm), stepped until the bodies rest on the hills.
Cast sets: (a) ground probes, an upright capsule of radius 0.4 whose lowest point is 1 m above the surface, moved 2 m down; (b) level casts,
the same capsule moved 20 m in a random horizontal direction, skimming the hills.  Device times come from HIP events on the world's stream
(torch.cuda.ExternalStream); the exhaustive scan runs on 256 of the casts through its blocking call (its copies included), next to the
accelerated blocking call on the same casts, as in tools/bench_sweep.py."""
import argparse
import json

import numpy as np

from query_bench_common import settled_world, stream_timer


def capsules_above(w, n, reach, rng):
    """n upright capsules (segment of 1, radius 0.4) with their lowest point 1 m above the surface, anywhere within `reach` of the map's centre."""
    from d3d12renderer_amd import capi
    xz = rng.uniform(-reach, reach, (n, 2)).astype(np.float32)
    ground = np.array([w.heightmap_height(float(x), float(z)) for x, z in xz], np.float32)
    c = np.stack([xz[:, 0], ground + 1.0 + 0.4 + 0.5, xz[:, 1]], axis=1)
    v = np.zeros(n, dtype=capi.query_volume_dtype)
    v["rotation"][:, 3] = 1.0
    v["type"] = capi.CAPSULE; v["shape"][:, :3] = c - (0, 0.5, 0); v["shape"][:, 3:6] = c + (0, 0.5, 0); v["shape"][:, 6] = 0.4
    return v


def measure(mi, sc, settle, reps, n):
    import torch
    from d3d12renderer_amd import capi
    w, s, st = settled_world(mi, sc, settle)
    timed = stream_timer(st, reps)
    rng = np.random.default_rng(1)
    hm = sc.heightmap
    reach = 0.5 * hm["chunks_per_dim"] * hm["chunk_size"] - 22.0   # (a level cast of 20 m stays on the map)
    out = {"casts": n, "bodies": int(len(sc.entities)), "cell_size": round(hm["chunk_size"] / 128.0, 4)}
    hits = torch.zeros(n * 48, dtype=torch.uint8, device="cuda")
    for name in ("ground_probe", "level_20m"):
        host = capsules_above(w, n, reach, rng)
        disp = np.zeros((n, 4), np.float32)
        if name == "ground_probe":
            disp[:, 1] = -2.0
        else:
            a = rng.uniform(0, 2 * np.pi, n)
            disp[:, 0] = 20.0 * np.cos(a); disp[:, 2] = 20.0 * np.sin(a)
        vols = torch.tensor(np.frombuffer(host.tobytes(), np.uint8).copy(), device="cuda")
        disp_d = torch.tensor(disp, device="cuda")
        torch.cuda.synchronize()
        for include in (capi.QUERY_TERRAIN, capi.QUERY_DEFAULT):
            run = lambda: w.sweep_device_async(n, vols.data_ptr(), disp_d.data_ptr(), hits.data_ptr(), include=include)   # noqa: E731
            run()
            torch.cuda.synchronize()
            ms = timed(run)
            rec = np.frombuffer(hits.cpu().numpy().tobytes(), dtype=capi.sweep_hit_dtype)
            sub, sub_d = host[:256], disp[:256, :3]
            w.debug_sweep_exhaustive(sub, sub_d, include)
            ex_ms = timed(lambda: w.debug_sweep_exhaustive(sub, sub_d, include), 3)
            grid_ms = timed(lambda: w.sweep(sub, sub_d, include), 3)
            out[f"{name}_include_{include}"] = {
                "ms": round(ms, 4), "casts_per_s": round(n / ms * 1e3),
                "hit_share": round(float((rec["entity"] != capi.RAY_MISS).mean()), 3), "terrain_share": round(float((rec["entity"] == capi.RAY_TERRAIN).mean()), 3),
                "initial_overlap_share": round(float(((rec["flags"] & 1) != 0).mean()), 3), "unconverged": int(((rec["flags"] & 2) != 0).sum()),
                "exhaustive_casts_per_s": round(len(sub) / ex_ms * 1e3), "accelerated_same_casts_per_s": round(len(sub) / grid_ms * 1e3),
                "speedup_same_casts": round(ex_ms / grid_ms, 1)}
        if name == "ground_probe":   # what the collider pass alone costs on these casts (include = 3: no terrain launch)
            run = lambda: w.sweep_device_async(n, vols.data_ptr(), disp_d.data_ptr(), hits.data_ptr(), include=3)   # noqa: E731
            run()
            torch.cuda.synchronize()
            out[f"{name}_include_3_ms"] = round(timed(run), 4)
    w.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--settle", type=int, default=120)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--casts", type=int, default=16384)
    a = ap.parse_args()
    import torch
    torch.cuda.init()
    import d3d12renderer_amd as mi
    from d3d12renderer_amd import scenes
    res = {"tool": "bench_sweep_terrain", "device": torch.cuda.get_device_name(0), "settle_steps": a.settle}
    res["terrain_big"] = measure(mi, scenes.terrain_big(), a.settle, a.reps, a.casts)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
