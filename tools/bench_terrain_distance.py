"""Terrain distance queries on the device: queries/s of ground-clearance probes through the accelerated ring walk (k_q_terrain_distance) and through
the exhaustive scan of the same build, for a largest distance of one cell, sixteen cells and +inf.  Prints one JSON line and writes it to
profiles/terrain_distance_bench.json (--out).

    python tools/bench_terrain_distance.py [--reps 10] [--queries 16384] [--out profiles/terrain_distance_bench.json]

Scene: the heightmap of terrain_big (4 x 4 chunks, 160 m, cells of 31 cm); the bodies play no part, the call is the terrain's alone.
Probe sets: (a) an upright capsule of radius 0.4 (a foot), its lowest point 0.2 to 3 m above the surface; (b) a box of 1.6 x 0.6 x 3.0 (a
chassis) turned about y, its centre 0.5 to 3.5 m above the surface.  Device times come from HIP events on the world's stream
(torch.cuda.ExternalStream); the exhaustive scan runs on 256 of the probes through its blocking call (its copies included), next to the
accelerated blocking call on the same probes, as in tools/bench_sweep_terrain.py.  Also timed: mi_world_distance followed by the merging
call (the nearest of anything) against mi_world_distance alone, on the world without bodies near the probes."""
import argparse
import json
from pathlib import Path

import numpy as np

from query_bench_common import settled_world, stream_timer


def probes(w, n, reach, rng, kind):
    from d3d12renderer_amd import capi, scenes
    xz = rng.uniform(-reach, reach, (n, 2)).astype(np.float32)
    ground = np.array([w.heightmap_height(float(x), float(z)) for x, z in xz], np.float32)
    v = np.zeros(n, dtype=capi.query_volume_dtype)
    v["rotation"][:, 3] = 1.0
    if kind == "capsule":
        c = np.stack([xz[:, 0], ground + rng.uniform(0.2, 3.0, n).astype(np.float32) + 0.4 + 0.5, xz[:, 1]], axis=1)
        v["type"] = capi.CAPSULE; v["shape"][:, :3] = c - (0, 0.5, 0); v["shape"][:, 3:6] = c + (0, 0.5, 0); v["shape"][:, 6] = 0.4
    else:
        v["type"] = capi.AABB; v["shape"][:, :6] = (-0.8, -0.3, -1.5, 0.8, 0.3, 1.5)
        v["position"] = np.stack([xz[:, 0], ground + rng.uniform(0.5, 3.5, n).astype(np.float32), xz[:, 1]], axis=1)
        v["rotation"] = np.stack([scenes.q_axis_angle((0, 1, 0), a) for a in rng.uniform(0, 2 * np.pi, n)]).astype(np.float32)
    return v


def measure(mi, sc, reps, n):
    import torch
    from d3d12renderer_amd import capi
    w, s, st = settled_world(mi, sc, 1)
    timed = stream_timer(st, reps)
    rng = np.random.default_rng(1)
    hm = sc.heightmap
    cell = hm["chunk_size"] / 128.0
    reach = 0.5 * hm["chunks_per_dim"] * hm["chunk_size"] - 4.0
    out = {"queries": n, "cell_size": round(cell, 4), "chunks_per_dim": int(hm["chunks_per_dim"])}
    recs = torch.zeros(n * 64, dtype=torch.uint8, device="cuda")
    for kind in ("capsule", "box"):
        host = probes(w, n, reach, rng, kind)
        vols = torch.tensor(np.frombuffer(host.tobytes(), np.uint8).copy(), device="cuda")
        for label, max_d in (("one_cell", cell), ("sixteen_cells", 16 * cell), ("inf", np.inf)):
            m_host = np.full(n, max_d, np.float32)
            m_dev = torch.tensor(m_host, device="cuda")
            torch.cuda.synchronize()
            run = lambda: w.terrain_distance_device_async(n, vols.data_ptr(), recs.data_ptr(), max_distances_ptr=m_dev.data_ptr())   # noqa: E731
            run()
            torch.cuda.synchronize()
            ms = timed(run)
            rec = np.frombuffer(recs.cpu().numpy().tobytes(), dtype=capi.distance_hit_dtype)
            sub, sub_m = host[:256], m_host[:256]
            ex = w.debug_terrain_distance_exhaustive(sub, sub_m)
            assert ex.tobytes() == rec[:256].tobytes(), "the accelerated records differ from the exhaustive ones"
            ex_ms = timed(lambda: w.debug_terrain_distance_exhaustive(sub, sub_m), 3)
            acc_ms = timed(lambda: w.terrain_distance(sub, sub_m), 3)
            hit = rec["entity"] != capi.RAY_MISS
            out[f"{kind}_{label}"] = {
                "ms": round(ms, 4), "queries_per_s": round(n / ms * 1e3), "hit_share": round(float(hit.mean()), 3),
                "overlap_share": round(float(((rec["flags"] & 1) != 0).mean()), 3), "unconverged": int(((rec["flags"] & 2) != 0).sum()),
                "mean_distance": round(float(rec["distance"][hit].mean()), 3) if hit.any() else None,
                "exhaustive_queries_per_s": round(len(sub) / ex_ms * 1e3), "accelerated_same_queries_per_s": round(len(sub) / acc_ms * 1e3),
                "speedup_same_queries": round(ex_ms / acc_ms, 1)}
        # the two-call pattern on the same probes: the colliders' records, then the terrain merged into them
        alone = lambda: w.distance_device_async(n, vols.data_ptr(), recs.data_ptr(), include=capi.QUERY_DEFAULT)   # noqa: E731

        def both():
            alone()
            w.terrain_distance_device_async(n, vols.data_ptr(), recs.data_ptr(), merge=1)
        both()
        torch.cuda.synchronize()
        out[f"{kind}_distance_alone_ms"] = round(timed(alone), 4)
        out[f"{kind}_distance_then_terrain_merged_ms"] = round(timed(both), 4)
    w.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--queries", type=int, default=16384)
    ap.add_argument("--out", default=str(Path(__file__).resolve().parent.parent / "profiles" / "terrain_distance_bench.json"))
    a = ap.parse_args()
    import torch
    torch.cuda.init()
    import d3d12renderer_amd as mi
    from d3d12renderer_amd import scenes
    sc = scenes.terrain_big(8, 1, 8)     # (the heightmap of terrain_big under a handful of bodies: the query reads the terrain alone)
    res = {"tool": "bench_terrain_distance", "device": torch.cuda.get_device_name(0)}
    res["terrain_big"] = measure(mi, sc, a.reps, a.queries)
    line = json.dumps(res)
    Path(a.out).write_text(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
