"""Terrain contact scene queries on the device (mi_world_terrain_contacts*): volumes/s and contacts/s of the device call on the heightmap
of the full-size terrain scene, and the device time of the query's passes.  Prints one JSON line.

    python tools/bench_terrain_contacts.py [--reps 10] [--volumes 16384]

World: scenes.terrain_big()'s heightmap (4 x 4 chunks of 40 m, cells of 31 cm) without its bodies — the query reads the terrain only.
Volumes: all six types in equal parts, sizes 0.3 .. 1.5, random rotations (every second AABB stays one), placed over the whole map
between 0.2 sizes above and one size into the surface.  Device times come from HIP events on the world's stream
(torch.cuda.ExternalStream): `ms` = the whole device call (volume rows, lowest-point pass, count passes, scan, write passes),
`count_only_ms` = the same with capacity 0 (no write passes); their difference is the write passes."""
import argparse
import json

import numpy as np

from query_bench_common import stream_timer
from bench_volume_contacts import mixed_volumes

CAPACITY = 1 << 21   # records (64 MiB); `truncated` says when a workload found more


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--volumes", type=int, default=16384)
    a = ap.parse_args()
    import torch
    torch.cuda.init()
    import d3d12renderer_amd as mi
    from d3d12renderer_amd import capi, scenes
    big = scenes.terrain_big(2, 1, 2)            # (its heightmap does not depend on the body counts)
    sc = scenes.Scene("terrain_only", scenes.make_entities(0), np.zeros(0, np.uint32), scenes.make_colliders(0, capi.SPHERE), 10,
                      hulls=[scenes.convex_hull_mesh(9)], heightmap=big.heightmap)
    w = sc.populate(mi.create_world(0))
    timed = stream_timer(torch.cuda.ExternalStream(w.stream_ptr()), a.reps)
    n = a.volumes
    rng = np.random.default_rng(1)
    hm = big.heightmap
    half = hm["chunks_per_dim"] * hm["chunk_size"] / 2
    host = mixed_volumes(n, (-0.98 * half, 0.0, -0.98 * half), (0.98 * half, 0.0, 0.98 * half), rng, True)
    size = np.where(host["type"] == capi.SPHERE, host["shape"][:, 3], np.where(host["type"] == capi.HULL, 1.0, np.abs(host["shape"][:, 4])))
    for i in range(n):
        host["position"][i, 1] = w.heightmap_height(float(host["position"][i, 0]), float(host["position"][i, 2])) + size[i] * rng.uniform(-1.0, 0.2)
    vols = torch.tensor(np.frombuffer(host.tobytes(), np.uint8).copy(), device="cuda")
    offs = torch.zeros(n + 1, dtype=torch.int32, device="cuda")
    recs = torch.zeros(CAPACITY * 32, dtype=torch.uint8, device="cuda")
    total = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    run = lambda: w.terrain_contacts_device_async(n, vols.data_ptr(), offs.data_ptr(), recs.data_ptr(), CAPACITY, total.data_ptr())   # noqa: E731
    count_only = lambda: w.terrain_contacts_device_async(n, vols.data_ptr(), offs.data_ptr(), 0, 0, total.data_ptr())                   # noqa: E731
    run(); count_only()
    torch.cuda.synchronize()
    ms = timed(run)
    count_ms = timed(count_only)
    contacts = int(total.cpu()[0])
    per = np.diff(offs.cpu().numpy().astype(np.int64))
    res = {"tool": "bench_terrain_contacts", "device": torch.cuda.get_device_name(0), "map": "terrain_big: 4 x 4 chunks of 40 m", "volumes": n,
           "ms": round(ms, 4), "count_only_ms": round(count_ms, 4), "write_passes_ms": round(ms - count_ms, 4),
           "volumes_per_s": round(n / ms * 1e3), "contacts": contacts, "contacts_per_s": round(contacts / ms * 1e3),
           "volumes_touching": int((per > 0).sum()), "volumes_past_the_stash": int((per > 16).sum()), "most_contacts_of_a_volume": int(per.max()),
           "truncated": contacts > CAPACITY}
    w.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
