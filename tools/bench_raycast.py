"""Ray-cast scene queries on the device: rays/s, query-structure rebuild, the exhaustive scan as the baseline, and what a batch between
steps costs the stepping.  Prints one JSON line.

    python tools/bench_raycast.py [--settle 30] [--reps 10]

Scenes: cfg3 (262 144 OBBs on the ground, settled) and the 65 536-body terrain scene (scenes.terrain_big).  Device times come from
HIP events on the world's stream (torch.cuda.ExternalStream), the exhaustive scan's included (256 rays, scaled per ray); the steps/s
figures are host wall time."""
import argparse
import json
import time

import numpy as np

from query_bench_common import settled_world, stream_timer


def rays_for(kind, n, lo, hi, rng):
    r = np.zeros((n, 8), np.float32)
    if kind == "down":      # height scan: a square lattice of vertical rays over the scene
        side = int(np.ceil(np.sqrt(n)))
        g = np.linspace(0.0, 1.0, side, dtype=np.float32)
        gx, gz = np.meshgrid(g, g)
        r[:, 0] = (lo[0] + gx.ravel()[:n] * (hi[0] - lo[0]))
        r[:, 2] = (lo[2] + gz.ravel()[:n] * (hi[2] - lo[2]))
        r[:, 1] = hi[1] + 5.0
        r[:, 4] = -1.0
        r[:, 6] = np.inf
    else:                   # random rays of bounded length (10 m) inside the scene's box
        r[:, :3] = rng.uniform(lo, hi, (n, 3))
        d = rng.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
        r[:, 3:6] = d
        r[:, 6] = 10.0
    return r


def measure(mi, sc, settle, reps, lo, hi):
    import torch
    from d3d12renderer_amd import capi
    w, s, st = settled_world(mi, sc, settle)
    timed = stream_timer(st, reps)
    rng = np.random.default_rng(1)

    out = {}
    bufs = {}
    for kind in ("down", "random"):
        for n in (65536, 1048576):
            rays = torch.tensor(rays_for(kind, n, lo, hi, rng), device="cuda")
            hits = torch.zeros(n * capi.ray_hit_dtype.itemsize, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            w.raycast_device_async(n, rays.data_ptr(), hits.data_ptr())
            torch.cuda.synchronize()
            ms = timed(lambda: w.raycast_device_async(n, rays.data_ptr(), hits.data_ptr()))
            h = hits.cpu().numpy().view(capi.ray_hit_dtype)
            out[f"{kind}_{n}"] = {"ms": round(ms, 4), "rays_per_s": round(n / ms * 1e3), "hit_fraction": round(float((h["entity"] != 0xFFFFFFFF).mean()), 4)}
            bufs[(kind, n)] = (rays, hits)
    # rebuild: a one-ray query with and without a new pose epoch (a body state written back unchanged bumps it)
    one, one_out = bufs[("random", 65536)]
    body = torch.tensor(w.entities_to_bodies([0]).astype(np.int32), device="cuda")
    state = torch.tensor(w.get_body_states([0]), device="cuda")
    torch.cuda.synchronize()
    plain = timed(lambda: w.raycast_device_async(1, one.data_ptr(), one_out.data_ptr()))
    w.set_body_states_device_async(1, body.data_ptr(), state.data_ptr())
    torch.cuda.synchronize()

    def rebuilt():
        w.set_body_states_device_async(1, body.data_ptr(), state.data_ptr())
        w.raycast_device_async(1, one.data_ptr(), one_out.data_ptr())
    with_rebuild = timed(rebuilt)
    write_only = timed(lambda: w.set_body_states_device_async(1, body.data_ptr(), state.data_ptr()))
    out["rebuild_ms"] = round(with_rebuild - plain - write_only, 4)
    # exhaustive scan on 256 rays: device time (HIP events on the world's stream around the blocking call: its kernel and the 256 rays' copies,
    # 8 KiB each way), per ray, against the grid per ray at 65 536 rays and against the grid on the same 256 rays (device path, events)
    for kind in ("down", "random"):
        rays_d, hits_d = bufs[(kind, 65536)]
        r = rays_d[:256].cpu().numpy()
        w.debug_raycast_exhaustive(r[:, :3], r[:, 3:6], r[:, 6])
        ex_ms = timed(lambda: w.debug_raycast_exhaustive(r[:, :3], r[:, 3:6], r[:, 6]), 3)
        grid256_ms = timed(lambda: w.raycast_device_async(256, rays_d.data_ptr(), hits_d.data_ptr()))
        grid_ms = out[f"{kind}_65536"]["ms"] / 65536 * 256
        out[f"exhaustive_{kind}_256_ms"] = round(ex_ms, 3)
        out[f"exhaustive_{kind}_rays_per_s"] = round(256 / ex_ms * 1e3)
        out[f"grid_{kind}_256_ms"] = round(grid256_ms, 4)
        out[f"speedup_{kind}_per_ray"] = round(ex_ms / grid_ms, 1)
        out[f"speedup_{kind}_same_256"] = round(ex_ms / grid256_ms, 1)
    # stepping with one 65 536-ray batch between steps
    rays, hits = bufs[("random", 65536)]
    k = 50
    w.step_fixed(s, sc.dt, 5)
    t0 = time.perf_counter(); w.step_fixed(s, sc.dt, k); torch.cuda.synchronize(); plain_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    for _ in range(k):
        w.step_fixed(s, sc.dt, 1)
        w.raycast_device_async(65536, rays.data_ptr(), hits.data_ptr())
    torch.cuda.synchronize(); batch_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    for _ in range(k):
        w.step_fixed(s, sc.dt, 1)
    torch.cuda.synchronize(); single_s = time.perf_counter() - t0
    out["steps_per_s"] = round(k / single_s, 1)
    out["steps_per_s_fixed_n"] = round(k / plain_s, 1)
    out["steps_per_s_with_batch"] = round(k / batch_s, 1)
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
    res = {"tool": "bench_raycast", "device": torch.cuda.get_device_name(0), "settle_steps": a.settle}
    res["cfg3_262144"] = measure(mi, scenes.obb_pile(), a.settle, a.reps, (-96.0, 0.0, -96.0), (96.0, 12.0, 96.0))
    res["terrain_65536"] = measure(mi, scenes.terrain_big(), a.settle, a.reps, (-80.0, 0.0, -80.0), (80.0, 12.0, 80.0))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
