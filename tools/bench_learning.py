"""Batched learning environments: the host path (updatePhysicsBatch: numpy in, numpy out) against the device-resident path
(updatePhysicsBatchDevice: torch tensors in and out) — ms per step and env-steps/s at 256, 4 096 and 16 384 environments, and the
host path's own phase breakdown (MI_LEARN_PROFILE).  Prints one JSON line; --out also writes it to a file.

    python tools/bench_learning.py [--envs 256,4096,16384] [--steps 100] [--rounds 3] [--out profiles/learning_device_first_bench.json]

Both paths run in this one process on one GPU, alternating (host window, device window, host window, ...), each window behind a
warm-up of the same length, every window's time kept: the spread between windows of one path is what a difference between the paths
has to be read against.  Times are host wall time around calls that return with the world's stream idle.  The actions are those of
tools/gpu_learning.sh (8 seeded batches, cycled); the device path holds them as torch tensors.  The yardstick is the host path as it
runs here, not a recorded number."""
import argparse
import json
import os
import re
import sys
import tempfile
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
os.environ["MI_LEARN_PROFILE"] = "1"   # read once when the library is loaded: one line on stderr per 100 host steps

import numpy as np  # noqa: E402

PHASES = ("actions", "pushes", "physics", "readback", "state+reward", "resets")


class StderrCapture:
    """The library prints its phase lines with fprintf(stderr): file descriptor 2 goes to a temporary file for the duration."""

    def __enter__(self):
        sys.stderr.flush()
        self.tmp = tempfile.TemporaryFile(mode="w+b")
        self.saved = os.dup(2)
        os.dup2(self.tmp.fileno(), 2)
        return self

    def __exit__(self, *exc):
        os.dup2(self.saved, 2); os.close(self.saved)
        self.tmp.seek(0)
        self.text = self.tmp.read().decode(errors="replace")
        self.tmp.close()

    def phases(self):
        lines = [ln for ln in self.text.splitlines() if ln.startswith("[learning] per step (ms):")]
        if not lines:
            return None
        vals = re.findall(r"([a-z+]+) ([0-9.]+)", lines[-1].split(":", 1)[1])
        return {k: float(v) for k, v in vals}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", default="256,4096,16384")
    ap.add_argument("--steps", type=int, default=100, help="steps per window (the phase breakdown is printed per 100 host steps: keep it a multiple)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_learning.py needs a GPU: nothing is measured without one")
    torch.cuda.init()
    from d3d12renderer_amd.learning import PhysicsDLL
    d = PhysicsDLL(); d.seed(1)
    _, _, amin, amax = d.ranges()
    result = {"steps_per_window": args.steps, "rounds": args.rounds, "device": torch.cuda.get_device_name(0), "envs": {}}
    for n in [int(x) for x in args.envs.split(",")]:
        d.shutdown()
        rng = np.random.default_rng(0)
        acts = [(rng.uniform(-1, 1, (n, 27)) * 0.15 * (amax - amin)).astype(np.float32) for _ in range(8)]
        dev_acts = [torch.from_numpy(a).cuda() for a in acts]
        torch.cuda.synchronize()
        host_ms, dev_ms, host_resets, dev_resets, phases = [], [], 0, 0, []
        for _ in range(args.rounds):
            with StderrCapture() as cap:
                d.reset_batch(n)
                for i in range(args.steps):
                    d.step_batch(acts[i % 8])
                t0 = time.perf_counter()
                flags = [d.step_batch(acts[i % 8])[2] for i in range(args.steps)]
                host_ms.append((time.perf_counter() - t0) / args.steps * 1e3)
                host_resets += int(np.sum(flags))
            if cap.phases():
                phases.append(cap.phases())
            d.reset_batch_device(n)
            for i in range(args.steps):
                d.step_batch_device(dev_acts[i % 8])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            flags = []
            for i in range(args.steps):
                flags.append(d.step_batch_device(dev_acts[i % 8])[2])
            torch.cuda.synchronize()
            dev_ms.append((time.perf_counter() - t0) / args.steps * 1e3)
            dev_resets += int(torch.stack(flags).sum().item())   # (counted outside the timed window)
        h, v = float(np.median(host_ms)), float(np.median(dev_ms))
        result["envs"][str(n)] = {
            "host": {"ms_per_step": round(h, 4), "env_steps_per_s": round(n / h * 1e3), "windows_ms": [round(x, 4) for x in host_ms], "resets": host_resets,
                     "phases_ms": {k: round(float(np.median([p[k] for p in phases])), 4) for k in PHASES} if phases else None},
            "device": {"ms_per_step": round(v, 4), "env_steps_per_s": round(n / v * 1e3), "windows_ms": [round(x, 4) for x in dev_ms], "resets": dev_resets},
            "host_over_device": round(h / v, 3),
        }
        print(f"# {n}: host {h:.3f} ms/step, device {v:.3f} ms/step, ratio {h / v:.2f}", file=sys.stderr, flush=True)
    d.shutdown()
    line = json.dumps(result)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
