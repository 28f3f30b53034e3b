"""What the query bench tools share (bench_raycast.py, bench_overlap.py, bench_volume_contacts.py): the settled world and the timer of
HIP events on the world's stream."""
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def settled_world(mi, sc, settle):
    """(world after `settle` steps, the step settings, the world's stream as a torch.cuda.ExternalStream)."""
    import torch
    w = sc.populate(mi.create_world(0))
    s = sc.settings()
    w.step_fixed(s, sc.dt, settle)
    return w, s, torch.cuda.ExternalStream(w.stream_ptr())


def stream_timer(stream, reps):
    """timed(fn, n=reps) -> device ms per call of fn, between two events recorded on `stream` around n calls."""
    import torch

    def timed(fn, n=reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        for _ in range(n):
            fn()
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b) / n
    return timed
