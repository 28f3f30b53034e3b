"""What the GPU tests of the scene queries share (tests/test_gpu_raycast.py, test_gpu_overlap.py, test_gpu_volume_contacts.py): the world
builder, the body selector, the CSR checks common to both record types, the accelerated-versus-exhaustive comparison, and the inputs of
that comparison (the dense cluster, the edge volumes).  A plain module: nothing here needs a GPU by itself."""
import numpy as np

import overlap_ref as R
from d3d12renderer_amd import capi, scenes


def world(mi, sc, steps=0):
    w = sc.populate(mi.create_world(0))
    if steps:
        w.step_fixed(sc.settings(), sc.dt, steps)
    return w


def bodies(sc):
    return np.flatnonzero((sc.entities["kind"] == capi.ENTITY_DYNAMIC) | (sc.entities["kind"] == capi.ENTITY_KINEMATIC)).astype(np.uint32)


def check_csr(offsets, recs, count, what=""):
    """CSR shape, the volume column, and every segment strictly ascending in collider index."""
    assert len(offsets) == count + 1 and offsets[0] == 0 and offsets[-1] == len(recs), what
    sizes = np.diff(offsets.astype(np.int64))
    assert (sizes >= 0).all(), what
    assert np.array_equal(recs["volume"], np.repeat(np.arange(count, dtype=np.uint32), sizes)), what
    if len(recs) > 1:
        same = recs["volume"][1:] == recs["volume"][:-1]
        assert (recs["collider"][1:][same] > recs["collider"][:-1][same]).all(), what


def accel_equals_exhaustive(accel_fn, exhaustive_fn, check, vols, include, ranges=None, what=""):
    """accel_fn(vols, include, ranges) gives the bytes of exhaustive_fn(vols, include, ranges), and check(offsets, records, count, what) holds."""
    ao, ar = accel_fn(vols, include, ranges)
    eo, er = exhaustive_fn(vols, include, ranges)
    assert ao.tobytes() == eo.tobytes(), f"{what}: offsets differ (first at {np.flatnonzero(ao != eo)[:4]})"
    if ar.tobytes() != er.tobytes():
        bad = [i for i in range(len(ar)) if ar[i].tobytes() != er[i].tobytes()]
        raise AssertionError(f"{what}: {len(bad)} of {len(ar)} records differ; first {bad[:4]}: {ar[bad[:2]]} vs {er[bad[:2]]}")
    check(ao, ar, len(vols), what)
    return ao, ar


def dense_cluster():
    """3000 static spheres in a unit cube (many per grid cell) and a sparse ring of bodies that keeps the cells small: a volume over the
    cube walks a few hundred cells and reports far more than the LDS sort bound of the ordered write (1024)."""
    rng = np.random.default_rng(77)
    n, m = 3000, 64
    e = np.concatenate([scenes.make_entities(m), scenes.make_entities(n, capi.ENTITY_STATIC)])
    ang = np.linspace(0, 2 * np.pi, m, endpoint=False)
    e["position"][:m] = np.stack([12 * np.cos(ang), np.full(m, 1.0), 12 * np.sin(ang)], axis=1)
    e["position"][m:] = rng.uniform(0.0, 1.0, (n, 3)) + (0, 0.5, 0)
    c = scenes.make_colliders(n + m, capi.SPHERE)
    c["shape"][:, 3] = 0.1
    return scenes.Scene("dense_cluster", e, np.arange(n + m, dtype=np.uint32), c, 10)


def edge_volumes(rng, lo, hi, hull_ok, counts, zero_spheres, zero_boxes):
    """Inside the grid, partly outside, wholly outside (counts = how many of each), larger than the whole grid, zero-radius spheres, zero-size
    boxes, every invalid kind (last).  Returns (volumes, number of invalid ones)."""
    lo = np.asarray(lo, float); hi = np.asarray(hi, float); span = hi - lo
    parts = [R.make_volumes(int(rng.integers(1 << 30)), counts[0], lo, hi, 0.15, 0.04 * float(span.max()) + 1.0),                       # inside
             R.make_volumes(int(rng.integers(1 << 30)), counts[1], lo - 0.1 * span, hi + 0.1 * span, 0.5, 0.3 * float(span.max())),   # partly outside, many cells
             R.make_volumes(int(rng.integers(1 << 30)), counts[2], hi + 2.0 * span, hi + 3.0 * span, 0.5, 3.0)]                          # wholly outside
    big = [capi.sphere_volume((lo + hi) / 2, 4.0 * float(span.max())), capi.box_volume((lo + hi) / 2, 3.0 * span),
           capi.box_volume(lo, 2.5 * span, rotation=(0.1, 0.2, 0.3, 0.9)), capi.capsule_volume(lo - span, hi + span, 0.5 * float(span.max()))]
    zero = [capi.sphere_volume(rng.uniform(lo, hi), 0.0) for _ in range(zero_spheres)] + [capi.box_volume(rng.uniform(lo, hi), (0, 0, 0)) for _ in range(zero_boxes)]
    bad = [capi.sphere_volume((np.nan, 0, 0), 1.0), capi.sphere_volume((0, 1, 0), -1.0), capi.sphere_volume((0, 1, 0), np.inf),
           capi.make_volume(9, [0, 0, 0, 1]), capi.make_volume(0xFF, [0, 0, 0, 1]), capi.hull_volume(99), capi.box_volume((0, 1, 0), (-1, 1, 1)),
           capi.box_volume((0, 1, 0), (1, -1, 1), rotation=(0, 0, 0, 1)), capi.capsule_volume((0, 0, 0), (0, 1, 0), -0.5),
           capi.make_volume(capi.SPHERE, [0, 1, 0, 50.0], position=(np.inf, 0, 0)), capi.make_volume(capi.SPHERE, [0, 1, 0, 50.0], rotation=(0, np.nan, 0, 1)),
           capi.make_volume(capi.SPHERE, [0, 1, 0, 50.0], position=(3e38, 3e38, 0), rotation=(0, 0, 1, 0))]
    vols = np.concatenate(parts + big + zero + bad)
    if not hull_ok:
        vols = vols[vols["type"] != capi.HULL]
    return vols, len([b for b in bad if hull_ok or b["type"][0] != capi.HULL])
