"""The ray cast against the heightmap terrain on the GPU, at its hard rays (tests/raycast_terrain_matrix.py), against the float64 reference of
the whole triangulated surface: one world per map, one call per family and map, every kept case without a budget.  Per case: the reference's
decision; entity = collider = the terrain's value (capi.RAY_TERRAIN) and a static object type; |t - t_ref| |d|, the point's distance from o + t d and from the surface,
and the normal's distance from the normal of a triangle that holds the reference's hit within delta, each within BOUNDS[family] x scale; a unit
normal.  Per call: the exhaustive kernel's bytes; misses all-zero with t = +inf.  The whole set again as one call per map and as calls of 1 and
65 rays (a partial workgroup)."""
import numpy as np
import pytest

import query_helpers as Q
import raycast_terrain_matrix as M

pytestmark = pytest.mark.gpu

MISS, TERRAIN, STATIC = 0xFFFFFFFF, 0xFFFFFFFE, 1
TERRAIN_ONLY, TERRAIN_AND_STATIC = 4, 6   # capi.QUERY_TERRAIN alone, and with capi.QUERY_STATIC: the `ordering` family's spheres


@pytest.fixture(scope="module")
def worlds(mi_lib):
    ws = {name: Q.world(mi_lib, M.scene(name)) for name in M.MAPS}
    yield ws
    for w in ws.values():
        w.close()


def _same_bytes(a, b, what):
    assert a.dtype == b.dtype and len(a) == len(b)
    bad = [i for i in range(len(a)) if a[i].tobytes() != b[i].tobytes()]
    assert not bad, f"{what}: {len(bad)} of {len(a)} records differ between the two kernels; first {bad[:4]}: {a[bad[:2]]} vs {b[bad[:2]]}"


def _call(w, cases, include, what):
    o, d = np.stack([c["o32"] for c in cases]), np.stack([c["d32"] for c in cases])
    max_t = np.array([c["max_t32"] for c in cases], np.float32)
    got = w.raycast(o, d, max_t=max_t, include=include)
    _same_bytes(got, w.debug_raycast_exhaustive(o, d, max_t=max_t, include=include), what)
    return got


def _is_miss_record(rec):
    return (rec["entity"] == MISS and rec["collider"] == MISS and np.isposinf(rec["t"]) and not rec["point"].any() and not rec["normal"].any()
            and rec["object_type"] == 0)


def _check(cases, got, worst):
    """Every record against the reference's answer of its case; returns (wrong decisions, other failures) and raises worst[family] to the largest
    measure per unit of scale: |dt| |d|, the point off o + t d, the point off the surface, the normal off the admissible ones."""
    leaks, bad = [], []
    spheres = len(M.family("ordering"))
    for c, rec in zip(cases, got):
        m, name = M.the_map(c["map"]), c["family"]
        who = f"{name} {c['map']} {c['tag']} (scale {c['scale']:.4g}, |d| {np.linalg.norm(c['d']):.3g})"
        if (rec["entity"] == MISS) == (c["t"] is not None):
            leaks.append(f"{who}: decision: the GPU {'misses' if rec['entity'] == MISS else 'hits at t = %.8g' % rec['t']}, the reference "
                         f"{'misses' if c['t'] is None else 'hits at t = %.8g' % c['t']}")
            continue
        if c["t"] is None:
            if not _is_miss_record(rec):
                bad.append(f"{who}: a miss record that is not all-miss: {rec}")
            continue
        bound, length = M.BOUNDS[name] * c["scale"], float(np.linalg.norm(c["d"]))
        t, p, n = float(rec["t"]), rec["point"].astype(np.float64), rec["normal"].astype(np.float64)
        if c.get("sphere_wins"):
            ent, dt = c["sphere"], abs(t - c["sphere_t"]) * length
            worst[name] = max(worst.get(name, 0.0), dt / c["scale"])   # (the sphere's entry is part of this family's measure: delta has to clear it)
            if rec["entity"] != ent or rec["collider"] != spheres - 1 - ent or rec["object_type"] != STATIC or dt > bound:
                bad.append(f"{who}: the sphere {ent} in front of the terrain, entry {c['sphere_t']:.8g}: got {rec}")
            continue
        if rec["entity"] != TERRAIN or rec["collider"] != TERRAIN or rec["object_type"] != STATIC:
            bad.append(f"{who}: entity {rec['entity']:#x}, collider {rec['collider']:#x}, object type {rec['object_type']}")
            continue
        if abs(np.linalg.norm(n) - 1) > 1e-5:
            bad.append(f"{who}: |n| - 1 = {np.linalg.norm(n) - 1:.2e}")
        if c.get("on_surface"):   # the origin on the surface: t = 0, the origin itself, -normalize(d)
            if t != 0 or not (rec["point"] == c["o32"]).all() or not np.allclose(n, -c["d"] / length, atol=1e-6):
                bad.append(f"{who}: the origin is on the surface: expected t = 0, the origin and -normalize(d); got t = {t:.6g}, point {p}, normal {n}")
            continue
        dl = M.delta(c)
        dt = abs(t - c["t"]) * length
        dp = float(np.linalg.norm(p - (c["o"] + t * c["d"])))
        under = m.holders(p, dl)
        ds = min((abs((p - m.a[k]) @ m.normal[k]) for k in under), default=np.inf)
        dn = min(float(np.linalg.norm(n - m.normal[k])) for k in m.holders(c["point"], dl))
        worst[name] = max(worst.get(name, 0.0), max(dt, dp, ds, dn) / c["scale"])
        if dt > bound:
            bad.append(f"{who}: |t - t_ref| |d| = {dt:.3e} > {bound:.3e} (t = {t:.9g}, the reference {c['t']:.9g})")
        if dp > bound or ds > bound:
            bad.append(f"{who}: the point lies {dp:.3e} off o + t d and {ds:.3e} off the surface (bound {bound:.3e})")
        if dn > bound:
            bad.append(f"{who}: normal {n}: {dn:.3e} off the normals of the triangles at the reference's hit (bound {bound:.3e})")
    return leaks, bad


def _report(leaks, bad, count):
    assert not leaks and not bad, (f"{len(leaks)} wrong decisions and {len(bad)} other failures in {count} cases:\n" + "\n".join(leaks + bad))


@pytest.mark.parametrize("name", M.FAMILIES)
def test_family(worlds, name):
    """One family, one call per map it uses."""
    kept, worst = M.kept(name), {}
    leaks, bad = [], []
    for mapname in M.MAPS:
        cases = [c for c in kept if c["map"] == mapname]
        if cases:
            got = _call(worlds[mapname], cases, TERRAIN_AND_STATIC if name == "ordering" else TERRAIN_ONLY, f"{name} on {mapname}")
            more = _check(cases, got, worst)
            leaks += more[0]; bad += more[1]
    print(f"{name}: {len(M.family(name))} generated, {len(kept)} kept, {len(leaks)} wrong decisions; the largest measure per unit of scale "
          f"{worst.get(name, 0.0):.2e} (bound {M.BOUNDS[name]:.0e})")
    _report(leaks, bad, len(kept))


def test_whole_set_in_one_call_and_in_small_calls(worlds):
    """Every kept case of a map in one call (`ordering` apart: its spheres would stand in the other families' rays), held to the same checks; then
    the first ray alone and the first 65, which must give the records the large call gave."""
    leaks, bad, count = [], [], 0
    for mapname in M.MAPS:
        cases = [c for name in M.FAMILIES if name != "ordering" for c in M.kept(name) if c["map"] == mapname]
        got = _call(worlds[mapname], cases, TERRAIN_ONLY, f"the whole set on {mapname}")
        more = _check(cases, got, {})
        leaks += more[0]; bad += more[1]; count += len(cases)
        for k in (1, 65):
            _same_bytes(_call(worlds[mapname], cases[:k], TERRAIN_ONLY, f"{k} rays on {mapname}"), got[:k], f"{k} rays on {mapname} against the whole call")
    order = M.kept("ordering")
    got = _call(worlds["rolling"], order, TERRAIN_AND_STATIC, "ordering")
    _same_bytes(_call(worlds["rolling"], order[:1], TERRAIN_AND_STATIC, "ordering, 1 ray"), got[:1], "ordering, 1 ray against the whole call")
    _report(leaks, bad, count)
