"""The shape cast against the heightmap terrain on the GPU, at its hard casts (tests/sweep_terrain_matrix.py), against the float64 reference of
tests/sweep_terrain_ref.py: one world per map, one call per family and map, every kept case without a budget.  Every call also runs the exhaustive
kernel and requires the same bytes (test_gpu_sweep_terrain._cast).  Per case: the reference's decision; for a hit entity = collider = the
terrain's value, a static object type and no flag; |t - t_ref| |d|, the point's distance from the surface and the shortfall of the separation
after backing the volume off along the reported normal (0.05, or a twentieth of that for the volumes of 1e-2; held against the reference's own
shortfall there: in a hollow the next triangle comes closer), each within BOUNDS[family] x scale; |n| = 1 and n . d <= 0; an initial overlap as
the header words it (t = 0, the flag, point = the pose's position, normal = -normalize(d)); no record unconverged.  `wide` also checks, by the
kernel's own footprint formula, that its casts span more than 64 blocks across the travel and that the touch lies in the second pass of 64.
`lattice` needs no reference cast: a few thousand vertical casts of spheres of radius 0 and 1e-3 through every kind of line of the grid.

The zero-radius spheres of `features` are held to the header's wording for a volume without a radius on an edge or a vertex (the normal is a
separating direction of the triangle hit): backed off along it they leave the terrain; how short of the full back-off is printed.
Measured on the MI355X, per unit of scale, at the bounds the cases were made with: sweep_terrain_matrix.MEASURED and BOUNDS, with a sentence per
family above 6e-6.  lattice: no miss on the rolling, offset and floor map (5 715, 5 749 and 3 620 casts per radius), the zero-radius sphere within
2.78e-6 of the surface's height and 2.76e-6 of mi_world_raycast's hit."""
import numpy as np
import pytest

import query_helpers as Q
import sweep_ref as S
import sweep_terrain_matrix as M
import sweep_terrain_ref as ST
from test_gpu_sweep_terrain import _cast

pytestmark = pytest.mark.gpu

MISS, TERRAIN, STATIC = 0xFFFFFFFF, 0xFFFFFFFE, 1
INITIAL_OVERLAP, UNCONVERGED = 1, 2
# Casts that may end with the unconverged flag (mi_sweep_hit.flags): {tag: the allowance on |t - t_ref| |d| per unit of scale, measured}.  None does.
KNOWN_UNCONVERGED = {}


class _Worlds:
    def __init__(self, mi):
        self.mi, self.open = mi, {}

    def __getitem__(self, name):
        if name not in self.open:
            self.open[name] = Q.world(self.mi, M.scene(name))
        return self.open[name]


@pytest.fixture(scope="module")
def worlds(mi_lib):
    ws = _Worlds(mi_lib)
    yield ws
    for w in ws.open.values():
        w.close()


def _call(w, cases, include, what):
    """One call of an odd number of casts (the first repeated where the cases are even in number)."""
    vols = np.concatenate([c["volume"] for c in cases]); disp = np.stack([c["disp"] for c in cases])
    if len(cases) % 2 == 0:
        vols, disp = np.concatenate([vols, vols[:1]]), np.concatenate([disp, disp[:1]])
    return _cast(w, vols, disp, include, what=what)[:len(cases)]


def _is_miss_record(rec):
    return (rec["entity"] == MISS and rec["collider"] == MISS and np.isposinf(rec["t"]) and not rec["point"].any() and not rec["normal"].any()
            and rec["object_type"] == 0 and rec["flags"] == 0)


def _back_off(c):
    return 0.05 * (0.05 if c.get("tiny") else 1.0)


def _check(cases, got, worst):
    """Every record against the reference's answer of its case: (wrong decisions, other failures); raises worst[volume type] = [|dt| |d|, point off
    the surface, separation short], each per unit of scale."""
    leaks, bad = [], []
    for c, rec in zip(cases, got):
        who = f"{c['family']} {c['map']} {c['tag']} (scale {c['scale']:.4g}, |d| {np.linalg.norm(c['d']):.3g})"
        want = c["expect"]
        if want in ("invalid", "miss"):
            if rec["entity"] != MISS:
                leaks.append(f"{who}: the reference misses (closest approach {c['clearance'] / max(M.delta(c), 1e-300):.1f} delta), the GPU hits at t = {rec['t']:.8g}, flags {rec['flags']}")
            elif not _is_miss_record(rec):
                bad.append(f"{who}: a miss record that is not all-miss: {rec}")
            continue
        if rec["entity"] == MISS:
            leaks.append(f"{who}: the reference {'starts in touch' if want == 'initial' else 'hits at t = %.8g' % c['ref'][0]}, the GPU misses")
            continue
        if rec["flags"] & UNCONVERGED and c["tag"] not in KNOWN_UNCONVERGED:
            bad.append(f"{who}: the unconverged flag at t = {rec['t']:.8g} (the reference: {c['ref'][0]:.8g})")
        if rec["entity"] != TERRAIN or rec["collider"] != TERRAIN or rec["object_type"] != STATIC:
            bad.append(f"{who}: entity {rec['entity']:#x}, collider {rec['collider']:#x}, object type {rec['object_type']}")
            continue
        d, scale = c["d"], c["scale"]
        length = float(np.linalg.norm(d))
        t, p, n = float(rec["t"]), rec["point"].astype(np.float64), rec["normal"].astype(np.float64)
        if want == "initial":
            back = -d / length if length > 0 else np.zeros(3)
            if rec["flags"] != INITIAL_OVERLAP or t != 0 or not (rec["point"] == c["volume"]["position"][0]).all() or not np.allclose(n, back, atol=1e-6):
                (leaks if not rec["flags"] & INITIAL_OVERLAP else bad).append(f"{who}: starts in touch: expected t = 0, the flag, the pose's position and -normalize(d); got {rec}")
            continue
        if rec["flags"] & INITIAL_OVERLAP:
            leaks.append(f"{who}: the reference hits at t = {c['ref'][0]:.8g} from {c['clearance'] / M.delta(c):.1f} delta clear, the GPU reports an initial overlap")
            continue
        bound = (KNOWN_UNCONVERGED.get(c["tag"]) or M.BOUNDS[c["family"]]) * scale
        dt = abs(t - c["ref"][0]) * length
        dp = abs(ST.point_gap(c["map"], p))
        off = _back_off(c)
        short = off - ST.separation(c["map"], c["conv"], t * d + off * n, n)
        short_ref = 0.0
        if short > 0:     # (the reference's own shortfall counts only against one of the GPU's)
            short_ref = off - ST.separation(c["map"], c["conv"], c["ref"][0] * d + off * c["ref"][1], c["ref"][1])
            short = short - max(short_ref, 0.0)
            worst["hollows"] = worst.get("hollows", 0) + (short_ref > 0)
        m = worst.setdefault(c["vt"], [0.0, 0.0, 0.0])
        m[0] = max(m[0], dt / scale); m[1] = max(m[1], dp / scale); m[2] = max(m[2], 0.0 if c.get("ruled_normal") else short / scale)
        if dt > bound:
            bad.append(f"{who}: |t - t_ref| |d| = {dt:.3e} > {bound:.3e} (t = {t:.9g}, the reference {c['ref'][0]:.9g})")
        if dp > bound:
            bad.append(f"{who}: the point lies {dp:.3e} off the surface (bound {bound:.3e})")
        if c.get("ruled_normal"):     # a volume without a radius on an edge or a vertex: a separating direction of the triangle hit (the header)
            worst["ruled"] = max(worst.get("ruled", 0.0), short / scale)
            if not short < off:
                bad.append(f"{who}: backed off {off:g} along the normal {n} the point does not leave the terrain (short by {short:.3e})")
        elif short > bound:
            bad.append(f"{who}: backed off {off:g} along the normal the volume is {short:.3e} short of that clear (bound {bound:.3e}; the reference's normal: {short_ref:.3e} short)")
        if abs(np.linalg.norm(n) - 1) > 1e-5 or n @ d > 0:
            bad.append(f"{who}: normal {n}: |n| - 1 = {np.linalg.norm(n) - 1:.2e}, n . d = {n @ d:.3e}")
        if c.get("normal_down") and not n[1] < 0:
            bad.append(f"{who}: a hit from below with the normal {n}")
    return leaks, bad


def _report(name, worst, leaks, bad, count, bound):
    hollows, ruled = worst.pop("hollows", 0), worst.pop("ruled", None)
    print(f"{name}: {hollows} cases counted the reference's own shortfall of the separation against the GPU's" + ("" if ruled is None else
          f"; zero-radius spheres on the features: the separation along the reported normal short by up to {ruled:.2e} per unit of scale (not bounded)"))
    for vt, m in sorted(worst.items()):
        print(f"{name}, {M.TYPES[vt]}, per unit of scale: largest |dt| |d| {m[0]:.2e}, point off the terrain {m[1]:.2e}, separation short by {m[2]:.2e}")
    largest = max((max(m) for m in worst.values()), default=0.0)
    print(f"{name}: {len(leaks)} wrong decisions in {count} cases; the largest measure per unit of scale {largest:.2e} (bound {bound:.0e})")
    assert not leaks and not bad, f"{len(leaks)} wrong decisions and {len(bad)} other failures in {count} cases:\n" + "\n".join(leaks + bad)


def _ordering(w, cases, worst):
    """include 7: the nearer of the family's own collider and the terrain; include 4 and 3: each alone."""
    leaks, bad = [], []
    n = len(M.family("ordering"))
    both, ter, col = (_call(w, cases, inc, f"ordering, include {inc}") for inc in (M.BOTH, M.TERRAIN_ONLY, M.COLLIDERS_ONLY))
    more = _check(cases, ter, worst)
    leaks += more[0]; bad += more[1]
    for c, rb, rt, rc in zip(cases, both, ter, col):
        who = f"ordering {c['tag']}"
        length, bound = float(np.linalg.norm(c["d"])), M.BOUNDS["ordering"] * c["scale"]
        i = c["col"]
        if rc["entity"] != i or rc["collider"] != n - 1 - i or rc["object_type"] != STATIC or rc["flags"] != 0:
            leaks.append(f"{who}: include 3: expected collider {i} at t = {c['col_ref'][0]:.8g}, got {rc}")
            continue
        dt = abs(float(rc["t"]) - c["col_ref"][0]) * length
        m = worst.setdefault(c["vt"], [0.0, 0.0, 0.0]); m[0] = max(m[0], dt / c["scale"])
        if dt > bound:
            bad.append(f"{who}: the collider's |t - t_ref| |d| = {dt:.3e} > {bound:.3e}")
        want = rc if c["collider_wins"] else rt
        if rb.tobytes() != want.tobytes():
            leaks.append(f"{who}: include 7 must name the {'collider' if c['collider_wins'] else 'terrain'} ({c['clearance'] / M.delta(c):.1f} delta nearer): got {rb}, "
                         f"the collider alone {rc}, the terrain alone {rt}")
    return leaks, bad


@pytest.mark.parametrize("name", M.FAMILIES)
def test_family(worlds, name):
    """One family, one call per map it uses."""
    kept, worst = M.kept(name), {}
    leaks, bad = [], []
    for mapname in sorted(set(c["map"] for c in kept)):
        cases = [c for c in kept if c["map"] == mapname]
        if name == "ordering":
            more = _ordering(worlds[mapname], cases, worst)
        else:
            more = _check(cases, _call(worlds[mapname], cases, M.TERRAIN_ONLY, f"{name} on {mapname}"), worst)
        leaks += more[0]; bad += more[1]
    if name == "wide":
        spans = [M.footprint_blocks(c) for c in kept]
        print("wide: blocks across the travel per cast:", [hi - lo + 1 for lo, hi in spans])
        assert sum(hi - lo >= 64 for lo, hi in spans) == len(kept) and sum(bool(c["second_pass"]) for c in kept) >= 8
    print(f"{name}: {len(M.family(name))} generated, {len(kept)} kept")
    _report(name, worst, leaks, bad, len(kept), M.BOUNDS[name])


@pytest.mark.parametrize("mapname", M.LATTICE_MAPS)
def test_lattice_is_watertight(worlds, mapname):
    """Vertical casts from above the highest to below the lowest height, straddling every kind of line of the grid by 0, +-1 and +-2 float32 ulps, in one
    call per radius: every cast hits; the zero-radius sphere at the surface's height (Map.height) and where mi_world_raycast hits; the sphere of 1e-3 no later."""
    from d3d12renderer_amd import capi
    xs, zs, h, kinds = M.lattice(mapname)
    m, w = M.the_map(mapname), worlds[mapname]
    y0 = np.float32(m.ymax + 1.0)
    drop = np.float32(m.ymax - m.ymin + 2.0)
    disp = np.tile(np.array([0.0, -drop, 0.0], np.float32), (len(xs), 1))
    origins = np.stack([xs, np.full(len(xs), y0, np.float32), zs], axis=1)
    scale = np.maximum(1.0, np.abs(np.concatenate([origins, origins + disp], axis=1)).max(axis=1).astype(np.float64))
    bound = M.LATTICE_BOUND * scale
    got = {r: _cast(w, np.concatenate([capi.sphere_volume(o, r) for o in origins]), disp, M.TERRAIN_ONLY, what=f"lattice r = {r:g} on {mapname}") for r in M.LATTICE_RADII}
    rays = w.raycast(origins, disp, max_t=1.0, include=M.TERRAIN_ONLY)
    bad = []
    for r, recs in got.items():
        missed = np.flatnonzero(recs["entity"] != TERRAIN)
        bad += [f"r = {r:g}: cast {i} over a {kinds[i]} at ({xs[i]!r}, {zs[i]!r}) misses (the ground there: {h[i]:.6f})" for i in missed[:20]]
        print(f"lattice on {mapname}, r = {r:g}: {len(missed)} misses in {len(recs)} casts")
    zero, fat = got[0.0], got[M.LATTICE_RADII[1]]
    hit = (zero["entity"] == TERRAIN) & (fat["entity"] == TERRAIN)
    want = (float(y0) - h) / float(drop)
    dt = np.abs(zero["t"].astype(np.float64) - want) * float(drop)
    late = (fat["t"].astype(np.float64) - zero["t"]) * float(drop)
    dray = np.abs(zero["t"].astype(np.float64) - rays["t"]) * float(drop)
    both = hit & (rays["entity"] == TERRAIN)
    print(f"lattice on {mapname}: {int((rays['entity'] != TERRAIN).sum())} rays miss; against the ray cast, per unit of scale, {np.max(dray[both] / scale[both]):.2e}")
    bad += [f"ray {i} over a {kinds[i]} at ({xs[i]!r}, {zs[i]!r}) misses" for i in np.flatnonzero(rays["entity"] != TERRAIN)[:20]]
    bad += [f"cast {i} over a {kinds[i]}: t |d| is {dray[i]:.3e} off the ray cast's (bound {bound[i]:.3e})" for i in np.flatnonzero(both & (dray > bound))[:20]]
    print(f"lattice on {mapname}: per unit of scale, |t - height| {np.max(dt[hit] / scale[hit]):.2e}, "
          f"the sphere of 1e-3 later than the point by at most {np.max(late[hit] / scale[hit]):.2e} (bound {M.LATTICE_BOUND:.0e})")
    bad += [f"cast {i} over a {kinds[i]}: t |d| is {dt[i]:.3e} off the surface's height (bound {bound[i]:.3e})" for i in np.flatnonzero(hit & (dt > bound))[:20]]
    bad += [f"cast {i} over a {kinds[i]}: the sphere of 1e-3 touches {late[i]:.3e} later than the point" for i in np.flatnonzero(hit & (late > bound))[:20]]
    assert (zero["flags"] == 0).all() and (fat["flags"][fat["entity"] == TERRAIN] == 0).all()
    assert not bad, f"{len(bad)} failures (at most 20 of a kind listed):\n" + "\n".join(bad)
