"""The pair-level test matrix of the contact manifolds (narrow.hpp and gjk.hpp: the step's k_narrow, k_narrow_clip and wave GJK / EPA, and
mi_world_volume_contacts' k_vc_narrow and k_vc_gjk): every volume type against every collider type, one collider at a time; numpy and the
oracle, no GPU.  tests/test_contact_matrix.py holds the oracle to the reference's own narrow phase on every case and checks the matrix's
coverage, tests/test_gpu_contact_matrix.py runs it on the GPU.

  * the CASES are those of tests/overlap_matrix.py, all ten families, unchanged (their geometric certificates are not used here: the yardstick
    is the reference's narrow phase), plus the family `hull_shapes`: hull geometries 3 (the unit cube as a hull of 8 vertices: exact ties in the
    support scan, flat faces) and 4 (a prism of 130 vertices: more vertices than a wave has lanes, 65 coplanar ones per cap) of
    sweep_matrix.hulls() against all six types in both roles: face, edge / side and vertex against the features of overlap_matrix's `features`
    family, a whole face tying along an axis-aligned support direction from above and from the side, and deep cases with each shape's centre
    inside the other;
  * the MANIFOLD of a case comes from one step of a two-entity world that sees exactly the float32 numbers of the case: the collider on a static
    entity, the volume as a dynamic body (contact_ref.oracle_manifolds' construction, one world per case so that no coordinate moves);
  * EQUAL TYPES: the step makes A whichever AABB starts earlier on its sweep axis, the query makes the volume A.  `query_items` reads from the
    oracle which shape was A and hands THAT shape to the query as the volume and the other as the static collider; a case without a manifold is
    queried in both orientations.  No case is left out."""
import numpy as np

import overlap_matrix as OM
import overlap_ref as R
import sweep_matrix as M
from d3d12renderer_amd import capi, scenes

TYPES, PAIRS = OM.TYPES, OM.PAIRS
FAMILIES = OM.FAMILIES + ("hull_shapes",)
UNIT_FAMILIES = ("generic", "features", "cylinder_caps", "thin", "containment", "degenerate", "hull_shapes")   # what the step worlds hold
APPLIES = dict(OM.APPLIES, hull_shapes=[(v, c) for v, c in PAIRS if R.HULL in (v, c)])
MANIFOLDS_ONLY = ("containment",)      # nothing there is apart
NEW_GEOMETRIES = (3, 4)
MIN_HITS = MIN_MISSES = 3              # THE CAP, per (family, pair the family applies to)
# The manifold sizes each family reaches on the reference (= the oracle, byte for byte).  A pair with a cylinder or a hull ends in EPA's single contact
# and the cases of the ten families are overlap_matrix's, unchanged, so not every family can hold every size (cylinder_caps and hull_shapes hold only
# pairs of that kind): each family keeps what it reaches, every manifold has 1 to 4 contacts, and the matrix as a whole reaches 1, 2, 3 and 4.
REACHES = dict(generic={1, 2, 4}, features={1, 2, 3, 4}, cylinder_caps={1}, size={1, 2, 3, 4}, size_ratio={1, 2, 3, 4}, far={1, 3, 4}, thin={1, 2, 3, 4},
               containment={1, 2, 4}, degenerate={1, 2, 3, 4}, ladder={1, 2, 3, 4}, hull_shapes={1})


# ---- hull_shapes
def _hull_poses(geometry):
    """(name, rotation) with the named feature of the geometry pointing along -y and, by its symmetry, one like it along +y."""
    z = lambda a: scenes.q_axis_angle((0, 0, 1), a)   # noqa: E731
    if geometry == 3:
        OM._feature_shapes(R.OBB, True)    # (computes the rotation that stands a cube on a vertex)
        return [("face", M.I4), ("edge", z(np.pi / 4)), ("vertex", OM._VERTEX_DOWN)]
    return [("cap", M.I4), ("side", z(np.pi / 2)), ("rim-vertex", z(0.5))]


def _hull_setups():
    for g in NEW_GEOMETRIES:
        for other in range(6):
            for hull_is_volume in (True, False):
                for hn, q in _hull_poses(g):
                    for on, shape in OM._feature_shapes(other, not hull_is_volume):
                        h = M.hull(q, g)
                        vol, col, tag = (h, shape, f"g{g}-{hn}/{on}") if hull_is_volume else (shape, h, f"{on}/g{g}-{hn}")
                        yield tag, M.shifted(vol, (0.3, 2.5, -0.2) if on == "skew" else (0.0, 2.5, 0.0)), col
                # a whole face ties from the side too: both shapes unturned, the volume along +x
                on, shape = OM._feature_shapes(other, True)[0]
                h = M.hull(M.I4, g)
                vol, col, tag = (h, shape, f"g{g}-from-x/{on}") if hull_is_volume else (shape, h, f"{on}/g{g}-from-x")
                yield tag, M.shifted(vol, (2.5, 0.0, 0.0)), col
        # the two new geometries against each other and themselves, flat on flat
        for go in NEW_GEOMETRIES:
            yield f"g{g}-flat/g{go}-flat", M.shifted(M.hull(M.I4, g), (0.0, 2.5, 0.0)), M.hull(M.I4, go)


def _hull_deep():
    """The centre of each shape inside the other."""
    off = np.array([0.05, 0.02, -0.03])
    for g in NEW_GEOMETRIES:
        for other in range(6):
            for k, (on, shape) in enumerate(OM._feature_shapes(other, True)[:2]):
                if other == R.HULL:
                    shape = OM._centred(shape)
                h = M.hull(_hull_poses(g)[k][1], g)
                for vol, col, tag in ((h, shape, f"g{g}-deep/{on}"), (shape, h, f"{on}/g{g}-deep")):
                    yield tag, M.shifted(vol, off), col, off


def hull_shapes():
    out = [c for tag, vol, col in _hull_setups() for c in OM.around_touch("hull_shapes", tag, vol, col)]
    for tag, vol, col, off in _hull_deep():
        c = OM.finish("hull_shapes", tag, vol, col, True, start=0.5 * off, step=0.05)
        c["setup"] = tag
        out.append(c)
    return out


_CACHE = {}


def family(name):
    if name == "hull_shapes":
        if name not in _CACHE:
            _CACHE[name] = hull_shapes()
        return _CACHE[name]
    return OM.family(name)


# ---- one case, one world
def _collider_of_volume(v):
    """The fields OM.scene_of reads, from a volume record: the very same numbers."""
    return dict(col_type=int(v["type"][0]), col_words=v["shape"][0].copy(), col_pos=v["position"][0].copy(), col_rot=v["rotation"][0].copy(), col_hull=int(v["hull_geometry"][0]))


def _volume_of_collider(c):
    return capi.make_volume(c["col_type"], c["col_words"], c["col_pos"], c["col_rot"], c["col_hull"])


def pair_scene(colliders, offsets=None, name="contact_matrix"):
    """Per item: a static entity with the item's collider (entity 2 i) and a dynamic body with its volume as the collider (2 i + 1; no gravity),
    both moved by offsets[i]."""
    n = len(colliders)
    e = scenes.make_entities(2 * n, capi.ENTITY_DYNAMIC)
    e["gravity_factor"] = 0.0
    c = scenes.make_colliders(2 * n, capi.SPHERE)
    for i, item in enumerate(colliders):
        off = np.zeros(3, np.float32) if offsets is None else np.asarray(offsets[i], np.float32)
        v = item["volume"][0]
        e["kind"][2 * i] = capi.ENTITY_STATIC
        e["position"][2 * i] = item["col_pos"] + off; e["rotation"][2 * i] = item["col_rot"]
        c["type"][2 * i] = item["col_type"]; c["shape"][2 * i, :12] = item["col_words"]; c["hull_geometry"][2 * i] = item["col_hull"]
        e["position"][2 * i + 1] = v["position"] + off; e["rotation"][2 * i + 1] = v["rotation"]
        c["type"][2 * i + 1] = v["type"]; c["shape"][2 * i + 1, :12] = v["shape"]; c["hull_geometry"][2 * i + 1] = v["hull_geometry"]
    return scenes.Scene(name, e, np.arange(2 * n, dtype=np.uint32), c, 10, hulls=list(M.hulls()))


def step_contacts(world_factory, case):
    """The contact list of one step of the case's own two-entity world (world collider 1 = the collider, 0 = the volume: created last)."""
    sc = pair_scene([case])
    w = sc.populate(world_factory())
    w.step_fixed(sc.settings(), sc.dt, 1)
    con = w.contacts()
    w.close()
    return con


def manifold_of(contacts):
    """None, or dict(volume_is_a, normal (3 f32), points ((n, 4) f32: xyz, depth)) of a two-collider world's contact list."""
    if len(contacts) == 0:
        return None
    a, b = int(contacts["collider_a"][0]), int(contacts["collider_b"][0])
    assert {a, b} == {0, 1} and (contacts["collider_a"] == a).all() and (contacts["collider_b"] == b).all() and 1 <= len(contacts) <= 4
    assert all(np.array_equal(k["normal"], contacts["normal"][0]) for k in contacts)
    return dict(volume_is_a=a == 0, normal=np.array(contacts["normal"][0], np.float32),
                points=np.array([[*k["point"], k["penetration_depth"]] for k in contacts], np.float32))


def oriented_manifold(w, a, b):
    """The oracle's narrow phase of the oriented pair (A, B) of the world's last step (ora_debug_intersect): None or dict(normal, points)."""
    import ctypes as C
    normal = np.zeros(3, np.float32); points = np.zeros((4, 4), np.float32); count = C.c_uint32(0)
    w.L.check(w.L.fn("debug_intersect")(w.h, C.c_uint32(a), C.c_uint32(b), normal.ctypes.data_as(C.c_void_p), points.ctypes.data_as(C.c_void_p), C.byref(count)), "debug_intersect")
    return None if count.value == 0 else dict(volume_is_a=a == 0, normal=normal, points=points[:count.value].copy())


_MANIFOLDS = {}


def _oracle_case(oracle_mod, case):
    """The manifold of the case's step; for equal types also what the narrow phase gives with the volume as A and with the collider as A.  The
    step took one of the two (whichever AABB starts earlier on its sweep axis): a manifold of the step is one of them, bit for bit, and a step
    without a manifold leaves at most the other orientation with one (the GJK of a cylinder or hull pair is not symmetric in A and B)."""
    sc = pair_scene([case])
    w = sc.populate(oracle_mod.create_world(oracle_mod.ORDER_REFERENCE))
    w.step_fixed(sc.settings(), sc.dt, 1)
    m = manifold_of(w.contacts())
    if case["vt"] == case["ct"]:
        both = {True: oriented_manifold(w, 0, 1), False: oriented_manifold(w, 1, 0)}
        if m is None:
            assert both[True] is None or both[False] is None, (case["tag"], "the step took neither orientation")
            m_alt = both
        else:
            mine = both[m["volume_is_a"]]
            assert mine is not None and mine["normal"].tobytes() == m["normal"].tobytes() and mine["points"].tobytes() == m["points"].tobytes(), case["tag"]
            m_alt = None
    else:
        m_alt = None
    w.close()
    return m, m_alt


def _oracle_family(oracle_mod, name):
    if name not in _MANIFOLDS:
        both = [_oracle_case(oracle_mod, c) for c in family(name)]
        _MANIFOLDS[name] = ([m for m, _ in both], [alt for _, alt in both])
    return _MANIFOLDS[name]


def oracle_manifolds(oracle_mod, name):
    """Per case of the family: the manifold of the oracle's step (ORDER_REFERENCE) or None."""
    return _oracle_family(oracle_mod, name)[0]


def oracle_orientations(oracle_mod, name):
    """Per case: None, or for an equal-type case whose step gave no manifold {volume is A: manifold or None} straight from the narrow phase."""
    return _oracle_family(oracle_mod, name)[1]


def coverage(cases, manifolds):
    """({pair: [manifolds, misses]}, the set of manifold sizes, the number of manifolds holding a non-finite number)."""
    table, sizes, bad = {}, set(), 0
    for c, m in zip(cases, manifolds):
        table.setdefault((c["vt"], c["ct"]), [0, 0])[0 if m is not None else 1] += 1
        if m is not None:
            sizes.add(len(m["points"]))
            bad += not (np.isfinite(m["normal"]).all() and np.isfinite(m["points"]).all())
    return table, sizes, bad


def check_cap(name, table, sizes, bad, what="", reaches=None):
    assert bad == 0, f"{what}{name}: {bad} manifolds of the oracle hold a non-finite number"
    for pair in APPLIES[name]:
        hits, misses = table.get(pair, (0, 0))
        assert hits >= MIN_HITS, f"{what}{name} {TYPES[pair[0]]} -> {TYPES[pair[1]]}: {hits} manifolds"
        assert misses >= MIN_MISSES or name in MANIFOLDS_ONLY, f"{what}{name} {TYPES[pair[0]]} -> {TYPES[pair[1]]}: {misses} misses"
    assert (REACHES[name] if reaches is None else reaches) <= sizes <= {1, 2, 3, 4}, f"{what}{name}: manifold sizes {sorted(sizes)}"


# ---- the query's orientation
def query_items(cases, manifolds, orientations):
    """The (volume, static collider, expectation) items the query is asked: a case as it stands when its volume was A or the types differ; with
    the roles swapped when the types are equal and the collider was A; in both orientations when equal types gave no manifold: the one the step
    took expects none, the other what the oracle's narrow phase gives for it (none too, but for a few cylinder and hull pairs at the GJK's
    thresholds).  expect = None or dict(normal, points, volume_is_b)."""
    items = []
    for i, (c, m, alt) in enumerate(zip(cases, manifolds, orientations)):
        plain = dict(case=i, volume=c["volume"], col_type=c["col_type"], col_words=c["col_words"], col_pos=c["col_pos"], col_rot=c["col_rot"], col_hull=c["col_hull"])
        swapped = dict(case=i, volume=_volume_of_collider(c), **_collider_of_volume(c["volume"]))
        equal = c["vt"] == c["ct"]
        if m is None:
            for item, volume_is_a in ((plain, True), (swapped, False)) if equal else ((plain, True),):
                e = alt[volume_is_a] if equal else None
                items.append(dict(item, expect=None if e is None else dict(normal=e["normal"], points=e["points"], volume_is_b=False)))
            continue
        if not equal:
            assert m["volume_is_a"] == (c["vt"] < c["ct"]), (i, c["tag"], "A is not the smaller world type")
        expect = dict(normal=m["normal"], points=m["points"], volume_is_b=not equal and not m["volume_is_a"])
        items.append(dict(swapped if equal and not m["volume_is_a"] else plain, expect=expect))
    return items


# ---- the step's worlds
GRID, SPACING, PER_WORLD = 8, 8.0, 512


def step_worlds(name):
    """The family in worlds of at most 512 cases on an 8 x 8 x 8 grid of spacing 8 (offsets are multiples of a power of two): [(scene, cases)]."""
    cases = family(name)
    out = []
    for start in range(0, len(cases), PER_WORLD):
        chunk = cases[start:start + PER_WORLD]
        k = np.arange(len(chunk))
        offsets = np.stack([k % GRID, (k // GRID) % GRID, k // (GRID * GRID)], axis=1).astype(np.float32) * np.float32(SPACING)
        out.append((pair_scene(chunk, offsets, f"contact_matrix {name} {start}"), chunk))
    return out


def pose_bits(transforms):
    """The bits of (positions, rotations) with every NaN replaced by one pattern.  A body of a degenerate volume has no mass and its pose becomes NaN in
    the first step, on the GPU and in the oracle alike; which NaN an invalid operation produces (its sign) is the hardware's choice, not IEEE 754's."""
    out = []
    for a in transforms:
        bits = np.ascontiguousarray(a, np.float32).view(np.uint32).copy()
        bits[np.isnan(a)] = 0x7FC00000
        out.append(bits.tobytes())
    return tuple(out)


_STEPS = {}


def oracle_steps(oracle_mod, name):
    """Per step world of the family: (scene, counts, contact set, poses) of one canonical-order step of the oracle, and the family's coverage
    (table, sizes) on the contacts of those very worlds: moving a case changes its low bits, so the cap is held on what the moved worlds give."""
    from helpers import contact_set
    if name not in _STEPS:
        out = []; table = {}; sizes = set(); bad = 0
        for sc, chunk in step_worlds(name):
            assert np.abs(sc.entities["position"]).max() <= 64.0
            o = sc.populate(oracle_mod.create_world(oracle_mod.ORDER_CANONICAL))
            o.step_fixed(sc.settings(), sc.dt, 1)
            con = o.contacts()
            out.append((sc, o.counts(), contact_set(con), pose_bits(o.physics_transforms())))
            o.close()
            t, s, b = coverage(chunk, step_coverage(chunk, con))
            for pair, (h, m) in t.items():
                row = table.setdefault(pair, [0, 0]); row[0] += h; row[1] += m
            sizes |= s; bad += b
        check_cap(name, table, sizes, bad, what="step worlds of ", reaches={1})
        _STEPS[name] = (out, table, sizes)
    return _STEPS[name]


def step_coverage(chunk, contacts):
    """The manifolds of a step world's contact list per case (pairs of a case's own two colliders only: world collider = 2 n - 1 - creation)."""
    n = len(chunk)
    groups = {}
    for k in contacts:
        a, b = 2 * n - 1 - int(k["collider_a"]), 2 * n - 1 - int(k["collider_b"])
        if a // 2 == b // 2:
            groups.setdefault(a // 2, []).append(k)
    return [manifold_of_size(groups.get(i)) for i in range(n)]


def manifold_of_size(ks):
    return None if not ks else dict(normal=np.array(ks[0]["normal"], np.float32), points=np.array([[*k["point"], k["penetration_depth"]] for k in ks], np.float32))
