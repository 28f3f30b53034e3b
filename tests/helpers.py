import numpy as np
from d3d12renderer_amd import capi, scenes


def single_body_scene(ctype, shape, pos=(0, 0, 0), rot=(0, 0, 0, 1), ground=True, density=1.0, friction=0.5, restitution=0.1,
                      lin_damping=0.4, ang_damping=0.4, iterations=30):
    e = scenes.make_entities(1)
    e["position"][0] = pos
    e["rotation"][0] = rot
    e["linear_damping"] = lin_damping
    e["angular_damping"] = ang_damping
    c = scenes.make_colliders(1, ctype, restitution=restitution, friction=friction, density=density)
    c["shape"][0, :len(shape)] = shape
    ents, cols, cent = [e], [c], [0]
    if ground:
        ge, gc = scenes._ground(100.0)
        ents.append(ge); cols.append(gc); cent.append(1)
    return scenes.Scene("single", np.concatenate(ents), np.asarray(cent, np.uint32), np.concatenate(cols), iterations)


def two_body_scene(descs, iterations=30, gravity=0.0):
    """descs: list of (ctype, shape, pos, rot, kind)."""
    n = len(descs)
    e = scenes.make_entities(n)
    c = scenes.make_colliders(n, 0)
    for i, (ctype, shape, pos, rot, kind) in enumerate(descs):
        e["position"][i] = pos
        e["rotation"][i] = rot
        e["kind"][i] = kind
        e["gravity_factor"][i] = gravity
        c["type"][i] = ctype
        c["shape"][i, :len(shape)] = shape
    return scenes.Scene("pair", e, np.arange(n, dtype=np.uint32), c, iterations)


def manifold_colors(w):
    """(oriented collider pairs (n, 2), first contact of each manifold, colour of each manifold) of a world's last step, from its own
    contact list and its own colour getter (the product and the oracle list both in the order of their contact list)."""
    con = w.contacts()
    nm = w.counts()["num_collisions"]
    colors = np.zeros(nm, np.uint32)
    import ctypes as C
    w.L.check(w.L.fn("world_get_manifold_colors")(w.h, colors.ctypes.data_as(C.c_void_p), C.c_uint32(nm)), "world_get_manifold_colors")
    first = np.r_[True, (con["collider_a"][1:] != con["collider_a"][:-1]) | (con["collider_b"][1:] != con["collider_b"][:-1])] if len(con) else np.zeros(0, bool)
    assert int(first.sum()) == nm, f"{int(first.sum())} runs of contacts, {nm} manifolds"
    pairs = np.stack([con["collider_a"][first], con["collider_b"][first]], axis=1).astype(np.uint32)
    return pairs, con[first], colors


def dynamic_bodies(w):
    """Body indices (as the contact list names them) of the bodies with an inverse mass: the only ones two manifolds of one colour may not share."""
    im = w.mass_properties()[0]
    ents = np.nonzero(im != 0.0)[0].astype(np.uint32)
    return set(int(b) for b in w.entities_to_bodies(ents)) if len(ents) else set()


def assert_schedule_valid(w, oracle_world=None, check_overflow=False, tag=""):
    """The rule k_emit_manifolds trusts the colour history with: no two manifolds of one colour below 64 share a dynamic body (colour 64 = overflow,
    solved one after the other; `check_overflow` holds it to the rule as well).  With `oracle_world`: every manifold has the oracle's colour too,
    manifolds matched by their oriented collider pair.  Returns the colours, in the order of the contact list."""
    pairs, heads, colors = manifold_colors(w)
    dyn = dynamic_bodies(w)
    for col in np.unique(colors):
        if col >= 64 and not check_overflow:
            continue
        sel = colors == col
        bodies = [int(b) for b in np.concatenate([heads["body_a"][sel], heads["body_b"][sel]]) if int(b) in dyn]
        if len(set(bodies)) != len(bodies):
            shared = sorted(b for b in set(bodies) if bodies.count(b) > 1)
            raise AssertionError(f"{tag}colour {col} reuses dynamic bodies {shared[:8]} ({int(sel.sum())} manifolds of that colour)")
    if oracle_world is not None:
        opairs, _, ocolors = manifold_colors(oracle_world)
        mine = {(int(a), int(b)): int(c) for (a, b), c in zip(pairs, colors)}
        theirs = {(int(a), int(b)): int(c) for (a, b), c in zip(opairs, ocolors)}
        assert len(mine) == len(pairs) and len(theirs) == len(opairs), f"{tag}a collider pair is listed twice"
        assert mine.keys() == theirs.keys(), f"{tag}manifolds differ: {sorted(mine.keys() ^ theirs.keys())[:8]}"
        diff = [(k, mine[k], theirs[k]) for k in sorted(mine) if mine[k] != theirs[k]]
        assert not diff, f"{tag}{len(diff)} of {len(mine)} manifold colours differ from the oracle's ((pair), product, oracle): {diff[:6]}"
    return colors


def contact_set(contacts):
    """Order-independent, bit-exact representation of a contact list."""
    rows = []
    for k in contacts:
        rows.append((int(k["collider_a"]), int(k["collider_b"]), k["point"].tobytes(), k["penetration_depth"].tobytes(),
                     k["normal"].tobytes(), int(k["friction_restitution"]), int(k["body_a"]), int(k["body_b"])))
    return sorted(rows)


# --------------------------------------------------------------------------------------------------------------------------------------
# Holding a library directly against the reference itself (oracle/_ref/libref.so stepping the reference's own physicsStep)
def manifold_order(contacts):
    """The oriented collider pairs (world indices A, B) of a contact list's manifolds, in list order (contacts of a manifold are consecutive)."""
    if len(contacts) == 0:
        return np.zeros((0, 2), np.uint32)
    ab = np.stack([contacts["collider_a"], contacts["collider_b"]], axis=1).astype(np.uint32)
    keep = np.ones(len(ab), bool); keep[1:] = (ab[1:] != ab[:-1]).any(axis=1)
    return ab[keep]


def overlap_census(aabbs, axis):
    """From the world AABBs (min xyz, max xyz per collider): (closed, touching) = the number of unordered pairs whose boxes overlap as CLOSED intervals on all
    three axes (bounding_volumes.h:352-358: what `aabbVsAABB` accepts), and how many of those merely TOUCH on the sweep axis (one box ends exactly where the
    other starts).  Sort-and-sweep along `axis`, vectorised per start point."""
    mn = aabbs[:, 0:3]; mx = aabbs[:, 3:6]
    order = np.argsort(mn[:, axis], kind="stable")
    mn = mn[order]; mx = mx[order]
    starts = mn[:, axis]
    closed = touching = 0
    for i in range(len(mn) - 1):
        j1 = np.searchsorted(starts, mx[i, axis], side="right")          # candidates: start <= my end
        if j1 <= i + 1:
            continue
        c = slice(i + 1, j1)
        hit = np.ones(j1 - i - 1, bool)
        for a in range(3):
            if a != axis:
                hit &= (mx[i, a] >= mn[c, a]) & (mn[i, a] <= mx[c, a])
        closed += int(hit.sum())
        touching += int((hit & (starts[c] == mx[i, axis])).sum())
    return closed, touching


def _same_counts(cc, cr, i, aabbs=None, axis=None):
    """Bodies, colliders, collisions (manifolds) and contacts: bit-exact.  AABB overlaps: the reference's sweep misses a pair whose intervals
    touch EXACTLY on the sweep axis when the end point happens to sort before the start point (collision_broad.cpp:87-166, 386-398: which way such
    a tie sorts depends on the history of its persistent endpoint array; terrain tiles laid edge to edge do that — static against static, never a
    collision pair); the grid finds every closed-interval overlap.  With the AABBs at hand the gap is BOUNDED exactly: the candidate
    counts every closed overlap, the reference at least all of them that do more than touch on the sweep axis."""
    for k in ("num_rigid_bodies", "num_colliders", "num_collisions", "num_contacts"):
        assert cc[k] == cr[k], f"step {i}: {k} {cc[k]} != reference {cr[k]}"
    assert cc["num_broadphase_overlaps"] >= cr["num_broadphase_overlaps"], f"step {i}: AABB overlaps {cc['num_broadphase_overlaps']} < reference {cr['num_broadphase_overlaps']}"
    if aabbs is not None and len(aabbs) <= 6000:
        closed, touching = overlap_census(aabbs, axis)
        assert cc["num_broadphase_overlaps"] == closed, f"step {i}: candidate counts {cc['num_broadphase_overlaps']} overlaps, the AABBs hold {closed} closed-interval ones"
        assert closed - touching <= cr["num_broadphase_overlaps"] <= closed, (f"step {i}: reference counts {cr['num_broadphase_overlaps']} overlaps; of the {closed} closed-interval "
                                                                               f"ones only {touching} merely touch on the sweep axis")
        return cc["num_broadphase_overlaps"] - cr["num_broadphase_overlaps"], touching
    return cc["num_broadphase_overlaps"] - cr["num_broadphase_overlaps"], None


def _same_contacts_up_to_sweep_ties(cand, ref, aabbs, axis, i):
    """The two contact lists as sets, bit for bit — except where the reference's orientation (A, B) of a pair of EQUAL shape type is decided by the
    history of its persistent endpoint array: AABB starts that tie EXACTLY on the sweep axis (stable insertion sort, collision_broad.cpp:386-398;
    spheres stacked in a column never move sideways, so their starts stay tied for good).  Such a pair may come out as (B, A): the same contacts with
    the normal negated and the bodies exchanged — checked as exactly that, and counted.  (The replay mode is told the orientation with the order.)"""
    a, b = set(contact_set(cand)), set(contact_set(ref))
    if a == b:
        return 0
    only_c, only_r = sorted(a - b), sorted(b - a)
    assert len(only_c) == len(only_r), f"step {i}: contact lists differ as sets ({len(only_c)} / {len(only_r)} unmatched)"
    turned = set()
    twins = {}
    for r in only_r:
        twins.setdefault((r[1], r[0], r[2], r[3], r[5], r[7], r[6]), []).append(np.frombuffer(r[4], np.float32))
    for r in only_c:
        cands = twins.get((r[0], r[1], r[2], r[3], r[5], r[6], r[7]), [])
        nrm = np.frombuffer(r[4], np.float32)
        k = next((j for j, n in enumerate(cands) if np.array_equal(-nrm, n)), None)       # (-0.0 == 0.0: a negated zero component)
        assert k is not None, f"step {i}: a contact of colliders ({r[0]}, {r[1]}) has no counterpart in the reference's list"
        cands.pop(k)
        assert aabbs[r[0]][axis] == aabbs[r[1]][axis], f"step {i}: colliders ({r[0]}, {r[1]}) are oriented differently without a tie on the sweep axis"
        turned.add((min(r[0], r[1]), max(r[0], r[1])))
    return len(turned)


def teacher_forced(make_candidate, make_reference, sc, steps, check_every=1):
    """Every step: the reference steps from its own state S_k; the candidate is put into S_k (and given the axis the reference swept along),
    steps ONCE in its own (canonical) constraint order, and is compared with the reference after that one step:
      * the contact list, as a set, bit for bit (points, depths, normals, materials, body pairs, collider pairs) and every count;
      * positions / orientations / velocities: the only order-dependent part — returned as the largest deviations seen.
    Returns dict(max_pos_rel, max_rot_abs, max_lin, max_ang, contacts_min, contacts_max, steps)."""
    ref = sc.populate(make_reference()); cand = sc.populate(make_candidate())
    s = sc.settings(); ids = np.arange(sc.num_bodies, dtype=np.uint32)
    # `ids` are ENTITY ids; scenes create the dynamic bodies first
    out = dict(max_pos_rel=0.0, max_rot_abs=0.0, max_lin=0.0, max_ang=0.0, max_lin_rel=0.0, contacts_min=1 << 30, contacts_max=0, steps=steps)
    for i in range(steps):
        before = ref.get_body_states(ids)
        ref.step_fixed(s, sc.dt, 1)
        cr = ref.counts()
        cand.set_body_states(ids, before)
        cand.debug_set_sweep_axis(cr["sorting_axis"])
        cand.step_fixed(s, sc.dt, 1)
        cc = cand.counts()
        check = i % check_every == 0 or i == steps - 1
        surplus, touching = _same_counts(cc, cr, i, ref.aabbs() if check else None, cr["sorting_axis"])
        out["surplus_overlaps"] = out.get("surplus_overlaps", 0) + surplus
        if touching is not None:
            out["touching_pairs_max"] = max(out.get("touching_pairs_max", 0), touching)
        if check:
            out["tie_flips"] = out.get("tie_flips", 0) + _same_contacts_up_to_sweep_ties(cand.contacts(), ref.contacts(), ref.aabbs(), cr["sorting_axis"], i)
        a = cand.get_body_states(ids).astype(np.float64); b = ref.get_body_states(ids).astype(np.float64)
        assert np.isfinite(a).all() and np.isfinite(b).all()
        scale = np.maximum(1.0, np.abs(b[:, 0:3]).max(axis=1))
        out["max_pos_rel"] = max(out["max_pos_rel"], float((np.abs(a[:, 0:3] - b[:, 0:3]).max(axis=1) / scale).max()))
        out["max_rot_abs"] = max(out["max_rot_abs"], float(np.abs(a[:, 3:7] - b[:, 3:7]).max()))
        out["max_lin"] = max(out["max_lin"], float(np.abs(a[:, 7:10] - b[:, 7:10]).max()))
        out["max_ang"] = max(out["max_ang"], float(np.abs(a[:, 10:13] - b[:, 10:13]).max()))
        vs = np.maximum(1.0, np.abs(b[:, 7:10]).max())
        out["max_lin_rel"] = max(out["max_lin_rel"], float(np.abs(a[:, 7:10] - b[:, 7:10]).max() / vs))
        out["contacts_min"] = min(out["contacts_min"], cr["num_contacts"]); out["contacts_max"] = max(out["contacts_max"], cr["num_contacts"])
    return out


def replay_reference_order(make_candidate, make_reference, sc, steps, dataflow=False, stats=None):
    """Free-running, no state is ever copied: every step the candidate is told the axis the reference swept along and the order in which the
    reference emitted (= solves) its contact manifolds, and solves sequentially in that order (joints in pool order).  It must then BE the
    reference: every count, the contact list in order, every pose and velocity bit, every step."""
    ref = sc.populate(make_reference()); cand = sc.populate(make_candidate())
    s = sc.settings(); ids = np.arange(sc.num_bodies, dtype=np.uint32)
    most = 0
    if dataflow:     # the order goes through the production solver (levels of the order as colours: include/mi_physics.h, mi_debug_set_solve_dataflow)
        cand.debug_set_solve_dataflow(True)
    for i in range(steps):
        ref.step_fixed(s, sc.dt, 1)
        cr = ref.counts(); con = ref.contacts()
        cand.debug_set_sweep_axis(cr["sorting_axis"])
        cand.debug_set_solve_order(manifold_order(con))
        cand.step_fixed(s, sc.dt, 1)
        cc = cand.counts()
        if dataflow and stats is not None:
            d = cand.debug_solve_order_depth()
            stats.append((d, cand.solver_kind() if d else -1, cr["num_contacts"], cr["num_collisions"]))
        _same_counts(cc, cr, i, ref.aabbs() if i % 8 == 0 else None, cr["sorting_axis"])
        assert contact_set(cand.contacts()) == contact_set(con), f"step {i}: contact lists"
        assert cand.get_body_states(ids).tobytes() == ref.get_body_states(ids).tobytes(), f"step {i}: body states differ from the reference's"
        most = max(most, cr["num_contacts"])
    return most


# --------------------------------------------------------------------------------------------------------------------------------------
# Caller-ordered steps (mi_debug_set_solve_order) among free ones
def next_manifolds(sc, oracle_mod, oracle_world):
    """The oriented collider pairs of the manifolds `oracle_world`'s NEXT step will find, in its list order: a scout oracle world loaded from a
    checkpoint of it takes that step (the world itself, its event queue included, is left alone)."""
    scout = sc.populate(oracle_mod.create_world(oracle_mod.ORDER_CANONICAL))
    scout.load_checkpoint(oracle_world.save_checkpoint())
    scout.step_fixed(sc.settings(), sc.dt, 1)
    pairs = manifold_order(scout.contacts())
    scout.close()
    return pairs


def make_order(pairs, prev_pairs, rng, kind):
    """A permutation of `pairs`: "random", or "new first" (the manifolds absent from the previous step's list first, each group shuffled)."""
    pairs = np.asarray(pairs, np.uint32).reshape(-1, 2)
    if kind == "random":
        return pairs[rng.permutation(len(pairs))]
    assert kind == "new first", kind
    old = {(int(a), int(b)) for a, b in np.asarray(prev_pairs).reshape(-1, 2)}
    is_new = np.array([(int(a), int(b)) not in old for a, b in pairs], bool)
    new, kept = pairs[is_new], pairs[~is_new]
    return np.concatenate([new[rng.permutation(len(new))], kept[rng.permutation(len(kept))]]).reshape(-1, 2)


def pair_priority(a, b):
    """pairPriority(colliderA, colliderB) (oracle/ora_world.cpp, kernels: the order of the greedy colouring), in Python integers."""
    m52 = (1 << 52) - 1
    x = (int(a) << 26) | int(b)
    x ^= x >> 25; x = (x * 0x9E3779B97F4A7) & m52
    x ^= x >> 27; x = (x * 0xC2B2AE3D27D4F) & m52
    x ^= x >> 23
    return x


def greedy_colors(pairs, heads, dyn):
    """Every manifold coloured from nothing: greedy in descending pair priority, the lowest colour below 64 free on both of its dynamic bodies
    (64 = overflow) — what a free step gives a manifold whose history colour is the overflow colour."""
    used = {}
    out = np.full(len(pairs), 64, np.uint32)
    for m in sorted(range(len(pairs)), key=lambda m: -pair_priority(*pairs[m])):
        bs = [int(b) for b in (heads["body_a"][m], heads["body_b"][m]) if int(b) in dyn]
        mask = 0
        for b in bs:
            mask |= used.get(b, 0)
        free = [c for c in range(64) if not (mask >> c) & 1]
        if free:
            out[m] = free[0]
            for b in bs:
                used[b] = used.get(b, 0) | (1 << free[0])
    return out
