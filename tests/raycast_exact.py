"""The independent yardstick of the ray cast (mi_world_raycast): where a ray enters the SOLID collider, by closed forms in float64 and with
no epsilon of its own.  Unlike tests/raycast_ref.py it shares no arithmetic with the kernel: every solid is an intersection (or, for the
capsule, a union) of convex sets whose ray intervals are exact - ball and infinite cylinder by their quadratics, slab and half-space by one
division - so a hull is clipped against its face planes and a ray cannot slip between two triangles.

  shape_of(ctype, words, position, rotation, hull)   the world shape of a collider (overlap_ref.world_shape; a hull with its face planes)
  cast(shape, o, d, max_t)        the entry: t, point, normal, the entering constraints [(t_i, normal_i)], whether o is inside, the exit
  sdf(shape, p)                   the signed distance of a point from the solid (negative inside)
  closest_approach(shape, o, d, max_t)   the least sdf over the segment o + s d, s in [0, max_t]: > 0 a miss by that much, < 0 a hit that deep
  bounds(shape)                   a world box holding the shape"""
import numpy as np

import overlap_ref as R

SPHERE, CAPSULE, CYLINDER, AABB, OBB, HULL = range(6)
INF = np.inf


def shape_of(ctype, words, position, rotation, hull=None):
    """(type, parameters): sphere (c, r); capsule / cylinder (a, b, r); box (c, half, R) for AABB and OBB alike; hull (vertices, unit face
    normals n, offsets h: the solid is n x <= h)."""
    t, p = R.world_shape(ctype, words, position, rotation)
    if t == AABB:
        return OBB, ((p[0] + p[1]) / 2, (p[1] - p[0]) / 2, np.eye(3))
    if t == HULL:
        verts, tris = hull
        v = p[0] + np.asarray(verts, np.float64) @ p[1].T
        a, b, c = (v[np.asarray(tris)[:, i]] for i in range(3))
        n = np.cross(b - a, c - a)
        n /= np.linalg.norm(n, axis=1, keepdims=True)
        return HULL, (v, n, np.einsum("ij,ij->i", n, a), (a, b, c))
    return t, p


def bounds(shape):
    t, p = shape
    if t == SPHERE:
        return p[0] - p[1], p[0] + p[1]
    if t in (CAPSULE, CYLINDER):
        return np.minimum(p[0], p[1]) - p[2], np.maximum(p[0], p[1]) + p[2]
    if t == OBB:
        e = np.abs(p[2]) @ p[1]
        return p[0] - e, p[0] + e
    return p[0].min(axis=0), p[0].max(axis=0)


# ---- ray intervals of the convex pieces: (t_in, t_out, normal at t_in or None); empty = None.  The ray is o + t d, t over all reals.
def _ball(o, d, c, r):
    m = o - c
    A, B, C = d @ d, m @ d, m @ m - r * r
    disc = B * B - A * C
    if disc < 0:
        return None
    s = np.sqrt(disc)
    t0 = (-B - s) / A
    return t0, (-B + s) / A, (m + t0 * d) / r


def _tube(o, d, a, u, r):
    """The infinite cylinder of radius r about the line a + y u (u unit)."""
    m = o - a
    mp, dp = m - (m @ u) * u, d - (d @ u) * u
    A, B, C = dp @ dp, mp @ dp, mp @ mp - r * r
    if A == 0:
        return (-INF, INF, None) if C <= 0 else None
    disc = B * B - A * C
    if disc < 0:
        return None
    s = np.sqrt(disc)
    t0 = (-B - s) / A
    return t0, (-B + s) / A, (mp + t0 * dp) / r


def _halfspaces(o, d, n, h):
    """The polytope n_i x <= h_i: (t_in, t_out, entering (t_i, n_i) list, exiting (t_i, n_i) list) or None."""
    den, num = n @ d, h - n @ o
    if np.any((den == 0) & (num < 0)):
        return None
    with np.errstate(divide="ignore", invalid="ignore"):
        t = num / den
    ent, ext = den < 0, den > 0
    t_in = t[ent].max() if ent.any() else -INF
    t_out = t[ext].min() if ext.any() else INF
    if t_in > t_out:
        return None
    return t_in, t_out, [(t[i], n[i]) for i in np.nonzero(ent)[0]], [(t[i], n[i]) for i in np.nonzero(ext)[0]]


def _intersect(parts):
    """The interval of an intersection of convex pieces, each (t_in, t_out, entering list, exiting list)."""
    if any(p is None for p in parts):
        return None
    t_in, t_out = max(p[0] for p in parts), min(p[1] for p in parts)
    if t_in > t_out:
        return None
    return t_in, t_out, [e for p in parts for e in p[2]], [e for p in parts for e in p[3]]


def _unit(v):
    return v / np.linalg.norm(v)


def _interval(shape, o, d):
    """(t_in, t_out, entering constraints [(t_i, outward unit normal_i)], exiting ones) of the whole line through the solid, or None."""
    t, p = shape
    if t == SPHERE:
        b = _ball(o, d, p[0], p[1])
        return None if b is None else (b[0], b[1], [(b[0], b[2])], [(b[1], _unit(o + b[1] * d - p[0]))])
    if t == CYLINDER:
        a, b, r = p
        h = np.linalg.norm(b - a); u = (b - a) / h
        tube = _tube(o, d, a, u, r)
        if tube is None:
            return None
        side = (tube[0], tube[1], [] if tube[2] is None else [(tube[0], tube[2])],
                [] if tube[2] is None else [(tube[1], _unit((lambda m: m - (m @ u) * u)(o + tube[1] * d - a)))])
        return _intersect([side, _halfspaces(o, d, np.array([u, -u]), np.array([u @ b, -(u @ a)]))])
    if t == CAPSULE:
        a, b, r = p
        parts = [q for q in (_interval((CYLINDER, p), o, d), _interval((SPHERE, (a, r)), o, d), _interval((SPHERE, (b, r)), o, d)) if q is not None]
        if not parts:
            return None
        t_in, t_out = min(q[0] for q in parts), max(q[1] for q in parts)   # a union of convex pieces that is convex: one interval

        def normal(s):
            x = o + s * d
            y = np.clip((x - a) @ (b - a) / ((b - a) @ (b - a)), 0, 1)
            return _unit(x - (a + y * (b - a)))
        return t_in, t_out, [(t_in, normal(t_in))], [(t_out, normal(t_out))]
    if t == OBB:
        c, half, Rm = p
        axes = Rm.T / np.linalg.norm(Rm.T, axis=1, keepdims=True)   # the box's axes as unit rows
        n = np.concatenate([axes, -axes])
        return _intersect([_halfspaces(o, d, n, np.concatenate([axes @ c + half, -(axes @ c) + half]))])
    return _intersect([_halfspaces(o, d, p[1], p[2])])


def cast(shape, o, d, max_t=INF):
    """The ray's entry into the solid: dict(t, point, normal, entries [(t_i, normal_i)] = every surface the line enters through, inside,
    t_exit, exits) - t None on a miss (the solid behind the origin, beyond max_t, or not met), t = 0 with inside = True when the origin is
    in the solid.  `normal` is that of the last surface entered; where several meet, `entries` holds the others at (nearly) the same t_i."""
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    iv = _interval(shape, o, d)
    miss = dict(t=None, point=None, normal=None, entries=[], inside=False, t_exit=None, exits=[])
    if iv is None or iv[1] < 0:
        return miss
    t_in, t_out, entries, exits = iv
    inside = t_in <= 0
    t = 0.0 if inside else float(t_in)
    if t > max_t:
        return miss
    normal = max(entries, key=lambda e: e[0])[1] if entries else None
    return dict(t=t, point=o + t * d, normal=normal, entries=entries, inside=bool(inside), t_exit=float(t_out), exits=exits)


# ---- signed distance
def _point_triangles(p, a, b, c):
    """Distances of the point p from the triangles (a_i, b_i, c_i) (Ericson, Real-Time Collision Detection 5.1.5, vectorised)."""
    ab, ac, ap = b - a, c - a, p - a
    d1, d2 = np.einsum("ij,ij->i", ab, ap), np.einsum("ij,ij->i", ac, ap)
    bp = p - b
    d3, d4 = np.einsum("ij,ij->i", ab, bp), np.einsum("ij,ij->i", ac, bp)
    cp = p - c
    d5, d6 = np.einsum("ij,ij->i", ab, cp), np.einsum("ij,ij->i", ac, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    with np.errstate(divide="ignore", invalid="ignore"):
        den = va + vb + vc
        v, w = vb / den, vc / den
        q = a + ab * v[:, None] + ac * w[:, None]                                       # the face region
        e_ab = a + ab * (d1 / (d1 - d3))[:, None]
        e_ac = a + ac * (d2 / (d2 - d6))[:, None]
        e_bc = b + (c - b) * ((d4 - d3) / ((d4 - d3) + (d5 - d6)))[:, None]
    q = np.where(((va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0))[:, None], e_bc, q)
    q = np.where(((vb <= 0) & (d2 >= 0) & (d6 <= 0))[:, None], e_ac, q)
    q = np.where(((vc <= 0) & (d1 >= 0) & (d3 <= 0))[:, None], e_ab, q)
    q = np.where(((d6 >= 0) & (d5 <= d6))[:, None], c, q)
    q = np.where(((d3 >= 0) & (d4 <= d3))[:, None], b, q)
    q = np.where(((d1 <= 0) & (d2 <= 0))[:, None], a, q)
    return np.linalg.norm(p - q, axis=1)


def sdf(shape, x):
    t, p = shape
    x = np.asarray(x, np.float64)
    if t == SPHERE:
        return float(np.linalg.norm(x - p[0]) - p[1])
    if t == CAPSULE:
        a, b, r = p
        y = np.clip((x - a) @ (b - a) / ((b - a) @ (b - a)), 0, 1)
        return float(np.linalg.norm(x - (a + y * (b - a))) - r)
    if t == CYLINDER:
        a, b, r = p
        h = np.linalg.norm(b - a); u = (b - a) / h
        y = (x - a) @ u
        dr, dy = np.linalg.norm(x - a - y * u) - r, abs(y - h / 2) - h / 2
        return float(min(max(dr, dy), 0.0) + np.hypot(max(dr, 0.0), max(dy, 0.0)))
    if t == OBB:
        c, half, Rm = p
        axes = Rm.T / np.linalg.norm(Rm.T, axis=1, keepdims=True)
        q = np.abs(axes @ (x - c)) - half
        return float(np.linalg.norm(np.maximum(q, 0.0)) + min(q.max(), 0.0))
    deepest = float((p[1] @ x - p[2]).max())
    return deepest if deepest <= 0 else float(_point_triangles(x, *p[3]).min())


def closest_approach(shape, o, d, max_t=INF):
    """(the least signed distance over the segment o + s d, 0 <= s <= max_t; the s it is reached at).  The signed distance from a convex
    solid is convex along a line: golden-section search, over the part of the segment in front of the far side of a ball holding the shape."""
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    mn, mx = bounds(shape)
    c, rad = (mn + mx) / 2, np.linalg.norm(mx - mn) / 2
    length = np.linalg.norm(d)
    lo, hi = 0.0, float(min(max_t, max(0.0, (c - o) @ d / (length * length) + rad / length)))
    f = lambda s: sdf(shape, o + s * d)   # noqa: E731
    g = (np.sqrt(5.0) - 1) / 2
    x1, x2 = hi - g * (hi - lo), lo + g * (hi - lo)
    f1, f2 = f(x1), f(x2)
    for _ in range(64):
        if f1 <= f2:
            hi, x2, f2 = x2, x1, f1
            x1 = hi - g * (hi - lo); f1 = f(x1)
        else:
            lo, x1, f1 = x1, x2, f2
            x2 = lo + g * (hi - lo); f2 = f(x2)
    best = min((f(0.0), 0.0), (f1, x1), (f2, x2), (f(hi), hi))
    return float(best[0]), float(best[1])
