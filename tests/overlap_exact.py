"""Float64 CERTIFICATES of the volume-overlap scene query (include/mi_physics.h, mi_world_overlap); numpy only, no GPU.

A verdict on two convex shapes is never taken from an iterative algorithm here.  It is a certificate that closed-form code verifies:

  * APART BY delta: a unit direction n with  -h_V(-n) - h_C(n) >= delta,  h the SUPPORT FUNCTION of a shape (`support_value`): the plane
    with normal n has all of C on one side and all of V at least delta further along n;
  * OVERLAPPING BY rho: a point p with the ball B(p, rho) inside both shapes, by the INSIDE DEPTH of p in each (`inside_depth`:
    how far p lies from the shape's boundary, negative outside): sphere r - |p - c|; capsule r - distance to the segment; cylinder the smaller
    of the radial and the axial slack; box the smallest half - |local|; hull the smallest plane slack over the geometry's triangles, each
    oriented away from the centroid.  For a DEGENERATE volume (no interior: a point, a segment, a flat box) the certificate is a point p of
    the volume (depth_V(p) >= -1e-9, counted against the certificate) that lies rho deep in the collider: the volume moved by less than rho
    still overlaps it.

Shapes are overlap_ref world shapes (type, parameters), a hull with its geometry: (HULL, (position, rotation matrix, vertices, planes)).
tests/sweep_ref.core_distance may PROPOSE n and p (`propose_*`); nothing counts until `verify_*` has checked it.  A zero-length cylinder has
no axis and is out of scope (support_value and inside_depth raise)."""
import numpy as np

import overlap_ref as R
import sweep_ref as S


def shape_of(ctype, words, pos, rot, hull=None):
    """The world shape of collider words under a pose; hull = (vertices, triangles) of the geometry for a hull."""
    t, p = R.world_shape(ctype, words, pos, rot)
    if t == R.HULL:
        verts, tris = np.asarray(hull[0], np.float64), np.asarray(hull[1], np.int64)
        p = (p[0], p[1], verts, _hull_planes(verts, tris))
    return t, p


def _hull_planes(verts, tris):
    """(unit normals, a point of each plane) of the geometry's triangles, every normal oriented away from the vertex centroid."""
    a, b, c = verts[tris[:, 0]], verts[tris[:, 1]], verts[tris[:, 2]]
    n = np.cross(b - a, c - a)
    n = n / np.linalg.norm(n, axis=1, keepdims=True)
    n = n * np.sign(np.einsum("ij,ij->i", n, a - verts.mean(axis=0)))[:, None]
    return n, a


def _axis(a, b):
    u = b - a
    n = np.linalg.norm(u)
    if not n > 0:
        raise ValueError("a zero-length cylinder has no axis: out of scope")
    return u / n, n


# ---- closed forms
def support_value(shape, u):
    """h(u) = max over the shape of x . u."""
    t, p = shape
    u = np.asarray(u, np.float64)
    if t == R.SPHERE:
        return float(p[0] @ u + p[1] * np.linalg.norm(u))
    if t == R.CAPSULE:
        return float(max(p[0] @ u, p[1] @ u) + p[2] * np.linalg.norm(u))
    if t == R.CYLINDER:
        ax, _ = _axis(p[0], p[1])
        return float(max(p[0] @ u, p[1] @ u) + p[2] * np.sqrt(max(0.0, u @ u - (u @ ax) ** 2)))
    if t == R.AABB:
        return float(np.maximum(p[0] * u, p[1] * u).sum())
    if t == R.OBB:
        return float(p[0] @ u + p[1] @ np.abs(p[2].T @ u))
    return float(p[0] @ u + (p[2] @ (p[1].T @ u)).max())


def _seg_distance(a, b, x):
    ab = b - a
    aa = ab @ ab
    s = min(1.0, max(0.0, (x - a) @ ab / aa)) if aa > 0 else 0.0
    return float(np.linalg.norm(x - (a + s * ab)))


def inside_depth(shape, x):
    """The radius of the largest ball about x inside the shape; negative: x is outside (then some lower bound of how far)."""
    t, p = shape
    x = np.asarray(x, np.float64)
    if t == R.SPHERE:
        return float(p[1] - np.linalg.norm(x - p[0]))
    if t == R.CAPSULE:
        return float(p[2] - _seg_distance(p[0], p[1], x))
    if t == R.CYLINDER:
        ax, ln = _axis(p[0], p[1])
        s = (x - p[0]) @ ax
        radial = p[2] - np.linalg.norm(x - p[0] - s * ax)
        return float(min(radial, s, ln - s))
    if t == R.AABB:
        return float(np.minimum(x - p[0], p[1] - x).min())
    if t == R.OBB:   # the image of the box under the matrix p[2] (a rotation up to the rounding of its quaternion): face i has the normal inv[i]
        inv = np.linalg.inv(p[2])
        return float(((p[1] - np.abs(inv @ (x - p[0]))) / np.linalg.norm(inv, axis=1)).min())
    pos, rot, _, (n, a) = p
    inv = np.linalg.inv(rot)                    # (the same: a local plane with normal n has the world normal inv^T n)
    return float((np.einsum("ij,ij->i", n, a - inv @ (x - pos)) / np.linalg.norm(n @ inv, axis=1)).min())


# ---- the checkers: the certificate's size, <= 0 when it proves nothing
def verify_apart(vol, col, n):
    """delta of the separating direction n (from the collider towards the volume); the direction must be of unit length."""
    n = np.asarray(n, np.float64)
    if not np.isfinite(n).all() or abs(np.linalg.norm(n) - 1.0) > 1e-9:
        return -np.inf
    return -support_value(vol, -n) - support_value(col, n)


def verify_overlap(vol, col, p, degenerate_volume=False):
    """rho of the common point p."""
    p = np.asarray(p, np.float64)
    if not np.isfinite(p).all():
        return -np.inf
    dv, dc = inside_depth(vol, p), inside_depth(col, p)
    if degenerate_volume:
        return dc + min(dv, 0.0) if dv >= -1e-9 else -np.inf
    return min(dv, dc)


# ---- proposals (not trusted)
def _convex(shape):
    t, p = shape
    return S.convex((R.HULL, (p[0], p[1])), p[2]) if t == R.HULL else S.convex(shape)


def propose_apart(vol, col):
    """A separating direction from the cores' closest points, or None where the cores meet."""
    dist, n, _ = S.core_distance(_convex(vol), _convex(col))
    return n if dist > 0 else None


def with_hull(world_shape, hull):
    """An overlap_ref world shape as the shape of this module: a hull gets its geometry (vertices, triangles)."""
    t, p = world_shape
    if t != R.HULL:
        return world_shape
    verts, tris = np.asarray(hull[0], np.float64), np.asarray(hull[1], np.int64)
    return t, (p[0], p[1], verts, _hull_planes(verts, tris))


def certify(vol, col):
    """(True, rho), (False, delta) or (None, 0.0) where neither certificate verifies: a proposal from the cores' closest points, checked."""
    cv, cc = _convex(vol), _convex(col)
    dist, n, pb = S.core_distance(cv, cc)
    if dist > 0:
        d = verify_apart(vol, col, n)
        if d > 0:
            return False, d
        start, step = pb + (S.margin(cc) + 0.5 * d) * n, max(-0.25 * d, 1e-4)   # (the middle of the overlap along n)
    else:
        n, start, step = None, pb, 0.02
    rho = verify_overlap(vol, col, propose_overlap(vol, col, start, step, n))
    return (True, rho) if rho > 0 else (None, 0.0)


def centre(shape):
    t, p = shape
    if t == R.SPHERE:
        return p[0]
    if t in (R.CAPSULE, R.CYLINDER, R.AABB):
        return (p[0] + p[1]) / 2
    if t == R.OBB:
        return p[0]
    return p[0] + p[1] @ p[2].mean(axis=0)


def nearest_core_point(vol, x):
    """The point of a degenerate volume (zero radius: its centre / segment; a box, flat or not: the box) nearest to x."""
    t, p = vol
    x = np.asarray(x, np.float64)
    if t == R.SPHERE:
        return p[0]
    if t in (R.CAPSULE, R.CYLINDER):
        ab = p[1] - p[0]
        aa = ab @ ab
        return p[0] + (min(1.0, max(0.0, (x - p[0]) @ ab / aa)) if aa > 0 else 0.0) * ab
    if t == R.AABB:
        return np.clip(x, p[0], p[1])
    return p[0] + p[2] @ np.clip(np.linalg.solve(p[2], x - p[0]), -p[1], p[1])


def propose_overlap(vol, col, start, step, n=None, degenerate_volume=False, rounds=60, also=()):
    """A common point of large depth by a pattern search from `start` (the depth is concave: any ascent helps; nothing needs the optimum);
    n = a direction to try first, in steps of `step`; also = further starting points."""
    f = lambda x: verify_overlap(vol, col, x, degenerate_volume)   # noqa: E731
    if degenerate_volume:
        return nearest_core_point(vol, start)   # (a search would leave the volume: the point of the core next to the caller's)
    best = np.asarray(start, np.float64); fb = f(best)
    cands = [centre(vol), centre(col), (centre(vol) + centre(col)) / 2] + [np.asarray(c, np.float64) for c in also]
    if n is not None:
        cands += [best + k * step * n for k in (-8, -4, -2, -1, -0.5, 0.5, 1, 2, 4, 8)]
    for cand in cands:
        fc = f(cand)
        if fc > fb:
            best, fb = cand, fc
    dirs = np.concatenate([np.eye(3), -np.eye(3)])
    if n is not None:
        dirs = np.concatenate([dirs, [n, -n]])
    for _ in range(rounds):
        moved = False
        for d in dirs:
            c = best + step * d
            fc = f(c)
            if fc > fb:
                best, fb, moved = c, fc, True
        if not moved:
            step *= 0.5
            if step < 1e-3 * max(fb, 1e-12):
                break
    return best
