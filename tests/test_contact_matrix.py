"""The contact-manifold matrix (tests/contact_matrix.py) without a GPU: the oracle against the reference's own narrow phase on every case, the
matrix's coverage on the oracle's output, and the truth table of min / max / clamp that the two restatements share with the reference.

Found by this matrix and fixed with it: the reference's max is `(a < b) ? b : a` (src/pch.h:64-67); the product and the oracle both had
`a > b ? a : b`, which differs when the two do not compare.  closestOnSegment on a zero-length segment computes clamp(0/0, 0, 1): the reference
goes on with t = 0, the restatements went on with NaN and dropped the pair.  27 cases of the `degenerate` family (a zero-length capsule volume
against a sphere, a zero-radius cylinder volume against a sphere and against a capsule: 9 each) had one finite contact in the reference and none
in the oracle; the GPU agreed with the oracle, so no GPU-versus-oracle test could see it."""
import subprocess

import numpy as np
import pytest

import contact_matrix as CM
from d3d12renderer_amd import build as hip_build

needs_reference = pytest.mark.skipif(not __import__("oracle").reference_available(), reason="neither /root/reference nor a prebuilt oracle/_ref/libref.so")


def _who(name, i, c):
    return f"{name}[{i}] {CM.TYPES[c['vt']]} -> {CM.TYPES[c['ct']]} {c['tag']}"


# ---- 1. the yardstick itself
@needs_reference
@pytest.mark.parametrize("name", CM.FAMILIES)
def test_reference_equals_oracle(oracle_mod, name):
    """One step of the case's two-entity world by the reference's own code and by the oracle in the reference's order: the same contact list,
    byte for byte, for every case of the family."""
    cases = CM.family(name)
    make_oracle = lambda: oracle_mod.create_world(oracle_mod.ORDER_REFERENCE)   # noqa: E731
    differ = []
    for i, c in enumerate(cases):
        r, o = CM.step_contacts(oracle_mod.create_reference_world, c), CM.step_contacts(make_oracle, c)
        if r.tobytes() != o.tobytes():
            differ.append(f"{_who(name, i, c)}: the reference has {len(r)} contacts, the oracle {len(o)}")
    print(f"{name}: {len(cases)} cases, {len(differ)} differ")
    assert not differ, f"{len(differ)} of {len(cases)} cases differ:\n" + "\n".join(differ[:30])


# ---- 2. the cap
@pytest.mark.parametrize("name", CM.FAMILIES)
def test_the_cap(oracle_mod, name):
    """On the oracle's output: every (family, pair) the family applies to has at least 3 manifolds and at least 3 misses (containment: manifolds
    only), every manifold has 1 to 4 contacts, the family reaches the sizes CM.REACHES lists for it, and no manifold holds a non-finite number."""
    cases, manifolds = CM.family(name), CM.oracle_manifolds(oracle_mod, name)
    table, sizes, bad = CM.coverage(cases, manifolds)
    print(f"{name}: {len(cases)} cases, {sum(m is not None for m in manifolds)} manifolds, sizes {sorted(sizes)}; fewest manifolds per pair "
          f"{min(table.get(p, (0, 0))[0] for p in CM.APPLIES[name])}, fewest misses {min(table.get(p, (0, 0))[1] for p in CM.APPLIES[name])}")
    CM.check_cap(name, table, sizes, bad)


def test_every_manifold_size_is_reached(oracle_mod):
    """Sizes 1, 2, 3 and 4 all occur in the matrix, and in the step worlds of the unit-scale families (on the oracle's output of the moved worlds,
    where each pair of each family keeps at least 3 manifolds and 3 misses too: CM.oracle_steps holds that)."""
    assert set().union(*(CM.coverage(CM.family(f), CM.oracle_manifolds(oracle_mod, f))[1] for f in CM.FAMILIES)) == {1, 2, 3, 4}
    per_family = {f: CM.oracle_steps(oracle_mod, f)[2] for f in CM.UNIT_FAMILIES}
    print({f: sorted(s) for f, s in per_family.items()})
    assert set().union(*per_family.values()) == {1, 2, 3, 4}


def test_every_equal_type_case_is_asked(oracle_mod):
    """The query items hold every case once, and an equal-type case without a manifold twice; a swapped item holds the other shape's very numbers."""
    for name in ("generic", "degenerate", "hull_shapes"):
        cases, manifolds = CM.family(name), CM.oracle_manifolds(oracle_mod, name)
        items = CM.query_items(cases, manifolds, CM.oracle_orientations(oracle_mod, name))
        per_case = np.bincount([it["case"] for it in items], minlength=len(cases))
        want = np.array([2 if m is None and c["vt"] == c["ct"] else 1 for c, m in zip(cases, manifolds)])
        assert np.array_equal(per_case, want), name
        swapped = [it for it in items if it["volume"].tobytes() != cases[it["case"]]["volume"].tobytes()]
        assert swapped and any(it["expect"] is not None for it in swapped) and any(it["expect"] is None for it in swapped), name
        for it in swapped:
            c = cases[it["case"]]; v = c["volume"][0]
            assert c["vt"] == c["ct"] and it["col_type"] == v["type"] and it["col_words"].tobytes() == v["shape"].tobytes() and it["col_pos"].tobytes() == v["position"].tobytes()
            w = it["volume"][0]
            assert w["type"] == c["col_type"] and w["shape"].tobytes() == c["col_words"].tobytes() and w["rotation"].tobytes() == c["col_rot"].tobytes()


def test_hull_shapes_geometries():
    """Geometry 3 is the unit cube, geometry 4 has at least 130 vertices with whole caps coplanar, and both are closed, outward-wound meshes."""
    import sweep_matrix as M
    cube, prism = M.hulls()[3], M.hulls()[4]
    assert len(cube[0]) == 8 and set(np.abs(cube[0]).ravel()) == {np.float32(0.5)}
    assert len(prism[0]) >= 130 and (prism[0][:, 1] == prism[0][0, 1]).sum() >= 65 and (prism[0][:, 1] == -prism[0][0, 1]).sum() >= 65
    for verts, tris in (cube, prism):
        v = verts.astype(np.float64)
        edges = {}
        for a, b, c in tris:
            assert np.dot(np.cross(v[b] - v[a], v[c] - v[a]), v[a] - v.mean(axis=0)) > 0
            for e in ((a, b), (b, c), (c, a)):
                edges[e] = edges.get(e, 0) + 1
        assert all(n == 1 and (b, a) in edges for (a, b), n in edges.items()) and set(np.unique(tris)) == set(range(len(verts)))


# ---- 3. the helpers' truth table, on the host
@pytest.mark.parametrize("header", ["dmath.hpp", "ora_math.h"])
def test_min_max_clamp_truth_table(tmp_path, header):
    """tests/dmath_minmax_check.cpp over the product's header (its routines are host and device ones: the host side of the HIP compiler, the library's floating-point flags)
    and over the oracle's (g++, the oracle's flags): max(0, NaN) = 0, max(NaN, 0) = NaN, max(+0, -0) = +0, max(-0, +0) = -0, min(0, NaN) = NaN,
    min(NaN, 0) = 0, clamp(NaN, 0, 1) = 0, clamp(-0, 0, 1) = +0, bit for bit."""
    src = str(hip_build.HERE.parent / "tests" / "dmath_minmax_check.cpp")
    exe = tmp_path / "dmath_minmax_check"
    if header == "dmath.hpp":
        cmd = [hip_build.hipcc(), "-x", "hip", "--cuda-host-only", "-std=c++17", "-O3", "-ffp-contract=off", "-fno-fast-math", src, "-o", str(exe)]
    else:
        cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-DCHECK_ORACLE", src, "-o", str(exe)]
    subprocess.run(cmd, check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    print(r.stdout)
    assert "rows wrong 0" in r.stdout and r.returncode == 0 and r.stdout.count(" ok\n") >= 8, r.stdout + r.stderr
