"""The yardstick of the terrain contact scene query, from the oracle alone (no GPU): the volume sets that tests/test_gpu_terrain_contacts.py
compares bit for bit hold every case the device pipeline treats differently, so that comparison is not vacuous.  Also the record layout of
the binding, the header's declarations and that the facade program compiles."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import terrain_contact_ref as T
from d3d12renderer_amd import capi

ROOT = Path(__file__).resolve().parent.parent
STASH = 16      # kHmStash (csrc/heightmap.hpp)
CAP = 255       # kHmMaxContacts


@pytest.fixture(scope="module")
def sets(oracle_mod):
    out = {}
    for name in T.MAPS:
        hm, vols, labels = T.volume_set(name)
        offsets, recs, boxes = T.expected(oracle_mod, name)
        out[name] = (hm, vols, labels, np.diff(offsets.astype(np.int64)), recs, boxes)
    return out


@pytest.mark.parametrize("name", list(T.MAPS))
def test_every_type_touches_the_terrain(sets, name):
    hm, vols, labels, n, recs, boxes = sets[name]
    print(f"{name}: {len(vols)} volumes, {len(recs)} contacts, counts up to {n.max()}")
    for t in T.TYPES:
        m = vols["type"] == t
        assert m.sum() >= 40 and 2 * (n[m] > 0).sum() >= m.sum(), f"type {t}: {(n[m] > 0).sum()} of {m.sum()} volumes touch the terrain"
    low_only = np.isin(vols["type"], (capi.CYLINDER, capi.HULL))
    assert (n[low_only] <= 1).all() and (n[low_only] == 1).any()
    first = np.concatenate([[0], np.cumsum(n)])[:-1]
    for v in np.flatnonzero(low_only & (n == 1)):
        assert tuple(recs["normal"][first[v]]) == (0.0, -1.0, 0.0)
    assert (recs["depth"] >= 0).all()


def test_the_boundaries_of_the_pipeline_are_in_the_sets(sets):
    counts = np.concatenate([sets[name][3] for name in T.MAPS])
    assert (counts == STASH).any() and (counts == STASH + 1).any(), "no volume at the stash boundary (16 and 17 contacts)"
    assert counts.max() == CAP
    hm, vols, labels, n, recs, boxes = sets["fine"]
    assert n[labels["cap"]] == CAP
    for cells in (64, 65):
        v = labels[f"window {cells}"]
        assert int(vols["type"][v]) in T.TRIANGLE_TYPES and T.largest_window(hm, boxes[v]) == cells and n[v] > 0, (cells, T.chunk_windows(hm, boxes[v]))
    windows = np.array([T.largest_window(h, b) for name in T.MAPS for h, b in ((sets[name][0], b) for b in sets[name][5])])
    assert (windows <= 64).sum() > 50 and (windows > 64).sum() > 50, "both the plain and the large-window instance need work"
    for name in T.MAPS:
        hm, vols, labels, n, recs, boxes = sets[name]
        two = [c for _, _, c in T.chunk_windows(hm, boxes[labels["two chunks"]])]; four = [c for _, _, c in T.chunk_windows(hm, boxes[labels["four chunks"]])]
        assert len(two) == 2 and min(two) > 0 and len(four) == 4 and min(four) > 0, (name, two, four)
        assert n[labels["two chunks"]] > 0 and n[labels["four chunks"]] > 0, name
        assert n[labels["outside"]] == 0 and n[labels["above"]] == 0 and n[labels["invalid"]] == 0, name
        assert T.is_invalid(vols).sum() == 1
    hm, vols, labels, n, recs, boxes = sets["coarse"]
    assert n[labels["hole"]] == 0 and n[labels["hole box"]] == 0
    assert [(x, z) for x, z, _ in T.chunk_windows(hm, boxes[labels["hole"]])] == [(1, 0)] and (1, 0) not in hm["chunks"]
    # the volume over the map's centre reaches into the hole chunk and reports only what the three others give
    assert (1, 0) in [(x, z) for x, z, _ in T.chunk_windows(hm, boxes[labels["four chunks"]])]
    seg = recs[np.cumsum(n)[labels["four chunks"]] - n[labels["four chunks"]]:np.cumsum(n)[labels["four chunks"]]]
    tri = seg[:-1] if tuple(seg["normal"][-1]) == (0.0, -1.0, 0.0) else seg
    assert not ((tri["point"][:, 0] > 0.02) & (tri["point"][:, 2] < -0.02)).any()


def test_the_facade_case(oracle_mod):
    hm, vols = T.sunk_sphere_case()
    offsets, recs, _ = T.oracle_terrain_contacts(oracle_mod, hm, vols)
    assert offsets[1] == 0 and offsets[2] == len(recs) >= 1
    last = recs[-1]
    assert tuple(last["normal"]) == (0.0, -1.0, 0.0) and 0.1000 < float(last["depth"]) < 0.1001 and int(last["volume"]) == 1


def test_record_layout_and_header():
    d = capi.terrain_contact_dtype
    assert d.itemsize == 32
    assert [d.fields[n][1] for n in ("point", "depth", "normal", "volume")] == [0, 12, 16, 28]
    header = (ROOT / "include" / "mi_physics.h").read_text()
    for symbol in ("mi_world_terrain_contacts", "mi_world_terrain_contacts_device_async"):
        assert re.search(rf"MI_API int {symbol}\(", header), symbol
    assert "typedef struct mi_terrain_contact" in header
    for name in ("terrain_contacts", "terrain_contacts_raw", "terrain_contacts_device_async"):
        assert callable(getattr(capi.World, name))


def build_facade(tmp_path):
    exe = tmp_path / "facade_terrain_contacts"
    libdir = ROOT / "d3d12renderer_amd"
    subprocess.run(["g++", "-std=c++17", f"-I{ROOT / 'include'}", str(ROOT / "tests" / "facade_terrain_contacts.cpp"), "-o", str(exe),
                    f"-L{libdir}", "-lmi_physics", f"-Wl,-rpath,{libdir}"], check=True)
    return exe


def test_facade_terrain_contacts_compiles_and_links(tmp_path, mi_lib):
    assert build_facade(tmp_path).exists()
    assert mi_lib.create_world is not None
    import ctypes
    lib = ctypes.CDLL(str(ROOT / "d3d12renderer_amd" / "libmi_physics.so"))
    assert lib.mi_world_terrain_contacts and lib.mi_world_terrain_contacts_device_async
