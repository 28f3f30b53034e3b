"""The contact-manifold query of the header-only C++ facade (include/physics_world.hpp: volumeContacts): compiled and linked with a plain
C++17 compiler everywhere, run where there is a GPU, against the bits the oracle gives for the program's single pair."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import contact_ref as CR

ROOT = Path(__file__).resolve().parent.parent


def _build(tmp_path, mi_lib):
    exe = tmp_path / "facade_volume_contacts"
    libdir = ROOT / "d3d12renderer_amd"
    subprocess.run(["g++", "-std=c++17", f"-I{ROOT / 'include'}", str(ROOT / "tests" / "facade_volume_contacts.cpp"), "-o", str(exe),
                    f"-L{libdir}", "-lmi_physics", f"-Wl,-rpath,{libdir}"], check=True)
    return exe


def test_facade_volume_contacts_compiles_and_links(tmp_path, mi_lib):
    assert _build(tmp_path, mi_lib).exists()


def test_the_oracle_pair_is_the_one_the_program_builds(oracle_mod):
    sc, vol = CR.sunk_sphere_case()
    expected, reversed_pairs, info = CR.oracle_manifolds(oracle_mod, sc, vol)
    assert list(expected) == [(0, 0)] and not reversed_pairs
    e = expected[(0, 0)]
    assert not e["volume_is_b"] and len(e["points"]) == 1 and abs(float(e["points"][0, 3]) - 0.1) < 1e-6 and tuple(e["normal"]) == (0.0, -1.0, 0.0)


@pytest.mark.gpu
def test_facade_volume_contacts_runs_on_gpu(tmp_path, mi_lib, oracle_mod):
    sc, vol = CR.sunk_sphere_case()
    e = CR.oracle_manifolds(oracle_mod, sc, vol)[0][(0, 0)]
    words = [*e["normal"].view(np.uint32), *e["points"][0].view(np.uint32), 1 | (256 if e["volume_is_b"] else 0)]
    r = subprocess.run([str(_build(tmp_path, mi_lib)), *(str(int(x)) for x in words)], capture_output=True, text=True)
    assert r.returncode == 0 and "facade volume contacts ok" in r.stdout, r.stdout + r.stderr
