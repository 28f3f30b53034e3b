"""The terrain distance queries of the header-only C++ facade (include/physics_world.hpp: terrainDistance, terrainClearanceOfSphere,
distanceWithTerrain): compiled and linked with a plain C++17 compiler everywhere, run where there is a GPU."""
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


def _build(tmp_path, mi_lib):
    exe = tmp_path / "facade_terrain_distance"
    libdir = ROOT / "d3d12renderer_amd"
    subprocess.run(["g++", "-std=c++17", f"-I{ROOT / 'include'}", str(ROOT / "tests" / "facade_terrain_distance.cpp"), "-o", str(exe),
                    f"-L{libdir}", "-lmi_physics", f"-Wl,-rpath,{libdir}"], check=True)
    return exe


def test_facade_terrain_distance_compiles_and_links(tmp_path, mi_lib):
    assert _build(tmp_path, mi_lib).exists()


@pytest.mark.gpu
def test_facade_terrain_distance_runs_on_gpu(tmp_path, mi_lib):
    r = subprocess.run([str(_build(tmp_path, mi_lib))], capture_output=True, text=True)
    assert r.returncode == 0 and "facade terrain distance ok" in r.stdout, r.stdout + r.stderr
