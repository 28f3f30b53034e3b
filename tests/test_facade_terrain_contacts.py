"""The terrain contact query of the header-only C++ facade (include/physics_world.hpp: terrainContacts) run on the GPU against the bits the
oracle gives for the program's sunk sphere (compiling and linking it is part of tests/test_terrain_contacts.py)."""
import subprocess

import numpy as np
import pytest

import terrain_contact_ref as T
from test_terrain_contacts import build_facade


@pytest.mark.gpu
def test_facade_terrain_contacts_runs_on_gpu(tmp_path, mi_lib, oracle_mod):
    hm, vols = T.sunk_sphere_case()
    _, recs, _ = T.oracle_terrain_contacts(oracle_mod, hm, vols)
    last = recs[-1]
    words = [*last["point"].view(np.uint32), int(last["depth"].view(np.uint32)), *last["normal"].view(np.uint32)]
    r = subprocess.run([str(build_facade(tmp_path)), *(str(int(x)) for x in words)], capture_output=True, text=True)
    assert r.returncode == 0 and "facade terrain contacts ok" in r.stdout, r.stdout + r.stderr
