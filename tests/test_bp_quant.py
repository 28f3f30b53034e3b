"""The compact candidate row of the broad phase (d3d12renderer_amd/csrc/bp_quant.hpp): the quantiser is conservative.  The header is plain C++; a small stand-alone
program (tests/bp_quant_check.cpp) is built with the host compiler and run: 1.2 million random box pairs on random frames — equal bounds, coinciding faces, denormals,
infinities, a NaN in every position, inverted boxes, bounds on and beyond the frame's ends, degenerate frames — and not one pair that the exact closed-interval test
accepts may fail the quantised test."""
import re
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def test_quantised_test_never_rejects_an_exact_overlap(tmp_path):
    exe = tmp_path / "bp_quant_check"
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", str(ROOT / "tests" / "bp_quant_check.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe), "1200000"], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    m = re.search(r"pairs (\d+) exact_overlaps (\d+) quantised_passes (\d+) nan_pairs (\d+) violations (\d+)", r.stdout)
    assert m, r.stdout + r.stderr
    pairs, exact, quant, nan_pairs, violations = map(int, m.groups())
    assert violations == 0 and r.returncode == 0, r.stdout[-4000:]
    assert pairs >= 1_000_000
    # the run is not vacuous: many exact overlaps were put to the test, NaN rows occurred, and the quantised test does reject pairs
    assert exact > pairs // 20 and nan_pairs > pairs // 100 and quant >= exact and quant < pairs
