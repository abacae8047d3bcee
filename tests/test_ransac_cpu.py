"""csrc/ransac.hpp on the host: tests/c/ransac_check.cpp instantiates the one RANSAC restatement with the host
compiler (no librspl, no GPU) and prints what it draws.

Pinned here: the live-generator sampler (the rspl_pnp_solve / rspl_fm_solve path) equals the oracles for both
model sizes; the walk of subset_at over the reduced table of raw draws (the gather kernels' path) finds the same
subsets; and draws_needed (the handles' table sizing) is the position at which that walk ends.  Count 8 is the
smallest count RANSAC runs at and the one with the most duplicate redraws."""
import json
import pathlib
import subprocess

import numpy as np
import pytest

import fm_ref

ROOT = pathlib.Path(__file__).resolve().parents[1]
EXE = ROOT / "tests" / "c" / "build" / "ransac_check"
ITERS = 100
CASES = [(5, 8), (5, 9), (5, 64), (5, 300), (7, 8), (7, 9), (7, 64)]


@pytest.fixture(scope="module")
def drawn():
    if not EXE.exists():
        subprocess.run(["make", "-C", str(ROOT / "tests" / "c"), "build/ransac_check"], check=True, capture_output=True)
    return json.loads(subprocess.run([str(EXE)], check=True, capture_output=True, text=True).stdout)


def test_every_case_is_printed(drawn):
    assert sorted((int(m), int(c)) for m, per in drawn.items() for c in per) == sorted(CASES)


@pytest.mark.parametrize("m,count", CASES)
def test_ransac_header_matches_the_oracles(drawn, m, count):
    import oracle
    got = drawn[str(m)][str(count)]
    live = np.asarray(got["live"], np.int32)
    ref = oracle.pnp_subsets(count, ITERS) if m == 5 else fm_ref.subsets(count, ITERS)[0]
    assert live.shape == (ITERS, m)
    np.testing.assert_array_equal(live, ref)
    # the device path: the same subsets from the table of raw draws
    np.testing.assert_array_equal(np.asarray(got["walk"], np.int32), live)
    # the table sizing: exactly the draws that walk consumed (every subset takes at least m draws)
    assert got["draws_needed"] == got["walk_end"] >= m * ITERS
