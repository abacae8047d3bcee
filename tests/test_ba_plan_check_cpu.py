"""The local BA's host-only pieces from C++ (tests/c/ba_plan_check.cpp, recipe tests/c/ba_plan_check.mk): the
line-workgroup packing of the staging into a table sized exactly by its bound, and the window plan against the chunk
plan and the update geometry spelled out.  The program makes no device call.  No GPU needed."""
import pathlib
import subprocess

import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]


@pytest.mark.parametrize("target", ["ba_plan_check", "ba_plan_check_san"])
def test_host_check_program(target):
    """plain: linked with the library's own objects; _san: the same program with ba_plan.cpp, ba_stage.cpp and
    common.cpp under ASan + UBSan, run directly, so a table entry past the bound is a reported heap overflow"""
    make = subprocess.run(["make", "-C", str(ROOT / "tests" / "c"), "-f", "ba_plan_check.mk", target],
                          capture_output=True, text=True)
    assert make.returncode == 0, make.stdout + make.stderr
    r = subprocess.run([str(ROOT / "tests" / "c" / "build" / target)], capture_output=True, text=True)
    assert r.returncode == 0 and "ba_plan_check: ok" in r.stdout, r.stdout + r.stderr
