"""CPU: the planner of the grouped merged backward grid (merged_groups_plan and its parts, dsrg_amd/csrc/igemm_plan.h) under
AddressSanitizer + UndefinedBehaviorSanitizer.  tests/igemm_merged_plan_check.cpp — a stand-alone program that includes nothing but
that header — is built with -fsanitize=address,undefined -fno-sanitize-recover=all and run as an ordinary child process, as
test_igemm_plan.py does for the planners that were there before.  It asserts, for the train step's fc6 x4 and fc7 x4, the shapes of
test_gpu_igemm_merged_groups.py and degenerate inputs (an empty half, single blocks, 8 and 304 CUs): every tile and every weight-
gradient workgroup is exactly one block's, both halves of the grid start at multiples of 8 and share no id, and the price of the
choice is never above the model's price of the two launches."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _runtime(name):
    path = subprocess.run(["g++", "-print-file-name=%s" % name], capture_output=True, text=True).stdout.strip()
    return path if os.path.isabs(path) and os.path.exists(path) else None


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ is not installed")
    if _runtime("libasan.a") is None or _runtime("libubsan.a") is None:
        pytest.skip("g++'s sanitizer runtimes are not installed")
    exe = str(tmp_path_factory.mktemp("igemm_merged_plan") / "igemm_merged_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                           "-static-libasan", "-static-libubsan",      # (the runtimes linked in: nothing the environment preloads matters)
                           "-I", os.path.join(ROOT, "dsrg_amd", "csrc"), os.path.join(ROOT, "tests", "igemm_merged_plan_check.cpp"),
                           "-o", exe])
    return exe


def _run(exe, *args):
    r = subprocess.run([exe] + list(args), capture_output=True, text=True, timeout=120)
    report = r.stdout[-3000:] + r.stderr[-3000:]
    assert r.returncode == 0, report
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, report
    return r.stdout


def test_merged_groups_planner_properties_hold_under_sanitizers(checker):
    assert "all properties hold" in _run(checker)


def test_the_step_layers_are_priced_and_take_the_merged_grid(checker):
    out = _run(checker, "--print")
    rows = [ln for ln in out.splitlines() if "cus 256" in ln and ("fc6 x4, step" in ln or "fc7 x4, step" in ln)]
    assert len(rows) == 2 and all("one grid" in ln and "us merged" in ln for ln in rows), out
