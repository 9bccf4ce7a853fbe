"""CPU: the implicit-GEMM launch planners (dsrg_amd/csrc/igemm_plan.h) under AddressSanitizer + UndefinedBehaviorSanitizer.
tests/igemm_plan_check.cpp — a stand-alone program that includes nothing but that header — is built with
-fsanitize=address,undefined -fno-sanitize-recover=all and run as an ordinary child process (leak detection on): once to
assert the planners' properties over the train step's, the ResNet mode's and a handful of edge-case geometries, once to print
every decision it takes for them, which must equal tests/golden/igemm_plan_decisions.txt byte for byte.  The golden file was
recorded from the planners as they stood inside conv_igemm.hip before they moved to the header; a change that moves a decision
on purpose regenerates it (`igemm_plan_check --dump`) and says so."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "igemm_plan_decisions.txt")


def _runtime(name):
    path = subprocess.run(["g++", "-print-file-name=%s" % name], capture_output=True, text=True).stdout.strip()
    return path if os.path.isabs(path) and os.path.exists(path) else None


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ is not installed")
    if _runtime("libasan.a") is None or _runtime("libubsan.a") is None:
        pytest.skip("g++'s sanitizer runtimes are not installed")
    exe = str(tmp_path_factory.mktemp("igemm_plan") / "igemm_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                           "-static-libasan", "-static-libubsan",      # (the runtimes linked in: nothing the environment preloads matters)
                           "-I", os.path.join(ROOT, "dsrg_amd", "csrc"), os.path.join(ROOT, "tests", "igemm_plan_check.cpp"), "-o", exe])
    return exe


def _run(exe, *args):
    r = subprocess.run([exe] + list(args), capture_output=True, text=True, timeout=120)
    report = r.stdout[-3000:] + r.stderr[-3000:]
    assert r.returncode == 0, report
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, report
    return r.stdout


def test_planner_properties_hold_under_sanitizers(checker):
    assert "all properties hold" in _run(checker)


def test_planner_decisions_match_the_golden_dump(checker):
    with open(GOLDEN) as f:
        golden = f.read()
    assert _run(checker, "--dump") == golden
