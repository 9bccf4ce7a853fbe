"""CPU: the host argument checks of the four training-input entries (dsrg_amd/csrc/train_input_check.h).

Through the library as built: every row of tests/train_input_refusal_cases.py — a valid call with one thing wrong — is refused
with the code and the message, byte for byte, that the library of commit ec489fe gave (tests/golden/train_input_refusals.json,
recorded by tools/record_train_input_refusals.py when each launcher still carried its own copy of the checks).

Under AddressSanitizer + UndefinedBehaviorSanitizer: tests/train_input_check.cpp — a stand-alone program that includes nothing but
that header — asserts what the library path cannot reach without a GPU, the ACCEPTED inputs: the filled argument blocks, 32 images,
pieces that end exactly at the buffer's end, and the extreme offsets and sizes without signed overflow.  Built with
-fsanitize=address,undefined -fno-sanitize-recover=all and run as an ordinary child process."""
import json
import os
import shutil
import subprocess

import pytest
import torch

import train_input_refusal_cases as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "train_input_refusals.json")


def test_every_refusal_equals_the_recorded_one():
    if torch.cuda.is_available():
        pytest.skip("GPU present: the rows carry made-up device pointers")
    from dsrg_amd import _lib
    L = _lib.lib()
    with open(GOLDEN) as f:
        recorded = {(r["entry"], r["case"]): (r["code"], r["message"]) for r in json.load(f)["rows"]}
    rows = R.rows()
    assert len(rows) == len(set((e, n) for e, n, _ in rows)) and set(recorded) == set((e, n) for e, n, _ in rows)
    assert all(code in (_lib.ERR_INVALID, _lib.ERR_UNSUPPORTED) for code, _ in recorded.values())
    for entry, name, args in rows:
        assert R.call(L, entry, args) == recorded[entry, name], (entry, name)


def _runtime(name):
    path = subprocess.run(["g++", "-print-file-name=%s" % name], capture_output=True, text=True).stdout.strip()
    return path if os.path.isabs(path) and os.path.exists(path) else None


def test_accepted_inputs_and_extremes_hold_under_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("g++ is not installed")
    if _runtime("libasan.a") is None or _runtime("libubsan.a") is None:
        pytest.skip("g++'s sanitizer runtimes are not installed")
    exe = str(tmp_path / "train_input_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                           "-static-libasan", "-static-libubsan",      # (the runtimes linked in: nothing the environment preloads matters)
                           "-I", os.path.join(ROOT, "dsrg_amd", "csrc"), os.path.join(ROOT, "tests", "train_input_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    report = r.stdout[-3000:] + r.stderr[-3000:]
    assert r.returncode == 0, report
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, report
    assert "all properties hold" in r.stdout
