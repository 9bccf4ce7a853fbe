#!/usr/bin/env python
"""Record what the four training-input entries answer to every row of tests/train_input_refusal_cases.py — return code and
dsrg_last_error() text — into tests/golden/train_input_refusals.json.  CPU only: the rows carry made-up device pointers, so the
tool refuses to run where a GPU is visible, and it aborts on a row that is not refused (DSRG_OK, or DSRG_ERR_HIP: the launch
was reached), since the table holds refusals only.

Run against the library of commit ec489fe, the last one in which each launcher carried its own copy of the checks (build that
commit and name its library in DSRG_LIB, or copy the cases module into a checkout of it); since then the checks are
dsrg_amd/csrc/train_input_check.h, and tests/test_train_input_refusals.py holds them to this file code for code and byte for byte.

usage: python tools/record_train_input_refusals.py [--out FILE]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main(argv):
    out_path = os.path.join(ROOT, "tests", "golden", "train_input_refusals.json")
    if "--out" in argv:
        out_path = argv[argv.index("--out") + 1]
    import torch
    if torch.cuda.is_available():
        sys.exit("a GPU is visible: a row that is not refused would launch on made-up pointers")
    import train_input_refusal_cases as R
    from dsrg_amd import _lib
    L = _lib.lib()
    rows = []
    for entry, name, args in R.rows():
        code, message = R.call(L, entry, args)
        if code in (_lib.OK, _lib.ERR_HIP):
            sys.exit("%s/%s is not refused (code %d): the table holds refusals only" % (entry, name, code))
        rows.append(dict(entry=entry, case=name, code=code, message=message))
    with open(out_path, "w") as f:
        json.dump(dict(commit="ec489fe", rows=rows), f, sort_keys=True, indent=0, separators=(",", ":"))
        f.write("\n")
    print("%d rows, %d bytes -> %s" % (len(rows), os.path.getsize(out_path), out_path))


if __name__ == "__main__":
    main(sys.argv[1:])
