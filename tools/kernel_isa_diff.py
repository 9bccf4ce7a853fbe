#!/usr/bin/env python
"""Are the kernels of two builds of one .hip file the same instructions?  No GPU needed.
usage: tools/kernel_isa_diff.py OLD.s NEW.s [--map 'OLD-NAME-REGEX=NEW-NAME' ...]
The two files are device assembly of the same source at two commits: the Makefile's CXXFLAGS plus --cuda-device-only -S.
Kernels are paired by demangled name (template arguments kept, parameter list dropped); --map renames an old kernel
first (re.sub on its name).  Before the comparison comments and directives are dropped, labels renumbered in order of
appearance and mangled symbol names replaced by a placeholder.  Prints one line per kernel: identical, or the first line
that differs, or the side that lacks it."""
import re, shutil, subprocess, sys


def kernels(path):
    """{demangled name: [instruction lines]} of every function of the file, in file order"""
    out, body = {}, None
    for ln in open(path):
        ln = ln.split(";")[0].rstrip()
        m = re.match(r"(_Z\w+):$", ln)
        if m:
            body = out.setdefault(m.group(1), [])
        elif re.match(r"\s*\.(section|text)\b", ln):
            body = None
        elif body is not None and ln.strip() and (not ln.lstrip().startswith(".") or ln.endswith(":")):
            body.append(ln.strip())
    filt = shutil.which("llvm-cxxfilt") or shutil.which("c++filt") or sys.exit("needs llvm-cxxfilt or c++filt on PATH")
    names = subprocess.run([filt] + list(out), stdout=subprocess.PIPE, check=True).stdout.decode().splitlines()
    return {re.sub(r"^void |\(anonymous namespace\)::|\(.*", "", d): normalise(b) for d, b in zip(names, out.values())}


def normalise(body):
    labels = {}
    def label(m):
        return labels.setdefault(m.group(0), ".L%d" % len(labels))
    return [re.sub(r"_Z\w+", "SYM", re.sub(r"\.L\w+", label, ln)) for ln in body]


def main(argv):
    cut = argv.index("--map") if "--map" in argv else len(argv)
    files, maps = argv[:cut], [a.split("=", 1) for a in argv[cut + 1:]]
    if len(files) != 2 or any(len(m) != 2 for m in maps):
        sys.exit(__doc__)
    old, new = kernels(files[0]), kernels(files[1])
    renamed = {}
    for name, body in old.items():
        for pat, to in maps:
            name = re.sub(pat, to, name)
        renamed[name] = body
    same = 0
    for name in sorted(set(renamed) | set(new)):
        a, b = renamed.get(name), new.get(name)
        if a is None or b is None:
            print("%-90s only in %s" % (name, "NEW" if a is None else "OLD"))
        elif a == b:
            same += 1
            print("%-90s identical (%d instructions and labels)" % (name, len(a)))
        else:
            i = next((k for k, (p, q) in enumerate(zip(a, b)) if p != q), min(len(a), len(b)))
            print("%-90s DIFFERS at line %d of %d / %d:\n    old: %s\n    new: %s" % (
                name, i + 1, len(a), len(b), a[i] if i < len(a) else "(end)", b[i] if i < len(b) else "(end)"))
    print("%d kernels identical, %d in OLD, %d in NEW" % (same, len(old), len(new)))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
