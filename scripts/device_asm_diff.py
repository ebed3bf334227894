"""Is the device code of every translation unit the same as in another commit?  No GPU needed.

    python scripts/device_asm_diff.py [--parent REV] [--jobs N] > profiles/<name>.txt

For every file of build.SOURCES the parent revision (default HEAD) and the working tree are compiled with
`hipcc <flags_for(src)> --offload-device-only -S`; the two assembly texts are compared after the lines that contain
`__hip_cuid_` are dropped (a hash of the compilation unit, which changes with any edit).  One line per file, and for a file
that differs one line per function (identical / CHANGED / new / gone: a file that gained a kernel differs as a whole); exit
status 1 if any file differs.
"""
import argparse
import difflib
import os
import re
import subprocess
import sys
import tarfile
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from schnetpack_amd.csrc import build as B  # noqa: E402

CSRC = os.path.join("schnetpack_amd", "csrc")


def device_asm(tree, src, out):
    path = os.path.join(tree, CSRC, src)
    if not os.path.exists(path):
        return None
    subprocess.check_call([B._hipcc()] + B.flags_for(src) + ["--offload-device-only", "-S", path, "-o", out],
                          stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    with open(out) as f:
        return [ln for ln in f if "__hip_cuid_" not in ln]


def functions(lines):
    """{symbol: its lines} of an assembly text: from the label of a mangled function to its .Lfunc_end."""
    out, cur = {}, None
    for ln in lines:
        if cur is None:
            m = re.match(r"^(_Z\w+):", ln)
            if m:
                cur = out.setdefault(m.group(1), [])
        elif ln.startswith(".Lfunc_end"):
            cur = None
        else:
            cur.append(ln)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default="HEAD")
    ap.add_argument("--jobs", type=int, default=8)
    args = ap.parse_args()
    rev = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", args.parent]).decode().strip()
    differ = 0
    with tempfile.TemporaryDirectory() as tmp:
        parent = os.path.join(tmp, "parent")
        os.makedirs(parent)
        tar = os.path.join(tmp, "parent.tar")
        subprocess.check_call(["git", "-C", ROOT, "archive", "-o", tar, args.parent, CSRC, "include"])
        with tarfile.open(tar) as t:
            t.extractall(parent)
        with ThreadPoolExecutor(args.jobs) as pool:
            jobs = [(s, pool.submit(device_asm, parent, s, os.path.join(tmp, "p_" + s + ".s")),
                     pool.submit(device_asm, ROOT, s, os.path.join(tmp, "b_" + s + ".s"))) for s in B.SOURCES]
            print("device assembly, parent %s against the working tree (lines with __hip_cuid_ dropped)" % rev)
            for s, fp, fb in jobs:
                a, b = fp.result(), fb.result()
                if a is None or b is None:
                    print("%-24s %s" % (s, "only in the working tree" if a is None else "only in the parent"))
                    differ += 1
                elif a == b:
                    print("%-24s identical  %6d lines" % (s, len(a)))
                else:
                    d = [ln for ln in difflib.unified_diff(a, b, "parent", "branch", n=0) if ln[0] in "+-" and ln[:3] not in ("+++", "---")]
                    print("%-24s DIFFERENT  %6d / %d lines, %d changed" % (s, len(a), len(b), len(d)))
                    # per function: a file that gained a kernel differs as a whole, its other kernels need not
                    fa, fb = functions(a), functions(b)
                    for name in sorted(set(fa) | set(fb)):
                        state = "new" if name not in fa else "gone" if name not in fb else "identical" if fa[name] == fb[name] else "CHANGED"
                        print("    %-9s %6d lines  %s" % (state, len(fb.get(name, fa.get(name))), name))
                    if any(n in fa and n in fb and fa[n] != fb[n] for n in fa):
                        sys.stdout.writelines("    " + ln for ln in d[:40])
                    differ += 1
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
