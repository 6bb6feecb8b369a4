#!/usr/bin/env python3
"""Compare the device code of two builds kernel by kernel: the check of a refactor that must not change a kernel.

  isa_diff.py OLD_DIR NEW_DIR [--show N]

Each directory holds the device assembly of one build (hipcc ... --offload-arch=gfx950 --save-temps=obj writes
NAME-hip-amdgcn-amd-amdhsa-gfx950.s next to the object). Kernels are paired by demangled name, whichever file they sit in. Per
kernel: VGPRs, SGPRs, scratch, LDS, occupancy and code length of both builds, and whether the instruction stream is equal once
comments are stripped and labels renumbered in order of appearance. Of a stream that differs, the number of differing lines, how
many of them lie inside a loop (between a label and a later branch back to it), and with --show the first N of them.
Exit status 1 if any kernel differs in a figure or in its stream, or exists on one side only. Host tool, no GPU needed."""
import argparse
import difflib
import glob
import os
import re
import subprocess
import sys

FIGURES = [("vgpr", "NumVgprs"), ("sgpr", "TotalNumSgprs"), ("scratch", "ScratchSize"), ("lds", "LDSByteSize"), ("occ", "Occupancy"), ("bytes", "codeLenInByte")]
_LABEL = re.compile(r"\.L[A-Za-z_]*\d+(?:_\d+)?")


def kernels(directory):
    """{mangled name: (figures, normalised instruction lines)} of every kernel in the directory's device assembly"""
    out = {}
    for fn in sorted(glob.glob(os.path.join(directory, "*amdgcn*.s"))):
        lines = open(fn, errors="replace").read().splitlines()
        names = {ln.split()[1] for ln in lines if ln.strip().startswith(".amdhsa_kernel ")}
        i = 0
        while i < len(lines):
            m = re.match(r"^([A-Za-z_][\w$.]*):", lines[i])
            if not (m and m.group(1) in names):
                i += 1
                continue
            name, body, labels = m.group(1), [], {}
            i += 1
            while i < len(lines) and not lines[i].startswith(".Lfunc_end"):
                s = lines[i].split(";")[0].strip()
                i += 1
                if not s or (s.startswith(".") and not s.startswith(".L")):      # comments, directives (the kernel descriptor among them)
                    continue
                body.append(_LABEL.sub(lambda t: labels.setdefault(t.group(0), "L%d" % len(labels)), s))
            fig = {}
            while i < len(lines) and "; Occupancy:" not in lines[i - 1]:
                for key, tag in FIGURES:
                    m2 = re.match(r";\s*%s\s*[:=]\s*(\d+)" % tag, lines[i])
                    if m2:
                        fig[key] = int(m2.group(1))
                i += 1
            out[name] = (fig, body)
    return out


def loop_lines(body):
    """indices of the lines that lie inside a loop"""
    pos = {ln[:-1]: k for k, ln in enumerate(body) if ln.endswith(":")}
    inside = set()
    for k, ln in enumerate(body):
        t = ln.split()
        if t[0].startswith(("s_cbranch", "s_branch")) and pos.get(t[-1], k) < k:
            inside.update(range(pos[t[-1]], k + 1))
    return inside


def demangle(names):
    try:
        res = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
        return {n: re.sub(r"^\(anonymous namespace\)::|^void |\(.*$", "", d.replace("void (anonymous namespace)::", "")) for n, d in zip(names, res)}
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old"); ap.add_argument("new")
    ap.add_argument("--show", type=int, default=0, metavar="N", help="print the first N differing lines of every kernel whose stream differs")
    a = ap.parse_args(argv)
    old, new = kernels(a.old), kernels(a.new)
    nice = demangle(sorted(set(old) | set(new)))
    bad = 0
    print("%-52s %s  stream" % ("kernel", " ".join("%9s" % k for k, _ in FIGURES)))
    for name in sorted(set(old) | set(new), key=lambda n: nice[n]):
        if name not in old or name not in new:
            print("%-52s only in %s" % (nice[name], a.old if name in old else a.new)); bad += 1
            continue
        (fo, bo), (fn, bn) = old[name], new[name]
        cols = " ".join("%9s" % (fo.get(k) if fo.get(k) == fn.get(k) else "%s>%s" % (fo.get(k), fn.get(k))) for k, _ in FIGURES)
        verdict, shown = "equal", []
        if bo != bn:
            lo, ln_ = loop_lines(bo), loop_lines(bn)
            ndiff = nloop = 0
            for tag, i1, i2, j1, j2 in difflib.SequenceMatcher(None, bo, bn, autojunk=False).get_opcodes():
                if tag == "equal":
                    continue
                ndiff += max(i2 - i1, j2 - j1)
                nloop += sum(i in lo for i in range(i1, i2)) + sum(j in ln_ for j in range(j1, j2))
                shown += ["    - " + s for s in bo[i1:i2]] + ["    + " + s for s in bn[j1:j2]]
            verdict = "DIFFERS: %d lines (%d -> %d instructions), %d inside a loop" % (ndiff, len(bo), len(bn), nloop)
        bad += verdict != "equal" or fo != fn
        print("%-52s %s  %s" % (nice[name][:52], cols, verdict))
        for s in shown[:a.show]:
            print(s)
    print("%d kernels (%d on both sides), %d differ or are on one side only" % (len(set(old) | set(new)), len(set(old) & set(new)), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
