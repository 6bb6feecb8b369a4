#!/usr/bin/env python3
"""Which template instantiations of the row-sweep and panel kernels exist in the built library, and which of them a run launched.

  kernel_inventory.py --compiled                 instantiations of each family, from `nm -C slepc_amd/libksgpu.so`
  kernel_inventory.py --launched TRACE.csv ...   per family: compiled / launched / never launched, from rocprofv3 --kernel-trace
                                                 CSV files (*_kernel_trace.csv; a directory is searched for them)
  --family NAME ...                              report these families only (a trace of part of the suite)

Host tool, no GPU needed. Instantiations no input can reach are listed in UNREACHABLE with the reason and reported apart."""
import argparse
import csv
import glob
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "slepc_amd", "libksgpu.so")
FAMILIES = ["k_gs_update", "k_dot_sweep", "k_dot_spmv_dict", "k_panel_mult", "k_panel_dot_direct", "k_panel_mult_direct", "k_multvec",
            "k_ritz_residual", "k_block_residual", "k_oblique_dot", "k_oblique_update", "k_restart_fused"]
_PAT = re.compile(r"\b(%s)<([^<>()]*)>\(" % "|".join(FAMILIES))

# instantiations no input reaches (the dispatch compiles them, nothing selects them)
UNREACHABLE = {
    "k_dot_spmv_dict<1,8,0>": "a Krylov step dots the new column and the one before it at least: ncols >= 2 (ks_gs.hip krylov_run, j + 2 columns)",
    "k_dot_spmv_dict<1,16,0>": "as k_dot_spmv_dict<1,8,0>",
    "k_dot_spmv_dict<1,8,5>": "as k_dot_spmv_dict<1,8,0> (the pair form of the same sweep)",
    "k_dot_spmv_dict<1,16,5>": "as k_dot_spmv_dict<1,8,0>",
}


def key(family, args):
    return "%s<%s>" % (family, ",".join(a.strip() for a in args.split(",")))


def compiled(lib=LIB):
    out = subprocess.run(["nm", "-C", lib], check=True, capture_output=True, text=True).stdout
    found = {f: set() for f in FAMILIES}
    for line in out.splitlines():
        if "__device_stub__" in line:
            continue
        m = _PAT.search(line)
        if m:
            found[m.group(1)].add(key(m.group(1), m.group(2)))
    return found


def launched(paths):
    files = []
    for p in paths:
        files += sorted(glob.glob(os.path.join(p, "**", "*kernel_trace.csv"), recursive=True)) if os.path.isdir(p) else [p]
    seen = {}
    for fn in files:
        with open(fn, newline="") as fh:
            for row in csv.DictReader(fh):
                name = row.get("Kernel_Name") or row.get("KernelName") or row.get("Name") or ""
                m = _PAT.search(name)
                if m:
                    k = key(m.group(1), m.group(2))
                    seen[k] = seen.get(k, 0) + 1
    return seen, files


def _sort_key(k):
    return [int(t) if t.isdigit() else t for t in re.split(r"[<>,]", k)]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--compiled", action="store_true", help="list the compiled instantiations")
    ap.add_argument("--launched", nargs="+", metavar="TRACE_CSV", help="rocprofv3 kernel-trace CSV files or directories")
    ap.add_argument("--lib", default=LIB)
    ap.add_argument("--family", nargs="+", choices=FAMILIES, metavar="NAME", help="report these families only")
    ap.add_argument("--verbose", action="store_true", help="with --launched: name every never-launched instantiation")
    a = ap.parse_args(argv)
    comp = compiled(a.lib)
    families = a.family or FAMILIES
    total = sum(len(comp[f]) for f in families)
    if a.compiled or not a.launched:
        for f in families:
            print("%-22s %4d" % (f, len(comp[f])))
            for k in sorted(comp[f], key=_sort_key):
                print("    " + k)
        print("total %d instantiations" % total)
    if a.launched:
        seen, files = launched(a.launched)
        print("trace files: %d" % len(files))
        print("%-22s %8s %8s %13s %11s" % ("family", "compiled", "launched", "never-launch", "unreachable"))
        never_all = []
        for f in families:
            c = comp[f]
            hit = {k for k in c if k in seen}
            unr = {k for k in c - hit if k in UNREACHABLE}
            never = sorted(c - hit - unr, key=_sort_key)
            never_all += never
            print("%-22s %8d %8d %13d %11d" % (f, len(c), len(hit), len(never), len(unr)))
            if a.verbose:
                for k in never:
                    print("    never: " + k)
                for k in sorted(unr, key=_sort_key):
                    print("    unreachable: %s  (%s)" % (k, UNREACHABLE[k]))
        print("never launched (not documented as unreachable): %d of %d" % (len(never_all), total))
        return 1 if never_all else 0
    return 0


if __name__ == "__main__":
    sys.exit(main())
