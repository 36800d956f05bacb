#!/usr/bin/env python3
"""Per-kernel comparison of the gfx950 device assembly of two source trees (no GPU needed).

    python scripts/kernel_isa_diff.py OLD_TREE NEW_TREE [--only SUBSTRING] [--quiet]
                                      [--map 'REGEX=REPLACEMENT']...

Every gnnflow_amd/csrc/*.hip of each tree is compiled with the FLAGS of gnnflow_amd/_build.py
plus `--cuda-device-only -S`, and the output is cut into one text per `.amdhsa_kernel` symbol:
the function from its label to `.Lfunc_end*`, which includes its `.amdhsa_*` descriptor block.
Only what a move between translation units must change is normalised:
  * the function index in local labels (.LBB<n>_<k>, .Lfunc_begin<n> / .Lfunc_end<n>,
    .L__unnamed_<n>, .str.<n>),
  * the kernel's own mangled symbol (it changes when a parameter type changes namespace),
  * comments: whole lines and the trailing ones, which name basic blocks by function index.
Registers, immediates, instruction order and descriptor values are compared as they are.
Kernels are matched by demangled name without `(anonymous namespace)::`.  Where a change renames
kernels on purpose (a template parameter added, a parameter type renamed), each `--map` is a
re.sub applied, in the order given, to the demangled names of BOTH trees before they are matched.
Prints `same` or a unified diff per kernel; exit status 1 if a kernel differs, 2 if the sets of
kernels differ.
"""
import argparse
import difflib
import glob
import importlib.util
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor


def build_flags(tree):
    spec = importlib.util.spec_from_file_location(
        "_gnnflow_build", os.path.join(tree, "gnnflow_amd", "_build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.FLAGS


def device_asm(tree, src, hipcc):
    csrc = os.path.join(tree, "gnnflow_amd", "csrc")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "out.s")
        cmd = [hipcc] + build_flags(tree) + ["--cuda-device-only", "-S", "-I", csrc,
                                             "-I", os.path.join(tree, "include"), src, "-o", out]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("hipcc failed:\n" + " ".join(cmd) + "\n" + r.stderr)
        with open(out) as f:
            return f.read()


LOCAL = [(re.compile(r"\.LBB\d+_"), ".LBB_"),
         (re.compile(r"\.Lfunc_(begin|end)\d+"), r".Lfunc_\1"),
         (re.compile(r"\.L__unnamed_\d+"), ".L__unnamed_"),
         (re.compile(r"\.str\.\d+"), ".str.")]


def kernels_of(asm):
    """{mangled symbol: normalised lines} of one assembly file"""
    lines = asm.splitlines()
    out = {}
    for sym in re.findall(r"^\s*\.amdhsa_kernel (\S+)$", asm, re.M):
        first = next(i for i, l in enumerate(lines) if l.startswith(sym + ":"))
        last = next(i for i in range(first, len(lines)) if re.match(r"\.Lfunc_end\d+:", lines[i]))
        body = []
        for line in lines[first:last + 1]:
            line = re.sub(r"\s*;.*$", "", line)   # (no instruction or directive here has a ';')
            if not line.strip():
                continue
            line = line.replace(sym, "<kernel>")
            for pat, rep in LOCAL:
                line = pat.sub(rep, line)
            body.append(line)
        out[sym] = body
    return out


def demangle(symbols):
    r = subprocess.run(["c++filt"], input="\n".join(symbols), capture_output=True, text=True)
    names = []
    for n in r.stdout.splitlines():
        n = n.replace("(anonymous namespace)::", "")
        names.append(re.sub(r"^void ", "", n))
    return names


def tree_kernels(tree, hipcc, maps=()):
    files = sorted(glob.glob(os.path.join(tree, "gnnflow_amd", "csrc", "*.hip")))
    with ThreadPoolExecutor(max_workers=4) as ex:
        asms = list(ex.map(lambda f: device_asm(tree, f, hipcc), files))
    out = {}
    for f, asm in zip(files, asms):
        ks = kernels_of(asm)
        for sym, name in zip(ks, demangle(list(ks))):
            for pat, rep in maps:
                name = pat.sub(rep, name)
            if name in out:   # a library template instantiated in two translation units
                name += " [" + os.path.basename(f) + "]"
            out[name] = (os.path.basename(f), ks[sym])
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--only", default="", help="compare kernels whose name contains this")
    ap.add_argument("--quiet", action="store_true", help="no diffs, the summary only")
    ap.add_argument("--map", action="append", default=[], metavar="REGEX=REPLACEMENT",
                    help="rename demangled kernel names of both trees before matching (repeatable)")
    ap.add_argument("--hipcc", default=os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))
    a = ap.parse_args()
    maps = []
    for m in a.map:
        pat, sep, rep = m.partition("=")
        if not sep:
            ap.error("--map needs REGEX=REPLACEMENT, got %r" % m)
        maps.append((re.compile(pat), rep))
    old, new = tree_kernels(a.old, a.hipcc, maps), tree_kernels(a.new, a.hipcc, maps)
    status = 0
    if set(old) != set(new):
        for n in sorted(set(old) - set(new)):
            print("%s only in %s (%s)" % (n, a.old, old[n][0]))
        for n in sorted(set(new) - set(old)):
            print("%s only in %s (%s)" % (n, a.new, new[n][0]))
        status = 2
    differ = []
    short = lambda n: n if len(n) <= 60 else n[:57] + "..."
    for n in sorted(set(old) & set(new)):
        if a.only not in n:
            continue
        (fo, lo), (fn, ln) = old[n], new[n]
        where = fo if fo == fn else "%s -> %s" % (fo, fn)
        if lo == ln:
            print("%-60s same     (%s, %d lines)" % (short(n), where, len(lo)))
            continue
        differ.append(n)
        print("%-60s DIFFERS  (%s, %d -> %d lines)" % (short(n), where, len(lo), len(ln)))
        if not a.quiet:
            sys.stdout.writelines(l + "\n" for l in difflib.unified_diff(
                lo, ln, "old/" + n, "new/" + n, lineterm="", n=2))
    print("%d kernels in %s, %d in %s; %d compared, %d differ%s" % (
        len(old), a.old, len(new), a.new, len([n for n in set(old) & set(new) if a.only in n]),
        len(differ), (": " + ", ".join(differ)) if differ else ""))
    return status or (1 if differ else 0)


if __name__ == "__main__":
    sys.exit(main())
