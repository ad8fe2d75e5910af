#!/usr/bin/env python3
"""Is the library's device code the same code as at another commit?  (No GPU needed.)

    python tools/isa_identity.py --base REV          # REV: a git revision, e.g. HEAD~1
    python tools/isa_identity.py --base-dir TREE     # or a checked-out tree of that revision
    python tools/isa_identity.py --base REV --only photometric_fast pattern_loss costvol_fast    # these files alone

Compiles every csrc/*.hip present in either tree (--only NAME ...: the files of those base names, where they exist), as
it is at the base and as it is in the working tree, to gfx950 assembly with
the flags of connecting_the_dots_amd/build.py plus `--cuda-device-only -S` (into a temporary directory, never into the
tree) and compares per kernel symbol, whichever file defines it:
  * the set of .amdhsa_kernel symbols (one that several files define -- a kernel in a header, with internal linkage or
    as a template -- counts once per file, as symbol@file, and is compared file by file);
  * the instruction stream from the kernel's label to its .Lfunc_end, and its .amdhsa_* descriptor block (register
    counts, LDS, scratch, ...), textually, after renumbering the function-local labels (.LBB<function>_<block>,
    .Lfunc_end<function>) and dropping comments.
Prints one line per differing kernel, a summary line, and exits non-zero on any difference.  Extra compiler flags go
after `--` (e.g. `-- -DCTD_STAMPS` compares the diagnostic build).
"""
import argparse
import difflib
import glob
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = "connecting_the_dots_amd/csrc"

sys.path.insert(0, ROOT)
from connecting_the_dots_amd.build import FLAGS, HIPCC  # noqa: E402


def names_in(tree):
    return {os.path.basename(s)[:-4] for s in glob.glob(os.path.join(tree, CSRC, "*.hip"))}


def compile_family(tree, family, out_dir, extra):
    srcs = [os.path.join(tree, CSRC, n + ".hip") for n in family]
    srcs = [s for s in srcs if os.path.exists(s)]
    os.makedirs(out_dir, exist_ok=True)

    def one(src):
        dst = os.path.join(out_dir, os.path.basename(src)[:-4] + ".s")
        subprocess.check_call([HIPCC] + FLAGS + extra + ["--cuda-device-only", "-S", src, "-o", dst])
        return dst

    with ThreadPoolExecutor(max_workers=8) as pool:
        return list(pool.map(one, srcs))


def normalise(line):
    line = line.split(";", 1)[0].rstrip()                         # comments (block names, register notes)
    line = re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", line)
    line = re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1", line)
    return line


def kernels_of(path):
    """{symbol: (instruction lines, descriptor lines)} of one .s file"""
    lines = open(path).read().split("\n")
    names = [m.group(1) for s in lines for m in [re.match(r"\s*\.amdhsa_kernel\s+(\S+)", s)] if m]
    out = {}
    for name in names:
        start = next(i for i, s in enumerate(lines) if s.startswith(name + ":"))
        code, desc, i = [], [], start + 1
        while not re.match(r"\.Lfunc_end\d+:", lines[i]):
            s = normalise(lines[i])
            if re.match(r"\s*\.amdhsa_", s):
                desc.append(s.strip())
            elif s.strip() and not re.match(r"\s*\.(section|p2align|end_amdhsa_kernel|text)", s):
                code.append(s.strip())
            i += 1
        assert name not in out, "kernel defined twice in %s: %s" % (path, name)
        out[name] = (code, desc)
    return out


def collect(paths):
    per_name = {}
    for p in paths:
        for name, k in kernels_of(p).items():
            per_name.setdefault(name, []).append(k + (os.path.basename(p),))
    return {name if len(ks) == 1 else "%s@%s" % (name, k[2]): k for name, ks in per_name.items() for k in ks}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    g = ap.add_mutually_exclusive_group(required=True)
    g.add_argument("--base", help="git revision to compare the working tree with")
    g.add_argument("--base-dir", help="checked-out tree of the base revision")
    ap.add_argument("--show", type=int, default=12, help="diff lines to print per differing kernel")
    ap.add_argument("--only", nargs="+", metavar="NAME", help="compare these csrc files only (base names, no .hip)")
    ap.add_argument("extra", nargs="*", help="extra compiler flags (after --)")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory(prefix="isa_identity_") as tmp:
        base_tree = args.base_dir
        if args.base:
            base_tree = os.path.join(tmp, "base_tree")
            os.makedirs(base_tree)
            tar = subprocess.Popen(["git", "-C", ROOT, "archive", args.base, CSRC, "include"], stdout=subprocess.PIPE)
            subprocess.check_call(["tar", "-x", "-C", base_tree], stdin=tar.stdout)
            assert tar.wait() == 0
        family = sorted(names_in(base_tree) | names_in(ROOT))       # a kernel may have moved to a file the base lacks
        if args.only:
            unknown = set(args.only) - set(family)
            if unknown:
                ap.error("no such csrc file in either tree: " + ", ".join(sorted(unknown)))
            family = sorted(args.only)
        old = collect(compile_family(base_tree, family, os.path.join(tmp, "base"), args.extra))
        new = collect(compile_family(ROOT, family, os.path.join(tmp, "new"), args.extra))
    bad = 0
    for name in sorted(set(old) | set(new)):
        if name not in old or name not in new:
            print("ONLY IN %s: %s" % ("base" if name in old else "working tree", name))
            bad += 1
            continue
        for what, a, b in (("instructions", old[name][0], new[name][0]), ("descriptor", old[name][1], new[name][1])):
            if a != b:
                bad += 1
                print("DIFFERENT %s: %s (%s -> %s)" % (what, name, old[name][2], new[name][2]))
                for s in list(difflib.unified_diff(a, b, lineterm="", n=0))[2:2 + args.show]:
                    print("    " + s)

    def scratch(ks):
        n = [int(s.split()[-1]) for k in ks.values() for s in k[1] if s.startswith(".amdhsa_private_segment_fixed_size")]
        return "%d with scratch 0, others %s" % (n.count(0), sorted(x for x in n if x))

    print("isa_identity: base %d kernels (%s) | working tree %d kernels (%s) | %d instructions compared | %s"
          % (len(old), scratch(old), len(new), scratch(new), sum(len(k[0]) for k in new.values()),
             "IDENTICAL" if bad == 0 else "%d DIFFERENCES" % bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
