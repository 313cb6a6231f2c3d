"""Are the kernels of two `hipcc -S --cuda-device-only` listings the same machine code?  Pairs the kernels by demangled name and
compares, kernel by kernel, the instruction stream and the .amdhsa_* descriptor with symbol names normalised (mangled names,
.LBB / .Ltmp / .Lfunc labels):
    python tools/isa_same.py old.s new.s [--map 'REGEX=>REPLACEMENT' ...] [--gone REGEX ...]
--map rewrites the demangled names of old.s first (a refactor that drops template parameters).  --gone: kernels of old.s alone
whose (rewritten) name matches are listed but expected (a refactor that retires kernels).  Exit status 1 on any other unpaired
or any differing kernel.  Listings: from inside aswstereomatch_amd/csrc, hipcc <CXXFLAGS of build.py> --cuda-device-only -S x.hip."""
import argparse
import difflib
import os
import re
import subprocess
import sys

CXXFILT = os.environ.get("CXXFILT", "c++filt")


def kernels(path):
    """{mangled name: normalised lines from the entry label to .end_amdhsa_kernel}"""
    lines = open(path).read().split("\n")
    out = {}
    for i, l in enumerate(lines):
        m = re.match(r"\s*\.amdhsa_kernel (\S+)", l)
        if not m:
            continue
        name = m.group(1)
        start = next(j for j in range(i, -1, -1) if lines[j].startswith(name + ":"))
        end = next(j for j in range(i, len(lines)) if ".end_amdhsa_kernel" in lines[j])
        tmp = {}
        body = []
        for t in lines[start:end + 1]:
            t = re.sub(r"\b_Z\w+", "SYM", t)
            t = re.sub(r"(?<!\w)(\.LBB|BB|\.Lfunc_begin|\.Lfunc_end)\d+", r"\1", t)
            t = re.sub(r"\.Ltmp\d+", lambda x: tmp.setdefault(x.group(0), ".Ltmp#%d" % len(tmp)), t)
            t = re.sub(r"\s*;.*$", "", t)  # comments carry block numbers and column padding
            if t:
                body.append(t)
        out[name] = body
    return out


def demangle(names):
    r = subprocess.run([CXXFILT], input="\n".join(names), stdout=subprocess.PIPE, text=True, check=True)
    return [re.sub(r"^void ", "", d).replace("(anonymous namespace)::", "") for d in r.stdout.split("\n")[:len(names)]]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--map", action="append", default=[], metavar="REGEX=>REPLACEMENT")
    ap.add_argument("--gone", action="append", default=[], metavar="REGEX")
    args = ap.parse_args()
    old, new = kernels(args.old), kernels(args.new)
    okey = {}
    for mangled, d in zip(old, demangle(list(old))):
        for m in args.map:
            pat, rep = m.split("=>", 1)
            d = re.sub(pat, rep, d)
        okey[d] = mangled
    nkey = dict(zip(demangle(list(new)), new))
    if len(okey) != len(old) or len(nkey) != len(new):
        print("two kernels of one listing share a name after demangling / --map: they cannot be paired")
        return 1
    same = bad = gone = 0
    for d in sorted(set(okey) | set(nkey)):
        if d not in nkey and any(re.search(g, d) for g in args.gone):
            print("GONE (old only, expected): %s" % d)
            gone += 1
            continue
        if d not in okey or d not in nkey:
            print("UNPAIRED (%s only): %s" % ("old" if d in okey else "new", d))
            bad += 1
            continue
        a, b = old[okey[d]], new[nkey[d]]
        if a == b:
            same += 1
            continue
        bad += 1
        print("DIFFERS: %s" % d)
        for t in list(difflib.unified_diff(a, b, "old", "new", n=0, lineterm=""))[:12]:
            print("    " + t)
    print("%d kernels old, %d new, %d paired and identical, %d gone, %d not" % (len(old), len(new), same, gone, bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
