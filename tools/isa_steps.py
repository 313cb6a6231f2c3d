"""VALU instructions between the loops of one kernel in an `hipcc -S --cuda-device-only` listing, in program order: what a
step of k_asw_bilateral_xq spends outside its row loops.  python tools/isa_steps.py listing.s <substring of the mangled
kernel name> [min VALU per loop]
Prints one line per stretch of straight-line code between two loops (VALU count, quarter-rate integer multiplies, s_barrier
count, LDS / global instructions by kind) followed by the loop's own VALU count.  The three wavefront paths of a kernel (wave 0,
the last-candidate unit's wavefront, plain) follow each other in the listing; s_barrier separates the steps."""
import re
import sys
from collections import Counter

lines = open(sys.argv[1]).read().split("\n")
key = sys.argv[2]
minv = int(sys.argv[3]) if len(sys.argv) > 3 else 40
start = next(i for i, l in enumerate(lines) if key in l and re.match(r"^_Z\S+:", l))
end = next(i for i in range(start, len(lines)) if "s_endpgm" in lines[i])
body = lines[start:end]
labels = {m.group(1): i for i, l in enumerate(body) for m in [re.match(r"^(\.LBB\d+_\d+):", l)] if m}


def count(a, b):
    c = Counter()
    for t in (x.strip().split() for x in body[a:b]):
        if not t or t[0][0] in ".;":
            continue
        op = t[0]
        if op.startswith(("ds_", "scratch_", "global_", "buffer_")) or op == "s_barrier":
            c[op] += 1
        elif op.startswith("v_"):
            c["VALU"] += 1
            if op.startswith(("v_mul_lo_u32", "v_mul_hi_u32", "v_mul_hi_i32")):
                c["quarter-rate"] += 1
    return c


loops = []
for i, l in enumerate(body):
    m = re.search(r"s_cbranch_\w+ (\.LBB\d+_\d+)", l)
    if m and m.group(1) in labels and labels[m.group(1)] < i and count(labels[m.group(1)], i + 1)["VALU"] >= minv:
        loops.append((labels[m.group(1)], i + 1))
pos = 0
for a, b in loops:
    c = count(pos, a)
    print("between %6d..%6d  VALU %4d  %s" % (pos, a, c.pop("VALU", 0), dict(c)))
    print("   loop %6d..%6d  VALU %4d" % (a, b, count(a, b)["VALU"]))
    pos = b
c = count(pos, len(body))
print("after   %6d..%6d  VALU %4d  %s" % (pos, len(body), c.pop("VALU", 0), dict(c)))
