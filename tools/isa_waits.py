"""How far ahead of their use are the LDS reads of a kernel's loops issued?  For every loop of one kernel in an
`hipcc -S --cuda-device-only` listing: the VALU instructions between each ds_read and the s_waitcnt that retires it (LDS
operations return in order: `s_waitcnt lgkmcnt(n)` retires all but the youngest n), as the smallest distance, the number of reads
below a threshold and a histogram.  Reads still in flight at the back edge are carried into a second pass over the body.
    python tools/isa_waits.py listing.s <substring of the mangled kernel name> [min VALU per loop] [--below N]"""
import re
import sys
from collections import Counter

argv = sys.argv[1:]
below = 12
if "--below" in argv:
    i = argv.index("--below")
    below = int(argv[i + 1])
    del argv[i:i + 2]
lines = open(argv[0]).read().split("\n")
key = argv[1]
minv = int(argv[2]) if len(argv) > 2 else 40
start = next(i for i, l in enumerate(lines) if key in l and re.match(r"^_Z\S+:", l))
end = next(i for i in range(start, len(lines)) if "s_endpgm" in lines[i])
body = lines[start:end]
labels = {}
for i, l in enumerate(body):
    m = re.match(r"^(\.LBB\d+_\d+):", l)
    if m:
        labels[m.group(1)] = i
for i, l in enumerate(body):
    m = re.search(r"s_cbranch_\w+ (\.LBB\d+_\d+)", l)
    if not (m and m.group(1) in labels and labels[m.group(1)] < i):
        continue
    ins = [t.strip().split(None, 1) for t in body[labels[m.group(1)]:i + 1]]
    ins = [t for t in ins if t and t[0][0] not in ".;"]
    nvalu = sum(1 for t in ins if t[0].startswith("v_"))
    if nvalu < minv:
        continue
    dist, queue, valu = [], [], 0  # queue: (VALU count at issue, counted?) of the LDS / scalar-memory operations in flight
    for rnd in range(2):  # the second pass sees the reads carried across the back edge; only it is counted
        for t in ins:
            op = t[0]
            if op.startswith("v_"):
                valu += 1
            elif op.startswith("ds_") or op.startswith("s_load") or op.startswith("s_buffer_load"):
                queue.append((valu, op.startswith("ds_read"), rnd))
            elif op == "s_waitcnt":
                w = re.search(r"lgkmcnt\((\d+)\)", t[1] if len(t) > 1 else "")
                if w:
                    keep = int(w.group(1))
                    while len(queue) > keep:
                        v0, isread, r0 = queue.pop(0)
                        if isread and rnd == 1:
                            dist.append(valu - v0)
    h = Counter(min(d // 4 * 4, 40) for d in dist)
    print(labels[m.group(1)], i, "VALU", nvalu, "ds_read retired", len(dist), "min", min(dist) if dist else None,
          "below %d:" % below, sum(1 for d in dist if d < below), "hist(4-wide bins)", dict(sorted(h.items())))
