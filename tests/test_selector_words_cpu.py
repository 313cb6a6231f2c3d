"""The selector's two packed words on the CPU: decode_algorithm and decode_disparity_type of csrc/asw_selector.h, through
tests/cpp/selector_words.cpp, against tests/golden/selector_words_v1.txt.xz -- what the decoders of the commit named in the record's
first line answered to the same cases (recorded once from that commit's code, never from the unit under test).  Every structured
row must be equal, the seeded sweeps must give the recorded counts and digest, and the record itself must hold every status of
every rule, so that a thin case list cannot pass.  A refused disparity_type row holds its status alone (selector_words.cpp)."""
import hashlib
import itertools
import lzma
import os
import subprocess
import sys
from collections import Counter

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from shim_build import PKG, ROOT, build_demo  # noqa: E402

RECORD = os.path.join(ROOT, "tests", "golden", "selector_words_v1.txt.xz")
OK, UNSUPPORTED, BAD = 0, 3, 7
SUB, CROSS, SCAN, VIEW = 0x300, 1 << 12, 1 << 24, 1
# traits of a disparity_type case: -1 = no row, else these bits
SERVED, NO_VOLUME, IGNORES, NO_SUBPIXEL, EXTRA = 1, 2, 4, 8, 16
TRAITS = [-1] + list(range(32))
RANGES = [(0, 1), (0, 2), (0, 64), (3, 5), (7, 1), (0, 1025), (0, 1026), (100, 1)]
SWEEP = 20000
SWEEP_TRAITS = [-1, 0, SERVED, SERVED | NO_VOLUME, SERVED | IGNORES, SERVED | NO_SUBPIXEL, SERVED | EXTRA]


def scan_word(a, u, r1):
    return SCAN | a << 1 | u << 25 | r1 << 28


def cross_word(s, q):
    return CROSS | s << 13 | q << 16


def disparity_words():
    views_subs = [v | s for v in (0, 1) for s in (0, 0x100, 0x200, 0x300)]
    scan = [scan_word(a, u, r1) for a in (0, 1, 127) for u in (0, 1, 7) for r1 in (0, 1, 7)]
    cross = [cross_word(s, q) for s in (0, 1, 2, 5, 6, 7) for q in (0, 1, 255)]
    words = [w | vs for w in scan + cross + [0] for vs in views_subs]
    valid = [scan_word(8, 5, 3), cross_word(3, 19), 0x100, 0, 1]
    words += [w | 1 << b for w in valid for b in range(32)]
    words += [valid[0] | valid[1] | vs for vs in views_subs]  # both steps
    clear = [valid[0] & ~SCAN, valid[1] & ~CROSS, 1 << 31, 1 << 10, 0xFE, 0x00FFE000]  # fields without their flag bit
    words += [w | v | s for w in clear for v in (0, 1) for s in (0, 0x100)]
    return list(dict.fromkeys(words))


def algorithm_words():
    flags = {30: 12, 29: 12, 28: 2, 27: 12}  # flag bit -> the encoding's low byte
    words = list(range(14)) + [255]
    valid = []
    for bit, low in flags.items():
        lam = (0, 1, 31) if bit == 29 else (0,)
        words += [1 << bit | l << 24 | p16 << 16 | p8 << 8 | low for l in lam for p16 in (0, 1, 255) for p8 in (0, 1, 255)]
        valid.append(1 << bit | (10 << 24 if bit == 29 else 0) | 30 << 16 | 20 << 8 | low)
    words += [(w & ~0xFF) | low for w in valid for low in list(range(14)) + [255]]
    tops = [1 << b for b in range(24, 32)] + [1 << a | 1 << b for a, b in itertools.combinations(range(24, 32), 2)]
    words += [w | t for w in valid + list(range(13)) for t in tops]
    words += [0xFFFFFFFF, 0x80000000, 0xFFFFFFF3, 0x8000000C, 0x80000002] + [w | 1 << 31 | 1 << 16 for w in valid]  # negative
    return list(dict.fromkeys(words))


def structured_cases():
    lines = ["A %08x %d" % (w, n) for w in algorithm_words() for n in (0, 1)]
    lines += ["D %08x %d %d %d" % (w, t, minD, numD) for w in disparity_words() for t in TRAITS for minD, numD in RANGES]
    return lines


def sweep_cases():
    rng = np.random.default_rng(20266)
    a = rng.integers(0, 1 << 32, SWEEP, dtype=np.uint64)
    d = rng.integers(0, 1 << 32, SWEEP, dtype=np.uint64)
    lines = ["A %08x %d" % (w, n) for w in a for n in (0, 1)]
    lines += ["D %08x %d 3 5" % (w, t) for w in d for t in SWEEP_TRAITS]
    return lines


def summarise(lines):
    """the sweep's output as the record keeps it: per decoder and status the number of lines, and one digest of them all"""
    counts = Counter((ln[0], ln.split(" -> ")[1].split()[0]) for ln in lines)
    rows = ["S %s status %s: %d" % (k, s, n) for (k, s), n in sorted(counts.items())]
    return rows + ["S sha256 " + hashlib.sha256("\n".join(lines).encode()).hexdigest()]


def run_cases(exe, cases):
    r = subprocess.run([exe], input="\n".join(cases) + "\n", capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return r.stdout.splitlines()


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build_demo("selector_words.cpp", tmp_path_factory.mktemp("selector_words") / "selector_words", link=False,
                      extra=("-Wextra", "-I" + os.path.join(PKG, "csrc")))


@pytest.fixture(scope="module")
def record():
    with lzma.open(RECORD, "rt") as f:
        lines = f.read().splitlines()
    assert lines[0].startswith("# decoders of commit ")
    return [ln for ln in lines[1:] if not ln.startswith("S ")], [ln for ln in lines[1:] if ln.startswith("S ")]


def test_structured_rows_equal_the_record(exe, record):
    got = run_cases(exe, structured_cases())
    want = record[0]
    assert len(got) == len(want)
    wrong = [(g, w) for g, w in zip(got, want) if g != w]
    assert not wrong, "%d rows differ, the first (got, recorded): %s" % (len(wrong), wrong[:10])


def test_sweep_equals_the_record(exe, record):
    cases = sweep_cases()
    assert len(cases) >= 2 * SWEEP
    got = run_cases(exe, cases)
    assert len(got) == len(cases)
    assert summarise(got) == record[1]


def parse(rows):
    a, d = [], []
    for ln in rows:
        left, right = ln.split(" -> ")
        left, right = left.split(), right.split()
        if left[0] == "A":
            a.append((int(left[1], 16), int(left[2]), int(right[0]), [float(x) for x in right[1:]]))
        else:
            d.append((int(left[1], 16), int(left[2]), int(left[3]), int(left[4]), int(right[0]), right[1:]))
    return a, d


def test_record_holds_every_rule(record):
    """Each rule of the two decoders, as a predicate on a case and the status the rule gives it: the record must answer at least one
    such case, and every one of them with that status."""
    alg, dis = parse(record[0])
    assert len({w for w, *_ in alg}) > 300 and len({w for w, *_ in dis}) > 500
    assert {(t, minD, numD) for _, t, minD, numD, _, _ in dis} == {(t, *r) for t in TRAITS for r in RANGES}

    flags = SUB | CROSS | SCAN
    scan_ok = lambda w: w & SCAN and not w & ~(0x7F0000FE | SUB | VIEW) and (w >> 1) & 0x7F and w & SUB != SUB  # noqa: E731
    cross_ok = lambda w: (w & (CROSS | SCAN) == CROSS and not w & ~(0x00FFF000 | SUB | VIEW) and 2 <= (w >> 13) & 7 <= 5  # noqa: E731
                          and (w >> 16) & 0xFF and w & SUB != SUB)
    usable = lambda t: t >= 0 and t & SERVED and not t & (NO_VOLUME | IGNORES | NO_SUBPIXEL)  # noqa: E731
    planes = lambda t, numD: numD + (t >> 4 & 1)  # noqa: E731

    def empty_level(w, t, minD, numD):
        last = minD + planes(t, numD) - 1
        return any((last >> s) - (minD >> s) + 1 - (t >> 4 & 1) < 1 for s in range(1, (w >> 13) & 7))

    ignored = lambda t: t >= 0 and bool(t & IGNORES)  # noqa: E731
    rules = {  # name: (predicate on (word, traits, minD, numD), status)
        "no flag bit, bit 31": (lambda w, t, a, n: not w & flags and w >> 31, OK),
        "no flag bit, bits 13-23": (lambda w, t, a, n: not w & flags and w & 0x00FFE000, OK),
        "no flag bit, bits 1-7": (lambda w, t, a, n: not w & flags and w & 0xFE, OK),
        "ignores_disparity_type": (lambda w, t, a, n: ignored(t) and w & flags, OK),
        "ignores_disparity_type, unserved (BM)": (lambda w, t, a, n: ignored(t) and not t & SERVED and w & SCAN and w & CROSS, OK),
        "scanline 1: with cross-scale, NCC": (lambda w, t, a, n: not ignored(t) and t > 0 and t & NO_SUBPIXEL and w & SCAN and w & CROSS, BAD),
        "scanline 1: with cross-scale, unserved": (lambda w, t, a, n: t == NO_VOLUME and w & SCAN and w & CROSS, BAD),
        "scanline 1: with cross-scale, no row": (lambda w, t, a, n: t == -1 and w & SCAN and w & CROSS, BAD),
        "scanline 2: stray bit": (lambda w, t, a, n: not ignored(t) and w & SCAN and w & ~(0x7F0000FE | SUB | VIEW), BAD),
        "scanline 2: a == 0": (lambda w, t, a, n: not ignored(t) and w & SCAN and not (w >> 1) & 0x7F, BAD),
        "scanline 2: both sub-pixel flags": (lambda w, t, a, n: not ignored(t) and w & SCAN and w & SUB == SUB, BAD),
        "scanline 3: no row": (lambda w, t, a, n: scan_ok(w) and t == -1, UNSUPPORTED),
        "scanline 3: unserved": (lambda w, t, a, n: scan_ok(w) and t == 0, UNSUPPORTED),
        "scanline 3: no volume": (lambda w, t, a, n: scan_ok(w) and t == SERVED | NO_VOLUME, UNSUPPORTED),
        "scanline 3: no sub-pixel": (lambda w, t, a, n: scan_ok(w) and t == SERVED | NO_SUBPIXEL and n > 1025, UNSUPPORTED),
        "scanline 4: 1026 planes": (lambda w, t, a, n: scan_ok(w) and usable(t) and planes(t, n) == 1026, BAD),
        "scanline 4: 1027 planes": (lambda w, t, a, n: scan_ok(w) and usable(t) and planes(t, n) == 1027, BAD),
        "scanline: 1025 planes": (lambda w, t, a, n: scan_ok(w) and usable(t) and planes(t, n) == 1025, OK),
        "scanline with a sub-pixel flag": (lambda w, t, a, n: scan_ok(w) and w & SUB and usable(t) and n < 1000, OK),
        "cross-scale 1: stray bit": (lambda w, t, a, n: not ignored(t) and w & (CROSS | SCAN) == CROSS and w & ~(0x00FFF000 | SUB | VIEW), BAD),
        "cross-scale 1: stray bit, NCC": (lambda w, t, a, n: t == SERVED | NO_SUBPIXEL and w & (CROSS | SCAN) == CROSS
                                          and w & ~(0x00FFF000 | SUB | VIEW), BAD),
        "cross-scale 2: S": (lambda w, t, a, n: not ignored(t) and w & (CROSS | SCAN) == CROSS and not 2 <= (w >> 13) & 7 <= 5, BAD),
        "cross-scale 2: q == 0": (lambda w, t, a, n: not ignored(t) and w & (CROSS | SCAN) == CROSS and not (w >> 16) & 0xFF, BAD),
        "cross-scale 2: both sub-pixel flags, NCC": (lambda w, t, a, n: t == SERVED | NO_SUBPIXEL and w & (CROSS | SCAN) == CROSS
                                                     and w & SUB == SUB, BAD),
        "cross-scale 3: no sub-pixel": (lambda w, t, a, n: cross_ok(w) and not ignored(t) and t > 0 and t & NO_SUBPIXEL, UNSUPPORTED),
        "cross-scale 4: no row": (lambda w, t, a, n: cross_ok(w) and t == -1, UNSUPPORTED),
        "cross-scale 4: unserved, an empty level": (lambda w, t, a, n: cross_ok(w) and t == EXTRA and empty_level(w, t, a, n), UNSUPPORTED),
        "cross-scale 4: no volume": (lambda w, t, a, n: cross_ok(w) and t == SERVED | NO_VOLUME, UNSUPPORTED),
        "cross-scale 5: an empty level": (lambda w, t, a, n: cross_ok(w) and usable(t) and empty_level(w, t, a, n), BAD),
        "cross-scale": (lambda w, t, a, n: cross_ok(w) and usable(t) and not empty_level(w, t, a, n), OK),
        "sub-pixel 1: both flags": (lambda w, t, a, n: not ignored(t) and not w & (CROSS | SCAN) and w & SUB == SUB, BAD),
        "sub-pixel 2: another bit": (lambda w, t, a, n: not ignored(t) and not w & (CROSS | SCAN) and w & SUB and w & ~(SUB | VIEW), BAD),
        "sub-pixel 2: another bit, NCC": (lambda w, t, a, n: t == SERVED | NO_SUBPIXEL and not w & (CROSS | SCAN) and w & SUB
                                          and w & ~(SUB | VIEW), BAD),
        "sub-pixel 3: no sub-pixel": (lambda w, t, a, n: t == SERVED | NO_SUBPIXEL and w in (0x100, 0x101, 0x200, 0x201), UNSUPPORTED),
        "sub-pixel": (lambda w, t, a, n: usable(t) and w in (0x100, 0x101, 0x200, 0x201), OK),
        "sub-pixel, no row": (lambda w, t, a, n: t == -1 and w in (0x100, 0x101, 0x200, 0x201), OK),
    }
    for name, (pred, status) in rules.items():
        hits = [row for row in dis if pred(*row[:4])]
        assert hits, name
        assert all(row[4] == status for row in hits), (name, [row for row in hits if row[4] != status][:5])
    for w, t, minD, numD, status, out in dis:  # untouched means untouched; an accepted flagged word keeps the view bit alone
        if status == OK:
            untouched = ignored(t) or not w & flags
            assert int(out[0], 16) == (w if untouched else w & VIEW), (w, t)
            assert untouched == (out[1:] == ["0", "0", "0", "0x0p+0", "0x0p+0"]), (w, t, out)

    top = lambda w: w >> 27 & 0xF  # bits 27..30  # noqa: E731
    low = lambda w: w & 0xFF  # noqa: E731
    arules = {  # name: (predicate on the word, status)
        "plain value": (lambda w: not top(w), OK),
        "plain value, negative": (lambda w: not top(w) and w >> 31, OK),
        "bit 27 under bit 28: a refused bit": (lambda w: top(w) == 0b0011, None),
        "bit 27 under bit 29: lambda_ad": (lambda w: top(w) & 0b1101 == 0b0101 and low(w) == 12 and not w >> 31 and w >> 16 & 0xFF, OK),
        "bit 28 under bit 29: lambda_ad": (lambda w: top(w) & 0b1110 == 0b0110 and low(w) == 12 and not w >> 31 and w >> 16 & 0xFF, OK),
        "bit 30 over bit 29": (lambda w: top(w) & 0b1100 == 0b1100 and low(w) == 12, BAD),
        "cross: low byte before fields": (lambda w: top(w) & 0b1000 and low(w) != 12, UNSUPPORTED),
        "adcensus: low byte before fields": (lambda w: top(w) & 0b1100 == 0b0100 and low(w) != 12, UNSUPPORTED),
        "twopass: low byte before fields": (lambda w: top(w) & 0b1110 == 0b0010 and low(w) != 2, UNSUPPORTED),
        "permeability: low byte before fields": (lambda w: top(w) == 0b0001 and low(w) != 12, UNSUPPORTED),
        "negative, wrong low byte": (lambda w: w >> 31 and top(w) == 0b0010 and low(w) != 2, UNSUPPORTED),
        "negative, right low byte": (lambda w: w >> 31 and top(w) and low(w) == (2 if top(w) & 0b1110 == 0b0010 else 12), BAD),
        "cross: trunc == 0": (lambda w: top(w) & 0b1000 and low(w) == 12 and not w >> 16 & 0xFF, BAD),
        "adcensus: lambda_ad == 0": (lambda w: top(w) & 0b1100 == 0b0100 and low(w) == 12 and not w >> 24 & 0x1F, BAD),
        "twopass: gamma_c == 0": (lambda w: top(w) & 0b1110 == 0b0010 and low(w) == 2 and not w >> 8 & 0xFF, BAD),
        "permeability: sigma == 0": (lambda w: top(w) == 0b0001 and low(w) == 12 and not w >> 8 & 0xFF, BAD),
        "cross": (lambda w: w >> 24 == 0x40 and low(w) == 12 and w >> 16 & 0xFF, OK),
        "twopass": (lambda w: w >> 24 == 0x10 and low(w) == 2 and w >> 16 & 0xFF and w >> 8 & 0xFF, OK),
        "permeability": (lambda w: w >> 24 == 0x08 and low(w) == 12 and w >> 16 & 0xFF and w >> 8 & 0xFF, OK),
    }
    for name, (pred, status) in arules.items():
        hits = [row for row in alg if pred(row[0])]
        assert hits, name
        if status is None:  # under bit 28 bit 27 is never accepted: the low byte's status, or ERR_BAD_ARGUMENT
            assert {row[2] for row in hits} == {UNSUPPORTED, BAD}, name
        else:
            assert all(row[2] == status for row in hits), (name, [hex(row[0]) for row in hits if row[2] != status][:5])
    with_mp = {w: status for w, null_mp, status, _ in alg if not null_mp}
    without = {w: status for w, null_mp, status, _ in alg if null_mp}
    assert with_mp == without and set(with_mp.values()) == {OK, UNSUPPORTED, BAD}
    defaults = [0, 30, 20, 0, 20, 20, 10, 30, 0, 8, 20]
    for w, null_mp, status, out in alg:  # the plain value, and the parameters only where a value is accepted into an mp
        assert out[0] == (w & 0xFF if status == OK and top(w) else w - (w >> 31 << 32)), hex(w)
        assert (out[1:] != defaults) == (status == OK and bool(top(w)) and not null_mp), hex(w)
