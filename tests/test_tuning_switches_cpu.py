"""The rule for AswTuning (csrc/asw_internal.h): an environment switch exists only if a GPU test uses it.

Every switch selects another kernel form or another launch geometry on the production path; one that no test sets runs code
nothing has checked since its sweep ended.  So the list read by AswTuning::read_environment is held to the names below, each
of them has to be set by some tests/test_gpu_*.py and documented, the library reads the environment nowhere else, csrc/ carries
no conditional compilation (a measurement build is a second program nobody tests), and the names of retired switches and
measurement builds stay out of the code, the tools and the user documentation (DESIGN.md and profiles/ keep them as history)."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "aswstereomatch_amd", "csrc")

SWITCHES = {
    "ASW_BILATERAL_XQ", "ASW_GEODESIC_XQ",
    "ASW_WMEDIAN_TILE", "ASW_WMEDIAN_TILE_CHUNK", "ASW_WMEDIAN_GEN_ROWS",
    "ASW_GUIDED_FUSED", "ASW_GUIDE_SHARE", "ASW_AB6_PAIR", "ASW_Q6_PAIR",
    "ASW_BAND_AB", "ASW_BAND_Q", "ASW_RING_AB", "ASW_RING_Q", "ASW_Q_WG_STRIPS",
}
RETIRED = ["ASW_WMEDIAN_TILE_SPLIT", "ASW_XQ_ABLAT", "ASW_SGBM_LINE_NO_PREFETCH"]


def read(path):
    with open(path, encoding="utf-8") as f:
        return f.read()


def csrc_files():
    return sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")))


def switches_set_by(text):
    """Names a test file hands to a context: spelled out, or as keywords of a helper that prefixes them ("ASW_" + k)."""
    names = set(re.findall(r"\bASW_[A-Z0-9_]+\b", text))
    if re.search(r'"ASW_"\s*\+', text):
        names |= {"ASW_" + k for k in re.findall(r"\b([A-Z][A-Z0-9_]+)=", text)}
    return names


def test_read_environment_reads_exactly_the_switches():
    found = re.findall(r'\bnum\("(ASW_[A-Z0-9_]+)"', read(os.path.join(CSRC, "asw_context.hip")))
    assert len(found) == len(set(found)), "a switch is read twice"
    assert set(found) == SWITCHES


def test_every_switch_is_used_by_a_gpu_test_and_documented():
    used = set()
    for p in glob.glob(os.path.join(ROOT, "tests", "test_gpu_*.py")):
        used |= switches_set_by(read(p))
    header = read(os.path.join(CSRC, "asw_internal.h"))
    guide = read(os.path.join(ROOT, "INTEGRATION.md"))
    for name in sorted(SWITCHES):
        assert name in used, name + ": no tests/test_gpu_*.py sets it"
        assert re.search(r"\b%s\b" % name, header), name + ": not described in asw_internal.h"
        assert re.search(r"\b%s\b" % name, guide), name + ": not listed in INTEGRATION.md"


def test_the_prefix_idiom_is_recognised():
    """what test_gpu_guided_forms.py does: ctx(BAND_Q=b) -> {"ASW_" + k: ...}"""
    assert switches_set_by('env={"ASW_" + k: str(v)}\nctx(BAND_Q=30, RING_AB=0)') == {"ASW_BAND_Q", "ASW_RING_AB"}
    assert switches_set_by("ctx(BAND_Q=30)") == set()
    assert switches_set_by('Context(0, env={"ASW_GEODESIC_XQ": "0"})') == {"ASW_GEODESIC_XQ"}


def test_the_library_reads_the_environment_in_two_places():
    hits = []
    for p in csrc_files():
        hits += [(os.path.basename(p), line.strip()) for line in read(p).split("\n") if "getenv" in line]
    assert len(hits) == 2, hits
    assert all(f == "asw_context.hip" for f, _ in hits)
    assert sum('getenv("ASW_QUIET")' in line for _, line in hits) == 1
    assert sum("auto num = [](const char* name, int dflt)" in line and "getenv(name)" in line for _, line in hits) == 1


def test_no_conditional_compilation_in_csrc():
    files = csrc_files()
    assert len(files) > 20
    for p in files:
        for i, line in enumerate(read(p).split("\n"), 1):
            assert not re.match(r"\s*#\s*(if|ifdef|ifndef)\b", line), "%s:%d: %s" % (os.path.basename(p), i, line)


def test_retired_names_are_gone():
    me = os.path.abspath(__file__)
    paths = [os.path.join(ROOT, "README.md"), os.path.join(ROOT, "INTEGRATION.md")]
    for top in ("aswstereomatch_amd", "tools", "tests", "include"):
        for d, _, names in os.walk(os.path.join(ROOT, top)):
            if os.path.basename(d) in ("__pycache__", "_build", "golden"):
                continue
            paths += [os.path.join(d, n) for n in names if not n.endswith((".so", ".o", ".pyc", ".npz", ".npy"))]
    assert len(paths) > 100
    for p in paths:
        if os.path.abspath(p) == me:
            continue
        try:
            text = read(p)
        except UnicodeDecodeError:
            continue  # a binary (a built micro-benchmark, a fixture)
        for name in RETIRED:
            assert name not in text, "%s names %s" % (os.path.relpath(p, ROOT), name)
