"""Which status a call returns, per method and per entry path: tools/record_method_matrix.py's table replayed against
tests/golden/method_matrix.json, which that tool recorded on the commit before the host layer got its method table.

Every other GPU file compares a method's outputs with the oracle; this one pins what they leave thin: the status of a refused call
(one fault, and the pairs of faults whose order of checks decides the answer) for every selector value through stereoMatching, the
resident path and the method's own entry point, and for the disp16 entry points; for a valid call also the volume planes handed
back against asw_volume_planes, timing()["aggregate_launches"] and a CRC-32 of the disparity bytes.  The golden file is never
regenerated to make this pass: a difference is a change of behaviour."""
import json
import os
import sys

import pytest

import aswstereomatch_amd as asw

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
import record_method_matrix as rec  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rows():
    with open(os.path.join(HERE, "golden", "method_matrix.json")) as fh:
        want = json.load(fh)
    return want, json.loads(json.dumps(rec.matrix(asw)))  # through JSON: lists and nulls as the file holds them


def test_same_table(rows):
    want, got = rows
    assert sorted(got) == sorted(want)
    assert len(want) > 1000


def test_valid_calls_agree_with_asw_volume_planes(rows):
    """what the golden file itself must satisfy: a selector call that kept its volume handed back asw_volume_planes planes"""
    want, _ = rows
    kept = [k for k, v in want.items() if k.split("/")[0] in ("host", "resident") and k.endswith("/vol") and v[0] == 0]
    assert "host/2/valid/vol" in kept and "resident/12/right/vol" in kept
    for k in kept:
        if k.startswith("resident/1/"):  # SGBM keeps no selector volume: the download is refused with ASW_ERR_NO_FRAME
            assert want[k][1] == "download status %d" % asw.ERR_NO_FRAME, k
        else:
            assert want[k][1] == want[k][2], k


@pytest.mark.parametrize("path", ["host", "resident", "own", "sgbm", "sgbm_paths", "stereoBM", "getDisparity_BM", "filterSpeckles"])
def test_rows_equal_the_recording(rows, path):
    want, got = rows
    keys = [k for k in want if k.split("/")[0] == path]
    assert keys
    diff = {k: (want[k], got.get(k)) for k in keys if want[k] != got.get(k)}
    assert not diff, "%d of %d rows differ (recorded, now): %s" % (len(diff), len(keys), sorted(diff.items())[:20])
