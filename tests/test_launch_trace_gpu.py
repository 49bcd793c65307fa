"""The eager launch sequence of one training step against tests/golden/launch_trace.json.

The Python programs (stfunet/program.py, unet.py, stf_lstm_unet.py, nhwc.py) are a schedule of
C-ABI calls; a recorded plan replays exactly that schedule.  The fixture was written by
tests/golden/make_golden_launch_trace.py from the commit before the programs were last
restructured: the order of the entry points, and the geometry of every implicit GEMM and weight
gradient, must still be that commit's.
"""
import json
import os

import pytest

import _launch_trace as lt
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "launch_trace.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("which", lt.CASES)
def test_launch_trace_matches_golden(golden, which):
    from stfunet import _lib
    table = dict(_lib._FNS.get(_lib.storage_dtype(), {}))
    want = golden["cases"][which]
    got = lt.capture(which)
    assert dict(_lib._FNS.get(_lib.storage_dtype(), {})) == table          # the wrappers are gone again
    assert golden["geom_fields"] == list(lt.GEOM) + ["Nout"]
    first = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    assert got == want, (f"{which}: {len(got)} launches, golden {len(want)}; first difference at {first}: "
                         f"{got[first:first + 3]} vs golden {want[first:first + 3]}")
