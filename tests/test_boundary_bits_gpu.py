"""The distance-transform kernels compute the bits, and ask for the scratch sizes, recorded in
tests/golden/boundary_bits.json.

The fixture was written by tests/golden/make_golden_boundary_bits.py on an MI355X from the build of the
commit before the three copies of the passes (image metrics, volume metrics, the boundary loss's maps)
became one family (its ``commit`` field); it holds names, seeds, sizes and SHA-256 digests only.  Each
case of tests/_boundary_bits.py calls the C entry points directly on outputs and scratch pre-filled with
0xAA: stf_edt_sq and stf_boundary_metrics on the image shapes, stf_edt3d_sq and stf_boundary3d_metrics on
the volume stacks, stf_sdf on the map shapes and stf_bloss_fwd / stf_bloss_bwd once.  Equal digests and
equal scratch sizes -- no tolerance.
"""
import json
import os

import pytest

import _boundary_bits as bb
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

with open(os.path.join(GOLDEN, "boundary_bits.json")) as _f:
    FIXTURE = json.load(_f)
ROWS = {r["case"]: r for r in FIXTURE["cases"]}


def test_fixture_covers_the_cases():
    assert sorted(ROWS) == sorted(bb.cases()) and len(ROWS) == 11
    assert FIXTURE["ignore_index"] == bb.IGNORE and FIXTURE["grad_out"] == bb.GRAD_OUT
    assert FIXTURE["alpha"] == bb.ALPHA
    assert all(r["seed"] == bb.seed_of(name) for name, r in ROWS.items())


@pytest.mark.parametrize("name", bb.cases())
def test_boundary_bits(name):
    want = {k: v for k, v in ROWS[name].items() if k not in ("case", "seed")}
    got = bb.digests(name)
    print(name, {k: v for k, v in got.items() if not isinstance(v, str) or len(v) < 40})
    assert sorted(got) == sorted(want)
    for key in sorted(want):
        assert got[key] == want[key], f"{key} differs from the build of {FIXTURE['commit']}"
