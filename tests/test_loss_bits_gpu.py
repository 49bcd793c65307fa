"""The criterion kernels compute the bits recorded in tests/golden/loss_bits.json.

The fixture was written by tests/golden/make_golden_loss_bits.py on an MI355X from the build of
the commit before the default and the option kernels became one template family (its ``commit``
field); it holds seeds, shapes and SHA-256 digests only.  Each case calls the C entry points
directly: the default pair, and the option pair with class weights, ``ignore_index=255`` on padded
bands plus one fully ignored image, Dice on (once with Dice off).  Equal digests of the loss, of
the documented leading floats of ``terms`` and of ``dlogits`` (pre-filled with NaN) -- no tolerance.
"""
import json
import os

import pytest

import _loss_bits as lb
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

with open(os.path.join(GOLDEN, "loss_bits.json")) as _f:
    FIXTURE = json.load(_f)
ROWS = {lb.case_id(r["family"], tuple(r["shape"])): r for r in FIXTURE["cases"]}


def test_fixture_covers_the_cases():
    assert sorted(ROWS) == sorted(lb.case_id(f, s) for f, s in lb.cases())
    assert FIXTURE["ignore_index"] == lb.IGNORE and FIXTURE["grad_out"] == lb.GRAD_OUT
    assert all(r["seed"] == lb.seed_of(tuple(r["shape"])) for r in ROWS.values())


@pytest.mark.parametrize("family,shape", lb.cases(), ids=[lb.case_id(f, s) for f, s in lb.cases()])
def test_loss_bits(family, shape):
    want = ROWS[lb.case_id(family, shape)]
    got = lb.digests(family, shape)
    print(lb.case_id(family, shape), "loss", got["loss_value"], "recorded", want["loss_value"])
    for key in ("loss", "terms", "dlogits"):
        assert got[key] == want[key], f"{key} differs from the build of {FIXTURE['commit']}"
