"""The criterion kernels compute the bits recorded in tests/golden/loss_bits.json and
tests/golden/loss_bits_manyclass.json.

The fixture was written by tests/golden/make_golden_loss_bits.py on an MI355X from the build of
the commit before the default and the option kernels became one template family (its ``commit``
field); it holds seeds, shapes and SHA-256 digests only.  Each case calls the C entry points
directly: the default pair, and the option pair with class weights, ``ignore_index=255`` on padded
bands plus one fully ignored image, Dice on (once with Dice off).  Equal digests of the loss, of
the documented leading floats of ``terms`` and of ``dlogits`` (pre-filled with NaN) -- no tolerance.

loss_bits_manyclass.json holds the same digests for the many-class pair (``stf_loss_mc_*``) and the focal /
Tversky pair (``stf_loss_ft_*``) under the option family's input rule, written from the build of the commit
before those two became one ``<KP, FT>`` template family (``mc_cases`` of tests/_loss_bits.py: each shape is
the smallest that reaches one seam of the kernels).
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
with open(os.path.join(GOLDEN, "loss_bits_manyclass.json")) as _f:
    MC_FIXTURE = json.load(_f)
MC_ROWS = {lb.case_id(r["family"], tuple(r["shape"])): r for r in MC_FIXTURE["cases"]}


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


def test_manyclass_fixture_covers_the_cases():
    assert sorted(MC_ROWS) == sorted(lb.case_id(f, s) for f, s in lb.mc_cases())
    assert len(MC_FIXTURE["cases"]) == len(MC_ROWS) == 16
    assert MC_FIXTURE["ignore_index"] == lb.IGNORE and MC_FIXTURE["grad_out"] == lb.GRAD_OUT
    assert all(r["seed"] == lb.seed_of(tuple(r["shape"])) for r in MC_ROWS.values())


@pytest.mark.parametrize("family,shape", lb.mc_cases(), ids=[lb.case_id(f, s) for f, s in lb.mc_cases()])
def test_manyclass_loss_bits(family, shape):
    want = MC_ROWS[lb.case_id(family, shape)]
    got = lb.digests(family, shape)
    print(lb.case_id(family, shape), "loss", got["loss_value"], "recorded", want["loss_value"])
    for key in ("loss", "terms", "dlogits"):
        assert got[key] == want[key], f"{key} differs from the build of {MC_FIXTURE['commit']}"
