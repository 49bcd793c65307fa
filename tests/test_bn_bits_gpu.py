"""The BatchNorm entry points compute the bits recorded in tests/golden/bn_bits.json.

The fixture was written by tests/golden/make_golden_bn_bits.py on an MI355X from the build of the
commit before csrc/bn.hip's streaming passes got one body per piece of arithmetic (its ``commit``
field); it holds case ids, seeds and SHA-256 digests only, for the bf16 and the fp16 library.  Each
case calls one C entry point directly on seeded inputs (tests/_bn_bits.py): every kernel, tail and
statistics-group path of the file.  Equal digests of every output buffer (pre-filled with NaN) --
no tolerance.  The cases no other test reaches (the generic apply kernel at C = 24, the
one-thread-per-window pooled reduce at C = 1024) are also compared with float64 on the CPU.
"""
import json
import os

import pytest

import _bn_bits as bb
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

with open(os.path.join(GOLDEN, "bn_bits.json")) as _f:
    FIXTURE = json.load(_f)
ROWS = {r["id"]: r for r in FIXTURE["cases"]}
CASES = [c for c in bb.cases() if bb.case_id(*c) not in FIXTURE["left_out"]]
IDS = [bb.case_id(*c) for c in CASES]


def test_fixture_covers_the_cases():
    assert sorted(list(ROWS) + FIXTURE["left_out"]) == sorted(bb.case_id(*c) for c in bb.cases())
    assert all(ROWS[bb.case_id(*c)]["seed"] == bb.seed_of(*c) for c in CASES)


@pytest.mark.parametrize("storage", list(bb.DTYPES))
@pytest.mark.parametrize("entry,shape,opts", CASES, ids=IDS)
def test_bn_bits(entry, shape, opts, storage):
    want = ROWS[bb.case_id(entry, shape, opts)][storage]
    outs, cpu = bb.run(entry, shape, opts, bb.DTYPES[storage])
    got = {k: bb._sha(v) for k, v in outs.items()}
    assert sorted(got) == sorted(want)
    for key in want:
        assert got[key] == want[key], f"{key} differs from the build of {FIXTURE['commit']}"
    if bb.is_ref(entry, shape, opts):
        errs = bb.ref_errors(entry, shape, opts, bb.DTYPES[storage], outs, cpu)
        print(bb.case_id(entry, shape, opts), storage, "rel-L2 vs float64", errs)
        assert max(errs.values()) <= bb.REF_BOUND, errs
