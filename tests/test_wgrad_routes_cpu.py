"""The weight-gradient routes are pinned: for every launch signature of tests/golden/wgrad_routes.json
(written by tests/golden/make_golden_wgrad_routes.py from the build of the commit recorded in the
file, the parent of the change that introduced csrc/wgrad.hip's route_of) both storage builds name
the same kernel and answer the same split count and workspace bytes.  Host-only calls: nothing is
launched.  "routes" carries the parity table and the model layers with their signatures; "sweep"
carries the answers of the whole completeness sweep at grid_blocks 0, 5 and 256, whose signatures
the generator lists in the same order (their count and SHA-256 are in the file).

The signatures carry their own workgroup budget (grid_blocks; 256 is the MI355X's CU count, which
the side stream passes), so the same fixture holds with and without a GPU.
"""
import importlib.util
import json
import os

import pytest
import torch

import _wgrad_variants as W
from conftest import GOLDEN


def _generator():
    spec = importlib.util.spec_from_file_location("make_golden_wgrad_routes",
                                                  os.path.join(GOLDEN, "make_golden_wgrad_routes.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "wgrad_routes.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_every_route_matches_the_parent_build(golden, dtype):
    from stfunet import _lib
    gen = _generator()
    assert tuple(golden["fields"]) == W.FIELDS and tuple(golden["results"]) == gen.RESULTS
    assert len(golden["commit"]) == 40 and golden["cus"] == 256 == W.CUS
    lib = _lib.load(dtype)
    names = golden["names"]
    pinned = golden["routes"] + [[list(s), r] for s, r in zip(gen.sweep_signatures(), golden["sweep"]["answers"])]
    assert len(pinned) == len(golden["routes"]) + golden["sweep"]["count"]
    bad = [(s, want, got) for s, (n, splits, ws) in pinned
           for want, got in [([names[n], splits, ws], gen.query(lib, s))] if got != want]
    assert not bad, f"{len(bad)} of {len(pinned)} routes changed, first: {bad[0]}"


def test_signature_lists_are_the_generators_and_reach_every_kernel(golden):
    gen = _generator()
    sigs = [tuple(s) for s, _ in golden["routes"]]
    assert sigs == gen.signatures()
    have = set(sigs)
    assert all(s in have for _, s, _ in W.cases()) and all(s in have for s in W.WIDE_4GIB.values())
    sweep = gen.sweep_signatures()
    sw = golden["sweep"]
    assert tuple(sw["budgets"]) == (0, 5, W.CUS)
    assert sw["count"] == len(sweep) == len(sw["answers"]) == 8820 and sw["sha256"] == gen.digest(sweep)
    for part in (golden["routes"], [[None, r] for r in sw["answers"]]):
        assert {golden["names"][r[0]] for _, r in part} == set(W.TABLE) == set(golden["names"])
