"""The BatchNorm routes are pinned: for every signature of tests/golden/bn_routes.json (written by
tests/golden/make_golden_bn_routes.py from the build of the commit recorded in the file, the parent of
the change that introduced csrc/bn.hip's bn_route) both storage builds answer the same partial rows
from stf_bn_bwd_tiles (pooled 0 and 1) and stf_bn_bwd_apply_tiles.  Host-only calls: nothing is
launched.  "routes" carries the parity tables and the models' BatchNorms with their signatures; "sweep"
carries the answers of the cap sweep, whose signatures the generator lists in the same order (their
count and SHA-256 are in the file).

The bias rows of stf_bn_bwd_apply have no query of their own: the caller allocates
stf_bn_bwd_apply_tiles rows for all groups together and the launch writes groups x (blocks per group).
tests/_bn_ref.g_tiles, the independent port of the file's constants, gives the blocks per group; where
groups x that exceeds the allocation (more groups than rows: every group needs a block of its own) the
call must be refused before anything is launched.
"""
import ctypes
import importlib.util
import json
import os

import pytest
import torch

import _bn_ref as R
from conftest import GOLDEN


def _generator():
    spec = importlib.util.spec_from_file_location("make_golden_bn_routes",
                                                  os.path.join(GOLDEN, "make_golden_bn_routes.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "bn_routes.json")) as f:
        return json.load(f)


def _pinned(golden, gen):
    return [(tuple(s), r) for s, r in golden["routes"]] + list(zip(gen.sweep_signatures(), golden["sweep"]["answers"]))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_every_route_matches_the_parent_build(golden, dtype):
    from stfunet import _lib
    gen = _generator()
    assert tuple(golden["fields"]) == gen.FIELDS and tuple(golden["results"]) == gen.RESULTS
    assert len(golden["commit"]) == 40
    lib = _lib.load(dtype)
    pinned = _pinned(golden, gen)
    assert len(pinned) == len(golden["routes"]) + golden["sweep"]["count"]
    bad = [(s, want, got) for s, want in pinned for got in [gen.query(lib, s)] if got != want]
    assert not bad, f"{len(bad)} of {len(pinned)} routes changed, first: {bad[0]}"


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_bias_rows_fit_the_allocation_or_the_call_is_refused(golden, dtype):
    from stfunet import _lib
    lib = _lib.load(dtype)
    fake = ctypes.c_void_p(1 << 20)                        # a refused call reads and launches nothing
    fits = refused = 0
    for (N, H, W, C, G), _ in _pinned(golden, _generator()):
        M = N * H * W
        if not R.cg_ok(C) or M // G * (C // 8) >= 1 << 31:
            continue                                       # refused for the shape alone
        alloc = lib.stf_bn_bwd_apply_tiles(M, C)
        rows = G * R.g_tiles(M // G * (C // 8), G, alloc)
        if rows <= alloc:
            fits += 1
        else:
            assert G > alloc, (N, H, W, C, G, rows, alloc)
            assert lib.stf_bn_bwd_apply(fake, C, fake, C, M, C, G, None, None, fake, fake, C, fake, fake,
                                        None) == R.EINVAL, (N, H, W, C, G)
            refused += 1
    assert fits > 500 and refused > 0


def test_signature_lists_are_the_generators_and_reach_every_cap(golden):
    gen = _generator()
    sigs = [tuple(s) for s, _ in golden["routes"]]
    assert sigs == gen.signatures()
    have = set(sigs)
    assert gen.table_signatures() <= have and (128, 128, 128, 64, 8) in have and (64, 256, 256, 64, 1) in have
    sweep = gen.sweep_signatures()
    sw = golden["sweep"]
    assert sw["count"] == len(sweep) == len(sw["answers"]) and sw["sha256"] == gen.digest(sweep)
    assert {s[3] for s in sweep} == set(gen.SWEEP_C) and {s[4] for s in sweep} == set(gen.SWEEP_G)
    # both sides of every cap: the reduce's rows per group and the bias rows at 1, between, and at the cap
    for G in gen.SWEEP_G:
        cap = -(-R.ROW_CAP // G)
        for k in (0, 1):
            got = {r[k] for s, r in zip(sweep, sw["answers"]) if s[4] == G}
            assert {1, cap} <= got and any(1 < t < cap for t in got), (G, k, sorted(got))
    got = {r[2] for r in sw["answers"]}
    assert {1, R.ROW_CAP} <= got and any(1 < t < R.ROW_CAP for t in got)
    # the block cap of the act / plain apply grid: units per group on both sides of (cap / groups) blocks
    for G in gen.SWEEP_G:
        per = max(R.ACT_CAP // G, 1)
        blocks = {-(-(s[0] // G * s[1] * s[2] * (s[3] // 8)) // (R.NT * R.UPT)) for s in sweep if s[4] == G}
        assert any(b < per for b in blocks) and any(b > per for b in blocks), G
