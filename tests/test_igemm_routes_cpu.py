"""The implicit-GEMM routes are pinned: for every launch signature of tests/golden/igemm_routes.json
(written by tests/golden/make_golden_routes.py from the build of the commit recorded in the file,
the parent of the change that introduced route_of) both storage builds name the same kernel and
answer the same statistics tiles, BN-backward tiles and split-K workspace bytes, with the statistics
pointer unset and set.  Host-only calls: nothing is launched.

The table assumes 256 compute units: that is the library's fallback when no GPU is present, and
it is the MI355X's count, so the same fixture holds on both machines.
"""
import importlib.util
import json
import os

import pytest
import torch

from conftest import GOLDEN

# Every entry of the igemm variant table (one slice per csrc/igemm_*.hip) that a launch can select
# without an environment override; the signatures must reach each of them.  Not listed: the two
# 128 x 256 'F' tile entries (STF_IGEMM_CFG=F only).  The three DIAG timing entries of the 16 x 32
# halo kernel are not in the shipped table (a -DHALO_DIAG build only).
DMA_A, DMA_B, DMA_C = "128, 128, 2, 2, 32, 4", "256, 128, 4, 2, 64, 3", "256, 256, 2, 4, 64, 2"
DMA_D, DMA_E = "512, 64, 8, 1, 64, 2", "256, 64, 4, 1, 32, 4"
REACHABLE = (
    ["conv3x3_c8_kernel", "conv3x3_halo4_kernel<0>"]
    + [f"conv3x3_wide_kernel<{v}>" for v in ("2, false", "1, false", "1, true")]
    + [f"conv3x3_halo2_kernel<{v}, false>" for v in ("2, false", "1, false", "1, true")]
    + [f"conv3x3_halo_kernel<16, {pw}, 8, 2, 0, {v}>" for pw in (16, 32)
       for v in ("2, false, false", "2, false, true", "1, false, true", "1, true, false", "1, true, true")]
    + [f"igemm_dma_kernel<{DMA_A}, {v}, false>"
       for v in ("false, false, 0", "false, false, 1", "false, false, 2", "false, true, 0", "true, false, 0")]
    + [f"igemm_dma_kernel<{DMA_E}, {v}, false>" for v in ("false, false, 0", "false, true, 0", "true, false, 0")]
    + [f"igemm_dma_kernel<{t}, false, false, 0, true>" for t in (DMA_A, DMA_E)]
    + [f"igemm_dma_kernel<{t}, false, {sc}, 0, false>" for t in (DMA_B, DMA_C, DMA_D) for sc in ("false", "true")]
    + [f"igemm_kernel<{t}, {smallc}, {v}, 0>" for t in ("128, 128, 2, 2", "256, 64, 4, 1")
       for smallc in ("false", "true") for v in ("false, false", "true, false", "false, true")]
    + [f"igemm_kernel<128, 128, 2, 2, false, false, false, {epi}>" for epi in (1, 2)]
)


def _generator():
    spec = importlib.util.spec_from_file_location("make_golden_routes", os.path.join(GOLDEN, "make_golden_routes.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "igemm_routes.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_every_route_matches_the_parent_build(golden, dtype):
    from stfunet import _lib
    gen = _generator()
    assert tuple(golden["fields"]) == gen.FIELDS and tuple(golden["results"]) == gen.RESULTS
    assert len(golden["commit"]) == 40 and golden["cus"] == 256
    lib = _lib.load(dtype)
    bad = [(s, want, got) for s, want in golden["routes"] for got in [gen.query(lib, s)] if got != want]
    assert not bad, f"{len(bad)} of {len(golden['routes'])} routes changed, first: {bad[0]}"


def test_signature_list_is_the_generators_and_reaches_every_variant(golden):
    gen = _generator()
    assert [tuple(s) for s, _ in golden["routes"]] == gen.signatures()
    seen = {r[0] for _, r in golden["routes"]}
    assert len(REACHABLE) == len(set(REACHABLE))
    assert seen == set(REACHABLE), (sorted(set(REACHABLE) - seen), sorted(seen - set(REACHABLE)))
