"""Connected-component post-processing without a GPU: the numpy restatement (tests/_components_ref.py)
against the scipy-generated fixture tests/golden/components.npz, the filter's rules on hand-made
masks, and the argument checks of the Python surface and of the C entry points (which refuse before
they launch, so fake pointers are enough)."""
import ctypes
import importlib.util
import inspect
import os

import numpy as np
import pytest
import torch

from _components_ref import GOLDEN, batch_filter, counts_of, filter_mask, fixture_cases, label

CASES = fixture_cases()
EINVAL = 100001


def _generator():
    spec = importlib.util.spec_from_file_location("make_golden_components",
                                                  os.path.join(GOLDEN, "make_golden_components.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_fixture_covers_the_planned_ground():
    by = {c["name"]: c for c in CASES}
    assert len(CASES) == 20 and os.path.getsize(os.path.join(GOLDEN, "components.npz")) < 64 * 1024
    for shape in ((33, 47), (97, 131)):
        for d in ("200", "500", "593", "800"):
            assert by[f"rand_{shape[0]}x{shape[1]}_d{d}"]["mask"].shape == shape
    assert by["checkerboard"]["n4"] == 2048 and by["checkerboard"]["n8"] == 1
    assert by["checkerboard"]["mask"].shape == by["spiral"]["mask"].shape == (64, 64)
    for name in ("diagonal", "antidiagonal"):
        assert by[name]["n8"] == 1 and by[name]["n4"] == int(by[name]["mask"].sum()) == 50
    for name in ("u_shape", "comb", "spiral", "serpentine", "full"):
        assert by[name]["n4"] == by[name]["n8"] == 1
    assert by["spiral"]["mask"].sum() > 2000                      # one chain through half the image
    assert by["ring_island"]["n4"] == by["ring_island"]["n8"] == 2 == by["tie"]["n8"]
    assert by["blob_specks"]["n8"] >= 10
    assert by["empty"]["n4"] == by["empty"]["n8"] == 0 and not by["empty"]["mask"].any()


def test_fixture_is_what_the_generator_makes():
    made = _generator().cases()
    assert [n for n, _ in made] == [c["name"] for c in CASES]
    for (_, m), c in zip(made, CASES):
        assert np.array_equal(m, c["mask"])


def test_fixture_labels_are_scipys():
    pytest.importorskip("scipy")
    gen = _generator()
    for c in CASES:
        for k in (4, 8):
            labels, n = gen.scipy_label(c["mask"], k)
            assert n == c[f"n{k}"] and np.array_equal(labels, c[f"labels{k}"]), (c["name"], k)


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_restatement_reproduces_the_fixture(c):
    for k in (4, 8):
        labels, n = label(c["mask"], k)
        assert labels.dtype == np.int32 and n == c[f"n{k}"]
        assert np.array_equal(labels, c[f"labels{k}"]), k


def test_filter_tie_goes_to_the_raster_first_component():
    tie = next(c for c in CASES if c["name"] == "tie")["mask"]
    out, n = filter_mask(tie, keep_largest=True)
    assert n == 2 and out[5:11, 60:64].all() and out.sum() == 24 and not out[8:12, 3:9].any()
    # three components, the two largest equal and the raster-first one of those not the first component
    m = np.zeros((8, 12), np.uint8)
    m[0, 0] = 1
    m[2:4, 8:11] = 1
    m[3:5, 1:4] = 1
    out, n = filter_mask(m, keep_largest=True)
    assert n == 3 and out[2:4, 8:11].all() and out.sum() == 6


def test_filter_min_size_is_inclusive_and_applies_first():
    m = np.zeros((8, 12), np.uint8)
    m[0, 0:3] = 1                                                 # area 3
    m[4:6, 4:8] = 1                                               # area 8
    m[7, 11] = 1                                                  # area 1
    assert filter_mask(m, min_size=3)[0].sum() == 11
    assert filter_mask(m, min_size=4)[0].sum() == 8
    assert filter_mask(m, min_size=8)[0].sum() == 8 and filter_mask(m, min_size=9)[0].sum() == 0
    assert filter_mask(m, keep_largest=True, min_size=8)[0].sum() == 8
    assert filter_mask(m, keep_largest=True, min_size=9)[0].sum() == 0
    out, n = filter_mask(m)
    assert n == 3 and np.array_equal(out, m)
    out, n = filter_mask(np.zeros((3, 3), np.uint8), keep_largest=True)
    assert n == 0 and not out.any()


def test_filter_keeps_class_ids_and_connectivity_matters():
    m = np.zeros((6, 10), np.uint8)
    m[0:2, 0:2] = 1
    m[2:4, 2:4] = 2                                               # touches the first block by a corner
    m[5, 9] = 3
    out, n = filter_mask(m, keep_largest=True, connectivity=8)
    assert n == 2 and np.array_equal(out, np.where(m == 3, 0, m))
    out, n = filter_mask(m, keep_largest=True, connectivity=4)
    assert n == 3 and np.array_equal(out, np.where(m == 1, m, 0))   # equal areas: the raster-first block


def test_counts_follow_the_mask_rules():
    m = np.array([[1, 1, 0, 0], [0, 0, 0, 2]], np.uint8)
    t = np.array([[1, 0, 0, 255], [3, 0, 0, 255]], np.int64)
    assert counts_of(m, t).tolist() == [2, 3, 4]
    assert counts_of(m, t, ignore=255).tolist() == [1, 2, 2]
    out, num, counts = batch_filter(m[None], keep_largest=True, target=t[None], ignore=255)
    assert num.tolist() == [2] and counts.tolist() == [[1, 2, 2]] and out[0, 1, 3] == 0


def test_python_argument_checks():
    from stfunet import predict as P
    import stfunet
    assert stfunet.connected_components is P.connected_components
    assert stfunet.filter_components is P.filter_components
    m = torch.zeros(2, 8, 8, dtype=torch.uint8)
    for bad in (0, 6, 2, "8", None, 8.5, True):
        with pytest.raises(ValueError, match="connectivity"):
            P.connected_components(m, connectivity=bad)
        with pytest.raises(ValueError, match="connectivity"):
            P.filter_components(m, connectivity=bad)
        with pytest.raises(ValueError, match="connectivity"):
            P.predict(torch.nn.Identity(), [], "cpu", connectivity=bad)
    for bad in (-1, 1.0, 2.5, "3", None, True, False, 1 << 63):
        with pytest.raises(ValueError, match="min_size"):
            P.filter_components(m, min_size=bad)
        with pytest.raises(ValueError, match="min_size"):
            P.predict(torch.nn.Identity(), [], "cpu", min_size=bad)
    for f in (P.connected_components, P.filter_components):
        with pytest.raises(ValueError, match="integer"):
            f(m.float())
        with pytest.raises(ValueError, match=r"\[B, H, W\]"):
            f(m[0])
        with pytest.raises(ValueError, match="4096"):
            f(torch.zeros(1, 1, 4097, dtype=torch.uint8))
        with pytest.raises(ValueError, match="2\\^31"):           # an expanded view: no memory behind it
            f(torch.zeros(1, 1, 1, dtype=torch.uint8).expand(128, 4096, 4096))
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            f(m)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            f(m.bool())
    with pytest.raises(ValueError, match="does not match"):
        P.filter_components(m, target=torch.zeros(2, 8, 9, dtype=torch.int64))
    with pytest.raises(ValueError, match="integer"):
        P.filter_components(m, target=torch.zeros(2, 8, 8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.filter_components(m, target=torch.zeros(2, 8, 8, dtype=torch.int64), min_size=np.int64(3))
    with pytest.raises(TypeError):
        P.predict(torch.nn.Identity(), [], "cpu", keep_largest_component=True)
    # an empty loader: the key appears with the options, and only then
    base = {"num", "dice", "iou", "mean_dice", "mean_iou"}
    assert set(P.predict(torch.nn.Identity(), [], "cpu")) == base
    assert set(P.predict(torch.nn.Identity(), [], "cpu", connectivity=4)) == base
    for kw in (dict(keep_largest=True), dict(min_size=5), dict(keep_largest=True, min_size=2, connectivity=4)):
        res = P.predict(torch.nn.Identity(), [], "cpu", **kw)
        assert set(res) == base | {"num_components"} and res["num_components"] is None


def test_predict_signature_keeps_its_order_and_defaults():
    from stfunet.predict import predict
    params = list(inspect.signature(predict).parameters.values())
    assert all(p.kind == p.POSITIONAL_OR_KEYWORD for p in params)
    got = [(p.name, p.default) for p in params]
    assert got == [("model", inspect.Parameter.empty), ("data_loader", inspect.Parameter.empty),
                   ("device", inspect.Parameter.empty), ("rule", "argmax"), ("channel", 0), ("threshold", 0.5),
                   ("ignore_index", None), ("output_dir", None), ("prefix", "unet"), ("color", (0, 255, 0)),
                   ("alpha", 0.5), ("paint", 1), ("keep_masks", False), ("boundary", False), ("spacing", 1.0),
                   ("keep_largest", False), ("min_size", 0), ("connectivity", 8)]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_library_refuses_bad_arguments_without_launch(dtype):
    """STF_EINVAL with fake non-null pointers: nothing is launched or dereferenced."""
    from stfunet import _lib
    lib = _lib.load(dtype)
    fake, other = ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 21)

    def at(offset):
        return ctypes.c_void_p((1 << 21) + offset)

    def lab(mask=fake, B=2, H=8, W=8, conn=8, labels=other, num=other, scratch=other):
        return lib.stf_ccl_label(mask, B, H, W, conn, labels, num, scratch, None)

    def fil(mask=fake, target=other, B=2, H=8, W=8, conn=8, keep=1, min_size=0, out=other, counts=other,
            num=other, scratch=other):
        return lib.stf_ccl_filter(mask, target, B, H, W, conn, keep, min_size, -1, out, counts, num, scratch, None)

    assert lab(mask=None) == EINVAL and lab(labels=None) == EINVAL and lab(num=None) == EINVAL
    assert lab(scratch=None) == EINVAL
    assert fil(mask=None) == EINVAL and fil(out=None) == EINVAL and fil(scratch=None) == EINVAL
    assert fil(target=None) == EINVAL                              # counts without target
    assert fil(out=fake) == EINVAL                                 # out == mask
    assert fil(min_size=-1) == EINVAL
    for f in (lab, fil):
        assert all(f(conn=c) == EINVAL for c in (0, 1, 2, 6, 9, -8))
        assert f(B=0) == EINVAL and f(H=0) == EINVAL and f(W=0) == EINVAL and f(B=-1) == EINVAL
        assert f(H=4097) == EINVAL and f(W=4097) == EINVAL
        assert f(B=128, H=4096, W=4096) == EINVAL                  # B * H * W = 2^31
        assert f(B=1 << 30, H=2, W=1) == EINVAL
        assert f(scratch=at(4)) == EINVAL and f(num=at(2)) == EINVAL
    assert lab(labels=at(2)) == EINVAL
    assert fil(counts=at(4)) == EINVAL and fil(target=at(4)) == EINVAL
    sb = lib.stf_ccl_scratch_bytes
    assert sb(0, 8, 8) == 0 and sb(1, 0, 8) == 0 and sb(1, 8, 4097) == 0 and sb(128, 4096, 4096) == 0
    # the selected roots (int32 per image, 256-byte rounded) and two int32 planes
    assert sb(1, 1, 1) == 256 + 8 and sb(3, 5, 7) == 256 + 8 * 105 and sb(65, 8, 8) == 512 + 8 * 65 * 64
    assert sb(64, 256, 256) == 256 + 8 * 64 * 256 * 256
    assert sb(127, 4096, 4096) == 512 + 8 * 127 * 4096 * 4096      # beyond 32 bits: size_t
