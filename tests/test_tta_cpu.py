"""Mirror test-time augmentation without a GPU (no launches): the declared and exported symbols,
the refusals of the new C entry points (they refuse before they launch, so fake non-null pointers
are enough), the view parser and the Python argument checks, which all come before any device work."""
import ctypes
import inspect
import os
import re

import pytest
import torch

from conftest import REPO

EINVAL = 100001
NEW = ("stf_flip_planes", "stf_tta_accumulate", "stf_predict_threshold")
BASE_KEYS = {"num", "dice", "iou", "mean_dice", "mean_iou"}


def test_header_symbols_are_the_exported_ones():
    from stfunet import _lib
    src = open(os.path.join(REPO, "include", "stfunet.h")).read()
    syms = set(re.findall(r"\b(stf_[a-z0-9_]+)\s*\(", src))
    assert syms == set(_lib.EXPORTED)
    assert set(NEW) <= syms
    for dtype in (torch.bfloat16, torch.float16):
        lib = _lib.load(dtype)
        assert all(hasattr(lib, s) for s in NEW)
        assert lib.stf_abi_version() == 17


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_flip_planes_refuses_bad_arguments_without_launch(dtype):
    from stfunet import _lib
    lib = _lib.load(dtype)
    fake, other = ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 21)

    def flip(x=fake, planes=6, H=8, W=8, code=1, y=other):
        return lib.stf_flip_planes(x, planes, H, W, code, y, None)

    assert flip(x=None) == EINVAL and flip(y=None) == EINVAL
    assert flip(y=fake) == EINVAL                                  # x == y
    assert flip(planes=0) == EINVAL and flip(H=0) == EINVAL and flip(W=0) == EINVAL
    assert flip(planes=-1) == EINVAL and flip(H=-3) == EINVAL and flip(W=-3) == EINVAL
    assert flip(code=-1) == EINVAL and flip(code=4) == EINVAL
    assert flip(planes=128, H=4096, W=4096) == EINVAL              # planes * H * W = 2^31
    assert flip(planes=1 << 31, H=1, W=1) == EINVAL
    assert flip(planes=1 << 62, H=4, W=1) == EINVAL                # would wrap a 64-bit product
    assert flip(planes=1, H=(1 << 31) - 1, W=(1 << 31) - 1) == EINVAL


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_tta_accumulate_refuses_bad_arguments_without_launch(dtype):
    from stfunet import _lib
    lib = _lib.load(dtype)
    fake, other = ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 21)

    def acc(logits=fake, B=2, K=3, H=8, W=8, rule=0, channel=0, code=0, first=1, n=0, out=other):
        return lib.stf_tta_accumulate(logits, B, K, H, W, rule, channel, code, first, n, out, None)

    assert acc(logits=None) == EINVAL and acc(out=None) == EINVAL
    assert acc(K=0) == EINVAL and acc(K=17) == EINVAL and acc(K=-1) == EINVAL
    assert acc(channel=3) == EINVAL and acc(channel=-1) == EINVAL and acc(K=16, channel=16) == EINVAL
    assert acc(rule=2) == EINVAL and acc(rule=-1) == EINVAL
    assert acc(code=4) == EINVAL and acc(code=-1) == EINVAL
    assert acc(B=0) == EINVAL and acc(H=0) == EINVAL and acc(W=0) == EINVAL and acc(B=-2) == EINVAL
    assert acc(n=-1) == EINVAL
    assert acc(B=8, K=16, H=4096, W=4096) == EINVAL                # B * K * H * W = 2^31
    assert acc(B=1 << 30, K=2, H=1, W=1) == EINVAL
    assert acc(B=(1 << 31) - 1, K=16, H=(1 << 31) - 1, W=(1 << 31) - 1) == EINVAL


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_mask_rules_past_sigmoid_stay_refused_and_threshold_checks_like_them(dtype):
    """stf_predict_mask keeps refusing every rule code but 0 and 1 (the threshold rule is an entry
    point of its own); stf_predict_threshold refuses what stf_predict_mask refuses."""
    from stfunet import _lib
    lib = _lib.load(dtype)
    fake = ctypes.c_void_p(1 << 20)
    for rule in (2, 3, -1):
        assert lib.stf_predict_mask(fake, fake, 2, 2, 64, rule, 0, 0.5, -1, fake, fake, None) == EINVAL

    def thr(K=2, channel=0, probs=fake, target=fake, out=fake, counts=fake, B=2, HW=64):
        return lib.stf_predict_threshold(probs, target, B, K, HW, channel, 0.5, -1, out, counts, None)

    assert thr(K=0) == EINVAL and thr(K=17) == EINVAL
    assert thr(channel=2) == EINVAL and thr(channel=-1) == EINVAL
    assert thr(probs=None) == EINVAL and thr(out=None) == EINVAL and thr(counts=None) == EINVAL
    assert thr(B=-1) == EINVAL and thr(HW=-1) == EINVAL
    assert thr(B=0) == 0                                           # an empty batch: nothing launched


def test_view_parser():
    from stfunet import predict as P
    assert P.parse_views(True) == ("none", "w", "h", "hw") == P.ALL_VIEWS
    assert P.parse_views(None) is None and P.parse_views(False) is None
    assert P.parse_views(("hw", "none")) == ("hw", "none") and P.parse_views(["h"]) == ("h",)
    assert P.VIEWS == {"none": 0, "w": 1, "h": 2, "hw": 3}         # bit 0 = W, bit 1 = H
    assert P.RULES == {"argmax": 0, "sigmoid": 1, "threshold": 2}
    for bad, what in (((), "empty"), ([], "empty"), (("w", "w"), "repeats"), (("none", "h", "none"), "repeats"),
                      (("x",), "unknown view"), (("wh",), "unknown view"), ((1,), "string"), ((None,), "string"),
                      (("w", 3), "string"), ("hw", "tuple"), (1, "tuple"), (3.5, "tuple")):
        with pytest.raises(ValueError, match=what):
            P.parse_views(bad)


class Boom(torch.nn.Module):
    """A model that must not run: the argument checks come before any forward."""

    def forward(self, x):
        raise AssertionError("the model ran")


def test_python_argument_checks_come_before_any_device_work():
    import stfunet
    from stfunet import predict as P
    assert stfunet.flip_planes is P.flip_planes and stfunet.tta_probabilities is P.tta_probabilities
    assert stfunet.predict_tta is P.predict_tta
    x = torch.zeros(2, 3, 4, 6)
    batches = [x]
    for bad in ((), ("x",), ("w", "w"), (2,), "hw"):
        with pytest.raises(ValueError):
            P.tta_probabilities(Boom(), x, bad)
        with pytest.raises(ValueError):
            P.predict_tta(Boom(), batches, "cpu", tta=bad)
    with pytest.raises(ValueError, match="view set"):
        P.tta_probabilities(Boom(), x, None)
    with pytest.raises(ValueError, match="keep_probs"):
        P.predict_tta(Boom(), batches, "cpu", tta=None, keep_probs=True)
    with pytest.raises(ValueError, match="keep_probs"):
        P.predict_tta(Boom(), batches, "cpu", tta=False, keep_probs=True)
    for f in (lambda: P.tta_probabilities(Boom(), x, True, rule="threshold"),
              lambda: P.tta_probabilities(Boom(), x, True, rule="softmax"),
              lambda: P.predict_tta(Boom(), batches, "cpu", rule="threshold")):
        with pytest.raises(ValueError, match="rule|argmax"):
            f()
    with pytest.raises(TypeError):
        P.predict_tta(Boom(), batches, "cpu", keep_largest_component=True)
    for bad in ("x", "wh", None, 1):
        with pytest.raises(ValueError, match="view"):
            P.flip_planes(x, bad)
    with pytest.raises(ValueError, match="2 dimensions"):
        P.flip_planes(torch.zeros(5), "w")
    with pytest.raises(ValueError, match="fp32"):
        P.flip_planes(x.double(), "w")
    with pytest.raises(ValueError, match="2\\^31"):                # an expanded view: no memory behind it
        P.flip_planes(torch.zeros(1, 1, 1).expand(128, 4096, 4096), "h")
    with pytest.raises(ValueError, match="channel"):
        P.predict_masks(x, rule="threshold", channel=3)
    # host tensors: the usual refusal, and the model's training mode is put back
    for f in (lambda: P.flip_planes(x, "hw"), lambda: P.predict_masks(x, rule="threshold"),
              lambda: P.tta_probabilities(Boom(), x)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            f()


def test_result_keys_and_signatures():
    from stfunet import predict as P
    ident = torch.nn.Identity()
    assert set(P.predict(ident, [], "cpu")) == BASE_KEYS
    assert set(P.predict_tta(ident, [], "cpu", tta=None)) == BASE_KEYS
    assert set(P.predict_tta(ident, [], "cpu")) == BASE_KEYS
    res = P.predict_tta(ident, [], "cpu", tta=("w",), keep_probs=True, keep_masks=True, rule="sigmoid")
    assert set(res) == BASE_KEYS | {"probs", "masks"} and res["probs"] == [] and res["num"] == 0
    # the shared loop takes predict's options with predict's defaults, in predict's order
    opts = list(inspect.signature(P.predict).parameters.values())[3:]
    loop = list(inspect.signature(P._predict).parameters.values())[5:]
    assert [(p.name, p.default) for p in opts] == [(p.name, p.default) for p in loop]
    got = [(p.name, p.default) for p in list(inspect.signature(P.predict_tta).parameters.values())[3:5]]
    assert got == [("tta", True), ("keep_probs", False)]


def test_tta_probabilities_restores_the_training_mode_on_error():
    from stfunet import predict as P
    x = torch.zeros(1, 2, 4, 4)
    for mode in (True, False):
        m = Boom().train(mode)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            P.tta_probabilities(m, x)
        assert m.training is mode
