"""CPU checks of the inference outputs (stfunet.predict, csrc/predict.hip): the tests'
restatement against the reference-generated fixture, the Python argument checks and the C
side's refusals (no kernel launches)."""
import ctypes

import numpy as np
import pytest
import torch

from _predict_ref import counts_ref, fixture_cases, mask_ref, metrics_ref, overlay_ref

CASES = fixture_cases()
EINVAL = 100001


def test_fixture_covers_the_planned_ground():
    shapes = {tuple(c["frames"].shape[1:]) for c in CASES}
    assert {(1, 1), (3, 5), (17, 19), (24, 40)} <= shapes
    assert {c["logits"].shape[1] for c in CASES} == {1, 2, 4}
    assert {c["rule"] for c in CASES} == {"argmax", "sigmoid"}
    assert {c["paint"] for c in CASES} == {0, 1}
    assert {c["alpha"] for c in CASES} >= {0.0, 0.5, 1.0, 0.37}
    assert {c["threshold"] for c in CASES} == {0.5, 0.3}
    assert any(c["rule"] == "sigmoid" and c["channel"] == c["logits"].shape[1] - 1 > 0 for c in CASES)
    assert any((c["target"] == 255).any() for c in CASES)
    assert any(torch.isnan(c["logits"]).any() and torch.isinf(c["logits"]).any() for c in CASES)
    assert any((c["frames"] < 0).any() for c in CASES)
    assert any((f == f.flatten()[0]).all() and f.numel() > 1 for c in CASES for f in c["frames"])
    assert any(c["counts"].sum() == 0 for c in CASES)


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_restatement_reproduces_the_reference(c):
    mask = mask_ref(c["logits"], c["rule"], c["channel"], c["threshold"])
    assert torch.equal(mask, c["mask"])
    counts = counts_ref(mask, c["target"])
    assert torch.equal(counts, c["counts"])
    dice, iou = metrics_ref(counts)
    assert np.allclose(dice.numpy(), c["dice"].numpy(), rtol=1e-6, atol=0)
    assert np.allclose(iou.numpy(), c["iou"].numpy(), rtol=1e-6, atol=0)
    assert torch.equal(overlay_ref(c["frames"], mask, c["color"], c["alpha"], c["paint"]), c["overlay"])
    if "counts_ign255" in c:
        counts = counts_ref(mask, c["target"], ignore=255)
        assert torch.equal(counts, c["counts_ign255"])
        dice, iou = metrics_ref(counts)
        assert np.allclose(dice.numpy(), c["dice_ign255"].numpy(), rtol=1e-6, atol=0)
        assert np.allclose(iou.numpy(), c["iou_ign255"].numpy(), rtol=1e-6, atol=0)


def test_image_metrics_formula():
    from stfunet import image_metrics
    counts = torch.tensor([[0, 0, 0], [3, 5, 4], [7, 7, 7], [0, 9, 0]])
    dice, iou = image_metrics(counts)
    rd, ri = metrics_ref(counts)
    assert dice.dtype == iou.dtype == torch.float64
    assert torch.equal(dice, rd) and torch.equal(iou, ri)
    assert dice[0] == 1 and iou[0] == 1 and dice[2] == 1


def test_python_argument_checks():
    import stfunet
    from stfunet import predict as P
    assert stfunet.predict is P and stfunet.predict_masks is P.predict_masks and stfunet.overlay is P.overlay
    x = torch.zeros(2, 2, 4, 4)
    with pytest.raises(ValueError, match="rule"):
        P.predict_masks(x, rule="softmax")
    with pytest.raises(ValueError, match="channel"):
        P.predict_masks(x, rule="sigmoid", channel=2)
    with pytest.raises(ValueError, match="channel"):
        P.predict_masks({"out": x}, channel=-1)
    with pytest.raises(ValueError, match="classes"):
        P.predict_masks(torch.zeros(1, 17, 4, 4))
    with pytest.raises(ValueError, match="target"):
        P.predict_masks(x, target=torch.zeros(2, 4, 5, dtype=torch.int64))
    with pytest.raises(ValueError, match=r"\[B, K, H, W\]"):
        P.predict_masks(torch.zeros(2, 4, 4))
    f, m = torch.zeros(2, 4, 4), torch.zeros(2, 4, 4, dtype=torch.uint8)
    with pytest.raises(ValueError, match="alpha"):
        P.overlay(f, m, alpha=1.5)
    with pytest.raises(ValueError, match="alpha"):
        P.overlay(f, m, alpha=float("nan"))
    with pytest.raises(ValueError, match="color"):
        P.overlay(f, m, color=(0, 256, 0))
    with pytest.raises(ValueError, match="color"):
        P.overlay(f, m, color=(0, 255))
    with pytest.raises(ValueError, match="paint"):
        P.overlay(f, m, paint=2)
    with pytest.raises(ValueError, match="mask"):
        P.overlay(f, torch.zeros(2, 4, 5, dtype=torch.uint8))
    with pytest.raises(ValueError, match="rule"):
        P.predict(torch.nn.Identity(), [], "cpu", rule="max")
    with pytest.raises(ValueError, match="alpha"):
        P.predict(torch.nn.Identity(), [], "cpu", alpha=-0.1)


def test_no_cpu_fallback():
    from stfunet import predict as P
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.predict_masks(torch.zeros(1, 2, 4, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.predict_masks(torch.zeros(1, 2, 4, 4), rule="sigmoid", target=torch.zeros(1, 4, 4, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.overlay(torch.zeros(1, 4, 4), torch.zeros(1, 4, 4, dtype=torch.uint8))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_library_refuses_bad_arguments_without_launch(dtype):
    """STF_EINVAL with fake non-null pointers: nothing is launched or dereferenced."""
    from stfunet import _lib
    lib = _lib.load(dtype)
    fake = ctypes.c_void_p(1 << 20)

    def mask(K=2, channel=0, rule=0, logits=fake, target=fake, out=fake, counts=fake, B=2, HW=64):
        return lib.stf_predict_mask(logits, target, B, K, HW, rule, channel, 0.5, -1, out, counts, None)

    assert mask(K=0) == EINVAL and mask(K=17) == EINVAL
    assert mask(channel=2) == EINVAL and mask(channel=-1) == EINVAL and mask(K=16, channel=16) == EINVAL
    assert mask(rule=2) == EINVAL and mask(rule=-1) == EINVAL
    assert mask(logits=None) == EINVAL and mask(out=None) == EINVAL and mask(counts=None) == EINVAL
    assert mask(B=-1) == EINVAL and mask(HW=-1) == EINVAL
    assert mask(B=0) == 0                        # an empty batch: nothing to do, nothing launched

    def ovl(alpha=0.5, color=(0, 255, 0), paint=1, frames=fake, m=fake, out=fake, scratch=fake, stride=64, B=2):
        return lib.stf_predict_overlay(frames, stride, m, B, 8, 8, color[0], color[1], color[2], alpha, paint, out,
                                       scratch, None)

    assert ovl(alpha=-0.01) == EINVAL and ovl(alpha=1.01) == EINVAL and ovl(alpha=float("nan")) == EINVAL
    assert ovl(color=(256, 0, 0)) == EINVAL and ovl(color=(0, -1, 0)) == EINVAL and ovl(color=(0, 0, 300)) == EINVAL
    assert ovl(paint=2) == EINVAL and ovl(stride=-1) == EINVAL
    assert ovl(frames=None) == EINVAL and ovl(m=None) == EINVAL and ovl(out=None) == EINVAL
    assert ovl(scratch=None) == EINVAL
    assert ovl(B=0) == 0
    # the scratch query: one (min, max) row per block of the min / max pass, never more than 64 per image
    assert lib.stf_predict_overlay_scratch_bytes(0, 64) == 0
    assert lib.stf_predict_overlay_scratch_bytes(1, 1) == 8
    assert lib.stf_predict_overlay_scratch_bytes(3, 323) == 3 * 2 * 8
    assert lib.stf_predict_overlay_scratch_bytes(1, 1 << 24) == 64 * 8
    assert lib.stf_predict_overlay_scratch_bytes(64, 256 * 256) == 64 * 32 * 8
    assert lib.stf_predict_overlay_scratch_bytes(5000, 256 * 256) == 5000 * 8


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_bn_backward_refuses_groups_past_32_bit_units(dtype):
    """A statistics group of 2^31 or more 16-byte units: STF_EINVAL from stf_bn_bwd_reduce (without
    dpool) and stf_bn_bwd_apply, with fake non-null pointers -- nothing is launched or dereferenced."""
    from stfunet import _lib
    lib = _lib.load(dtype)
    fake = ctypes.c_void_p(1 << 20)
    N, H, W, C = 1 << 13, 1 << 9, 1 << 9, 8              # one group of 2^31 pixels x one 8-channel chunk
    assert (N * H * W) * (C // 8) == 1 << 31

    def reduce(N=N, C=C, groups=1):
        return lib.stf_bn_bwd_reduce(fake, C, None, fake, C, N, H, W, C, groups, fake, fake, fake, fake, 1, None, 0,
                                     fake, fake, None)

    def apply(M=N * H * W, C=C, groups=1):
        return lib.stf_bn_bwd_apply(fake, C, fake, C, M, C, groups, None, None, fake, fake, C, None, None, None)

    assert reduce() == EINVAL and apply() == EINVAL
    assert reduce(N=N // 2, C=16) == EINVAL and apply(C=16, M=N * H * W // 2) == EINVAL     # 2^30 pixels x 2 chunks
    assert reduce(N=2 * N, groups=2) == EINVAL and apply(M=2 * N * H * W, groups=2) == EINVAL
