"""Inference outputs on the GPU (csrc/predict.hip through stfunet.predict): masks, per-image
counts and overlay bytes equal the reference-generated fixture (tests/golden/predict.npz) and,
on shapes the fixture does not hold, the restatement in tests/_predict_ref.py.

Masks, counts and overlays are compared for equality.  Dice / IoU are compared at relative 1e-6
(the reference mixes float32 and float64; the device computes float64 from exact counts).

The kernel-level tests call the C entry points on buffers with 64 guard bytes on each side and
run every case twice, the buffers prefilled with 0xAA and then 0x55: equal results show that
every output byte is written and that two runs agree bit for bit; the guards must keep their fill.
"""
import os

import numpy as np
import pytest
import torch

from _predict_ref import away_from_ties, counts_ref, fixture_cases, mask_ref, metrics_ref, overlay_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
CASES = fixture_cases()
RULES = {"argmax": 0, "sigmoid": 1}


class Guarded:
    """``nbytes`` of device memory between two guards, everything prefilled with ``fill``."""

    def __init__(self, nbytes, fill):
        self.fill, self.n = fill, nbytes
        self.raw = torch.full((nbytes + 2 * GUARD,), fill, dtype=torch.uint8, device=DEV)
        self.body = self.raw[GUARD:GUARD + nbytes]

    def guards_intact(self):
        return bool((self.raw[:GUARD] == self.fill).all() and (self.raw[GUARD + self.n:] == self.fill).all())


def run_kernels(logits, target, frames, rule, channel, threshold, color, alpha, paint, ignore=-1, fill=0xAA):
    """Mask, counts and overlay through the C entry points on guarded buffers.  ``frames`` may be
    any [B, H, W] device view whose last two dimensions are contiguous."""
    from stfunet import _lib
    from stfunet._lib import call, stream
    B, K, H, W = logits.shape
    HW = H * W
    mask, counts, pic = Guarded(B * HW, fill), Guarded(B * 24, fill), Guarded(B * HW * 3, fill)
    scratch = Guarded(_lib.load().stf_predict_overlay_scratch_bytes(B, HW), fill)
    assert frames.stride(2) == 1 and frames.stride(1) == W
    call("stf_predict_mask", logits.data_ptr(), target.data_ptr(), B, K, HW, RULES[rule], channel, threshold, ignore,
         mask.body.data_ptr(), counts.body.data_ptr(), stream())
    call("stf_predict_overlay", frames.data_ptr(), frames.stride(0), mask.body.data_ptr(), B, H, W, color[0], color[1],
         color[2], alpha, paint, pic.body.data_ptr(), scratch.body.data_ptr(), stream())
    torch.cuda.synchronize()
    for g in (mask, counts, pic, scratch):
        assert g.guards_intact()
    return (mask.body.view(B, H, W).cpu(), counts.body.view(torch.int64).view(B, 3).cpu(),
            pic.body.view(B, H, W, 3).cpu())


def run_twice(*args, **kw):
    first = run_kernels(*args, fill=0xAA, **kw)
    second = run_kernels(*args, fill=0x55, **kw)
    for a, b in zip(first, second):
        assert torch.equal(a, b)
    return first


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_fixture_cases_through_the_kernels(c):
    from stfunet import image_metrics
    mask, counts, pic = run_twice(c["logits"].to(DEV), c["target"].to(DEV), c["frames"].to(DEV), c["rule"],
                                  c["channel"], c["threshold"], c["color"], c["alpha"], c["paint"])
    assert torch.equal(mask, c["mask"])
    assert torch.equal(counts, c["counts"])
    assert torch.equal(pic, c["overlay"])
    dice, iou = image_metrics(counts.to(DEV))
    assert dice.is_cuda and dice.dtype == torch.float64
    assert np.allclose(dice.cpu().numpy(), c["dice"].numpy(), rtol=1e-6, atol=0)
    assert np.allclose(iou.cpu().numpy(), c["iou"].numpy(), rtol=1e-6, atol=0)
    if "counts_ign255" in c:
        _, counts, _ = run_twice(c["logits"].to(DEV), c["target"].to(DEV), c["frames"].to(DEV), c["rule"],
                                 c["channel"], c["threshold"], c["color"], c["alpha"], c["paint"], ignore=255)
        assert torch.equal(counts, c["counts_ign255"])
        dice, iou = image_metrics(counts.to(DEV))
        assert np.allclose(dice.cpu().numpy(), c["dice_ign255"].numpy(), rtol=1e-6, atol=0)
        assert np.allclose(iou.cpu().numpy(), c["iou_ign255"].numpy(), rtol=1e-6, atol=0)


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_fixture_cases_through_the_python_surface(c):
    from stfunet import overlay, predict_masks
    mask, counts = predict_masks({"out": c["logits"].to(DEV)}, c["rule"], c["channel"], c["threshold"],
                                 target=c["target"].to(DEV))
    assert mask.dtype == torch.uint8 and mask.is_cuda and counts.dtype == torch.int64
    assert torch.equal(mask.cpu(), c["mask"]) and torch.equal(counts.cpu(), c["counts"])
    only = predict_masks(c["logits"].to(DEV), c["rule"], c["channel"], c["threshold"])
    assert torch.equal(only, mask)
    pic = overlay(c["frames"].to(DEV), mask, c["color"], c["alpha"], c["paint"])
    assert pic.dtype == torch.uint8 and torch.equal(pic.cpu(), c["overlay"])


# HW = 1, 15, 255, 256, 257, 323: below / at / above a quad, a wave and a block, odd image bases
SEAMS = [(1, 1), (3, 5), (15, 17), (16, 16), (1, 257), (17, 19)]


@pytest.mark.parametrize("rule,K,channel,threshold", [("argmax", 3, 0, 0.5), ("sigmoid", 2, 1, 0.3)])
@pytest.mark.parametrize("H,W", SEAMS)
def test_seam_shapes_against_the_restatement(H, W, rule, K, channel, threshold):
    g = torch.Generator().manual_seed(1000 * H + W)
    B = 3
    logits = away_from_ties(torch.randn(B, K, H, W, generator=g) * 2, rule, channel, threshold, margin=1e-3)
    target = torch.randint(0, 2, (B, H, W), generator=g)
    frames = torch.randn(B, H, W, generator=g) * 3 - 1
    color, alpha, paint = (200, 17, 255), 0.37, (H + W) % 2
    mask, counts, pic = run_twice(logits.to(DEV), target.to(DEV), frames.to(DEV), rule, channel, threshold, color,
                                  alpha, paint)
    ref = mask_ref(logits, rule, channel, threshold)
    assert torch.equal(mask, ref)
    assert torch.equal(counts, counts_ref(ref, target))
    assert torch.equal(pic, overlay_ref(frames, ref, color, alpha, paint))


@pytest.mark.parametrize("B,H,W", [(16, 512, 512), (3, 419, 421)])
def test_more_pixels_than_one_grid_pass(B, H, W):
    """Above the 2048-block grid cap, so lanes stride over their image: 16 x 512 x 512 on the quad
    path (65,536 quads per image against 128 blocks of 256 lanes) and 3 x 419 x 421 on the scalar
    path (176,399 pixels against 682 blocks).  The counts equal a torch.bincount count of the same
    predictions."""
    from stfunet import overlay, predict_masks
    g = torch.Generator().manual_seed(77)
    K = 2
    logits = away_from_ties(torch.randn(B, K, H, W, generator=g), margin=1e-3).to(DEV)
    target = (torch.rand(B, H, W, generator=g) < 0.3).long().to(DEV)
    frames = torch.randn(B, H, W, generator=g).to(DEV)
    mask, counts = predict_masks(logits, target=target)
    pred = logits.argmax(1)
    assert torch.equal(mask, pred.to(torch.uint8))
    for b in range(B):
        n = torch.bincount((2 * (pred[b] > 0) + (target[b] > 0)).flatten(), minlength=4)
        assert counts[b].tolist() == [n[3].item(), (n[2] + n[3]).item(), (n[1] + n[3]).item()]
    pic = overlay(frames, mask, (0, 255, 0), 0.5, 0)
    assert torch.equal(pic.cpu(), overlay_ref(frames, mask, (0, 255, 0), 0.5, 0))


def test_strided_frame_view_is_read_in_place():
    from stfunet import overlay
    from stfunet.predict import shown_frame
    g = torch.Generator().manual_seed(5)
    x = torch.randn(3, 4, 2, 17, 19, generator=g).to(DEV)
    logits = away_from_ties(torch.randn(3, 2, 17, 19, generator=g), margin=1e-3)
    target = torch.randint(0, 2, (3, 17, 19), generator=g)
    view = shown_frame(x)
    assert view.data_ptr() == x.data_ptr() and view.stride() == (4 * 2 * 17 * 19, 19, 1)
    mask, _, pic = run_twice(logits.to(DEV), target.to(DEV), view, "argmax", 0, 0.5, (0, 255, 0), 0.5, 1)
    _, _, pic_copy = run_twice(logits.to(DEV), target.to(DEV), view.contiguous(), "argmax", 0, 0.5, (0, 255, 0), 0.5, 1)
    assert torch.equal(pic, pic_copy)
    assert torch.equal(pic, overlay_ref(view, mask, (0, 255, 0), 0.5, 1))
    assert torch.equal(overlay(view, mask.to(DEV)).cpu(), pic)
    x4 = x[:, :, 0]                                  # a 4-D model input: the shown frame is inputs[:, 0]
    assert shown_frame(x4).data_ptr() == x.data_ptr() and torch.equal(shown_frame(x4), view)
    # an aligned strided view takes the quad path: [2, 3, 1, 8, 12], batch stride 288
    y = torch.randn(2, 3, 1, 8, 12, generator=g).to(DEV)
    m = (torch.rand(2, 8, 12, generator=g) < 0.5).to(torch.uint8)
    assert torch.equal(overlay(shown_frame(y), m.to(DEV), (9, 8, 7), 0.25, 0).cpu(),
                       overlay_ref(shown_frame(y), m, (9, 8, 7), 0.25, 0))


def test_ignore_drops_exactly_the_padded_pixels():
    from stfunet import predict_masks
    g = torch.Generator().manual_seed(9)
    B, H, W = 3, 15, 17
    logits = away_from_ties(torch.randn(B, 2, H, W, generator=g), margin=1e-3)
    target = torch.randint(0, 2, (B, H, W), generator=g)
    target[0, :, 11:] = 255
    target[1, 9:, :] = 255
    target[2] = 255
    mask, plain = predict_masks(logits.to(DEV), target=target.to(DEV))
    mask2, dropped = predict_masks(logits.to(DEV), target=target.to(DEV), ignore_index=255)
    ref = mask_ref(logits)
    assert torch.equal(mask.cpu(), ref) and torch.equal(mask2, mask)       # the mask never depends on the target
    assert torch.equal(plain.cpu(), counts_ref(ref, target))
    assert torch.equal(dropped.cpu(), counts_ref(ref, target, ignore=255))
    pad = target == 255
    on_pad = counts_ref(ref * pad, target * pad)                            # a 255 pad counts as foreground
    assert torch.equal(plain.cpu() - dropped.cpu(), on_pad)
    assert dropped[2].tolist() == [0, 0, 0]


def _unet_and_loader():
    from oracle.cases import dce_case
    from oracle.init import canonical_state_dict
    from stfunet.unet import UNet
    model = UNet(in_channels=8, num_classes=2, base_c=8)
    model.load_state_dict(canonical_state_dict(model.state_dict(), seed=0))
    loader = [dce_case(300 + i, 2, 8, 32, 32) for i in range(3)]
    return model.to(DEV), loader


def test_predict_end_to_end_unet(tmp_path):
    from PIL import Image
    from stfunet import engine, overlay
    from stfunet.predict import predict, shown_frame
    model, loader = _unet_and_loader()
    model.train()
    res = predict(model, loader, torch.device(DEV), output_dir=str(tmp_path / "pics"), prefix="unet",
                  keep_masks=True)
    assert not model.training
    assert all(p.grad is None for p in model.parameters())
    assert res["num"] == 6 and res["dice"].shape == (6,) and res["dice"].dtype == torch.float64
    idx, total = 0, torch.zeros(3, dtype=torch.int64)
    with torch.no_grad():
        for (x5, t), mask in zip(loader, res["masks"]):
            x = engine.preprocess_input(x5, model).to(DEV)
            assert torch.equal(mask, model(x)["out"].argmax(1).to(torch.uint8))
            total += counts_ref(mask, t).sum(0)
            pics = overlay(shown_frame(x), mask).cpu().numpy()
            for pic in pics:
                with Image.open(os.path.join(str(tmp_path / "pics"), f"unet_{idx}.png")) as im:
                    assert im.mode == "RGB" and np.array_equal(np.asarray(im), pic)
                idx += 1
    assert idx == 6 and len(os.listdir(str(tmp_path / "pics"))) == 6
    dice, iou = metrics_ref(torch.cat([counts_ref(m, t) for (_, t), m in zip(loader, res["masks"])]))
    assert np.allclose(res["dice"].cpu().numpy(), dice.numpy(), rtol=1e-12, atol=0)
    assert np.allclose(res["iou"].cpu().numpy(), iou.numpy(), rtol=1e-12, atol=0)
    assert abs(res["mean_dice"].item() - dice.mean().item()) < 1e-12
    mat = engine.evaluate(model, loader, torch.device(DEV), num_classes=2)["confusion_matrix"].mat.cpu()
    assert total.tolist() == [mat[1, 1].item(), mat[:, 1].sum().item(), mat[1, :].sum().item()]


def test_predict_sigmoid_recipe_and_loader_without_targets(tmp_path):
    """rule="sigmoid", channel=0, paint=0 is test.py's recipe; a loader of bare inputs gives no scores."""
    from PIL import Image
    from stfunet import engine
    from stfunet.predict import predict
    model, loader = _unet_and_loader()
    bare = [x for x, _ in loader[:1]]
    res = predict(model, bare, torch.device(DEV), rule="sigmoid", channel=0, paint=0,
                  output_dir=str(tmp_path), prefix="s", keep_masks=True)
    assert res["num"] == 2 and res["dice"] is None and res["mean_iou"] is None
    with torch.no_grad():
        x = engine.preprocess_input(bare[0], model).to(DEV)
        logits = model(x)["out"].cpu()
    ch0 = logits[:, 0]
    sure = (ch0.abs() >= 1e-3)                  # sigmoid(x) > 0.5 <=> x > 0; ulps of expf matter only at 0
    mask = res["masks"][0].cpu()
    assert torch.equal(mask[sure], (ch0 > 0).to(torch.uint8)[sure])
    ref = overlay_ref(x[:, 0], mask, (0, 255, 0), 0.5, 0).numpy()
    for j in range(2):
        with Image.open(os.path.join(str(tmp_path), f"s_{j}.png")) as im:
            assert np.array_equal(np.asarray(im), ref[j])


def test_predict_stf_five_dimensional_input(tmp_path):
    """STFLSTMUNet takes [B, T, C, H, W] and, like the reference's, returns logits at H/2 x W/2
    (SURVEY.md section 0): masks and per-image scores against half-resolution targets work, the
    shown frame is the view inputs[:, 0, 0], and painting a half-size mask over it is refused (the
    reference's merge_images fails on the same mismatch)."""
    from conftest import GOLDEN
    from oracle.init import canonical_state_dict
    from stfunet import STFLSTMUNet
    from stfunet.predict import predict, shown_frame
    g = np.load(os.path.join(GOLDEN, "stf_t4.npz"))
    x, t = torch.from_numpy(g["x"]), torch.from_numpy(g["target"])
    model = STFLSTMUNet(time_steps=4)
    model.load_state_dict(canonical_state_dict(model.state_dict(), seed=0))
    model = model.to(DEV)
    res = predict(model, [(x, t)], torch.device(DEV), keep_masks=True)
    with torch.no_grad():
        ref = model(x.to(DEV))["out"].argmax(1).to(torch.uint8)
    assert res["num"] == 2 and tuple(res["masks"][0].shape) == (2, 32, 32)
    assert torch.equal(res["masks"][0], ref)
    dice, iou = metrics_ref(counts_ref(ref, t))
    assert np.allclose(res["dice"].cpu().numpy(), dice.numpy(), rtol=1e-12, atol=0)
    assert np.allclose(res["iou"].cpu().numpy(), iou.numpy(), rtol=1e-12, atol=0)
    xd = x.to(DEV)
    assert shown_frame(xd).data_ptr() == xd.data_ptr() and tuple(shown_frame(xd).shape) == (2, 64, 64)
    with pytest.raises(ValueError, match="does not match"):
        predict(model, [(x, t)], torch.device(DEV), output_dir=str(tmp_path))
