"""``STFLSTMUNet(..., output_size="input")``: full-resolution logits as the program's last op.

A ``full`` model must be the ``half`` model (the reference's H/2 x W/2 output, same state_dict)
followed by ``stfunet.upsample_logits``, bit for bit: outputs in train and eval mode, parameter
gradients, BatchNorm running statistics, the input gradient, under bf16 and fp16 storage, replayed
from a recorded plan or run eagerly.  With the output at the target's size the engine works on
full-resolution masks unchanged: ``criterion`` (against the tests' float64 restatement on torch's CPU
``F.interpolate`` of the half model's logits, tolerance of test_criterion_options_gpu.py),
``evaluate``, ``predict(output_dir=...)`` and ``train_one_epoch``.
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _criterion_ref import ref_loss_and_grad

pytestmark = pytest.mark.gpu

DEV = "cuda"
LOSS_TOL = 1e-5          # test_criterion_options_gpu.py's bound for its loss-value comparison
B = 2
#        name: (T, PK maps, classes, H, W)
CASES = {"64": (3, 0, 2, 64, 64),
         "66x70": (3, 0, 2, 66, 70),       # not divisible by 32: the size fallback, logits 34 x 36
         "pk": (2, 3, 2, 64, 64),
         "k7": (3, 0, 7, 64, 64)}          # the many-class head


def pair(name, seed=0):
    """(half, full) with the same state_dict, in train mode on the device."""
    from stfunet import STFLSTMUNet
    T, P, K, _, _ = CASES[name]
    torch.manual_seed(seed)
    half = STFLSTMUNet(1, K, time_steps=T, use_pk_maps=P > 0)
    full = STFLSTMUNet(1, K, time_steps=T, use_pk_maps=P > 0, output_size="input")
    full.load_state_dict(half.state_dict())
    return half.to(DEV).train(), full.to(DEV).train()


def batch(name, seed=0):
    """Frames [B, T + P, 1, H, W] and a full-resolution int64 mask [B, H, W] (classes 0..K-1)."""
    from stfunet.synthetic import dce_batch
    T, P, K, H, W = CASES[name]
    x, t = dce_batch(B, T, H, W, seed=900 + seed, device=DEV, pk_channels=P)
    if K > 2:
        g = torch.Generator(device=DEV).manual_seed(seed)
        t = t * torch.randint(1, K, t.shape, generator=g, device=DEV)
    assert t.dtype == torch.int64 and t.shape[-2:] == x.shape[-2:]
    return x, t


def grads(model):
    return {k: p.grad.detach().clone() for k, p in model.named_parameters()}


def assert_same_dict(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("name", list(CASES))
def test_output_is_the_resized_half_output(name):
    from stfunet import upsample_logits
    half, full = pair(name)
    x, _ = batch(name)
    H, W = x.shape[-2:]
    for mode in ("train", "eval"):
        getattr(half, mode)()
        getattr(full, mode)()
        with torch.no_grad():
            lo = half(x)["out"]
            out = full(x)["out"]
            assert out.shape == (B, CASES[name][2], H, W) and out.shape[-2:] == x.shape[-2:]
            assert lo.shape[-2:] != out.shape[-2:]
            assert torch.equal(out, upsample_logits(lo, (H, W))), mode
    # with autograd recording too (the plan runtime's first, eager step)
    half.train(), full.train()
    assert torch.equal(full(x)["out"], upsample_logits(half(x)["out"], (H, W)))


@pytest.mark.parametrize("fp16", [False, True], ids=["bf16", "fp16"])
@pytest.mark.parametrize("name", list(CASES))
def test_gradients_and_running_stats_match_half_model(name, fp16):
    from stfunet import upsample_logits
    half, full = pair(name)
    x, _ = batch(name)
    H, W = x.shape[-2:]
    g = torch.randn(B, CASES[name][2], H, W, generator=torch.Generator(device=DEV).manual_seed(3), device=DEV)
    with torch.autocast("cuda", dtype=torch.float16, enabled=fp16):
        out = full(x)["out"]
        ref = upsample_logits(half(x)["out"], (H, W))
    assert out.dtype == torch.float32 and torch.equal(out, ref)
    out.backward(g)
    ref.backward(g)                 # = half(x)["out"].backward(resize backward of g)
    torch.cuda.synchronize()
    ga, gb = grads(full), grads(half)
    assert all(torch.isfinite(v).all() for v in ga.values())
    assert any(v.abs().max() > 0 for v in ga.values())
    assert_same_dict(ga, gb)
    assert_same_dict(dict(full.named_buffers()), dict(half.named_buffers()))


@pytest.mark.parametrize("name", list(CASES))
def test_loss_on_full_resolution_masks(name):
    from stfunet import engine
    half, full = pair(name)
    x, target = batch(name)
    K = CASES[name][2]
    assert target.shape[-2:] == x.shape[-2:]
    loss = engine.criterion(full(x), target, num_classes=K)
    with torch.no_grad():
        lo = half(x)["out"].float().cpu()
    up = F.interpolate(lo, size=tuple(x.shape[-2:]), mode="bilinear", align_corners=False)
    ref, _ = ref_loss_and_grad(up, target.cpu())
    print(f"{name}: loss {loss.item():.7f}  reference {ref:.7f}  |d| {abs(loss.item() - ref):.3e}")
    assert abs(loss.item() - ref) < LOSS_TOL
    loss.backward()
    torch.cuda.synchronize()
    for k, p in full.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), k


def _three_steps(name, plan_on):
    from stfunet import engine
    from stfunet.optim import AdamW
    os.environ["STF_PLAN"] = "1" if plan_on else "0"
    try:
        _, full = pair(name)
        opt = AdamW(full.parameters(), lr=1e-3, weight_decay=1e-4)
        batches = [batch(name, seed=i) for i in range(2)]
        logits = []
        for i in range(3):
            x, t = batches[i % 2]
            out = full(x)
            logits.append(out["out"].detach().clone())
            loss = engine.criterion(out, t, num_classes=CASES[name][2])
            opt.zero_grad()
            loss.backward()
            opt.step()
        torch.cuda.synchronize()
        rt = full.program.runtime
        return (logits, {k: v.detach().clone() for k, v in full.state_dict().items()},
                rt.fwd is not None and rt.bwd is not None)
    finally:
        os.environ.pop("STF_PLAN", None)


@pytest.mark.parametrize("name", ["64", "66x70"])
def test_plan_replay_bitwise_vs_eager(name):
    """Warm-up step, recorded step, replayed step: the resize pair is in the plan, the static logits
    and the static incoming gradient are the full-size ones."""
    le, se, pe = _three_steps(name, False)
    lp, sp, pp = _three_steps(name, True)
    assert pp and not pe
    H, W = CASES[name][3:]
    for a, b in zip(le, lp):
        assert a.shape[-2:] == (H, W) and torch.equal(a, b)
    assert_same_dict(se, sp)


@pytest.mark.parametrize("name", ["64", "pk"])
def test_input_gradient(name):
    from stfunet import upsample_logits
    half, full = pair(name)
    x, _ = batch(name)
    H, W = x.shape[-2:]
    g = torch.randn(B, CASES[name][2], H, W, generator=torch.Generator(device=DEV).manual_seed(4), device=DEV)
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    full(xa)["out"].backward(g)
    upsample_logits(half(xb)["out"], (H, W)).backward(g)
    torch.cuda.synchronize()
    assert xa.grad is not None and xa.grad.shape == x.shape and torch.isfinite(xa.grad).all()
    assert xa.grad.abs().max() > 0
    assert torch.equal(xa.grad, xb.grad)
    assert_same_dict(grads(full), grads(half))


def _loader(name):
    return [tuple(v.cpu() for v in batch(name, seed=10 + i)) for i in range(2)]


def test_evaluate_on_full_resolution_masks():
    from stfunet import engine, upsample_logits
    half, full = pair("66x70")
    loader = _loader("66x70")
    res = engine.evaluate(full, loader, torch.device(DEV), num_classes=2)
    half.eval()
    confmat = engine.ConfusionMatrix(2)
    dice = engine.DiceCoefficient(num_classes=2, ignore_index=255)
    with torch.no_grad():
        for x, t in loader:
            out = upsample_logits(half(x.to(DEV))["out"], tuple(t.shape[-2:]))
            engine.eval_update(out, t.to(DEV), confmat, dice)
    assert res["dice"] == dice.value.item()
    assert torch.equal(res["confusion_matrix"].mat.cpu(), confmat.mat.cpu())
    assert int(confmat.mat.sum()) == 2 * B * 66 * 70


def test_predict_writes_full_size_overlays(tmp_path):
    from PIL import Image
    from stfunet import overlay
    from stfunet.predict import predict, shown_frame
    half, full = pair("66x70")
    loader = _loader("66x70")
    out_dir = str(tmp_path / "pics")
    res = predict(full, loader, torch.device(DEV), output_dir=out_dir, prefix="stf")
    assert res["num"] == 2 * B and sorted(os.listdir(out_dir)) == [f"stf_{i}.png" for i in range(2 * B)]
    idx = 0
    with torch.no_grad():
        for x, _ in loader:
            x = x.to(DEV)
            mask = full(x)["out"].argmax(1).to(torch.uint8)
            assert tuple(mask.shape) == (B, 66, 70)
            for pic in overlay(shown_frame(x), mask).cpu().numpy():
                with Image.open(os.path.join(out_dir, f"stf_{idx}.png")) as im:
                    assert im.size == (70, 66) and np.array_equal(np.asarray(im), pic)
                idx += 1
    with pytest.raises(ValueError, match="does not match"):         # the half-size mask is still refused
        predict(half, [x for x, _ in loader], torch.device(DEV), output_dir=str(tmp_path / "half"))


def test_train_one_epoch_on_full_resolution_masks():
    import math
    from stfunet import engine
    from stfunet.optim import AdamW
    _, full = pair("64")
    loader = _loader("64")
    opt = AdamW(full.parameters(), lr=1e-3, weight_decay=1e-4)
    sched = engine.create_lr_scheduler(opt, len(loader), 1)
    mean_loss, lr = engine.train_one_epoch(full, opt, loader, torch.device(DEV), 0, 2, lr_scheduler=sched)
    assert math.isfinite(mean_loss) and mean_loss > 0
