"""Criterion options on the gfx950 kernels (stf_loss_opt_fwd / stf_loss_opt_bwd).

Reference-generated fixture entries through ``stfunet.criterion``; shapes chosen for the
kernels' seams against the tests' float64 restatement on the same logits; exact zeros at
ignored pixels; the GradScaler path; run-to-run determinism; the default configuration
unchanged; and ``engine.train_one_epoch`` on a mixed-size batch padded with 255.
Tolerances are the project's for the loss kernels: |dloss| < 1e-5, gradient rel-L2 < 1e-4.
"""
import pytest
import torch

from _criterion_ref import fixture_entries, ref_loss_and_grad, rel_l2

pytestmark = pytest.mark.gpu

DEV = "cuda"
ENTRIES = fixture_entries()
LOSS_TOL, GRAD_TOL = 1e-5, 1e-4


def run(logits, target, weight=None, ignore_index=-100, dice=True, grad_out=None):
    """loss (device scalar) and d/d(logits) through stfunet.criterion."""
    from stfunet import criterion
    x = logits.to(DEV).clone().requires_grad_(True)
    loss = criterion({"out": x}, target.to(DEV), loss_weight=weight, num_classes=logits.shape[1], dice=dice,
                     ignore_index=ignore_index)
    if grad_out is None:
        loss.backward()
    else:
        loss.backward(torch.tensor(float(grad_out), device=DEV))
    return loss.detach(), x.grad


def check(tag, loss, grad, ref_loss, ref_grad):
    dl = abs(loss.item() - ref_loss)
    if ref_grad.norm().item() < 1e-12:      # K = 1: softmax is constant, the true gradient is 0
        dg = grad.abs().max().item()
        print(f"{tag}: |dloss| {dl:.3e}, reference gradient is zero, max |grad| {dg:.3e}")
        assert dg < 1e-12
    else:
        dg = rel_l2(grad, ref_grad)
        print(f"{tag}: |dloss| {dl:.3e}, grad rel-L2 {dg:.3e}")
        assert dg < GRAD_TOL
    assert dl < LOSS_TOL


@pytest.mark.parametrize("e", ENTRIES, ids=[e["name"] for e in ENTRIES])
def test_fixture_entries_through_criterion(e):
    loss, grad = run(e["logits"], e["target"], e["weight"], e["ignore_index"], e["dice"])
    check(e["name"], loss, grad, e["loss"], e["grad"])
    if e["ignore_index"] >= 0:
        assert (grad.cpu().permute(0, 2, 3, 1)[e["target"] == e["ignore_index"]] == 0).all()


def _seam_case(N, K, H, W):
    """logits, a target with ignored column / row bands, scattered ignored pixels and one fully
    ignored image when N > 1, the same target without any 255, and class weights."""
    g = torch.Generator().manual_seed(1000 * N + 10 * K + H)
    logits = torch.randn(N, K, H, W, generator=g) * 3.0
    clean = torch.randint(0, K, (N, H, W), generator=g)
    target = clean.clone()
    target[0, :, W - max(1, W // 4):] = 255
    target[-1, H - max(1, H // 4):, :] = 255
    target[torch.rand(N, H, W, generator=g) < 0.05] = 255
    if N > 1:
        target[N // 2] = 255
    weight = [0.5 + 0.75 * k for k in range(K)]
    return logits, target, clean, weight


SEAMS = [(2, 2, 136, 136),      # 18,496 pixels > LCHUNK * 256: a second, ragged grid-stride trip
         (65, 2, 4, 4),         # the finalize's second block of 64 images
         (1, 4, 16, 16),        # the largest K
         (2, 1, 8, 8)]          # the smallest K
CONFIGS = ["all_on", "no_weight", "no_ignore", "no_dice"]


@pytest.mark.parametrize("config", CONFIGS)
@pytest.mark.parametrize("N,K,H,W", SEAMS)
def test_kernel_seams_against_restatement(N, K, H, W, config):
    logits, target, clean, weight = _seam_case(N, K, H, W)
    ign, dice = 255, True
    if config == "no_weight":
        weight = None
    elif config == "no_ignore":
        target, ign = clean, -100
    elif config == "no_dice":
        dice = False
    ref_loss, ref_grad = ref_loss_and_grad(logits, target, weight, ign, dice)
    loss, grad = run(logits, target, weight, ign, dice)
    check(f"N{N} K{K} {H}x{W} {config}", loss, grad, ref_loss, ref_grad)
    if ign >= 0:
        assert (grad.cpu().permute(0, 2, 3, 1)[target == ign] == 0).all()


def _direct(logits, target, weight, ign, dice, fill):
    """The C entry points themselves, dlogits pre-filled with ``fill``."""
    from stfunet import _lib
    from stfunet._lib import call, stream
    from stfunet.nhwc import _p
    x, t = logits.to(DEV).contiguous(), target.to(DEV).contiguous()
    N, K, H, W = x.shape
    w = torch.tensor(weight, dtype=torch.float32, device=DEV) if weight is not None else None
    terms = torch.empty(_lib.load().stf_loss_opt_scratch_floats(N, K), device=DEV)
    loss = torch.empty(1, device=DEV)
    wp = _p(w) if w is not None else None
    call("stf_loss_opt_fwd", _p(x), _p(t), N, H, W, K, wp, ign, int(dice), _p(terms), _p(loss), stream())
    dl = torch.full_like(x, fill)
    go = torch.ones(1, device=DEV)
    call("stf_loss_opt_bwd", _p(x), _p(t), N, H, W, K, wp, ign, int(dice), _p(terms), _p(go), _p(dl), stream())
    torch.cuda.synchronize()
    return loss[0], dl


def test_ignored_pixels_get_a_stored_zero():
    logits, target, _, weight = _seam_case(3, 2, 16, 24)
    assert (target[1] == 255).all()                       # the fully ignored image
    loss, dl = _direct(logits, target, weight, 255, True, float("nan"))
    ref_loss, ref_grad = ref_loss_and_grad(logits, target, weight, 255, True)
    assert not torch.isnan(dl).any()
    assert (dl.cpu().permute(0, 2, 3, 1)[target == 255] == 0).all()
    assert (dl[1] == 0).all()                              # D = 1 for that image, no gradient
    check("nan-prefilled", loss, dl, ref_loss, ref_grad)
    # the ignored image's D = 1 is in the mean: without that image, the Dice mean is over 2 images
    keep = torch.tensor([0, 2])
    two, _ = ref_loss_and_grad(logits[keep], target[keep], weight, 255, True)
    ce, _ = ref_loss_and_grad(logits, target, weight, 255, False)
    dice3, dice2 = ref_loss - ce, two - ce
    assert abs((1 - dice3) - ((1 - dice2) * 2 + 1) / 3) < 1e-9     # the restatement's own bookkeeping
    # NaN logits under ignored pixels do not reach the sums
    bad = logits.clone()
    bad.permute(0, 2, 3, 1)[target == 255] = float("nan")
    loss_b, dl_b = _direct(bad, target, weight, 255, True, float("nan"))
    assert torch.equal(loss_b, loss) and torch.equal(dl_b, dl)


def test_all_ignored_batch_is_nan():
    logits = torch.randn(2, 2, 8, 8)
    target = torch.full((2, 8, 8), 255)
    loss, dl = _direct(logits, target, [1.0, 2.0], 255, True, float("nan"))
    assert torch.isnan(loss).item()
    assert (dl == 0).all()
    loss2, grad2 = run(logits, target, None, 255, False)
    assert torch.isnan(loss2).item() and (grad2 == 0).all()


def test_grad_out_two_doubles_the_gradient():
    logits, target, _, weight = _seam_case(2, 3, 16, 16)
    l1, g1 = run(logits, target, weight, 255, True)
    l2, g2 = run(logits, target, weight, 255, True, grad_out=2.0)
    assert torch.equal(l1, l2)
    assert torch.equal(g2, 2 * g1)            # a factor of two is exact in binary floating point
    assert g1.abs().max().item() > 0


def test_two_runs_are_bit_identical():
    logits, target, _, weight = _seam_case(2, 2, 136, 136)
    l1, g1 = run(logits, target, weight, 255, True)
    l2, g2 = run(logits, target, weight, 255, True)
    assert torch.equal(l1, l2) and torch.equal(g1, g2)


def test_defaults_unchanged():
    from stfunet import _lib
    from stfunet._lib import call, stream
    from stfunet.nhwc import _p
    logits, _, clean, _ = _seam_case(2, 2, 136, 136)
    loss, grad = run(logits, clean)
    x, t = logits.to(DEV), clean.to(DEV)
    N, K, H, W = x.shape
    terms = torch.empty(_lib.load().stf_loss_scratch_floats(N, K), device=DEV)
    dloss, dl, go = torch.empty(1, device=DEV), torch.empty_like(x), torch.ones(1, device=DEV)
    call("stf_loss_fwd", _p(x), _p(t), N, H, W, K, _p(terms), _p(dloss), stream())
    call("stf_loss_bwd", _p(x), _p(t), N, H, W, K, _p(terms), _p(go), _p(dl), stream())
    assert torch.equal(loss, dloss[0]) and torch.equal(grad, dl)
    # neutral options through the option kernels: same value up to fp32 rounding
    lo, go_ = run(logits, clean, [1.0, 1.0], 255, True)
    print("neutral options: |dloss|", abs(lo.item() - loss.item()), "grad rel-L2", rel_l2(go_, grad))
    assert abs(lo.item() - loss.item()) < 1e-6
    assert rel_l2(go_, grad) < GRAD_TOL


def test_aux_head_rule_applies_to_every_configuration():
    from stfunet import criterion
    logits, target, _, weight = _seam_case(2, 2, 16, 16)
    x, t = logits.to(DEV), target.to(DEV)
    kw = dict(loss_weight=weight, num_classes=2, dice=False, ignore_index=255)
    out = criterion({"out": x}, t, **kw)
    aux = criterion({"out": x * 0.5}, t, **kw)
    both = criterion({"out": x, "aux": x * 0.5}, t, **kw)
    assert torch.equal(both, out + 0.5 * aux)


def test_train_one_epoch_mixed_size_batch(monkeypatch):
    """Two samples of 32x32 and 32x48 collated with the dataset's cat_list (255 padding), three
    steps (the third a replayed plan step): every step's loss equals the restatement on that
    step's logits."""
    from stfunet import UNet, engine
    from stfunet.dataset import cat_list
    from stfunet.optim import AdamW
    torch.manual_seed(0)
    model = UNet(8, 2, 8).to(DEV)
    sizes = [(32, 32), (32, 48)]
    images = cat_list([torch.rand(8, 1, h, w) for h, w in sizes], fill_value=0)
    targets = cat_list([(torch.rand(h, w) > 0.7).long() for h, w in sizes], fill_value=255)
    assert images.shape == (2, 8, 1, 32, 48) and (targets[0, :, 32:] == 255).all()
    assert (targets[0, :, :32] != 255).all() and (targets[1] != 255).all()
    seen = []
    real = engine.criterion

    def recording(inputs, target, **kw):
        loss = real(inputs, target, **kw)
        seen.append((inputs["out"].detach().clone(), target.clone(), loss.detach().clone()))
        return loss

    monkeypatch.setattr(engine, "criterion", recording)
    opt = AdamW(model.parameters(), lr=1e-3, weight_decay=1e-4)
    sched = engine.create_lr_scheduler(opt, 3, 2)
    weight = [1.0, 2.0]
    mean, _ = engine.train_one_epoch(model, opt, [(images, targets)] * 3, torch.device(DEV), 0, 2,
                                     lr_scheduler=sched, print_freq=10, ignore_index=255, loss_weight=weight)
    assert len(seen) == 3
    assert model.program.runtime.bwd is not None          # the step was recorded and replayed
    losses = []
    for i, (logits, target, loss) in enumerate(seen):
        ref, _ = ref_loss_and_grad(logits, target, weight, 255, True)
        print(f"step {i}: loss {loss.item():.6f} restatement {ref:.6f}")
        assert torch.isfinite(loss).item() and abs(loss.item() - ref) < LOSS_TOL
        losses.append(loss.item())
    assert abs(mean - sum(losses) / 3) < 1e-6
    assert len(set(losses)) == 3                           # the optimizer moved the model
