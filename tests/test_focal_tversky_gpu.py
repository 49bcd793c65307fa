"""Focal cross-entropy and Tversky overlap on the gfx950 kernels (stf_loss_ft_fwd / stf_loss_ft_bwd).

Shapes chosen for the kernels' seams, through ``stfunet.criterion``, against the tests' float64
restatement (``_focal_ref``) on the same logits; exact zeros at ignored pixels; the C entry points with
NaN-prefilled gradients; saturated logits (1-q exactly 0); agreement with the option and many-class
kernels at gamma = 0, alpha = beta = 1/2; ``grad_out`` scaling and a GradScaler step; run-to-run
determinism; the default routes unchanged bit for bit; ``engine.train_one_epoch`` end to end.
Tolerances are the project's for the loss kernels: |dloss| < 1e-5, gradient rel-L2 < 1e-4.
"""
import pytest
import torch

from _criterion_ref import rel_l2
from _focal_ref import ref_loss_and_grad
from test_criterion_options_gpu import _seam_case

pytestmark = pytest.mark.gpu

DEV = "cuda"
LOSS_TOL, GRAD_TOL = 1e-5, 1e-4


def run(logits, target, weight=None, ignore_index=-100, dice=True, gamma=0.0, tversky=None, grad_out=None):
    """loss (device scalar) and d/d(logits) through stfunet.criterion."""
    from stfunet import criterion
    x = logits.to(DEV).clone().requires_grad_(True)
    loss = criterion({"out": x}, target.to(DEV), loss_weight=weight, num_classes=logits.shape[1], dice=dice,
                     ignore_index=ignore_index, focal_gamma=gamma, tversky=tversky)
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


SEAMS = [(2, 2, 136, 136),      # 18,496 pixels > LCHUNK * 256: a second, ragged grid-stride trip
         (65, 2, 4, 4),         # the finalize's second block of 64 images
         (1, 4, 16, 16),        # the largest K at KP 4
         (2, 1, 8, 8),          # K = 1
         (3, 7, 24, 16),        # KP 8
         (2, 5, 8, 8),          # the smallest many-class K
         (2, 16, 8, 8)]         # KP 16
OPTIONS = [(2.0, 0.5, 0.5), (0.0, 0.3, 0.7), (0.5, 0.7, 0.3), (2.0, 0.3, 0.7)]


@pytest.mark.parametrize("gamma,alpha,beta", OPTIONS)
@pytest.mark.parametrize("N,K,H,W", SEAMS)
def test_kernel_seams_against_restatement(N, K, H, W, gamma, alpha, beta):
    logits, target, _, weight = _seam_case(N, K, H, W)
    ref_loss, ref_grad = ref_loss_and_grad(logits, target, weight, 255, True, gamma, alpha, beta)
    loss, grad = run(logits, target, weight, 255, True, gamma, (alpha, beta))
    check(f"N{N} K{K} {H}x{W} gamma {gamma} tversky ({alpha}, {beta})", loss, grad, ref_loss, ref_grad)
    assert (grad.cpu().permute(0, 2, 3, 1)[target == 255] == 0).all()


@pytest.mark.parametrize("N,K,H,W", SEAMS)
def test_kernel_seams_without_weights_and_ignore(N, K, H, W):
    logits, _, clean, _ = _seam_case(N, K, H, W)
    ref_loss, ref_grad = ref_loss_and_grad(logits, clean, None, -100, True, 2.0, 0.3, 0.7)
    loss, grad = run(logits, clean, None, -100, True, 2.0, (0.3, 0.7))
    check(f"N{N} K{K} {H}x{W} plain", loss, grad, ref_loss, ref_grad)


def test_focal_without_dice():
    logits, target, _, weight = _seam_case(3, 7, 24, 16)
    ref_loss, ref_grad = ref_loss_and_grad(logits, target, weight, 255, False, 2.0)
    loss, grad = run(logits, target, weight, 255, False, 2.0)
    check("no dice", loss, grad, ref_loss, ref_grad)


def _direct(sym, logits, target, weight, ign, dice, extra, fill):
    """The C entry points ``stf_loss_<sym>_*`` themselves, dlogits pre-filled with ``fill``; ``extra``:
    the arguments after ``dice``."""
    from stfunet import _lib
    from stfunet._lib import call, stream
    from stfunet.nhwc import _p
    x, t = logits.to(DEV).contiguous(), target.to(DEV).contiguous()
    N, K, H, W = x.shape
    w = torch.tensor(weight, dtype=torch.float32, device=DEV) if weight is not None else None
    terms = torch.empty(getattr(_lib.load(), f"stf_loss_{sym}_scratch_floats")(N, K), device=DEV)
    loss = torch.empty(1, device=DEV)
    wp = _p(w) if w is not None else None
    call(f"stf_loss_{sym}_fwd", _p(x), _p(t), N, H, W, K, wp, ign, int(dice), *extra, _p(terms), _p(loss), stream())
    dl = torch.full_like(x, fill)
    go = torch.ones(1, device=DEV)
    call(f"stf_loss_{sym}_bwd", _p(x), _p(t), N, H, W, K, wp, ign, int(dice), *extra, _p(terms), _p(go), _p(dl),
         stream())
    torch.cuda.synchronize()
    return loss[0], dl, terms[:N * K * 3].reshape(N, K, 3).clone()


@pytest.mark.parametrize("K", [2, 7])
def test_ignored_pixels_get_a_stored_zero(K):
    logits, target, _, weight = _seam_case(3, K, 16, 24)
    assert (target[1] == 255).all()                       # the fully ignored image
    ft = (2.0, 0.3, 0.7)
    loss, dl, terms = _direct("ft", logits, target, weight, 255, True, ft, float("nan"))
    ref_loss, ref_grad = ref_loss_and_grad(logits, target, weight, 255, True, *ft)
    assert not torch.isnan(dl).any()
    assert (dl.cpu().permute(0, 2, 3, 1)[target == 255] == 0).all()
    assert (dl[1] == 0).all() and (terms[1] == 0).all()    # no sums for that image: D = 1, no gradient
    check("nan-prefilled", loss, dl, ref_loss, ref_grad)
    # the ignored image's D = 1 is in the mean: without that image, the overlap mean is over 2 images
    keep = torch.tensor([0, 2])
    two, _ = ref_loss_and_grad(logits[keep], target[keep], weight, 255, True, *ft)
    ce, _ = ref_loss_and_grad(logits, target, weight, 255, False, ft[0])
    d3, d2 = ref_loss - ce, two - ce
    assert abs((1 - d3) - ((1 - d2) * 2 + 1) / 3) < 1e-9           # the restatement's own bookkeeping
    # NaN logits under ignored pixels do not reach the sums
    bad = logits.clone()
    bad.permute(0, 2, 3, 1)[target == 255] = float("nan")
    loss_b, dl_b, _ = _direct("ft", bad, target, weight, 255, True, ft, float("nan"))
    assert torch.equal(loss_b, loss) and torch.equal(dl_b, dl)


def test_all_ignored_batch_is_nan():
    logits = torch.randn(2, 2, 8, 8)
    target = torch.full((2, 8, 8), 255)
    loss, dl, _ = _direct("ft", logits, target, [1.0, 2.0], 255, True, (2.0, 0.3, 0.7), float("nan"))
    assert torch.isnan(loss).item()
    assert (dl == 0).all()
    loss2, grad2 = run(logits, target, None, 255, False, 0.5)
    assert torch.isnan(loss2).item() and (grad2 == 0).all()


@pytest.mark.parametrize("gamma", [0.5, 2.0])
def test_saturated_logits(gamma):
    """K = 2 logits of +-60: the other class's exponential underflows in fp32 and 1-q is exactly 0 where
    the pixel is confidently right; the other half is confidently wrong (1-q = 1, nll = 120)."""
    z = torch.tensor([60.0, -60.0]).reshape(1, 2, 1, 1).expand(2, 2, 8, 8).contiguous()
    target = torch.zeros(2, 8, 8, dtype=torch.long)
    target[:, 4:] = 1
    for tv in ((0.5, 0.5), (0.3, 0.7)):
        ref_loss, ref_grad = ref_loss_and_grad(z, target, None, -100, True, gamma, *tv)
        loss, grad = run(z, target, None, -100, True, gamma, tv)
        assert torch.isfinite(loss).item() and torch.isfinite(grad).all()
        assert ref_loss > 50 and ref_grad.abs().max().item() > 1e-3
        check(f"saturated gamma {gamma} tversky {tv}", loss, grad, ref_loss, ref_grad)


@pytest.mark.parametrize("sym,K", [("opt", 2), ("mc", 7)])
def test_neutral_values_agree_with_the_existing_kernels(sym, K):
    logits, target, _, weight = _seam_case(3, K, 24, 16)
    for dice in (True, False):
        l0, g0, t0 = _direct(sym, logits, target, weight, 255, dice, (), float("nan"))
        l1, g1, t1 = _direct("ft", logits, target, weight, 255, dice, (0.0, 0.5, 0.5), float("nan"))
        print(f"{sym} K{K} dice {dice}: |dloss| {abs(l0.item() - l1.item()):.3e}, grad rel-L2 {rel_l2(g1, g0):.3e}")
        assert abs(l0.item() - l1.item()) < LOSS_TOL and rel_l2(g1, g0) < GRAD_TOL
        assert rel_l2(t1, t0) < 1e-6                       # the same (I, sum p, sum t) layout


def test_grad_out_scales_the_gradient():
    logits, target, _, weight = _seam_case(2, 3, 16, 16)
    kw = dict(gamma=2.0, tversky=(0.3, 0.7))
    l1, g1 = run(logits, target, weight, 255, True, **kw)
    l2, g2 = run(logits, target, weight, 255, True, grad_out=2.0, **kw)
    assert torch.equal(l1, l2)
    assert torch.equal(g2, 2 * g1)            # a factor of two is exact in binary floating point
    assert g1.abs().max().item() > 0
    _, g3 = run(logits, target, weight, 255, True, grad_out=0.37, **kw)
    _, ref = ref_loss_and_grad(logits, target, weight, 255, True, 2.0, 0.3, 0.7, grad_out=0.37)
    assert rel_l2(g3, ref) < GRAD_TOL
    assert rel_l2(g3, 0.37 * g1.double()) < 1e-6           # one more fp32 rounding per element (2^-24)


@pytest.mark.parametrize("N,K,H,W", [(2, 2, 136, 136), (3, 7, 24, 16)])
def test_two_runs_are_bit_identical(N, K, H, W):
    logits, target, _, weight = _seam_case(N, K, H, W)
    l1, g1 = run(logits, target, weight, 255, True, 2.0, (0.3, 0.7))
    l2, g2 = run(logits, target, weight, 255, True, 2.0, (0.3, 0.7))
    assert torch.equal(l1, l2) and torch.equal(g1, g2)
    assert torch.isfinite(l1).item() and g1.abs().max().item() > 0


def _recorded_names(monkeypatch):
    from stfunet import loss
    names, real = [], loss.call
    monkeypatch.setattr(loss, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    return names


def test_default_path_unchanged(monkeypatch):
    """One case per existing route: the defaults and explicit ``focal_gamma=0.0, tversky=None`` launch
    the same entry points and give the same bits."""
    from stfunet import criterion
    names = _recorded_names(monkeypatch)
    routes = [((2, 2, 136, 136), dict(), "stf_loss_fwd"),
              ((2, 3, 16, 16), dict(loss_weight="w", ignore_index=255), "stf_loss_opt_fwd"),
              ((3, 7, 24, 16), dict(loss_weight="w", ignore_index=255), "stf_loss_mc_fwd")]
    for (N, K, H, W), kw, fwd in routes:
        logits, target, clean, weight = _seam_case(N, K, H, W)
        t = (target if kw else clean).to(DEV)
        kw = {k: (weight if v == "w" else v) for k, v in kw.items()}
        got = []
        for extra in (dict(), dict(focal_gamma=0.0, tversky=None)):
            del names[:]
            x = logits.to(DEV).clone().requires_grad_(True)
            loss = criterion({"out": x}, t, num_classes=K, **kw, **extra)
            loss.backward()
            assert names == [fwd, fwd.replace("_fwd", "_bwd")]
            got.append((loss.detach(), x.grad))
        assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1])
        assert torch.isfinite(got[0][0]).item()
        del names[:]
        criterion({"out": logits.to(DEV)}, t, num_classes=K, focal_gamma=1.0, **kw)
        assert names == ["stf_loss_ft_fwd"]


def test_aux_head_sum_applies_the_values_to_both_heads():
    from stfunet import criterion
    logits, target, _, weight = _seam_case(2, 2, 16, 16)
    x, t = logits.to(DEV), target.to(DEV)
    kw = dict(loss_weight=weight, num_classes=2, ignore_index=255, focal_gamma=2.0, tversky=(0.3, 0.7))
    out = criterion({"out": x}, t, **kw)
    aux = criterion({"out": x * 0.5}, t, **kw)
    both = criterion({"out": x, "aux": x * 0.5}, t, **kw)
    assert torch.equal(both, out + 0.5 * aux)
    ref_out, _ = ref_loss_and_grad(logits, target, weight, 255, True, 2.0, 0.3, 0.7)
    ref_aux, _ = ref_loss_and_grad(logits * 0.5, target, weight, 255, True, 2.0, 0.3, 0.7)
    assert abs(both.item() - (ref_out + 0.5 * ref_aux)) < 1.5 * LOSS_TOL      # LOSS_TOL per head, aux at 0.5


def _train(monkeypatch, steps, scaler):
    from stfunet import UNet, engine
    from stfunet.optim import AdamW
    torch.manual_seed(0)
    model = UNet(8, 2, 8).to(DEV)
    g = torch.Generator().manual_seed(3)
    batches = []
    for _ in range(steps):
        target = (torch.rand(2, 32, 32, generator=g) > 0.8).long()
        target[0, :, 28:] = 255
        batches.append((torch.rand(2, 8, 1, 32, 32, generator=g), target))
    seen = []
    real = engine.criterion

    def recording(inputs, target, **kw):
        loss = real(inputs, target, **kw)
        seen.append((inputs["out"].detach().clone(), target.clone(), loss.detach().clone(), kw))
        return loss

    monkeypatch.setattr(engine, "criterion", recording)
    opt = AdamW(model.parameters(), lr=1e-3, weight_decay=1e-4)
    sched = engine.create_lr_scheduler(opt, steps, 2)
    mean, _ = engine.train_one_epoch(model, opt, batches, torch.device(DEV), 0, 2, lr_scheduler=sched, print_freq=10,
                                     scaler=scaler, focal_gamma=2, tversky=(0.3, 0.7), ignore_index=255,
                                     loss_weight=[1, 2])
    return mean, seen


def test_train_one_epoch_end_to_end(monkeypatch):
    mean, seen = _train(monkeypatch, 2, None)
    assert len(seen) == 2
    losses = []
    for i, (logits, target, loss, kw) in enumerate(seen):
        assert kw["focal_gamma"] == 2 and kw["tversky"] == (0.3, 0.7)
        ref, _ = ref_loss_and_grad(logits, target, [1.0, 2.0], 255, True, 2.0, 0.3, 0.7)
        plain, _ = ref_loss_and_grad(logits, target, [1.0, 2.0], 255, True)
        print(f"step {i}: loss {loss.item():.6f} restatement {ref:.6f} (CE + Dice would be {plain:.6f})")
        assert torch.isfinite(loss).item() and abs(loss.item() - ref) < LOSS_TOL
        assert abs(ref - plain) > 1e-3                     # the two terms are in the logged number
        losses.append(loss.item())
    assert abs(mean - sum(losses) / 2) < 1e-6
    assert losses[0] != losses[1]


def test_gradscaler_step(monkeypatch):
    scaler = torch.amp.GradScaler("cuda")
    mean, seen = _train(monkeypatch, 1, scaler)
    logits, target, loss, _ = seen[0]
    ref, _ = ref_loss_and_grad(logits, target, [1.0, 2.0], 255, True, 2.0, 0.3, 0.7)
    print(f"fp16 + GradScaler: loss {loss.item():.6f} restatement {ref:.6f}")
    assert torch.isfinite(loss).item() and abs(loss.item() - ref) < LOSS_TOL and abs(mean - loss.item()) < 1e-6
    assert scaler.get_scale() == 65536.0                   # the scaled gradient was finite: no step skipped
