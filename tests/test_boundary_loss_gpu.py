"""Boundary loss on the gfx950 kernels (stf_sdf, stf_bloss_fwd / stf_bloss_bwd).

The maps bit for bit against the scipy restatement (``_boundary_loss_ref.sdf_ref``) on shapes at the
kernels' seams; the term and its gradient against the float64 restatement at the loss tests' seams, with
and without ignored pixels; composition with the four criterion routes through ``boundary_criterion``; a zero weight
that launches nothing new; ``engine.train_one_epoch`` end to end.
Tolerances: |dloss| <= 1e-5 * max(1, sum of the absolute terms), gradient rel-L2 < 1e-4.
"""
import numpy as np
import pytest
import torch

from _boundary_loss_ref import (abs_loss, absent_and_full, blobs, boundary_loss_ref, checkerboard, empty_rows,
                                one_pixel, padded, sdf_ref)
from _criterion_ref import rel_l2
from test_criterion_options_gpu import _seam_case

pytestmark = pytest.mark.gpu

DEV = "cuda"
LOSS_TOL, GRAD_TOL = 1e-5, 1e-4

MAP_SHAPES = [(1, 2, 1, 1),
              (2, 2, 1, 65),        # a row that spans two ballot words
              (1, 2, 3, 64),
              (1, 2, 65, 1),        # a single column
              (2, 3, 17, 129),
              (1, 2, 2, 257),       # a second block of columns
              (65, 2, 4, 4),
              (1, 16, 8, 8)]
CONTENTS = {"blobs02": lambda N, K, H, W: blobs(N, K, H, W, 0.02, 11),
            "blobs50": lambda N, K, H, W: blobs(N, K, H, W, 0.5, 12),
            "blobs97": lambda N, K, H, W: blobs(N, K, H, W, 0.97, 13),
            "one_pixel": one_pixel,
            "checkerboard": checkerboard,
            "absent_and_full": lambda N, K, H, W: absent_and_full(N, K, H, W, 14),
            "empty_rows": lambda N, K, H, W: empty_rows(N, K, H, W, 15),
            "padded": lambda N, K, H, W: padded(N, K, H, W, 16)}


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def device_map(target, K, ignore=None):
    from stfunet import signed_distance_maps
    phi = signed_distance_maps(target.to(DEV), K, ignore)
    torch.cuda.synchronize()
    return phi.cpu()


@pytest.mark.parametrize("content", list(CONTENTS))
@pytest.mark.parametrize("N,K,H,W", MAP_SHAPES)
def test_maps_equal_the_restatement(N, K, H, W, content):
    target = CONTENTS[content](N, K, H, W)
    ignore = 255 if content == "padded" else None
    ref = torch.from_numpy(sdf_ref(target.numpy(), K, ignore))
    got = device_map(target, K, ignore)
    assert got.shape == (N, K - 1, H, W) and got.dtype == torch.float32
    assert torch.equal(got, ref)
    assert same_bits(got, ref)                             # no -0.0 on the innermost border either


@pytest.mark.parametrize("H,W", [(4096, 3), (3, 4096), (4096, 96), (96, 4096)])
@pytest.mark.parametrize("dtype", [torch.int64, torch.uint8])
def test_longest_distances_take_the_double_square_root(H, W, dtype):
    """One foreground pixel in a corner of the longest images.  At 4096 x 3 the largest squared distance
    is 4095^2 + 2^2 = 16,769,029, still below 2^24; 96 pixels across it is 4095^2 + 95^2 > 2^24, past the
    integers a float holds exactly."""
    target = one_pixel(1, 2, H, W, corner=True)
    ref = sdf_ref(target.numpy(), 2)
    assert (float(ref.max()) ** 2 > 2 ** 24) == (min(H, W) == 96)
    got = device_map(target.to(dtype), 2)
    assert same_bits(got, torch.from_numpy(ref))


def test_an_image_alone_and_inside_a_batch():
    target = blobs(5, 3, 33, 70, 0.1, 21)
    target[3, 10:20, 30:50] = 2
    batch = device_map(target, 3)
    alone = device_map(target[3:4], 3)
    assert same_bits(batch[3:4], alone)
    assert same_bits(batch, device_map(target, 3))         # and from run to run
    assert same_bits(batch, torch.from_numpy(sdf_ref(target.numpy(), 3)))


def test_ignore_index_only_matters_when_it_is_declared_a_class_value():
    target = padded(2, 3, 12, 20, 22)
    assert same_bits(device_map(target, 3, 255), device_map(target, 3, None))
    assert same_bits(device_map(target, 3, -100), device_map(target, 3, None))


# ---------------------------------------------------------------- the term
SEAMS = [(2, 2, 136, 136),      # 18,496 pixels > LCHUNK * 256: a second, ragged grid-stride trip
         (65, 2, 4, 4),         # 4,160 partial pairs: several per finalize thread
         (1, 4, 16, 16),        # the largest K at KP 4
         (3, 7, 24, 16),        # KP 8
         (2, 5, 8, 8),
         (2, 16, 8, 8)]         # KP 16


def run_term(logits, target, ignore, dist=None, grad_out=None):
    from stfunet import boundary_loss
    x = logits.to(DEV).clone().requires_grad_(True)
    loss = boundary_loss(x, target.to(DEV), ignore_index=ignore, dist=dist)
    if grad_out is None:
        loss.backward()
    else:
        loss.backward(torch.tensor(float(grad_out), device=DEV))
    torch.cuda.synchronize()
    return loss.detach().cpu(), x.grad.cpu()


@pytest.mark.parametrize("ignore", [255, -100])
@pytest.mark.parametrize("N,K,H,W", SEAMS)
def test_term_and_gradient_against_restatement(N, K, H, W, ignore):
    logits, target, clean, _ = _seam_case(N, K, H, W)
    t = target if ignore >= 0 else clean
    phi = sdf_ref(t.numpy(), K, ignore)
    ref_loss, ref_grad = boundary_loss_ref(logits, t, phi, ignore)
    scale = max(1.0, abs_loss(logits, t, phi, ignore))
    loss, grad = run_term(logits, t, ignore)
    dl, dg = abs(loss.item() - ref_loss), rel_l2(grad, ref_grad)
    print(f"N{N} K{K} {H}x{W} ignore {ignore}: loss {loss.item():.6f} |dloss| {dl:.3e} (bound "
          f"{LOSS_TOL * scale:.3e}), grad rel-L2 {dg:.3e}")
    assert dl <= LOSS_TOL * scale
    assert dg < GRAD_TOL
    if ignore >= 0:
        assert (grad.permute(0, 2, 3, 1)[t == ignore] == 0).all()


def test_all_ignored_batch_is_nan():
    logits = torch.randn(2, 3, 8, 8)
    target = torch.full((2, 8, 8), 255)
    loss, grad = run_term(logits, target, 255)
    assert torch.isnan(loss).item()
    assert (grad == 0).all()


def test_saturated_logits_stay_finite():
    logits, target, _, _ = _seam_case(2, 3, 16, 16)
    big = torch.where(logits > 0, torch.tensor(1e4), torch.tensor(-1e4))
    loss, grad = run_term(big, target, 255)
    assert torch.isfinite(loss).item() and torch.isfinite(grad).all()
    phi = sdf_ref(target.numpy(), 3, 255)
    ref_loss, _ = boundary_loss_ref(big, target, phi, 255)
    assert abs(loss.item() - ref_loss) <= LOSS_TOL * max(1.0, abs_loss(big, target, phi, 255))


def test_grad_out_scales_the_gradient_and_runs_repeat():
    logits, target, _, _ = _seam_case(2, 5, 8, 8)
    l1, g1 = run_term(logits, target, 255)
    l2, g2 = run_term(logits, target, 255)
    assert same_bits(l1, l2) and same_bits(g1, g2)
    _, g3 = run_term(logits, target, 255, grad_out=3.0)
    assert rel_l2(g3, 3.0 * g1.double()) < 1e-6 and g1.abs().max().item() > 0


def test_precomputed_maps_give_the_same_bits():
    from stfunet import signed_distance_maps
    logits, target, _, _ = _seam_case(2, 4, 16, 16)
    dist = signed_distance_maps(target.to(DEV), 4, 255)
    l1, g1 = run_term(logits, target, 255)
    l2, g2 = run_term(logits, target, 255, dist=dist)
    assert same_bits(l1, l2) and same_bits(g1, g2)


# ---------------------------------------------------------------- composition with the criterion
ROUTES = [((2, 2, 136, 136), dict(), "stf_loss_fwd"),
          ((2, 3, 16, 16), dict(loss_weight="w", ignore_index=255), "stf_loss_opt_fwd"),
          ((3, 7, 24, 16), dict(loss_weight="w", ignore_index=255), "stf_loss_mc_fwd"),
          ((2, 2, 16, 16), dict(loss_weight="w", ignore_index=255, focal_gamma=2.0, tversky=(0.3, 0.7)),
           "stf_loss_ft_fwd")]


def _route_case(shape, kw):
    logits, target, clean, weight = _seam_case(*shape)
    t = target if "ignore_index" in kw else clean
    return logits, t, {k: (weight if v == "w" else v) for k, v in kw.items()}


def run_criterion(logits, target, K, grad_out=None, **kw):
    """``criterion``, or ``boundary_criterion`` when the call names a ``boundary_weight``"""
    import stfunet
    fn = stfunet.boundary_criterion if "boundary_weight" in kw else stfunet.criterion
    x = logits.to(DEV).clone().requires_grad_(True)
    loss = fn({"out": x}, target.to(DEV), num_classes=K, **kw)
    if grad_out is None:
        loss.backward()
    else:
        loss.backward(torch.tensor(float(grad_out), device=DEV))
    torch.cuda.synchronize()
    return loss.detach().cpu(), x.grad.cpu()


def _recorded_names(monkeypatch):
    from stfunet import loss
    names, real = [], loss.call
    monkeypatch.setattr(loss, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    return names


@pytest.mark.parametrize("shape,kw,fwd", ROUTES, ids=[r[2] for r in ROUTES])
def test_criterion_adds_the_weighted_term(monkeypatch, shape, kw, fwd):
    names = _recorded_names(monkeypatch)
    logits, t, kw = _route_case(shape, kw)
    K, ignore, a = shape[1], kw.get("ignore_index", -100), 0.05
    plain_loss, plain_grad = run_criterion(logits, t, K, **kw)
    term_loss, term_grad = run_term(logits, t, ignore)
    del names[:]
    loss, grad = run_criterion(logits, t, K, boundary_weight=a, **kw)
    assert names == [fwd, "stf_sdf", "stf_bloss_fwd", fwd.replace("_fwd", "_bwd"), "stf_bloss_bwd"] or \
        names == ["stf_sdf", fwd, "stf_bloss_fwd", fwd.replace("_fwd", "_bwd"), "stf_bloss_bwd"]
    phi = sdf_ref(t.numpy(), K, ignore)
    scale = max(1.0, abs(plain_loss.item()) + a * abs_loss(logits, t, phi, ignore))
    dl = abs(loss.item() - (plain_loss.item() + a * term_loss.item()))
    dg = rel_l2(grad, plain_grad.double() + a * term_grad.double())
    print(f"{fwd}: loss {loss.item():.6f} = {plain_loss.item():.6f} + {a} * {term_loss.item():.6f}, "
          f"|dloss| {dl:.3e}, grad rel-L2 {dg:.3e}")
    assert dl <= LOSS_TOL * scale and dg < GRAD_TOL
    # and against the float64 restatement of the term, on top of the route's own result
    ref_loss, ref_grad = boundary_loss_ref(logits, t, phi, ignore)
    assert abs(loss.item() - (plain_loss.item() + a * ref_loss)) <= LOSS_TOL * scale
    assert rel_l2(grad, plain_grad.double() + a * ref_grad) < GRAD_TOL
    if ignore >= 0:
        assert (grad.permute(0, 2, 3, 1)[t == ignore] == 0).all()
    # grad_out scales the whole gradient; a second run gives the same bits
    l2, g2 = run_criterion(logits, t, K, boundary_weight=a, **kw)
    assert same_bits(loss, l2) and same_bits(grad, g2)
    _, g3 = run_criterion(logits, t, K, grad_out=0.25, boundary_weight=a, **kw)
    assert rel_l2(g3, 0.25 * grad.double()) < 1e-6


def test_aux_head_shares_one_set_of_maps(monkeypatch):
    from stfunet import boundary_criterion as criterion
    names = _recorded_names(monkeypatch)
    logits, target, _, weight = _seam_case(2, 3, 16, 16)
    x, t = logits.to(DEV), target.to(DEV)
    kw = dict(loss_weight=weight, num_classes=3, ignore_index=255, boundary_weight=0.02)
    out = criterion({"out": x}, t, **kw)
    aux = criterion({"out": x * 0.5}, t, **kw)
    del names[:]
    both = criterion({"out": x, "aux": x * 0.5}, t, **kw)
    assert names.count("stf_sdf") == 1 and names.count("stf_bloss_fwd") == 2
    assert torch.equal(both, out + 0.5 * aux)


@pytest.mark.parametrize("shape,kw,fwd", ROUTES, ids=[r[2] for r in ROUTES])
def test_weight_zero_is_the_criterion_as_it_was(monkeypatch, shape, kw, fwd):
    names = _recorded_names(monkeypatch)
    logits, t, kw = _route_case(shape, kw)
    got = []
    for extra in (dict(), dict(boundary_weight=0), dict(boundary_weight=0.0)):
        del names[:]
        got.append(run_criterion(logits, t, shape[1], **kw, **extra))
        assert names == [fwd, fwd.replace("_fwd", "_bwd")]
    for loss, grad in got[1:]:
        assert same_bits(got[0][0], loss) and same_bits(got[0][1], grad)
    assert torch.isfinite(got[0][0]).item()


# ---------------------------------------------------------------- end to end
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
    real = engine.boundary_criterion

    def recording(inputs, target, **kw):
        loss = real(inputs, target, **kw)
        seen.append((inputs["out"].detach().clone(), target.clone(), loss.detach().clone(), kw))
        return loss

    monkeypatch.setattr(engine, "boundary_criterion", recording)
    opt = AdamW(model.parameters(), lr=1e-3, weight_decay=1e-4)
    sched = engine.create_lr_scheduler(opt, steps, 2)
    before = [p.detach().clone() for p in model.parameters()]
    mean, _ = engine.train_one_epoch(model, opt, batches, torch.device(DEV), 0, 2, lr_scheduler=sched, print_freq=10,
                                     scaler=scaler, ignore_index=255, boundary_weight=0.01)
    changed = sum(int(not torch.equal(a, p.detach())) for a, p in zip(before, model.parameters()))
    return mean, seen, changed


@pytest.mark.parametrize("amp", [False, True], ids=["fp32", "gradscaler"])
def test_train_one_epoch_end_to_end(monkeypatch, amp):
    from stfunet import criterion
    scaler = torch.amp.GradScaler("cuda") if amp else None
    mean, seen, changed = _train(monkeypatch, 2, scaler)
    assert len(seen) == 2 and changed > 0
    for i, (logits, target, loss, kw) in enumerate(seen):
        assert kw["boundary_weight"] == 0.01
        plain = criterion({"out": logits}, target, num_classes=2, ignore_index=255)
        phi = sdf_ref(target.cpu().numpy(), 2, 255)
        ref, _ = boundary_loss_ref(logits.cpu(), target.cpu(), phi, 255)
        print(f"step {i}: loss {loss.item():.6f} = CE + Dice {plain.item():.6f} + 0.01 * {ref:.6f}")
        assert torch.isfinite(loss).item()
        assert abs(loss.item() - (plain.item() + 0.01 * ref)) <= 2 * LOSS_TOL * max(1.0, abs(loss.item()))
    assert np.isfinite(mean)
    if amp:
        assert scaler.get_scale() == 65536.0               # the scaled gradient was finite: no step skipped
