"""Five to sixteen classes on the gfx950 kernels (stf_head_mc_* / stf_loss_mc_*).

Reference-generated fixture entries through ``stfunet.loss.ce_dice_loss``; the new kernels at
K = 2, 3 on the existing fixture; the loss kernels' seams against the tests' float64 restatement;
the head against torch autograd in float64 on the storage-rounded activations; whole models
against the oracle; replayed plans against eager steps; and the training / evaluation / inference
loop at K = 6.  Tolerances are the project's (tests/test_criterion_options_gpu.py, DESIGN "Parity"):
loss |d| <= 1e-5 * max(1, |loss|) (1e-5 was set at losses of order 1; CE at K = 16 is ~3.5),
dlogits rel-L2 <= 1e-4, head fp32 outputs rel-L2 <= 2e-3 (bf16 storage) / 1e-3 (fp16), outputs in
the storage type 1e-2 / 2e-3.
"""
import os

import pytest
import torch

from _criterion_ref import criterion_ref, fixture_entries, ref_loss_and_grad, rel_l2
from _multiclass import MC_ENTRIES

pytestmark = pytest.mark.gpu

DEV = "cuda"
LOSS_TOL, GRAD_TOL = 1e-5, 1e-4
K23_ENTRIES = fixture_entries()


def run(logits, target, weight=None, ignore_index=-100, dice=True, grad_out=None):
    """loss (device scalar) and d/d(logits) through stfunet.loss.ce_dice_loss."""
    from stfunet.loss import ce_dice_loss
    x = logits.to(DEV).clone().requires_grad_(True)
    loss = ce_dice_loss(x, target.to(DEV), weight, ignore_index, dice)
    if grad_out is None:
        loss.backward()
    else:
        loss.backward(torch.tensor(float(grad_out), device=DEV))
    return loss.detach(), x.grad


def direct(logits, target, weight, ign, dice, fill=float("nan"), grad_out=1.0):
    """The many-class C entry points themselves, dlogits pre-filled with ``fill``."""
    from stfunet import _lib
    from stfunet._lib import call, stream
    from stfunet.nhwc import _p
    x, t = logits.to(DEV).contiguous(), target.to(DEV).contiguous()
    N, K, H, W = x.shape
    w = torch.as_tensor(weight, dtype=torch.float32).to(DEV) if weight is not None else None
    terms = torch.empty(_lib.load().stf_loss_mc_scratch_floats(N, K), device=DEV)
    loss = torch.empty(1, device=DEV)
    wp = _p(w) if w is not None else None
    call("stf_loss_mc_fwd", _p(x), _p(t), N, H, W, K, wp, ign, int(dice), _p(terms), _p(loss), stream())
    dl = torch.full_like(x, fill)
    go = torch.full((1,), float(grad_out), device=DEV)
    call("stf_loss_mc_bwd", _p(x), _p(t), N, H, W, K, wp, ign, int(dice), _p(terms), _p(go), _p(dl), stream())
    torch.cuda.synchronize()
    return loss[0], dl


def check(tag, loss, grad, ref_loss, ref_grad):
    dl = abs(loss.item() - ref_loss)
    dg = rel_l2(grad, ref_grad)
    print(f"{tag}: loss {loss.item():.6f} |dloss| {dl:.3e}, grad rel-L2 {dg:.3e}")
    assert dl <= LOSS_TOL * max(1.0, abs(ref_loss))
    assert dg <= GRAD_TOL


def ignored_are_zero(grad, target, ign):
    return bool((grad.cpu().permute(0, 2, 3, 1)[target == ign] == 0).all())


# ------------------------------------------------------------------ 1, 2: the reference's fixtures
@pytest.mark.parametrize("e", MC_ENTRIES, ids=[e["name"] for e in MC_ENTRIES])
def test_reference_entries_through_ce_dice_loss(e):
    loss, grad = run(e["logits"], e["target"], e["weight"], e["ignore_index"], e["dice"])
    check(e["name"], loss, grad, e["loss"], e["grad"])
    if e["ignore_index"] >= 0:
        assert ignored_are_zero(grad, e["target"], e["ignore_index"])


@pytest.mark.parametrize("e", K23_ENTRIES, ids=[e["name"] for e in K23_ENTRIES])
def test_new_kernels_on_the_two_and_three_class_fixture(e):
    loss, grad = direct(e["logits"], e["target"], e["weight"], e["ignore_index"], e["dice"])
    check(e["name"], loss, grad, e["loss"], e["grad"])
    if e["ignore_index"] >= 0:
        assert ignored_are_zero(grad, e["target"], e["ignore_index"])


# ------------------------------------------------------------------ 3: loss seams
def _seam_case(N, K, H, W):
    """logits, a target with ignored column / row bands, scattered ignored pixels and one fully
    ignored image when N > 1, and class weights."""
    g = torch.Generator().manual_seed(1000 * N + 10 * K + H)
    logits = torch.randn(N, K, H, W, generator=g) * 3.0
    target = torch.randint(0, K, (N, H, W), generator=g)
    target[0, :, W - max(1, W // 4):] = 255
    target[-1, H - max(1, H // 4):, :] = 255
    target[torch.rand(N, H, W, generator=g) < 0.05] = 255
    if N > 1:
        target[N // 2] = 255
    weight = [0.5 + 0.25 * ((5 * k) % K) for k in range(K)]
    return logits, target, weight


SHAPES = [(1, 7, 9),            # fewer pixels than one block
          (65, 4, 4),           # the finalize's second batch of 64 images
          (2, 129, 135)]        # 17,415 pixels (odd) > one grid stride of 64 x 256: a thread loops twice


@pytest.mark.parametrize("N,H,W", SHAPES)
@pytest.mark.parametrize("K", [5, 8, 9, 16])
def test_loss_shapes_against_restatement(K, N, H, W):
    logits, target, weight = _seam_case(N, K, H, W)
    go = 65536.0                                          # a GradScaler's scale: exact in binary fp
    ref_loss, ref_grad = ref_loss_and_grad(logits, target, weight, 255, True, grad_out=go)
    loss, grad = run(logits, target, weight, 255, True, grad_out=go)
    check(f"K{K} N{N} {H}x{W}", loss, grad, ref_loss, ref_grad)
    assert ignored_are_zero(grad, target, 255)
    if N > 1:
        assert (target[N // 2] == 255).all() and (grad[N // 2] == 0).all()     # D = 1, no gradient
    loss2, grad2 = run(logits, target, weight, 255, True, grad_out=go)
    assert torch.equal(loss, loss2) and torch.equal(grad, grad2)
    # the other configurations on the same case: no weights, cross-entropy only
    for w, dice in ((None, True), (weight, False)):
        rl, rg = ref_loss_and_grad(logits, target, w, 255, dice)
        l, g = run(logits, target, w, 255, dice)
        check(f"K{K} N{N} {H}x{W} weights {w is not None} dice {dice}", l, g, rl, rg)


@pytest.mark.parametrize("K", [5, 16])
def test_saturated_logits_and_an_absent_class(K):
    g = torch.Generator().manual_seed(K)
    N, H, W = 2, 12, 20
    target = torch.randint(0, K - 1, (N, H, W), generator=g)           # class K-1 in no image ...
    target[1][target[1] == 0] = 1                                      # ... and class 0 not in image 1
    logits = torch.full((N, K, H, W), -80.0)
    hot = torch.randint(0, K, (N, H, W), generator=g)                  # the +80 class: right or wrong
    logits.scatter_(1, hot[:, None], 80.0)
    ref_loss, ref_grad = ref_loss_and_grad(logits, target)
    for weight, ign in ((None, -100), ([1.0 + 0.5 * k for k in range(K)], 255)):
        rl, rg = ref_loss_and_grad(logits, target, weight, ign, True)
        loss, grad = run(logits, target, weight, ign, True)
        assert torch.isfinite(loss).item() and torch.isfinite(grad).all()
        check(f"saturated K{K} weights {weight is not None}", loss, grad, rl, rg)
    assert ref_loss > 10.0                                             # wrong +80 pixels: CE ~ 160 each


def _restatement_with_foreign_targets(logits, target, weight, ign, dice, eps=1e-6):
    """criterion_ref where a target outside [0, K) that is not the ignore value is kept as a pixel
    (its probabilities count in sum p) but is no class: weight 0 in the cross-entropy, no one-hot."""
    N, K = logits.shape[:2]
    z = logits.reshape(N, K, -1)
    t = target.reshape(N, -1).long()
    m = t != ign
    v = m & (t >= 0) & (t < K)
    tc = torch.where(v, t, torch.zeros_like(t))
    w = torch.as_tensor(weight).to(z.dtype)
    wt = w[tc] * v
    nll = -torch.log_softmax(z, 1).gather(1, tc[:, None]).squeeze(1)
    loss = (wt * nll).sum() / wt.sum()
    if dice:
        p = torch.softmax(z, 1) * m[:, None].to(z.dtype)
        oh = torch.nn.functional.one_hot(tc, K).permute(0, 2, 1).to(z.dtype) * v[:, None].to(z.dtype)
        inter, sets = (p * oh).sum(-1), p.sum(-1) + oh.sum(-1)
        loss = loss + 1 - torch.where(sets == 0, torch.ones_like(sets), (2 * inter + eps) / (sets + eps)).mean()
    return loss


def test_out_of_range_targets_weigh_nothing():
    K = 6
    logits, target, weight = _seam_case(3, K, 16, 24)
    x = logits.double().requires_grad_(True)
    same = _restatement_with_foreign_targets(x, target, weight, 255, True)
    assert abs(same.item() - criterion_ref(logits.double(), target, weight, 255, True).item()) < 1e-12
    target[0, 3, :5] = 300
    target[2, 1::4, 2] = -7
    target[2, 5, 5] = K
    x = logits.double().requires_grad_(True)
    ref = _restatement_with_foreign_targets(x, target, weight, 255, True)
    ref.backward()
    loss, grad = run(logits, target, weight, 255, True)
    check("foreign targets", loss, grad, ref.item(), x.grad)
    assert ignored_are_zero(grad, target, 255)
    assert (grad.cpu().permute(0, 2, 3, 1)[target == 300] != 0).any()      # kept pixels: the Dice term's gradient


def test_all_ignored_batch_is_nan_and_nan_logits_stay_out():
    logits, target, weight = _seam_case(3, 7, 16, 24)
    loss, dl = direct(logits, target, weight, 255, True)
    assert not torch.isnan(dl).any() and ignored_are_zero(dl, target, 255)
    bad = logits.clone()
    bad.permute(0, 2, 3, 1)[target == 255] = float("nan")
    loss_b, dl_b = direct(bad, target, weight, 255, True)
    assert torch.equal(loss_b, loss) and torch.equal(dl_b, dl)
    loss_n, dl_n = direct(logits, torch.full_like(target, 255), weight, 255, True)
    assert torch.isnan(loss_n).item() and (dl_n == 0).all()


# ------------------------------------------------------------------ 4: the head
def _head_run(K, C, N, H, W, dt, real_bn, seed):
    """Forward and backward of the head through stfunet.nhwc on storage-rounded activations, and the
    float64 torch autograd result of conv1x1(relu(y * scale + shift)) on the same values."""
    from stfunet import _lib, nhwc
    g = torch.Generator().manual_seed(seed)
    y = (torch.randn(N, H, W, C, generator=g) * 1.5).to(dt).to(DEV)
    conv = torch.nn.Conv2d(C, K, 1).to(DEV)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(K, C, 1, 1, generator=g) / C ** 0.5)
        conv.bias.copy_(torch.randn(K, generator=g))
    dl = torch.randn(N, K, H, W, generator=g).to(DEV)
    with _lib.storage(dt):
        if real_bn:
            st = nhwc.BNState(C, DEV, N * H * W)
            mean, invstd = torch.randn(C, generator=g) * 0.3, torch.rand(C, generator=g) + 0.5
            gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3
            st.mean.copy_(mean.view(1, C))
            st.invstd.copy_(invstd.view(1, C))
            st.scale.copy_((gamma * invstd).view(1, C))
            st.shift.copy_((beta - mean * gamma * invstd).view(1, C))
        else:
            st = nhwc.BNState.identity(C, DEV)
        yf = nhwc.Feat(y.reshape(-1), N, H, W, C, C, 0)
        logits = torch.empty(N, K, H, W, device=DEV)
        head_w = nhwc.head_fwd(yf, st, conv, logits)
        dw, db = torch.empty(K * C, device=DEV), torch.empty(K, device=DEV)
        gf, bnp, tiles = nhwc.head_bwd(dl, yf, st, head_w, dw, db)
        torch.cuda.synchronize()
    got = dict(logits=logits, g=gf.dense(), graw=gf.buf.clone(), dw=dw.view(K, C), db=db,
               sums=bnp.view(tiles, 2, C).double().sum(0), bnp=bnp)
    # float64 reference
    yd = y.double().requires_grad_(True)                                   # [N, H, W, C]
    wd = conv.weight.detach().double().view(K, C).requires_grad_(True)
    bd = conv.bias.detach().double().requires_grad_(True)
    z = yd * st.scale.double().view(C) + st.shift.double().view(C)
    a = torch.relu(z)
    a.retain_grad()
    ref_logits = (a @ wd.t() + bd).permute(0, 3, 1, 2)
    ref_logits.backward(dl.double())
    gref = a.grad * (z > 0)                                                # gradient w.r.t. BN(y), ReLU-masked
    xhat = (yd.detach() - st.mean.double().view(C)) * st.invstd.double().view(C)
    ref = dict(logits=ref_logits.detach(), g=gref.permute(0, 3, 1, 2), dw=wd.grad, db=bd.grad,
               sums=torch.stack([gref.sum((0, 1, 2)), (gref * xhat).sum((0, 1, 2))]))
    return got, ref


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("C", [8, 32, 64, 512])
@pytest.mark.parametrize("K", [5, 7, 16])
def test_head_forward_backward_vs_autograd(K, C, dt):
    f32_tol, st_tol = (2e-3, 1e-2) if dt == torch.bfloat16 else (1e-3, 2e-3)
    for N, H, W in ((3, 9, 7), (2, 64, 64)):             # fewer units than one block at C = 8; several tiles
        for real_bn in (True, False):                    # a real BatchNorm state; the identity state STF passes
            got, ref = _head_run(K, C, N, H, W, dt, real_bn, seed=K * 1000 + C + N)
            errs = {k: rel_l2(got[k], ref[k]) for k in ("logits", "dw", "db", "sums", "g")}
            print(f"K{K} C{C} {N}x{H}x{W} bn {real_bn} {dt}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
            for k in ("logits", "dw", "db", "sums"):
                assert errs[k] <= f32_tol, (k, errs[k])
            assert errs["g"] <= st_tol, errs["g"]
            again, _ = _head_run(K, C, N, H, W, dt, real_bn, seed=K * 1000 + C + N)
            for k in ("logits", "graw", "dw", "db", "bnp"):
                assert torch.equal(got[k], again[k]), k


# ------------------------------------------------------------------ 5, 6: whole models
def _rel(a, b):
    return rel_l2(torch.as_tensor(a), torch.as_tensor(b))


def _bn_fed_bias(k):
    return k.endswith((".0.bias", ".3.bias")) and not k.startswith(("up", "out_conv"))


def _unet6(storage=None):
    from oracle.init import canonical_state_dict
    from stfunet import UNet
    m = UNet(in_channels=8, num_classes=6, base_c=8)
    sd = canonical_state_dict(m.state_dict(), seed=0)
    m.load_state_dict(sd)
    m.storage_dtype = storage
    return m.to(DEV).train(), sd


def _case6(size, seed=1):
    from oracle.cases import dce_case
    x5, _ = dce_case(seed, 2, 8, size, size)
    t = torch.randint(0, 6, (2, size, size), generator=torch.Generator().manual_seed(seed))
    return x5.flatten(1, 2), t


def _oracle6(sd, x, t, fwd, grad=True):
    from oracle import loss as o_loss
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    p = {k: v.clone().requires_grad_(grad and v.is_floating_point() and "running" not in k) for k, v in sd.items()}
    with torch.set_grad_enabled(grad):
        out = fwd(p, x, training=True)["out"]
        loss = o_loss.criterion(out, t, num_classes=6)
    if grad:
        loss.backward()
    return p, out.detach(), loss.item()


@pytest.mark.parametrize("size", [32, 64])
def test_unet_six_classes_vs_oracle(size):
    from oracle import unet as o_unet, unet_bf16 as o_unet_bf16
    from stfunet.loss import criterion
    model, sd = _unet6()
    x, t = _case6(size)
    p, ref_out, ref_loss = _oracle6(sd, x, t, o_unet.forward)
    pe, _, _ = _oracle6(sd, x, t, o_unet_bf16.forward)
    out = model(x.to(DEV))["out"]
    assert out.shape == (2, 6, size, size)
    loss = criterion({"out": out}, t.to(DEV), num_classes=6)
    loss.backward()
    print(f"size {size}: logits rel {_rel(out.detach(), ref_out):.3e}, loss {loss.item():.5f} oracle {ref_loss:.5f}")
    assert _rel(out.detach(), ref_out) < 3e-2
    assert abs(loss.item() - ref_loss) < 1e-2
    named = dict(model.named_parameters())
    bad = []
    for k, v in p.items():
        if v.grad is None:
            continue
        got = named[k].grad
        if _bn_fed_bias(k):
            scale = v.grad.abs().max().item() + p[k.replace("bias", "weight")].grad.abs().mean().item()
            if got.abs().max().item() > 0.05 * scale + 1e-5:
                bad.append((k, "bias", got.abs().max().item()))
            continue
        e_hip, e_emu = _rel(got, v.grad), _rel(pe[k].grad, v.grad)
        if e_hip > 2 * e_emu + 0.03:
            bad.append((k, e_hip, e_emu))
    assert not bad, bad


@pytest.mark.parametrize("size", [32, 64])
def test_unet_six_classes_fp16_vs_oracle(size):
    """The bands of test_fp16_gpu.test_model_fp16_vs_oracle: logits within 1.5x the fp16 emulation's
    error + 2e-3, loss within 2x the emulation's loss error + 1e-4."""
    import oracle.unet_bf16 as o_q
    from oracle import unet as o_unet
    from stfunet.loss import criterion
    model, sd = _unet6(torch.float16)
    x, t = _case6(size)
    with torch.no_grad():
        out = model(x.to(DEV))["out"]
        loss = criterion({"out": out}, t.to(DEV), num_classes=6).item()
    assert model.program.packs.dtype == torch.float16
    _, ref, ref_loss = _oracle6(sd, x, t, o_unet.forward, grad=False)
    with o_q.storage(torch.float16):
        _, emu_out, emu_loss = _oracle6(sd, x, t, o_q.forward, grad=False)
    e_emu = _rel(emu_out, ref)
    print(f"size {size}: logits rel {_rel(out, ref):.3e} emulation {e_emu:.3e}, loss {loss:.6f} oracle {ref_loss:.6f} "
          f"emulation {emu_loss:.6f}")
    assert _rel(out, ref) <= 1.5 * e_emu + 2e-3
    assert abs(loss - ref_loss) <= 2 * abs(emu_loss - ref_loss) + 1e-4


def _stf5():
    from oracle.init import canonical_state_dict
    from stfunet import STFLSTMUNet
    m = STFLSTMUNet(num_classes=5, time_steps=2)
    sd = canonical_state_dict(m.state_dict(), seed=0)
    gen = torch.Generator().manual_seed(3)
    for k, v in sd.items():
        if "running_mean" in k:
            sd[k] = torch.rand(v.shape, generator=gen) * 0.2 - 0.1
        if "running_var" in k:
            sd[k] = torch.rand(v.shape, generator=gen) * 0.5 + 0.75
    m.load_state_dict(sd)
    x = torch.rand(1, 2, 1, 32, 32, generator=gen)
    return m.to(DEV), sd, x


def test_stf_five_classes_eval_vs_oracle():
    import oracle.unet_bf16 as o_q
    from oracle import stf as o_stf, stf_bf16 as o_emu
    m, sd, x = _stf5()
    m.eval()
    with torch.no_grad():
        out = m(x.to(DEV))["out"]
        ref = o_stf.forward(sd, x, False)["out"]
        with o_q.storage(torch.bfloat16):
            emu = o_emu.forward(sd, x, False)["out"]
    assert out.shape == (1, 5, 16, 16)
    e_emu = _rel(emu, ref)
    print(f"stf K=5 eval: logits rel {_rel(out, ref):.3e}, emulation {e_emu:.3e}")
    assert _rel(out, ref) <= 2 * e_emu + 2e-3


def test_stf_five_classes_training_step_head_gradients():
    """One training step: finite gradients everywhere, and final.weight / final.bias equal torch
    autograd of the 1x1 head on the model's own last activation and the criterion's dlogits."""
    from stfunet.loss import criterion
    m, _, x = _stf5()
    m.train()
    t = torch.randint(0, 5, (1, 16, 16), generator=torch.Generator().manual_seed(9))
    out = m(x.to(DEV))["out"]
    act = out.grad_fn.saved.fr.out.dense().double()            # [1, 32, 16, 16], ReLU applied (identity state)
    out.retain_grad()
    loss = criterion({"out": out}, t.to(DEV), num_classes=5, loss_weight=[1.0, 2.0, 0.5, 1.5, 1.0])
    loss.backward()
    assert torch.isfinite(loss).item()
    for k, p in m.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), k
    dl = out.grad.double()
    dw_ref = torch.einsum("nkhw,nchw->kc", dl, act)
    e_w = _rel(m.final.weight.grad.view(5, 32), dw_ref)
    e_b = _rel(m.final.bias.grad, dl.sum((0, 2, 3)))
    print(f"stf K=5 head gradients: dW rel {e_w:.3e}, db rel {e_b:.3e}")
    assert dw_ref.norm().item() > 0 and e_w <= 2e-3 and e_b <= 2e-3


# ------------------------------------------------------------------ 7: plans
def _train6(monkeypatch, plan_on, steps=5):
    from stfunet import UNet, engine
    from stfunet.optim import AdamW
    monkeypatch.setenv("STF_PLAN", "1" if plan_on else "0")
    torch.manual_seed(0)
    model = UNet(in_channels=8, num_classes=6, base_c=8).cuda().train()
    opt = AdamW(model.parameters(), lr=1e-3, weight_decay=1e-4)
    g = torch.Generator().manual_seed(70)
    batches = [(torch.rand(2, 8, 64, 64, generator=g).to(DEV), torch.randint(0, 6, (2, 64, 64), generator=g).to(DEV))
               for _ in range(3)]
    losses = []
    for i in range(steps):
        x, t = batches[i % 3]
        loss = engine.criterion(model(x), t, num_classes=6)
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(loss.detach().clone())
    torch.cuda.synchronize()
    state = {k: v.detach().clone() for k, v in model.state_dict().items()}
    return torch.stack(losses), state, model.program.runtime.bwd is not None


def test_replayed_plan_steps_equal_eager_steps(monkeypatch):
    """Five steps: eager, recorded, then three replayed ones, against five eager steps bit for bit."""
    l0, s0, planned0 = _train6(monkeypatch, False)
    l1, s1, planned1 = _train6(monkeypatch, True)
    assert planned1 and not planned0
    assert torch.equal(l0, l1), (l0, l1)
    for k in s0:
        assert torch.equal(s0[k], s1[k]), k
    assert len(set(l0.tolist())) == 5


# ------------------------------------------------------------------ 8: end to end
def test_train_evaluate_predict_six_classes():
    from stfunet import UNet, engine
    from stfunet.optim import AdamW
    from stfunet.predict import predict_masks
    K = 6
    torch.manual_seed(0)
    model = UNet(8, K, 8).to(DEV)
    g = torch.Generator().manual_seed(11)
    batches = []
    for _ in range(2):
        t = torch.randint(0, K, (2, 32, 32), generator=g)
        t[0, :, 28:] = 255
        batches.append((torch.rand(2, 8, 1, 32, 32, generator=g), t))
    opt = AdamW(model.parameters(), lr=1e-3, weight_decay=1e-4)
    sched = engine.create_lr_scheduler(opt, 2, 2)
    before = model.out_conv.weight.detach().clone()
    mean, _ = engine.train_one_epoch(model, opt, batches, torch.device(DEV), 0, K, lr_scheduler=sched, print_freq=10,
                                     ignore_index=255, loss_weight=[1.0, 2.0, 0.5, 1.5, 1.0, 3.0])
    assert mean == mean and not torch.equal(before, model.out_conv.weight.detach())
    clean = [(x, torch.randint(0, K, (2, 32, 32), generator=g)) for x, _ in batches]
    res = engine.evaluate(model, clean, torch.device(DEV), K)
    want = torch.zeros(K * K, dtype=torch.int64)
    model.eval()
    with torch.no_grad():
        for x, t in clean:
            logits = model(x.flatten(1, 2).to(DEV))["out"]
            pred = logits.argmax(1)
            want += torch.bincount((K * t.to(DEV) + pred).flatten(), minlength=K * K).cpu()
            mask = predict_masks({"out": logits}, rule="argmax")
            assert mask.dtype == torch.uint8 and torch.equal(mask.long(), pred)
    assert torch.equal(res["confusion_matrix"].mat.cpu().long().flatten(), want)
    assert want.sum().item() == 2 * 2 * 32 * 32
