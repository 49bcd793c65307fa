"""Mirror test-time augmentation on the GPU (csrc/tta.hip, rule "threshold" of csrc/predict.hip,
stfunet.predict.flip_planes / tta_probabilities / predict_tta).

Exact where the definition is exact: the flip against torch.flip, the un-flip indexing (the same
per-pixel arithmetic at another position), the fold (one fp32 add per view, one fp32 divide), the
threshold rule against numpy, and predict_tta's bookkeeping.  The probabilities are compared with
a float64 restatement within a bound derived below from the roundings the definition lists.


The bound (``bound64``)
-----------------------
u = 2^-24 is the unit roundoff of fp32; every listed operation rounds once (relative error <= u),
and the device ``expf`` is documented at 1 ulp (HIP's device math table), i.e. a relative error
<= 2^-23 = 2u.  The logits of a view are the same fp32 numbers on both sides, so m is exact.

rule "argmax", one view, one pixel, D = max_k (m - z_k):
  d_k = z_k - m            one rounding: absolute error <= |d_k| u, which exp turns into a relative
                           error |d_k| u of e_k; with expf's 2u:  e_k is within (|d_k| + 2) u
  s = e_0 + e_1 + ...      positive terms, K - 1 roundings:       s is within (D + 2 + K - 1) u
  p_k = e_k / s            one rounding:                          p_k is within (2 D + K + 4) u
rule "sigmoid":
  t = expf(-z)             2u;  a = 1 + t: t's error counts t / (1 + t) < 1 times, plus one rounding: 3u
  p = 1 / a                one rounding:                          p is within 4 u
so view v contributes an absolute error <= p_v c_v u with c_v = 2 D_v + K + 4 (or 4).

The fold: acc = p_0, then n - 1 fp32 adds of non-negative numbers, each rounding by at most u times
a partial sum that is at most the final sum n * mean; the final divide rounds once more.  Hence
  |mean_fp32 - mean_64| <= u * [ (1 / n) sum_v p_v c_v  +  (n - 1) mean  +  mean ]
                         =  u * [ mean_v(p_v c_v) + n * mean ],
times 1.001 for the second-order terms (c u < 1e-5 while D <= 80, which the test asserts, and which
also keeps every e_k a normal number).  Nothing in it comes from what the kernels return.
"""
import os

import numpy as np
import pytest
import torch

from _predict_ref import counts_ref, mask_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
VIEWS = ("none", "w", "h", "hw")
CODE = {"none": 0, "w": 1, "h": 2, "hw": 3}
DIMS = {"none": (), "w": (-1,), "h": (-2,), "hw": (-2, -1)}
SHAPES = [(3, 2, 32, 48), (2, 5, 6, 50), (1, 16, 7, 33), (2, 1, 1, 5), (1, 3, 5, 1)]
IDS = ["x".join(map(str, s)) for s in SHAPES]
REPORT = {}                         # test id -> largest err / bound, printed as the tests go


def tflip(x, view):
    return x.flip(DIMS[view]).contiguous() if DIMS[view] else x.clone()


def accumulate(z, rule, channel, view, first=True, n=0, acc=None):
    """One stf_tta_accumulate launch; a first view writes into a buffer prefilled with NaN."""
    from stfunet._lib import call, stream
    B, K, H, W = z.shape
    if acc is None:
        assert first
        acc = torch.full((B, K if rule == "argmax" else 1, H, W), float("nan"), device=DEV)
    else:
        acc = acc.clone()
    call("stf_tta_accumulate", z.data_ptr(), B, K, H, W, 0 if rule == "argmax" else 1, channel, CODE[view],
         int(first), n, acc.data_ptr(), stream())
    return acc


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def divide(acc, n):
    """``acc / (float)n`` as one IEEE fp32 divide in torch on the device: a tensor divisor (torch's
    division of a device tensor by a Python number multiplies by the rounded reciprocal, which is
    another number for n = 3).  numpy's fp32 divide on the host must give the same bits."""
    out = torch.div(acc, torch.full_like(acc, float(n)))
    assert same_bits(out, torch.from_numpy(acc.cpu().numpy() / np.float32(n)).to(acc.device))
    return out


def probs64(z, rule, channel):
    """(p, c): float64 probabilities of fp32 logits ``z`` [B, K, H, W] (numpy) and the per-pixel
    constant c of the docstring."""
    z = z.astype(np.float64)
    if rule == "sigmoid":
        x = z[:, channel:channel + 1]
        return 1.0 / (1.0 + np.exp(-x)), np.full(x.shape, 4.0)
    m = z.max(1, keepdims=True)
    D = (m - z.min(1, keepdims=True))
    assert D.max() <= 80
    e = np.exp(z - m)
    return e / e.sum(1, keepdims=True), 2 * D + z.shape[1] + 4


def mean64(zs, views, rule, channel):
    """The float64 restatement and its bound.  ``zs[i]``: the fp32 logits of view ``views[i]``, as
    the model gave them (in the flipped frame)."""
    n = len(views)
    total, werr = 0.0, 0.0
    for z, v in zip(zs, views):
        p, c = probs64(z, rule, channel)
        axes = tuple(a + 4 for a in DIMS[v])
        total = total + (np.flip(p, axes) if axes else p)
        werr = werr + (np.flip(p * c, axes) if axes else p * c)
    mean = total / n
    return mean, 1.001 * U * (werr / n + n * mean)


def report(name, got, mean, bound):
    err = np.abs(got.astype(np.float64) - mean)
    ratio = float((err / bound).max())
    REPORT[name] = ratio
    print(f"\n[tta] {name}: max err {err.max():.3e}, largest err / bound {ratio:.4f}")
    return ratio


# ------------------------------------------------------------------ 1. flip
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_flip_planes_is_torch_flip(shape):
    from stfunet import flip_planes
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(shape, generator=g).to(DEV)
    for v in VIEWS:
        y = flip_planes(x, v)
        assert y.data_ptr() != x.data_ptr() and y.is_contiguous() and y.dtype == torch.float32
        assert torch.equal(y.view(torch.int32), tflip(x, v).view(torch.int32)), v


def test_flip_planes_5d_unaligned_and_strided():
    from stfunet import flip_planes
    g = torch.Generator().manual_seed(5)
    x5 = torch.randn(2, 4, 1, 32, 48, generator=g).to(DEV)
    flat = torch.randn(3 * 32 * 48 + 1, generator=g).to(DEV)
    off = flat[1:].view(3, 32, 48)                                 # base 4 bytes past a 16-byte boundary
    assert off.data_ptr() % 16 == 4 and off.is_contiguous()
    strided = torch.randn(2, 3, 8, 24, generator=g).to(DEV)[..., ::2]
    assert not strided.is_contiguous()
    for v in VIEWS:
        for x in (x5, off, strided):
            assert torch.equal(flip_planes(x, v).view(torch.int32), tflip(x, v).view(torch.int32)), v


# ------------------------------------------------------------------ 2. indexing, exact
@pytest.mark.parametrize("rule", ["argmax", "sigmoid"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_unflip_indexing_and_fold_are_exact(shape, rule):
    B, K, H, W = shape
    g = torch.Generator().manual_seed(100 + sum(shape))
    z = (torch.randn(shape, generator=g) * 2).to(DEV)
    z2 = (torch.randn(shape, generator=g) * 2).to(DEV)
    ch = K - 1
    plain = accumulate(z, rule, ch, "none")
    assert not torch.isnan(plain).any() and plain.shape == (B, K if rule == "argmax" else 1, H, W)
    if rule == "sigmoid":                                          # the arithmetic of the mask's sigmoid rule
        from stfunet import predict_masks
        assert torch.equal(predict_masks(z, "sigmoid", ch, 0.3), (plain[:, 0] > 0.3).to(torch.uint8))
    single2 = accumulate(z2, rule, ch, "none")
    for v in VIEWS:
        # the same per-pixel arithmetic, only the position differs
        got = accumulate(tflip(z, v), rule, ch, v)
        assert torch.equal(got.view(torch.int32), plain.view(torch.int32)), v
        # a second view on top: one fp32 add
        two = accumulate(tflip(z2, v), rule, ch, v, first=False, acc=plain)
        assert torch.equal(two.view(torch.int32), (plain + single2).view(torch.int32)), v
        # the final divide, in the same pass
        for n in (1, 2, 3, 4):
            last = accumulate(tflip(z2, v), rule, ch, v, first=False, n=n, acc=plain)
            assert same_bits(last, divide(plain + single2, n)), (v, n)
        only = accumulate(tflip(z, v), rule, ch, v, first=True, n=3)
        assert same_bits(only, divide(plain, 3)), v


def test_accumulate_on_an_unaligned_base_equals_the_aligned_result():
    g = torch.Generator().manual_seed(9)
    z = (torch.randn(2, 3, 8, 16, generator=g) * 2).to(DEV)
    flat = torch.zeros(z.numel() + 1, device=DEV)
    off = flat[1:].view(z.shape)
    off.copy_(z)
    assert off.data_ptr() % 16 == 4
    for v in VIEWS:
        a, b = accumulate(z, "argmax", 0, v), accumulate(off, "argmax", 0, v)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), v


# ------------------------------------------------------------------ 3. probabilities against float64
@pytest.mark.parametrize("rule", ["argmax", "sigmoid"])
@pytest.mark.parametrize("shape", SHAPES[:3], ids=IDS[:3])
def test_probabilities_against_float64(shape, rule):
    """Gaussian logits (standard deviation 2, seed 0), four views: every element of the mean within
    ``bound64`` of the float64 restatement (the module docstring derives it).  Measured on an
    MI355X, largest err / bound: see DESIGN.md 5.13."""
    g = torch.Generator().manual_seed(0)
    zs = [torch.randn(shape, generator=g) * 2 for _ in VIEWS]
    ch = shape[1] // 2
    acc = None
    for i, (z, v) in enumerate(zip(zs, VIEWS)):
        acc = accumulate(z.to(DEV), rule, ch, v, first=i == 0, n=4 if i == 3 else 0, acc=acc)
    mean, bound = mean64([z.numpy() for z in zs], VIEWS, rule, ch)
    ratio = report(f"kernel {rule} {'x'.join(map(str, shape))}", acc.cpu().numpy(), mean, bound)
    assert ratio <= 1.0


# ------------------------------------------------------------------ 4. threshold rule, exact
@pytest.mark.parametrize("shape", [(2, 3, 8, 8), (2, 3, 7, 10), (1, 1, 1, 1)], ids=["quad", "scalar", "one"])
def test_threshold_rule_is_numpy(shape):
    from stfunet import predict_masks
    B, K, H, W = shape
    g = torch.Generator().manual_seed(H * W)
    thr = 0.375
    values = torch.tensor([0.0, 0.125, 0.25, 0.375, 0.5, 0.75, 1.0, float("nan"), float("inf"), float("-inf")])
    p = values[torch.randint(0, len(values), shape, generator=g)]
    p.view(-1)[:min(len(values), p.numel())] = values[:min(len(values), p.numel())]
    target = torch.randint(0, 3, (B, H, W), generator=g)
    target[torch.rand(B, H, W, generator=g) < 0.2] = 255
    ch = K - 1
    with np.errstate(invalid="ignore"):
        ref = (p[:, ch].numpy() > np.float32(thr)).astype(np.uint8)
    mask, counts = predict_masks(p.to(DEV), "threshold", ch, thr, target=target.to(DEV), ignore_index=255)
    assert mask.dtype == torch.uint8 and np.array_equal(mask.cpu().numpy(), ref)
    t = target.numpy()
    keep = t != 255
    want = [[int(((ref[b] > 0) & (t[b] > 0) & keep[b]).sum()), int(((ref[b] > 0) & keep[b]).sum()),
             int(((t[b] > 0) & keep[b]).sum())] for b in range(B)]
    assert counts.cpu().tolist() == want
    assert np.array_equal(predict_masks(p.to(DEV), "threshold", ch, thr).cpu().numpy(), ref)
    # the two older rules on the same tensors: their bytes and counts are what they were
    for rule in ("argmax", "sigmoid"):
        m, c = predict_masks(p.to(DEV), rule, ch, thr, target=target.to(DEV), ignore_index=255)
        old = mask_ref(p, rule, ch, thr)
        assert torch.equal(m.cpu(), old) and torch.equal(c.cpu(), counts_ref(old, target, ignore=255)), rule


# ------------------------------------------------------------------ 5. through the models
MODEL_CASES = ["unet", "stf", "stf_input"]
_CACHE = {}


def model_case(which):
    """(model, loader inputs [B, T, C, H, W], model inputs, targets): seeded weights, eval mode."""
    if which in _CACHE:
        return _CACHE[which]
    from stfunet import STFLSTMUNet, UNet
    from stfunet.engine import preprocess_input
    torch.manual_seed(0)
    g = torch.Generator().manual_seed(1)
    if which == "unet":
        model = UNet(8, 2, 8)
        raw = torch.randn(3, 8, 1, 32, 48, generator=g)
    else:
        model = STFLSTMUNet(time_steps=4, **({"output_size": "input"} if which == "stf_input" else {}))
        raw = torch.randn(2, 4, 1, 64, 96, generator=g)
    model = model.to(DEV).eval()
    raw = raw.to(DEV)
    x = preprocess_input(raw, model)
    with torch.no_grad():
        h, w = model(x)["out"].shape[-2:]
    assert (h, w) == ((32, 48) if which == "stf" else tuple(raw.shape[-2:]))
    targets = torch.randint(0, 2, (raw.shape[0], h, w), generator=g)
    targets[torch.rand(targets.shape, generator=g) < 0.05] = 255
    _CACHE[which] = (model, raw, x, targets.to(DEV))
    return _CACHE[which]


def restatement(which, rule, channel, views=VIEWS):
    key = (which, rule, channel, views)
    if key not in _CACHE:
        model, _, x, _ = model_case(which)
        with torch.no_grad():
            zs = [model(x.flip(DIMS[v]) if DIMS[v] else x)["out"].float().cpu().numpy() for v in views]
        _CACHE[key] = mean64(zs, views, rule, channel)
    return _CACHE[key]


def mask64(mean, bound, rule, thr):
    """(float64 mask, the pixels whose margin exceeds what the bound allows)."""
    if rule == "sigmoid":
        t = np.float64(np.float32(thr))
        return (mean[:, 0] > t).astype(np.uint8), np.abs(mean[:, 0] - t) > bound[:, 0]
    order = np.argsort(-mean, axis=1, kind="stable")
    top = np.take_along_axis(mean, order[:, :2], 1)
    b = np.take_along_axis(bound, order[:, :2], 1)
    return np.argmax(mean, 1).astype(np.uint8), (top[:, 0] - top[:, 1]) > (b[:, 0] + b[:, 1])


@pytest.mark.parametrize("rule", ["argmax", "sigmoid"])
@pytest.mark.parametrize("which", MODEL_CASES)
def test_models_probabilities_and_masks(which, rule):
    """tta_probabilities within ``bound64`` of the float64 restatement made from the model's own
    logits on torch.flip'ped inputs, and predict_tta's mask equal to the float64 mask wherever the
    float64 margin (top-1 minus top-2 of the mean; |mean - threshold| for "sigmoid") exceeds the
    bound of the elements compared.  At most 1 % of the pixels may be left out."""
    from stfunet import predict_tta, tta_probabilities
    model, raw, x, targets = model_case(which)
    thr, ch = 0.3, 1
    mean, bound = restatement(which, rule, ch)
    probs = tta_probabilities(model, x, True, rule, ch)
    assert probs.dtype == torch.float32 and tuple(probs.shape) == mean.shape
    assert report(f"model {which} {rule}", probs.cpu().numpy(), mean, bound) <= 1.0
    res = predict_tta(model, [(raw, targets)], DEV, tta=True, keep_probs=True, rule=rule, channel=ch, threshold=thr,
                      keep_masks=True, ignore_index=255)
    assert torch.equal(res["probs"][0].view(torch.int32), probs.view(torch.int32))
    ref, sure = mask64(mean, bound, rule, thr)
    left_out = 1.0 - sure.mean()
    print(f"[tta] model {which} {rule}: {100 * left_out:.3f} % of {sure.size} pixels inside the margin")
    assert left_out <= 0.01
    mask = res["masks"][0].cpu().numpy()
    assert mask.dtype == np.uint8 and np.array_equal(mask[sure], ref[sure])


@pytest.mark.parametrize("which", MODEL_CASES)
def test_models_exact_properties(which):
    from stfunet import boundary_metrics, filter_components, image_metrics, predict_tta
    from stfunet.predict import predict
    model, raw, x, targets = model_case(which)
    loader = [(raw, targets)]
    res = predict_tta(model, loader, DEV, keep_masks=True, keep_probs=True, ignore_index=255)
    mask = res["masks"][0]
    # dice / iou are image_metrics of the returned mask's counts
    counts = counts_ref(mask, targets, ignore=255)
    dice, iou = image_metrics(counts)
    assert torch.equal(res["dice"].cpu(), dice) and torch.equal(res["iou"].cpu(), iou)
    assert res["num"] == raw.shape[0]
    # the same bits from run to run
    again = predict_tta(model, loader, DEV, keep_masks=True, keep_probs=True, ignore_index=255)
    assert torch.equal(again["masks"][0], mask)
    assert torch.equal(again["probs"][0].view(torch.int32), res["probs"][0].view(torch.int32))
    # one view "none" runs the TTA path and agrees with the plain loop outside the margin
    mean, bound = restatement(which, "argmax", 0, ("none",))
    ref, sure = mask64(mean, bound, "argmax", 0.5)
    assert 1.0 - sure.mean() <= 0.01
    one = predict_tta(model, loader, DEV, tta=("none",), keep_masks=True, ignore_index=255)
    plain = predict(model, loader, DEV, keep_masks=True, ignore_index=255)
    assert set(plain) == {"num", "dice", "iou", "mean_dice", "mean_iou", "masks"}
    assert set(one) == set(plain) and set(res) == set(plain) | {"probs"}
    assert np.array_equal(one["masks"][0].cpu().numpy()[sure], plain["masks"][0].cpu().numpy()[sure])
    assert np.array_equal(plain["masks"][0].cpu().numpy()[sure], ref[sure])
    # the component filter and the boundary metrics see the TTA mask
    full = predict_tta(model, loader, DEV, keep_masks=True, ignore_index=255, keep_largest=True, boundary=True)
    fm, fc = filter_components(mask, keep_largest=True, target=targets, ignore_index=255)
    assert torch.equal(full["masks"][0], fm)
    d2, i2 = image_metrics(fc)
    assert torch.equal(full["dice"], d2) and torch.equal(full["iou"], i2)
    bm = boundary_metrics(fm, targets, 255)
    for k in ("hd", "hd95", "assd"):
        assert torch.equal(full[k].view(torch.int64), bm[k].view(torch.int64)), k


def test_training_mode_is_restored():
    from stfunet import tta_probabilities
    model, _, x, _ = model_case("unet")
    try:
        model.train()
        with torch.no_grad():
            before = {k: v.clone() for k, v in model.state_dict().items()}
        tta_probabilities(model, x, ("w",))
        assert model.training
        for k, v in model.state_dict().items():                    # eval forwards: no running statistic moved
            assert torch.equal(v, before[k]), k
        model.eval()
        tta_probabilities(model, x, ("w",))
        assert not model.training
    finally:
        model.eval()


def test_overlay_is_painted_on_the_unflipped_frame(tmp_path):
    from PIL import Image
    from stfunet import overlay, predict_tta
    from stfunet.predict import shown_frame
    model, raw, x, _ = model_case("unet")
    res = predict_tta(model, [raw], DEV, output_dir=str(tmp_path), keep_masks=True)
    pics = overlay(shown_frame(x), res["masks"][0]).cpu().numpy()
    for j, pic in enumerate(pics):
        assert np.array_equal(np.asarray(Image.open(os.path.join(tmp_path, f"unet_{j}.png"))), pic)


def test_launch_trace(monkeypatch):
    """With TTA off the loop issues the launches it issued before it knew of TTA: the forward's and
    one stf_predict_mask.  With it, per view one flip (none for "none"), the forward's and one
    accumulate, then one mask launch."""
    from _launch_trace import tracing
    from stfunet import predict_tta
    from stfunet.predict import predict
    monkeypatch.setenv("STF_PLAN", "0")
    model, raw, x, targets = model_case("unet")
    loader = [(raw, targets)]
    with torch.no_grad(), tracing() as fwd:
        model(x)
    fwd = list(fwd)
    assert fwd and not any(n in fwd for n in ("stf_predict_mask", "stf_flip_planes", "stf_tta_accumulate"))
    with tracing() as t:
        predict(model, loader, DEV)
    assert list(t) == fwd + ["stf_predict_mask"]
    with tracing() as t:
        predict_tta(model, loader, DEV, tta=None)
    assert list(t) == fwd + ["stf_predict_mask"]
    with tracing() as t:
        predict_tta(model, loader, DEV)
    want = fwd + ["stf_tta_accumulate"]
    for _ in range(3):
        want += ["stf_flip_planes"] + fwd + ["stf_tta_accumulate"]
    assert list(t) == want + ["stf_predict_mask"]
    with tracing() as t:
        predict_tta(model, loader, DEV, tta=("h", "none"), rule="sigmoid")
    assert list(t) == ["stf_flip_planes"] + fwd + ["stf_tta_accumulate"] + fwd + ["stf_tta_accumulate",
                                                                                 "stf_predict_threshold"]
    torch.cuda.synchronize()
