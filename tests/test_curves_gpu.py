"""Score histograms and threshold curves on the GPU (csrc/curves.hip through the C entry point and
stfunet.predict) against the numpy restatement of tests/_curves_ref.py, which tests/test_curves_cpu.py pins
to tests/golden/curves.npz.

The histogram is integers, so every comparison of it is equality, element for element.  The float64 curves
are compared exactly where they are elementwise (Dice, IoU, the best point) and within 1e-12 where a sum of
at most 4097 terms in [0, 1] may be taken in another order (4097 * 2^-53 < 5e-13).

The kernel-level tests call the C entry point on a histogram with 64 guard bytes on each side and run every
case twice, the buffer prefilled with 0xAA and then with 0xFF: equal results show that every output byte is
written, that nothing is read before it is written and that two runs agree bit for bit; the guards must
keep their fill.
"""
import numpy as np
import pytest
import torch

import _curves_ref as ref
import _launch_trace as lt

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
EINVAL = 100001
SOURCE = {"softmax": 0, "sigmoid": 1, "probs": 2}
SHAPES = [(1, 1), (1, 3), (3, 5), (4, 8), (17, 23), (64, 64)]


class Guarded:
    """``nbytes`` of device memory between two guards, everything prefilled with ``fill``."""

    def __init__(self, nbytes, fill):
        self.fill, self.n = fill, nbytes
        self.raw = torch.full((nbytes + 2 * GUARD,), fill, dtype=torch.uint8, device=DEV)
        self.body = self.raw[GUARD:GUARD + nbytes]
        assert self.raw.data_ptr() % 64 == 0

    def guards_intact(self):
        return bool((self.raw[:GUARD] == self.fill).all() and (self.raw[GUARD + self.n:] == self.fill).all())

    def ptr(self):
        return self.body.data_ptr()


def _scores_on_device(scores, offset):
    """fp32 [N, K, H, W] on the device, its base 16-B aligned or (``offset``) 4 bytes past that."""
    flat = torch.from_numpy(np.ascontiguousarray(scores, np.float32)).reshape(-1)
    buf = torch.empty(flat.numel() + 4, dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    view = buf[1:1 + flat.numel()] if offset else buf[:flat.numel()]
    view.copy_(flat)
    return buf, view


def run(scores, target, source, channel, bins, positive=None, ignore=None, fill=0xAA, offset=False):
    """One stf_score_hist call on a guarded histogram: int64 [N, 2, bins + 1]."""
    from stfunet import _lib
    N, K, H, W = scores.shape
    keep, src = _scores_on_device(scores, offset)
    t = torch.from_numpy(np.ascontiguousarray(target, np.int64)).to(DEV)
    hist = Guarded(N * 2 * (bins + 1) * 8, fill)
    _lib.call("stf_score_hist", src.data_ptr(), N, K, H, W, SOURCE[source], channel, t.data_ptr(),
              -1 if positive is None else positive, -1 if ignore is None else ignore, bins, hist.ptr(), _lib.stream())
    torch.cuda.synchronize()
    assert hist.guards_intact()
    return hist.body.cpu().numpy().view(np.int64).reshape(N, 2, bins + 1)


def check(scores, target, channel, bins, positive=None, ignore=None, offset=False, want=None):
    """Two runs on planes of probabilities, the second on a buffer poisoned with 0xFF, agree byte for byte and
    equal the restatement (or ``want``)."""
    scores = np.asarray(scores, np.float32)
    if scores.ndim == 3:
        scores = scores[:, None]
    first = run(scores, target, "probs", channel, bins, positive, ignore, 0xAA, offset)
    second = run(scores, target, "probs", channel, bins, positive, ignore, 0xFF, offset)
    assert first.tobytes() == second.tobytes()
    if want is None:
        want = ref.histogram(scores[:, channel], target, bins, positive, ignore)
    assert np.array_equal(first, want)
    return first


# ---------------------------------------------------------------- the named cases
@pytest.mark.parametrize("c", ref.cases(), ids=[c["name"] for c in ref.cases()])
def test_cases_equal_the_fixture_and_the_restatement(c):
    got = check(c["scores"], c["target"], 0, c["bins"], c["positive"], c["ignore"])
    assert np.array_equal(got.sum(0), ref.fixture()[c["name"]][0])


# ---------------------------------------------------------------- shapes and paths
@pytest.mark.parametrize("H,W", SHAPES, ids=[f"{h}x{w}" for h, w in SHAPES])
def test_shapes_batches_and_both_paths(H, W):
    """HW % 4 != 0 and a base 4 bytes off take the scalar path, the rest the quad path."""
    for N in (1, 3, 5):
        rng = np.random.default_rng(1000 * H + 10 * W + N)
        s = rng.random((N, 2, H, W)).astype(np.float32)
        t = rng.integers(0, 2, (N, H, W))
        t[rng.random(t.shape) < 0.1] = 255
        for offset in (False, True):
            got = check(s, t, 1, 16, None, 255, offset)
            assert got.sum() == (t != 255).sum()


@pytest.mark.parametrize("bins", (256, 4096))
def test_many_blocks_flush_into_one_image(bins):
    rng = np.random.default_rng(bins)
    s = rng.random((1, 1, 256, 256)).astype(np.float32)
    t = (rng.random((1, 256, 256)) < s[:, 0]).astype(np.int64)
    for offset in (False, True):
        assert check(s, t, 0, bins, offset=offset).sum() == 256 * 256


# ---------------------------------------------------------------- scores
@pytest.mark.parametrize("bins", ref.BINS)
def test_row_rule_on_edges_and_special_values(bins):
    e = ref.edge_scores(bins)
    few = e if bins <= 256 else np.concatenate([e[::61], e[-14:]])    # bounds the [N, 2, bins + 1] table below
    e = np.concatenate([e, np.full(-len(e) % 4, 0.5, np.float32)])
    t = (np.arange(e.size) % 2).reshape(1, -1, 4)
    for offset in (False, True):
        check(e.reshape(1, 1, -1, 4), t, 0, bins, offset=offset)
    # one pixel per image: the histogram names the row
    got = check(few.reshape(-1, 1, 1, 1), np.ones((few.size, 1, 1), np.int64), 0, bins)
    assert np.array_equal(got[:, 1].argmax(1), ref.rows(few, bins)) and (got.sum((1, 2)) == 1).all()
    assert got[-14:, 1].argmax(1).tolist() == ref.special_rows(bins)


@pytest.mark.parametrize("bins", ref.BINS)
def test_uniform_and_end_row_scores(bins):
    rng = np.random.default_rng(7 + bins)
    t = rng.integers(0, 2, (2, 40, 52))
    check(rng.random((2, 1, 40, 52)), t, 0, bins)
    zero = check(np.where(rng.random((2, 1, 40, 52)) < 0.5, 0.0, -1.0), t, 0, bins)     # the register path alone
    assert zero[:, :, 1:].sum() == 0 and zero[:, :, 0].sum() == t.size
    top = check(np.where(rng.random((2, 1, 40, 52)) < 0.5, 1.0, np.inf), t, 0, bins)
    assert top[:, :, :-1].sum() == 0 and top[:, :, -1].sum() == t.size
    check(ref._trained_like(rng, (2, 1, 40, 52)), t, 0, bins)


# ---------------------------------------------------------------- targets
def test_positive_class_ignore_and_one_sided_targets():
    from stfunet import threshold_curves
    rng = np.random.default_rng(3)
    s = rng.random((3, 3, 17, 23)).astype(np.float32)
    t = rng.integers(0, 3, (3, 17, 23))
    t[1, 4] = 255
    for positive in (None, 0, 1, 2):
        for ignore in (None, 255, 1):
            for ch in (0, 2):
                check(s, t, ch, 16, positive, ignore)
    for fill, empty in ((0, 1), (1, 0)):
        got = check(s, np.full_like(t, fill), 1, 16)
        assert got[:, empty].sum() == 0
        c = threshold_curves(torch.from_numpy(got).to(DEV))
        assert bool(torch.isnan(c["auroc"]).all()) and bool(torch.isnan(c["average_precision"]).all())
        assert not bool(torch.isnan(c["dice"]).any())


def test_rows_above_j_are_the_threshold_rule_counts():
    """bins = 16, every j: TP_j / FP_j equal what stf_predict_threshold counts at j / 16 on the same plane."""
    from stfunet import predict_masks, score_histogram, threshold_curves
    rng = np.random.default_rng(16)
    e = ref.edge_scores(16)
    e = e[~(e > 1)]                                                # the identity is stated for p <= 1
    plane = np.concatenate([e, rng.random(17 * 23 * 2 - e.size).astype(np.float32)]).reshape(2, 1, 17, 23)
    t = rng.integers(0, 2, (2, 17, 23))
    t[0, 3] = 255
    s, T = torch.from_numpy(plane).to(DEV), torch.from_numpy(t).to(DEV)
    c = threshold_curves(score_histogram(s, T, bins=16, ignore_index=255))
    for j in range(17):
        _, counts = predict_masks(s, "threshold", 0, j / 16, target=T, ignore_index=255)
        assert torch.equal(c["tp"][:, j], counts[:, 0]) and torch.equal(c["tp"][:, j] + c["fp"][:, j], counts[:, 1])
        assert torch.equal(c["tp"][:, j] + c["fn"][:, j], counts[:, 2])


# ---------------------------------------------------------------- sources 0 and 1
@pytest.mark.parametrize("K", (1, 2, 3, 5, 9, 16))
def test_logit_sources_equal_the_accumulate_pass_bit_for_bit(K):
    """softmax / sigmoid histograms equal the source-2 histogram of stf_tta_accumulate's plane for the single
    view "none": the same arithmetic, divided by 1."""
    from stfunet._lib import call, stream
    rng = np.random.default_rng(K)
    for (N, H, W), offset in (((2, 12, 16), False), ((3, 7, 9), False), ((2, 12, 16), True)):
        z = (rng.standard_normal((N, K, H, W)) * 4).astype(np.float32)
        z[0, 0, 0, 0], z[0, K - 1, 0, 1], z[0, 0, 0, 2], z[0, 0, 1, 0] = np.inf, -np.inf, np.nan, 90.0
        t = rng.integers(0, 2, (N, H, W))
        zd = torch.from_numpy(z).to(DEV)
        for rule, source in ((0, "softmax"), (1, "sigmoid")):
            for ch in sorted({0, K - 1}):
                acc = torch.full((N, K if rule == 0 else 1, H, W), float("nan"), device=DEV)
                call("stf_tta_accumulate", zd.data_ptr(), N, K, H, W, rule, ch, 0, 1, 1, acc.data_ptr(), stream())
                plane = acc[:, ch if rule == 0 else 0].cpu().numpy()
                for bins in (16, 4096):
                    want = ref.histogram(plane, t, bins)
                    a = run(z, t, source, ch, bins, fill=0xAA, offset=offset)
                    b = run(z, t, source, ch, bins, fill=0xFF, offset=offset)
                    assert a.tobytes() == b.tobytes() and np.array_equal(a, want)


# ---------------------------------------------------------------- depths
def test_depths_sum_the_slices_of_each_volume():
    from stfunet import score_histogram
    rng = np.random.default_rng(5)
    s = rng.random((6, 2, 9, 13)).astype(np.float32)
    t = rng.integers(0, 2, (6, 9, 13))
    S, T = torch.from_numpy(s).to(DEV), torch.from_numpy(t).to(DEV)
    per_image = ref.histogram(s[:, 1], t, 16)
    assert np.array_equal(score_histogram(S, T, channel=1, bins=16).cpu().numpy(), per_image)
    stack = score_histogram(S, T, channel=1, bins=16, depths=[2, 1, 3])
    assert stack.dtype == torch.int64 and np.array_equal(stack.cpu().numpy(), ref.by_volume(per_image, [2, 1, 3]))
    assert stack.sum((1, 2)).tolist() == [2 * 117, 117, 3 * 117]
    at = 0
    for v, d in enumerate((2, 1, 3)):                               # a volume alone: the same bits
        alone = score_histogram(S[at:at + d], T[at:at + d], channel=1, bins=16, depths=[d])
        assert torch.equal(alone, stack[v:v + 1])
        at += d
    one = score_histogram(S[:1], T[:1], channel=1, bins=16, depths=[1])
    assert np.array_equal(one.cpu().numpy(), per_image[:1])
    assert tuple(score_histogram(S[:0], T[:0], bins=16).shape) == (0, 2, 17)
    assert np.array_equal(score_histogram(S[:, 1], T, bins=16).cpu().numpy(), per_image)               # one plane
    assert np.array_equal(score_histogram({"out": S}, T, channel=1, bins=16).cpu().numpy(), per_image)


# ---------------------------------------------------------------- curves on the device
def test_threshold_curves_equal_the_restatement():
    from stfunet import threshold_curves
    for c in ref.cases():
        hist = ref.histogram(c["scores"], c["target"], c["bins"], c["positive"], c["ignore"])
        groups = min(16, c["bins"])
        got = threshold_curves(torch.from_numpy(hist).to(DEV), groups)
        assert all(v.is_cuda for v in got.values())
        for n in range(hist.shape[0]):
            want = ref.curves(hist[n], groups)
            for k in ("tp", "fp", "fn", "tn", "dice", "iou", "best_threshold", "best_dice"):
                assert np.array_equal(got[k][n].cpu().numpy(), want[k]), (c["name"], k)
            for k in ("auroc", "average_precision", "ece", "reliability"):
                g = got[k][n].cpu().numpy()
                assert np.allclose(g, want[k], rtol=0, atol=1e-12, equal_nan=True), (c["name"], k)
                assert np.array_equal(np.isnan(g), np.isnan(want[k])), (c["name"], k)
        pooled = threshold_curves(torch.from_numpy(hist.sum(0)).to(DEV), groups)
        _, auroc, ap = ref.fixture()[c["name"]]
        assert np.allclose(pooled["auroc"].item(), auroc, rtol=0, atol=1e-12, equal_nan=True)
        assert np.allclose(pooled["average_precision"].item(), ap, rtol=0, atol=1e-12, equal_nan=True)


# ---------------------------------------------------------------- refusals
def test_c_abi_refusals_leave_the_histogram_untouched():
    from stfunet import _lib
    lib = _lib.load()
    N, K, H, W, bins = 2, 3, 4, 5, 16
    src = torch.rand(N, K, H, W, device=DEV)
    t = torch.zeros(N, H, W, dtype=torch.int64, device=DEV)
    hist = Guarded(N * 2 * (bins + 1) * 8, 0xAA)
    good = dict(src=src.data_ptr(), N=N, K=K, H=H, W=W, source=0, channel=1, target=t.data_ptr(), positive=-1,
                ignore=-1, bins=bins, hist=hist.ptr())

    def call(**kw):
        a = dict(good, **kw)
        return lib.stf_score_hist(a["src"], a["N"], a["K"], a["H"], a["W"], a["source"], a["channel"], a["target"],
                                  a["positive"], a["ignore"], a["bins"], a["hist"], _lib.stream())

    for kw in ([dict(bins=b) for b in (3, 8192, 0, 1, -16)] + [dict(K=17), dict(K=0), dict(channel=K), dict(channel=-1),
               dict(src=None), dict(target=None), dict(hist=None), dict(source=3), dict(N=0), dict(H=0), dict(W=4097),
               dict(N=1 << 20, H=64, W=64), dict(target=t.data_ptr() + 4), dict(hist=hist.ptr() + 4)]):
        assert call(**kw) == EINVAL, kw
    torch.cuda.synchronize()
    assert bool((hist.raw == 0xAA).all())
    assert call() == 0                                              # and the good call is taken
    torch.cuda.synchronize()
    assert hist.guards_intact() and int(hist.body.view(torch.int64).sum()) == N * H * W


def test_python_refusals_come_before_device_work():
    from stfunet import score_histogram
    s = torch.rand(2, 3, 4, 5, device=DEV)
    t = torch.zeros(2, 4, 5, dtype=torch.int64, device=DEV)
    with lt.tracing() as trace:
        for kw in (dict(bins=3), dict(bins=8192), dict(bins=0), dict(channel=3), dict(source="logits"),
                   dict(positive=-1), dict(depths=[3]), dict(target=t[:1]), dict(target=t.float())):
            with pytest.raises(ValueError):
                score_histogram(s, kw.pop("target", t), **kw)
        with pytest.raises(ValueError):
            score_histogram(torch.rand(2, 17, 4, 5, device=DEV), t)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            score_histogram(s.cpu(), t)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            score_histogram(s, t.cpu())
        assert list(trace) == []


# ---------------------------------------------------------------- the predict loops
def _unet_and_loader():
    from oracle.cases import dce_case
    from oracle.init import canonical_state_dict
    from stfunet.unet import UNet
    model = UNet(in_channels=8, num_classes=2, base_c=16)
    model.load_state_dict(canonical_state_dict(model.state_dict(), seed=0))
    loader = [dce_case(500 + i, 3, 8, 32, 32) for i in range(2)]
    loader[1][1][1].zero_()                                        # image 4 of 6: an empty target
    loader[0][1][0, :, 28:] = 255
    return model.to(DEV), loader


def _names(trace):
    return [e if isinstance(e, str) else e[0] for e in trace]


def _check_curve_keys(res, hist):
    """The loop's curve keys against the restatement on the histogram ``hist`` (numpy, per image or case)."""
    from stfunet.predict import CURVE_KEYS
    assert all(k in res for k in CURVE_KEYS)
    assert res["score_hist"].dtype == torch.int64 and np.array_equal(res["score_hist"].cpu().numpy(), hist)
    per = [ref.curves(h) for h in hist]
    pooled = ref.curves(hist.sum(0))
    for k in ("tp", "fp", "fn", "tn", "dice", "iou", "best_threshold", "best_dice"):
        assert np.array_equal(res["curves"][k].cpu().numpy(), pooled[k]), k
    for k in ("auroc", "average_precision", "ece"):
        assert np.allclose(res["curves"][k].item(), pooled[k], rtol=0, atol=1e-12, equal_nan=True), k
    for k, r in (("case_auroc", "auroc"), ("case_average_precision", "average_precision")):
        assert np.allclose(res[k].cpu().numpy(), [p[r] for p in per], rtol=0, atol=1e-12, equal_nan=True), k
    mean = np.stack([p["dice"] for p in per]).mean(0)
    assert np.allclose(res["mean_case_dice_curve"].cpu().numpy(), mean, rtol=0, atol=1e-12)
    assert float(res["best_case_threshold"]) in pooled["thresholds"]
    got = res["mean_case_dice_curve"]
    assert float(res["best_case_threshold"]) == float(pooled["thresholds"][int((got == got.max()).nonzero()[0])])


def test_the_loops_report_the_histogram_of_the_probabilities_they_keep():
    from stfunet import predict_volumes, score_histogram
    from stfunet.predict import predict, predict_tta
    model, loader = _unet_and_loader()
    dev = torch.device(DEV)
    T = torch.cat([t for _, t in loader]).to(DEV)
    old = set(predict(model, loader, dev))
    assert old == {"num", "dice", "iou", "mean_dice", "mean_iou"}
    for views in (("none", "w"), ("none",)):
        for rule, channel, plane in (("argmax", 0, 1), ("sigmoid", 1, 0)):
            res = predict_tta(model, loader, dev, tta=views, keep_probs=True, curves=True, rule=rule, channel=channel,
                              ignore_index=255, keep_largest=True)
            want = score_histogram(torch.cat(res["probs"]), T, "probs", plane, 256, ignore_index=255).cpu().numpy()
            _check_curve_keys(res, want)
            assert want[:, :, 1:-1].sum() > 0 and want.sum() == (T != 255).sum()
            if views == ("none",):                                 # the plain loop scores the logits: the same bits
                plain = predict_tta(model, loader, dev, tta=None, curves=True, rule=rule, channel=channel,
                                    ignore_index=255)
                assert np.array_equal(plain["score_hist"].cpu().numpy(), want)
                assert set(plain) == old | set(res) - {"probs", "num_components"}
                for depths in ((1, 3, 2), (6,), (3, 3)):
                    vol = predict_volumes(model, loader, dev, depths, curves=True, rule=rule, channel=channel,
                                          ignore_index=255)
                    _check_curve_keys(vol, ref.by_volume(want, depths))
            else:
                vol = predict_volumes(model, loader, dev, (1, 3, 2), tta=views, curves=True, curve_bins=16, rule=rule,
                                      channel=channel, ignore_index=255, keep_largest=True)
                want16 = score_histogram(torch.cat(res["probs"]), T, "probs", plane, 16, ignore_index=255)
                _check_curve_keys(vol, ref.by_volume(want16.cpu().numpy(), (1, 3, 2)))
    bare = predict_tta(model, [x for x, _ in loader], dev, tta=None, curves=True)
    assert bare["score_hist"] is None and bare["curves"] is None and bare["best_case_threshold"] is None


def test_one_histogram_launch_per_batch_and_none_by_default():
    from stfunet import predict_volumes
    from stfunet.predict import predict, predict_tta
    model, loader = _unet_and_loader()
    dev = torch.device(DEV)

    def traced(fn, *args, **kw):
        with lt.tracing() as trace:
            res = fn(model, loader, dev, *args, **kw)
            torch.cuda.synchronize()
            return _names(trace), set(res)

    predict(model, loader, dev)                                     # the first forward packs the weights: once
    base, keys = traced(predict)
    assert "stf_score_hist" not in base
    for fn, args, kw in ((predict_tta, (), dict(tta=None)), (predict_tta, (), dict(tta=("none", "h"))),
                         (predict_volumes, ((1, 3, 2),), dict()), (predict_volumes, ((1, 3, 2),), dict(keep_largest=True))):
        off, off_keys = traced(fn, *args, **kw)
        assert "stf_score_hist" not in off and not any("curve" in k or "score_hist" in k for k in off_keys)
        if fn is predict_tta and kw["tta"] is None:
            assert off == base and off_keys == keys                 # the default call: the old keys, the old launches
        on, on_keys = traced(fn, *args, curves=True, **kw)
        assert on.count("stf_score_hist") == len(loader)
        assert [e for e in on if e != "stf_score_hist"] == off
        assert on_keys - off_keys == {"score_hist", "curves", "case_auroc", "case_average_precision",
                                      "mean_case_dice_curve", "best_case_threshold"}
