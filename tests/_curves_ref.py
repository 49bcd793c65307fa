"""numpy restatement of the score histogram and the threshold curves (tests only; nothing but numpy is
imported), in float32 / int64 for the histogram and float64 for the curves.

    row(p) = 0                                            if not (p > 0)     (0, -0, negatives, NaN)
           = min(bins, int(ceil(float32(p) * float32(bins))))  otherwise     (+inf and p > 1: row bins)
    hist[n, s, r] = pixels of image n with row r on side s; side 1 is target > 0 (positive None) or
    target == positive, side 0 every other pixel; target == ignore (>= 0) is in neither.

``tests/golden/curves.npz`` (make_golden_curves.py: rows by counting thresholds in float64, AUROC and
average precision by scikit-learn on the rows) pins it on ``cases()``.
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BINS = (2, 16, 256, 4096)


def rows(p, bins):
    """int64 rows of the float32 scores ``p``."""
    p = np.asarray(p, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        c = np.minimum(np.ceil(p * np.float32(bins)), np.float32(bins))      # float32 throughout
        return np.where(p > 0, c, np.float32(0)).astype(np.int64)            # a NaN compares false


def histogram(scores, target, bins, positive=None, ignore=None):
    """int64 [N, 2, bins + 1] of scores float32 [N, H, W] (probabilities already) and target [N, H, W]."""
    scores, target = np.asarray(scores, np.float32), np.asarray(target, np.int64)
    N = scores.shape[0]
    hist = np.zeros((N, 2, bins + 1), np.int64)
    for n in range(N):
        r, t = rows(scores[n], bins).ravel(), target[n].ravel()
        keep = np.ones(t.shape, bool) if ignore is None or ignore < 0 else t != ignore
        side = (t > 0) if positive is None else (t == positive)
        for s in (0, 1):
            hist[n, s] = np.bincount(r[keep & (side == bool(s))], minlength=bins + 1)
    return hist


def by_volume(hist, depths):
    at = np.concatenate([[0], np.cumsum(depths)])
    return np.stack([hist[a:b].sum(0) for a, b in zip(at[:-1], at[1:])])


def sigmoid(x):
    """torch.sigmoid in fp32, one rounding per operation: 1 / (1 + expf(-x)) (expf by numpy's float32 exp
    is not the device's: use only where the result is far from a row edge)."""
    x = np.asarray(x, np.float32)
    return (np.float32(1) / (np.float32(1) + np.exp(-x))).astype(np.float32)


def first_max(v):
    return int(np.flatnonzero(v == v.max())[0]) if not np.isnan(v).any() else len(v) - 1


def curves(hist, cal_groups=None, smooth=1e-5):
    """The dict of stfunet.predict.threshold_curves for one table ``hist`` int64 [2, bins + 1], in float64
    (``cal_groups`` None: 16, or ``bins`` below that)."""
    hist = np.asarray(hist, np.int64)
    bins = hist.shape[1] - 1
    cal_groups = min(16, bins) if cal_groups is None else cal_groups
    total = hist.sum(1)
    above = total[:, None] - np.cumsum(hist, 1)
    fp, tp = above
    n_neg, n_pos = total
    fn, tn = n_pos - tp, n_neg - fp
    f = np.float64
    inter, p, t = tp.astype(f), (tp + fp).astype(f), (tp + fn).astype(f)
    dice = (2 * inter + smooth) / (p + t + smooth)
    iou = (inter + smooth) / (p + t - inter + smooth)
    thresholds = np.arange(bins + 1, dtype=f) / bins
    best = first_max(dice)
    with np.errstate(invalid="ignore", divide="ignore"):
        tpr, fpr = tp.astype(f) / f(n_pos), fp.astype(f) / f(n_neg)
        x, y = np.concatenate([[1.0], fpr]), np.concatenate([[1.0], tpr])
        auroc = ((x[:-1] - x[1:]) * (y[:-1] + y[1:])).sum() * 0.5
        at = np.cumsum(hist[:, ::-1], 1).astype(f)
        fp_k, tp_k = at
        recall = tp_k / f(n_pos)
        precision = np.where(tp_k + fp_k > 0, tp_k / np.maximum(tp_k + fp_k, 1), 1.0)
        ap = ((recall - np.concatenate([[0.0], recall[:-1]])) * precision).sum()
        if n_pos == 0 or n_neg == 0:
            auroc = ap = f("nan")
        G = cal_groups
        rows_ = hist.sum(0).astype(f)
        conf = (np.arange(1, bins + 1, dtype=f) - 0.5) / bins
        count = rows_[1:].reshape(G, bins // G).sum(1)
        count[0] += rows_[0]
        conf_sum = (rows_[1:] * conf).reshape(G, bins // G).sum(1)
        pos_sum = hist[1, 1:].astype(f).reshape(G, bins // G).sum(1)
        pos_sum[0] += hist[1, 0]
        mean_conf, pos_frac = conf_sum / count, pos_sum / count
        gap = np.where(count > 0, count * np.abs(pos_frac - mean_conf), 0.0)
        ece = gap.sum() / count.sum()
    return {"thresholds": thresholds, "tp": tp, "fp": fp, "fn": fn, "tn": tn, "dice": dice, "iou": iou,
            "best_threshold": thresholds[best], "best_dice": dice[best], "auroc": auroc, "average_precision": ap,
            "reliability": np.stack([count, mean_conf, pos_frac], 1), "ece": ece}


def edge_scores(bins):
    """float32: every j / bins with both nextafter neighbours, and the special values of the row rule."""
    e = (np.arange(bins + 1, dtype=np.float32) / np.float32(bins)).astype(np.float32)
    lo, hi = np.nextafter(e, np.float32(-np.inf)), np.nextafter(e, np.float32(np.inf))
    tiny = np.float32(1e-45)                                        # the smallest denormal
    special = np.array([0.0, -0.0, -1.0, -tiny, np.nan, np.inf, -np.inf, 1.0, 1.5, 3e38, tiny, 1e-40, 1.1754942e-38,
                        np.float32(1.1754944e-38)], np.float32)
    return np.concatenate([e, lo, hi, special]).astype(np.float32)


def special_rows(bins):
    """The rows the special values of ``edge_scores`` must land in, in its order."""
    return [0, 0, 0, 0, 0, bins, 0, bins, bins, bins, 1, 1, 1, 1]


def _trained_like(rng, shape, frac=0.97):
    """Scores of a trained lesion model: ``frac`` of the pixels in the end rows (exact 0 / 1 and beyond)."""
    u = rng.random(shape).astype(np.float32)
    ends = rng.random(shape)
    u = np.where(ends < frac * 0.9, np.float32(0), u)
    return np.where(ends > 1 - frac * 0.1, np.float32(1), u).astype(np.float32)


def cases():
    """Named (scores float32 [N, H, W], target int64 [N, H, W], bins, positive, ignore) cases of the fixture."""
    out = []
    rng = np.random.default_rng(20251021)
    for bins in BINS:
        s = rng.random((2, 17, 23)).astype(np.float32)
        t = (rng.random((2, 17, 23)) < 0.3 * s + 0.1).astype(np.int64)
        out.append(dict(name=f"uniform_b{bins}", scores=s, target=t, bins=bins, positive=None, ignore=None))
    e = edge_scores(16)
    e = np.concatenate([e, np.zeros(-len(e) % 8, np.float32)]).reshape(1, -1, 8)
    out.append(dict(name="edges_b16", scores=e, target=(np.arange(e.size).reshape(e.shape) % 3 == 0).astype(np.int64),
                    bins=16, positive=None, ignore=None))
    s = _trained_like(rng, (3, 16, 16))
    t = (s > 0.4).astype(np.int64)
    t[rng.random(t.shape) < 0.05] ^= 1
    out.append(dict(name="trained_like", scores=s, target=t, bins=256, positive=None, ignore=None))
    t3 = rng.integers(0, 3, (2, 9, 11)).astype(np.int64)
    t3[0, :, 5] = 255
    s3 = rng.random((2, 9, 11)).astype(np.float32)
    out.append(dict(name="positive_2_ignore_255", scores=s3, target=t3, bins=16, positive=2, ignore=255))
    out.append(dict(name="ignore_255", scores=s3, target=t3, bins=16, positive=None, ignore=255))
    out.append(dict(name="all_negative", scores=s3, target=np.zeros_like(t3), bins=16, positive=None, ignore=None))
    out.append(dict(name="all_positive", scores=s3, target=np.ones_like(t3), bins=16, positive=None, ignore=None))
    out.append(dict(name="separable", scores=np.where(t3 > 0, np.float32(0.9), np.float32(0.1)), target=t3, bins=16,
                    positive=None, ignore=None))
    return out


def fixture():
    """name -> (hist int64 [2, bins + 1] pooled over the case's images, auroc, average_precision)."""
    with np.load(os.path.join(GOLDEN, "curves.npz")) as z:
        names = [str(n) for n in z["names"]]
        return {n: (z[f"hist_{i}"], float(z["auroc"][i]), float(z["ap"][i])) for i, n in enumerate(names)}
