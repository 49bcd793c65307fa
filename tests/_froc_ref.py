"""numpy restatement of lesion confidence and FROC (tests only; nothing but numpy is imported), built on
``label`` / ``split`` of tests/_components3d_ref.py, ``sides`` / ``volume_metrics`` of tests/_lesion_ref.py and
``rows`` of tests/_curves_ref.py.

Per volume ``[D, H, W]`` (an image is a volume one slice deep), with P, T, the labelling and the matched
rule of tests/_lesion_ref.py and ``row(p)`` of tests/_curves_ref.py on the score plane:

    conf(c) = max row(p) over the voxels of candidate c (a component of P)
    det(t)  = max conf(c) over the MATCHED candidates that share a voxel with lesion t; 0 without one
    summary int64 [4]                  = tests/_lesion_ref.py's
    table   int64 [2, max_lesions, 3]  = its (area, hit) and a third column: det on side 0, conf on side 1
    hist    int64 [3, bins + 1]        : side 0 the unmatched candidates by conf, side 1 the lesions by
                                         det, side 2 the matched candidates by conf

``tests/golden/froc.npz`` (make_golden_froc.py: the same with scipy's labels) holds ``cases()`` with their
inputs.  Scores are probabilities that are exact multiples of ``1 / (2 bins)``, so no case hangs on an ulp.
"""
import os

import numpy as np

from _components3d_ref import FLAT, label, split
from _curves_ref import rows
from _lesion_ref import TO_3D, sides, volume_metrics

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RATES = (0.125, 0.25, 0.5, 1, 2, 4, 8)


def volume_froc(mask, scores, target, bins=256, connectivity=26, min_overlap=0.0, max_lesions=64, ignore=None,
                labeller=label):
    """(summary int64 [4], table int64 [2, max_lesions, 3], hist int64 [3, bins + 1]) of one volume."""
    summary, two = volume_metrics(mask, target, connectivity, min_overlap, max_lesions, ignore, labeller)
    T, P = sides(mask, target, ignore)
    row = rows(scores, bins)
    lt, n_t = labeller(T, connectivity)
    lp, n_p = labeller(P, connectivity)
    conf = np.zeros(n_p, np.int64)
    np.maximum.at(conf, lp[P] - 1, row[P])
    area = np.bincount(lp.ravel(), minlength=n_p + 1)[1:].astype(np.int64)
    hit = np.bincount(lp[T].ravel(), minlength=n_p + 1)[1:].astype(np.int64)
    matched = (hit >= 1) & (hit.astype(np.float64) >= np.float64(min_overlap) * area.astype(np.float64))
    det = np.zeros(n_t, np.int64)
    both = T & P
    c, t = lp[both] - 1, lt[both] - 1
    np.maximum.at(det, t[matched[c]], conf[c[matched[c]]])
    table = np.zeros((2, max_lesions, 3), np.int64)
    table[:, :, :2] = two
    table[0, :min(n_t, max_lesions), 2] = det[:max_lesions]
    table[1, :min(n_p, max_lesions), 2] = conf[:max_lesions]
    hist = np.stack([np.bincount(conf[~matched], minlength=bins + 1), np.bincount(det, minlength=bins + 1),
                     np.bincount(conf[matched], minlength=bins + 1)]).astype(np.int64)
    return summary, table, hist


def stack_froc(mask, scores, target, depths=None, bins=256, connectivity=26, min_overlap=0.0, max_lesions=64,
               ignore=None, labeller=label):
    """(summary [V, 4], table [V, 2, max_lesions, 3], hist [V, 3, bins + 1]) of a stack of volumes."""
    res = [volume_froc(m, s, t, bins, connectivity, min_overlap, max_lesions, ignore, labeller)
           for m, s, t in zip(split(mask, depths), split(scores, depths), split(target, depths))]
    return tuple(np.stack([r[k] for r in res]) for k in range(3))


def image_froc(mask, scores, target, bins=256, connectivity=8, min_overlap=0.0, max_lesions=64, ignore=None,
               labeller=label):
    """The same per image of a batch ``[B, H, W]`` at connectivity 4 or 8."""
    return stack_froc(mask, scores, target, [1] * len(mask), bins, TO_3D[connectivity], min_overlap, max_lesions,
                      ignore, labeller)


def curves(hist, cases=None, rates=RATES):
    """``froc_curves`` in numpy: hist [3, bins + 1] (cases default 1) or [V, 3, bins + 1] (pooled, default V)."""
    hist = np.asarray(hist, np.int64)
    if hist.ndim == 3:
        cases = hist.shape[0] if cases is None else cases
        hist = hist.sum(0)
    cases = 1 if cases is None else cases
    bins = hist.shape[-1] - 1
    total = hist.sum(-1, keepdims=True)
    false, detected, matched = total - np.cumsum(hist, -1)
    n = total[1, 0]
    with np.errstate(invalid="ignore", divide="ignore"):
        sens = detected.astype(np.float64) / np.float64(n)
        predicted = (matched + false).astype(np.float64)
        precision = np.where(predicted > 0, matched.astype(np.float64) / predicted, 1.0)
    at = []
    for r in rates:
        ok = false.astype(np.float64) <= np.float64(r) * np.float64(cases)
        at.append(sens[int(np.argmax(ok))])                     # the smallest j that qualifies; j = bins always does
    at = np.array(at, np.float64)
    return {"thresholds": np.arange(bins + 1, dtype=np.float64) / bins, "detected": detected, "false_findings": false,
            "matched": matched, "n_lesions": n, "sensitivity": sens,
            "fp_per_case": false.astype(np.float64) / np.float64(cases), "precision": precision,
            "sensitivity_at": at, "cpm": at.mean()}


def dyadic_scores(rng, shape, bins, levels=None):
    """float32 probabilities k / (2 bins), k in 0..2 bins: row edges and midpoints, exact in fp32.  ``levels``
    (a power of two below 2 bins) draws from that many equally spaced values and 1 only: a fixture that
    stores them stays small."""
    step = 1 if levels is None else 2 * bins // levels
    k = rng.integers(0, 2 * bins // step + 1, shape) * step
    return (k.astype(np.float32) / np.float32(2 * bins)).astype(np.float32)


def _case(name, mask, scores, target, depths=None, bins=256, connectivity=26, min_overlap=0.0, max_lesions=64,
          ignore=None):
    mask, scores, target = np.asarray(mask, np.uint8), np.asarray(scores, np.float32), np.asarray(target, np.int64)
    if mask.ndim == 2:
        mask, scores, target = mask[None], scores[None], target[None]
    depths = [mask.shape[0]] if depths is None else list(depths)
    return dict(name=name, mask=mask, scores=scores, target=target, depths=depths, bins=bins,
                connectivity=connectivity, min_overlap=min_overlap, max_lesions=max_lesions, ignore=ignore)


def _blank(*shape):
    return np.zeros(shape, np.uint8), np.zeros(shape, np.float32), np.zeros(shape, np.int64)


def hand_cases():
    """The cases tests/test_froc_cpu.py counts by hand, by name."""
    out = {}
    # two candidates of different confidence on one lesion: the lesion takes the larger
    m, s, t = _blank(5, 70)
    t[1:4, 10:60] = 1
    m[0:2, 12:15], s[0:2, 12:15] = 1, 0.25
    s[1, 13] = 0.5                                       # conf 128
    m[3:5, 50:66], s[3:5, 50:66] = 1, 0.75               # conf 192
    out["two_on_one"] = _case("two_on_one", m, s, t)
    # one candidate on two lesions: both take it
    m, s, t = _blank(5, 70)
    t[1:3, 2:6] = t[1:3, 60:66] = 1
    m[2, 4:63], s[2, 4:63] = 1, 0.125
    s[2, 30] = 0.625                                     # conf 160, outside both lesions
    out["one_on_two"] = _case("one_on_two", m, s, t)
    # a candidate that touches a lesion but fails min_overlap 0.5: a false finding that lends nothing
    m, s, t = _blank(4, 40)
    t[0:2, 0:4] = 1                                      # 8 voxels, hit 1: fails on the target side too
    m[1, 3:11], s[1, 3:11] = 1, 0.5                      # 8 voxels, hit 1 of 8
    t[3, 20:24] = 1                                      # hit 2 of 4: found on the target side
    m[3, 22:32], s[3, 22:32] = 1, 1.0                    # 10 voxels, hit 2 of 10: fails
    out["grazing"] = _case("grazing", m, s, t, min_overlap=0.5)
    # a candidate whose scores are all <= 0 or NaN: conf 0
    m, s, t = _blank(3, 10)
    t[1, 2:6] = 1
    m[1, 3:8] = 1
    s[1, 3:8] = [0.0, -0.0, -1.0, np.nan, -np.inf]
    out["zero_conf"] = _case("zero_conf", m, s, t, bins=16)
    # +inf and p > 1: row bins
    m, s, t = _blank(3, 12)
    t[0, 0:3] = t[2, 8:12] = 1
    m[0, 1:4], m[2, 6:10] = 1, 1
    s[0, 1:4] = [0.25, np.inf, 0.5]
    s[2, 6:10] = [0.125, 1.5, 0.0, 0.25]
    out["above_one"] = _case("above_one", m, s, t, bins=16)
    # ignored voxels split a candidate: two candidates with their own confidences
    m, s, t = _blank(3, 70)
    t[1, 5:30] = 1
    m[1, 3:67], s[1, 3:67] = 1, 0.25
    s[1, 10], s[1, 66] = 0.75, 0.5
    t[:, 64] = 255
    out["ignore_splits"] = _case("ignore_splits", m, s, t, depths=(1,), ignore=255)
    return out


def cases():
    """The named cases: dicts with name, mask uint8, scores float32 (one plane of probabilities), target
    int64 (all [N, H, W]), depths, bins, connectivity (6 / 18 / 26), min_overlap, max_lesions and ignore.  Cases
    whose depths are all 1 are also run through the image entry point at ``FLAT[connectivity]``."""
    out = list(hand_cases().values())
    rng = np.random.default_rng(11)
    # ragged depths across the chunk seam, the table cut, the smallest and the largest table
    m = (rng.random((6, 5, 65)) < 0.35).astype(np.uint8)
    t = (rng.random((6, 5, 65)) < 0.35).astype(np.int64) * 2
    t[4, :, 20] = 255
    for bins, conn, frac, cap in ((2, 6, 0.0, 64), (256, 18, 0.25, 5), (4096, 26, 0.5, 0)):
        out.append(_case("ragged_%d" % bins, m, dyadic_scores(rng, m.shape, bins, min(32, bins)), t, (1, 3, 2), bins,
                         conn, frac, cap, 255))
    # images: depth one everywhere, blobs rather than noise
    m, s, t = _blank(4, 9, 130)
    for z in range(4):
        for _ in range(5):
            y, x, h, w = rng.integers(0, 7), rng.integers(0, 120), rng.integers(1, 4), rng.integers(1, 70)
            m[z, y:y + h, x:x + w] = 1
            y, x, h, w = rng.integers(0, 7), rng.integers(0, 120), rng.integers(1, 4), rng.integers(1, 40)
            t[z, y:y + h, x:x + w] = 1
    s = np.repeat(dyadic_scores(rng, (4, 9, 13), 64), 10, axis=2)          # plateaus ten voxels wide
    out.append(_case("blobs", m, s, t, (1, 1, 1, 1), 64, 26, 0.25, 16))
    # empty sides
    out.append(_case("empty_prediction", np.zeros_like(m), s, t, (2, 2), 64))
    out.append(_case("empty_target", m, s, np.zeros_like(t), (2, 2), 64))
    return out


def fixture():
    """{name: (case dict with the stored inputs, (summary, table, hist))} of tests/golden/froc.npz."""
    g = np.load(os.path.join(GOLDEN, "froc.npz"))
    out = {}
    for name in g["names"].tolist():
        p = g[name + "/params"]
        c = dict(name=name, mask=g[name + "/mask"], scores=g[name + "/scores"], target=g[name + "/target"].astype(np.int64),
                 depths=g[name + "/depths"].tolist(), bins=int(p[0]), connectivity=int(p[1]),
                 min_overlap=float(g[name + "/min_overlap"]), max_lesions=int(p[2]),
                 ignore=None if p[3] < 0 else int(p[3]))
        out[name] = (c, (g[name + "/summary"], g[name + "/table"], g[name + "/hist"]))
    return out


def run_case(c, labeller=label):
    return stack_froc(c["mask"], c["scores"], c["target"], c["depths"], c["bins"], c["connectivity"], c["min_overlap"],
                      c["max_lesions"], c["ignore"], labeller)


__all__ = ["FLAT", "RATES", "cases", "curves", "dyadic_scores", "fixture", "hand_cases", "image_froc", "run_case",
           "stack_froc", "volume_froc"]
