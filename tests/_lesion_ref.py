"""numpy restatement of the lesion-level detection metrics (tests only; nothing but numpy is imported),
built on ``label`` / ``split`` of tests/_components3d_ref.py.

A stack ``[N, H, W]`` is cut into volumes of ``depths[v]`` slices (``None``: one volume); an image is
a volume one slice deep, where connectivity 6 means 4 and 18 / 26 mean 8.  Per volume:

    P = (mask != 0) & (target != ignore)      T = (target > 0) & (target != ignore)
    (``ignore`` None or negative: nothing is ignored; ignored voxels are background on both sides)
    either side is labelled on its own (scipy.ndimage.label's numbering)
    target lesion t:        area = |t|, hit = |t & P|
    predicted component p:  area = |p|, hit = |p & T|
    matched  iff  hit >= 1 and float(hit) >= min_overlap * float(area)      (one double multiply)
    summary int64 [4] = (n_T, matched_T, n_P, matched_P)
    table   int64 [2, max_lesions, 2]: side 0 the target, side 1 the prediction; row l - 1 = (area,
            hit) of label l; rows past n are zero; labels above max_lesions are left out

``tests/golden/lesions.npz`` (make_golden_lesions.py: the same with scipy's labels) pins it on ``cases()``.
"""
import os

import numpy as np

from _components3d_ref import FLAT, label, split

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TO_3D = {4: 6, 8: 26}                              # an image as a volume one slice deep


def sides(mask, target, ignore=None):
    """(T, P) bool arrays of the definition; side 0 is the target."""
    mask, target = np.asarray(mask), np.asarray(target)
    keep = np.ones(target.shape, bool) if ignore is None or ignore < 0 else target != ignore
    return (target > 0) & keep, (mask != 0) & keep


def volume_metrics(mask, target, connectivity=26, min_overlap=0.0, max_lesions=64, ignore=None, labeller=label):
    """(summary int64 [4], table int64 [2, max_lesions, 2]) of one volume ``[D, H, W]``."""
    fg = sides(mask, target, ignore)
    summary = np.zeros(4, np.int64)
    table = np.zeros((2, max_lesions, 2), np.int64)
    for s in (0, 1):
        labels, n = labeller(fg[s], connectivity)
        area = np.bincount(labels.ravel(), minlength=n + 1)[1:].astype(np.int64)
        hit = np.bincount(labels[fg[1 - s]].ravel(), minlength=n + 1)[1:].astype(np.int64)
        matched = (hit >= 1) & (hit.astype(np.float64) >= np.float64(min_overlap) * area.astype(np.float64))
        summary[2 * s], summary[2 * s + 1] = n, matched.sum()
        k = min(n, max_lesions)
        table[s, :k, 0], table[s, :k, 1] = area[:k], hit[:k]
    return summary, table


def stack_metrics(mask, target, depths=None, connectivity=26, min_overlap=0.0, max_lesions=64, ignore=None,
                  labeller=label):
    """(summary int64 [V, 4], table int64 [V, 2, max_lesions, 2]) of a stack of volumes."""
    res = [volume_metrics(m, t, connectivity, min_overlap, max_lesions, ignore, labeller)
           for m, t in zip(split(mask, depths), split(target, depths))]
    return np.stack([r[0] for r in res]), np.stack([r[1] for r in res])


def image_metrics(mask, target, connectivity=8, min_overlap=0.0, max_lesions=64, ignore=None, labeller=label):
    """The same per image of a batch ``[B, H, W]`` at connectivity 4 or 8."""
    return stack_metrics(mask, target, [1] * len(mask), TO_3D[connectivity], min_overlap, max_lesions, ignore,
                         labeller)


def ratios(summary):
    """(sensitivity, precision) float64 [V]; NaN where the denominator is 0."""
    s = np.asarray(summary, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return s[:, 1] / s[:, 0], s[:, 3] / s[:, 2]


def _case(name, mask, target, depths=None, connectivity=26, min_overlap=0.0, max_lesions=64, ignore=None):
    mask, target = np.asarray(mask, np.uint8), np.asarray(target, np.int64)
    if mask.ndim == 2:
        mask, target = mask[None], target[None]
    depths = [mask.shape[0]] if depths is None else list(depths)
    return dict(name=name, mask=mask, target=target, depths=depths, connectivity=connectivity,
                min_overlap=min_overlap, max_lesions=max_lesions, ignore=ignore)


def _zeros(*shape):
    return np.zeros(shape, np.uint8), np.zeros(shape, np.int64)


def cases():
    """The named cases: dicts with name, mask uint8 [N, H, W], target int64 [N, H, W], depths,
    connectivity (6 / 18 / 26), min_overlap, max_lesions and ignore.  Cases whose depths are all 1 are
    also run through the image entry point at ``FLAT[connectivity]``."""
    out = []
    # one predicted blob bridges two target lesions: both matched, one matched prediction
    m, t = _zeros(5, 70)
    t[1:3, 2:6] = t[1:3, 60:66] = 1
    m[2, 4:63] = 1
    out.append(_case("bridge", m, t))
    # one target lesion hit by two predicted components, and a third prediction elsewhere
    m, t = _zeros(5, 70)
    t[1:4, 10:60] = 2
    m[0:2, 12:15] = m[3:5, 50:66] = m[0, 68:70] = 1
    out.append(_case("two_hits", m, t))
    # touching edge to edge / corner to corner with no shared voxel: unmatched on both sides
    m, t = _zeros(2, 4, 8)
    t[0, 1, 1:3] = t[1, 2, 5] = 1
    m[0, 2, 1:3] = m[0, 1, 3] = m[0, 3, 6] = 1
    out.append(_case("edge_touch", m, t, connectivity=6))
    out.append(_case("corner_touch", m, t, connectivity=26))
    # identical, disjoint and empty sides
    rng = np.random.default_rng(5)
    r = (rng.random((3, 5, 65)) < 0.4).astype(np.uint8)
    out.append(_case("identical", r, r.astype(np.int64) * 3, connectivity=18))
    m, t = _zeros(3, 5, 65)
    m[:, :, :30], t[:, :, 32:] = r[:, :, :30], r[:, :, 32:]
    out.append(_case("disjoint", m, t))
    out.append(_case("empty_prediction", np.zeros_like(r), r))
    out.append(_case("empty_target", r, np.zeros(r.shape, np.int64)))
    out.append(_case("both_empty", *_zeros(2, 3, 7)))
    # a run across the 64-voxel chunk seam on either side, and a row of one-voxel runs
    m, t = _zeros(2, 130)
    t[0, 60:70] = t[1, 120:130] = 1
    m[0, 63:66] = m[1, 126:129] = m[1, 0] = 1
    out.append(_case("seam_run", m, t))
    m, t = _zeros(1, 130)
    t[0, ::2] = 1
    m[0, 1::4] = m[0, 64] = m[0, 128] = 1
    out.append(_case("one_voxel_runs", m, t))
    # the checkerboard at connectivity 4 / 6: H W / 2 components per side, the table is cut
    yy, xx = np.mgrid[0:8, 0:64]
    board = ((yy + xx) % 2 == 0).astype(np.uint8)
    pred = np.where(xx < 40, board, 1 - board).astype(np.uint8)
    out.append(_case("checkerboard_image", pred, board, connectivity=6))
    zz, yy, xx = np.mgrid[0:2, 0:8, 0:64]
    board = ((zz + yy + xx) % 2 == 0).astype(np.uint8)
    pred = np.where(xx < 40, board, 1 - board).astype(np.uint8)
    out.append(_case("checkerboard_volume", pred, board, connectivity=6))
    # min_overlap at exact equality with dyadic fractions, one voxel fewer, and 1.0
    m, t = _zeros(1, 6, 40)
    t[0, 0:2, 0:4] = t[0, 0:2, 10:14] = t[0, 0:2, 20:24] = t[0, 0:2, 30:34] = 1      # four lesions of 8 voxels
    m[0, 0, 0:4] = 1                                   # hit 4 of 8 = 0.5
    m[0, 0, 10:13] = 1                                 # hit 3 of 8
    m[0, 1, 22:26] = 1                                 # hit 2 of 8 = 0.25; the prediction: 2 of 4 = 0.5
    m[0, 1, 33:37] = 1                                 # hit 1 of 8; the prediction: 1 of 4 = 0.25
    t[0, 4:6, 0:4] = m[0, 4:6, 0:4] = 1                # a lesion found whole: 1.0 on both sides
    m[0, 4:6, 10:14], t[0, 4, 10:14] = 1, 1            # a prediction twice its lesion: 1.0 and 0.5
    for frac in (0.25, 0.5, 1.0):
        out.append(_case("overlap_%g" % frac, m, t, min_overlap=frac))
    # ignore_index cuts a component in two on each side, and ignored voxels are in no count
    m, t = _zeros(2, 3, 70)
    t[0, 1, 5:69], m[0, 1, 3:67] = 1, 1
    t[0, :, 64] = t[0, 0, 10] = 255
    m[1, 0:2, 20:30], t[1, 1:3, 25:35] = 1, 2
    t[1, 1, 25:30] = 255
    out.append(_case("ignore_255", m, t, depths=(1, 1), ignore=255))
    out.append(_case("ignore_none", m, t, depths=(1, 1)))
    # the table's capacity below, at and above n, and no table; ragged depths in one call
    m = (rng.random((6, 5, 65)) < 0.3).astype(np.uint8)
    t = (rng.random((6, 5, 65)) < 0.3).astype(np.int64)
    n = int(stack_metrics(m, t, (1, 3, 2), 26)[0][:, [0, 2]].max())
    for name, cap in (("below", n - 1), ("equal", n), ("above", n + 3), ("none", 0)):
        out.append(_case("capacity_" + name, m, t, depths=(1, 3, 2), max_lesions=cap))
    return out


def fixture():
    """{name: (summary int64 [V, 4], table int64 [V, 2, max_lesions, 2])} of tests/golden/lesions.npz."""
    g = np.load(os.path.join(GOLDEN, "lesions.npz"))
    return {name: (g[name + "/summary"], g[name + "/table"]) for name in g["names"].tolist()}


__all__ = ["FLAT", "TO_3D", "cases", "fixture", "image_metrics", "ratios", "sides", "stack_metrics", "volume_metrics"]
