"""numpy restatement of the boundary metrics (tests only; nothing but numpy is imported).

Per image, for binary masks P (prediction) and T (ground truth) at unit pixel spacing:

    border    dM = M & ~erode(M), erosion with the 4-neighbour cross, background outside the image
    d2        for p in dP: min over q in dT of (py - qy)^2 + (px - qx)^2, an exact integer; likewise
              from dT to dP; distances are sqrt(float64(d2))
    hd        sqrt(max d2 over both directions)
    hd95      numpy's linear percentile of the concatenated distances: s sorted, r = 0.95 (n - 1),
              lo = floor(r), hi = min(lo + 1, n - 1), s[lo] + (s[hi] - s[lo]) (r - lo)
    assd      (mean of the P->T distances + mean of the T->P distances) / 2
    undefined an empty dP or dT gives NaN for all three

Brute force over the border pixels.  ``tests/golden/boundary.npz`` (make_golden_boundary.py: scipy's
binary_erosion, distance_transform_edt and np.percentile) pins it.
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
INT32_MAX = 2 ** 31 - 1


def masks_of(mask, target, ignore=None):
    """Boolean (P, T) of a predicted mask and an integer target, ``ignore`` pixels background in both."""
    mask, target = np.asarray(mask), np.asarray(target)
    keep = np.ones(target.shape, bool) if ignore is None else target != ignore
    return (mask != 0) & keep, (target > 0) & keep


def border(m):
    m = np.asarray(m) != 0
    q = np.pad(m, 1)
    inner = q[1:-1, 1:-1] & q[:-2, 1:-1] & q[2:, 1:-1] & q[1:-1, :-2] & q[1:-1, 2:]
    return m & ~inner


def d2_all(sites, chunk=256):
    """int64 [H, W]: squared distance of every pixel to the nearest nonzero pixel of ``sites``
    (INT32_MAX everywhere when there is none), by brute force."""
    sites = np.asarray(sites) != 0
    H, W = sites.shape
    out = np.full((H, W), INT32_MAX, np.int64)
    ys, xs = np.nonzero(sites)
    Y, X = np.mgrid[0:H, 0:W]
    for i in range(0, len(ys), chunk):
        dy = Y[None] - ys[i:i + chunk, None, None]
        dx = X[None] - xs[i:i + chunk, None, None]
        out = np.minimum(out, (dy * dy + dx * dx).min(0))
    return out


def directed_d2(src_border, dst_border):
    """d2 of every pixel of ``src_border`` (row-major order) to the nearest pixel of ``dst_border``."""
    ys, xs = np.nonzero(src_border)
    qy, qx = np.nonzero(dst_border)
    out = np.empty(len(ys), np.int64)
    for i in range(0, len(ys), 256):
        dy = ys[i:i + 256, None] - qy[None]
        dx = xs[i:i + 256, None] - qx[None]
        out[i:i + 256] = (dy * dy + dx * dx).min(1)
    return out


def metrics(P, T):
    """(hd, hd95, assd, (|dP|, |dT|), max d2) of one image; NaN x3 and max d2 None when a border is empty."""
    bp, bt = border(P), border(T)
    counts = (int(bp.sum()), int(bt.sum()))
    if 0 in counts:
        return float("nan"), float("nan"), float("nan"), counts, None
    a, b = directed_d2(bp, bt), directed_d2(bt, bp)
    da, db = np.sqrt(a.astype(np.float64)), np.sqrt(b.astype(np.float64))
    s = np.sort(np.concatenate([da, db]))
    n = len(s)
    r = 0.95 * (n - 1)
    lo = int(np.floor(r))
    hi = min(lo + 1, n - 1)
    hd95 = s[lo] + (s[hi] - s[lo]) * (r - lo)
    mx = int(max(a.max(), b.max()))
    return float(np.sqrt(np.float64(mx))), float(hd95), float(0.5 * (da.mean() + db.mean())), counts, mx


def batch_metrics(mask, target, ignore=None):
    """``metrics`` of every image of [B, H, W] arrays: (out float64 [B, 3], counts int64 [B, 2], max d2 list)."""
    out, counts, mx = [], [], []
    for m, t in zip(np.asarray(mask), np.asarray(target)):
        P, T = masks_of(m, t, ignore)
        hd, hd95, assd, c, d = metrics(P, T)
        out.append((hd, hd95, assd))
        counts.append(c)
        mx.append(d)
    return np.array(out, np.float64).reshape(-1, 3), np.array(counts, np.int64).reshape(-1, 2), mx


def fixture_cases():
    """The cases of tests/golden/boundary.npz: dicts with name, P, T (uint8 [H, W]) and scipy's
    border_p, border_t (bool), hd, hd95, assd (float64, NaN when undefined)."""
    g = np.load(os.path.join(GOLDEN, "boundary.npz"))
    bits = {k: g[k] for k in ("P", "T", "border_p", "border_t")}
    out, at = [], 0
    for name, (H, W), (hd, hd95, assd) in zip(g["names"].tolist(), g["shapes"].tolist(), g["metrics"].tolist()):
        nbytes = (H * W + 7) // 8
        unpack = lambda k: np.unpackbits(bits[k][at:at + nbytes])[:H * W].reshape(H, W)
        out.append(dict(name=name, P=unpack("P"), T=unpack("T"), border_p=unpack("border_p").astype(bool),
                        border_t=unpack("border_t").astype(bool), hd=hd, hd95=hd95, assd=assd))
        at += nbytes
    assert all(at == len(v) for v in bits.values())
    return out
