"""numpy restatement of the per-volume boundary metrics (tests only; nothing but numpy is imported).

Per volume, for binary masks P (prediction) and T (ground truth) of shape [D, H, W] and a voxel
spacing (sz, sy, sx) -- MedPy's hd / hd95 / assd with ``voxelspacing=(sz, sy, sx)``, ``connectivity=1``:

    border    dM = M & ~erode(M), erosion with the 6-neighbour cross, background outside the volume
              (D = 1: every foreground voxel is a border voxel)
    d2        for p in dP: min over q in dT of ((dz sz)^2 + (dy sy)^2) + (dx sx)^2 in float64, every
              product and sum rounded once, in this order (the order of scipy's
              distance_transform_edt(sampling=...)); likewise from dT to dP; distances are sqrt(d2)
    hd        the largest distance of both directions
    hd95      np.percentile(all distances, 95): numpy's linear percentile, s sorted, r = 0.95 (n - 1),
              lo = floor(r), hi = min(lo + 1, n - 1), s[lo] + (s[hi] - s[lo]) (r - lo)
    assd      (mean of the P->T distances + mean of the T->P distances) / 2, each mean over the
              border voxels in raster order (np.mean)
    undefined an empty dP or dT gives NaN for all three

Brute force over the border voxels.  ``tests/golden/boundary3d.npz`` (make_golden_boundary3d.py:
scipy's binary_erosion, distance_transform_edt and np.percentile) pins it bit for bit.
"""
import os

import numpy as np

from _boundary_ref import masks_of  # noqa: F401  (the same foreground rule)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
U = 2.0 ** -53                                   # unit roundoff of float64


def border3(m):
    m = np.asarray(m) != 0
    q = np.pad(m, 1)
    c = q[1:-1, 1:-1, 1:-1]
    inner = (c & q[:-2, 1:-1, 1:-1] & q[2:, 1:-1, 1:-1] & q[1:-1, :-2, 1:-1] & q[1:-1, 2:, 1:-1]
             & q[1:-1, 1:-1, :-2] & q[1:-1, 1:-1, 2:])
    return m & ~inner


def _d2(dz, dy, dx, spacing):
    sz, sy, sx = (np.float64(s) for s in spacing)
    a, b, c = dz.astype(np.float64) * sz, dy.astype(np.float64) * sy, dx.astype(np.float64) * sx
    return (a * a + b * b) + c * c


def d2_all3(sites, spacing=(1.0, 1.0, 1.0), chunk=64):
    """float64 [D, H, W]: squared weighted distance of every voxel to the nearest nonzero voxel of
    ``sites`` (+inf everywhere when there is none), by brute force."""
    sites = np.asarray(sites) != 0
    D, H, W = sites.shape
    out = np.full((D, H, W), np.inf)
    zs, ys, xs = np.nonzero(sites)
    Z, Y, X = np.mgrid[0:D, 0:H, 0:W]
    for i in range(0, len(zs), chunk):
        pick = lambda a: a[i:i + chunk, None, None, None]
        out = np.minimum(out, _d2(Z[None] - pick(zs), Y[None] - pick(ys), X[None] - pick(xs), spacing).min(0))
    return out


def directed_d2(src_border, dst_border, spacing):
    """d2 of every voxel of ``src_border`` (raster order) to the nearest voxel of ``dst_border``."""
    z, y, x = np.nonzero(src_border)
    qz, qy, qx = np.nonzero(dst_border)
    out = np.empty(len(z), np.float64)
    for i in range(0, len(z), 256):
        s = slice(i, i + 256)
        out[s] = _d2(z[s, None] - qz[None], y[s, None] - qy[None], x[s, None] - qx[None], spacing).min(1)
    return out


def metrics3(P, T, spacing=(1.0, 1.0, 1.0)):
    """(hd, hd95, assd, (|dP|, |dT|), max d2) of one volume; NaN x3 and max d2 None when a border is empty."""
    bp, bt = border3(P), border3(T)
    counts = (int(bp.sum()), int(bt.sum()))
    if 0 in counts:
        return float("nan"), float("nan"), float("nan"), counts, None
    a, b = directed_d2(bp, bt, spacing), directed_d2(bt, bp, spacing)
    da, db = np.sqrt(a), np.sqrt(b)
    hd = max(da.max(), db.max())
    hd95 = np.percentile(np.hstack((da, db)), 95)
    assd = np.mean((da.mean(), db.mean()))
    return float(hd), float(hd95), float(assd), counts, float(max(a.max(), b.max()))


def as_rows(spacing, V):
    """``spacing`` (a number, a triple or V triples) as a list of V (sz, sy, sx) tuples."""
    s = np.asarray(spacing, np.float64)
    if s.ndim == 0:
        return [(float(s),) * 3] * V
    if s.ndim == 1:
        return [tuple(s.tolist())] * V
    assert s.shape == (V, 3)
    return [tuple(r) for r in s.tolist()]


def stack_metrics(mask, target, depths=None, spacing=1.0, ignore=None):
    """``metrics3`` of every volume of a [N, H, W] stack: (out float64 [V, 3], counts int64 [V, 2], max d2 list)."""
    mask, target = np.asarray(mask), np.asarray(target)
    depths = [mask.shape[0]] if depths is None else list(depths)
    rows = as_rows(spacing, len(depths))
    out, counts, mx, at = [], [], [], 0
    for d, sp in zip(depths, rows):
        P, T = masks_of(mask[at:at + d], target[at:at + d], ignore)
        hd, hd95, assd, c, m = metrics3(P, T, sp)
        out.append((hd, hd95, assd))
        counts.append(c)
        mx.append(m)
        at += d
    assert at == mask.shape[0]
    return np.array(out, np.float64).reshape(-1, 3), np.array(counts, np.int64).reshape(-1, 2), mx


def stack_d2(sites, depths=None, spacing=1.0, where=None):
    """``d2_all3`` of every volume of a stack, -1 where ``where`` (or None) is zero."""
    sites = np.asarray(sites)
    depths = [sites.shape[0]] if depths is None else list(depths)
    rows = as_rows(spacing, len(depths))
    out, at = [], 0
    for d, sp in zip(depths, rows):
        out.append(d2_all3(sites[at:at + d], sp))
        at += d
    out = np.concatenate(out)
    return out if where is None else np.where(np.asarray(where) != 0, out, -1.0)


def fixture_cases():
    """The cases of tests/golden/boundary3d.npz: dicts with name, P, T (uint8 [D, H, W]), scipy's
    border_p, border_t (bool) and metrics, float64 [S, 3] = (hd, hd95, assd) at each of the
    fixture's spacings (NaN when undefined); ``fixture_spacings()`` lists those."""
    g = np.load(os.path.join(GOLDEN, "boundary3d.npz"))
    bits = {k: g[k] for k in ("P", "T", "border_p", "border_t")}
    out, at = [], 0
    for name, (D, H, W), m in zip(g["names"].tolist(), g["shapes"].tolist(), g["metrics"]):
        n = D * H * W
        nbytes = (n + 7) // 8
        unpack = lambda k: np.unpackbits(bits[k][at:at + nbytes])[:n].reshape(D, H, W)
        out.append(dict(name=name, P=unpack("P"), T=unpack("T"), border_p=unpack("border_p").astype(bool),
                        border_t=unpack("border_t").astype(bool), metrics=np.array(m, np.float64)))
        at += nbytes
    assert all(at == len(v) for v in bits.values())
    return out


def fixture_spacings():
    g = np.load(os.path.join(GOLDEN, "boundary3d.npz"))
    return [tuple(s) for s in g["spacings"].tolist()]
