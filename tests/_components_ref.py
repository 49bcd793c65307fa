"""numpy restatement of the connected-component post-processing (tests only; nothing but numpy is
imported).

Per image, for a mask M (any integer or bool array, foreground M != 0):

    components  the classes of the foreground under 4-connectivity (edge neighbours) or
                8-connectivity (edges and corners); pixels outside the image are background
    labels      0 on the background, 1..n on the components, numbered in raster order of each
                component's first pixel: ``scipy.ndimage.label(M, generate_binary_structure(2, 1 or 2))``
    filter      a component passes when its area is >= min_size and, with keep_largest, it is the one
                ``np.argmax(np.bincount(labels.ravel())[1:])`` picks: the largest, equal areas going
                to the lower label; a passing pixel keeps its own value, every other pixel is 0
    counts      (|P' & T|, |P'|, |T|) with P' = filtered != 0, T = target > 0, pixels whose target
                equals ``ignore`` left out of all three

``label`` is the classic two-pass algorithm with a union-find over provisional labels.
``tests/golden/components.npz`` (make_golden_components.py: scipy's labels) pins it.
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CONNECTIVITIES = (4, 8)


def label(mask, connectivity=8):
    """(labels int32 [H, W], n) of one image."""
    if connectivity not in CONNECTIVITIES:
        raise ValueError(connectivity)
    fg = np.asarray(mask) != 0
    H, W = fg.shape
    prov = np.zeros((H, W), np.int64)
    parent = [0]

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    before = [(0, -1), (-1, 0)] if connectivity == 4 else [(0, -1), (-1, -1), (-1, 0), (-1, 1)]
    for y in range(H):
        for x in range(W):
            if not fg[y, x]:
                continue
            roots = {find(prov[y + dy, x + dx]) for dy, dx in before
                     if 0 <= y + dy and 0 <= x + dx < W and fg[y + dy, x + dx]}
            if not roots:
                parent.append(len(parent))
                prov[y, x] = len(parent) - 1
            else:
                low = min(roots)                        # the lowest provisional label is the earliest pixel
                prov[y, x] = low
                for r in roots:
                    parent[r] = low
    out = np.zeros((H, W), np.int32)
    number = {}
    for y in range(H):
        for x in range(W):
            if fg[y, x]:
                out[y, x] = number.setdefault(find(prov[y, x]), len(number) + 1)
    return out, len(number)


def filter_mask(mask, keep_largest=False, min_size=0, connectivity=8):
    """(filtered mask, same dtype; n before filtering) of one image."""
    mask = np.asarray(mask)
    labels, n = label(mask, connectivity)
    areas = np.bincount(labels.ravel(), minlength=n + 1)
    passes = areas >= min_size
    passes[0] = False
    if keep_largest and n:
        only = np.zeros_like(passes)
        first = 1 + int(np.argmax(areas[1:]))
        only[first] = passes[first]
        passes = only
    return np.where(passes[labels], mask, 0).astype(mask.dtype), n


def counts_of(filtered, target, ignore=None):
    """int64 [3] = (|P' & T|, |P'|, |T|) of one image with stf_predict_mask's rules."""
    filtered, target = np.asarray(filtered), np.asarray(target)
    keep = np.ones(target.shape, bool) if ignore is None else target != ignore
    P, T = (filtered != 0) & keep, (target > 0) & keep
    return np.array([(P & T).sum(), P.sum(), T.sum()], np.int64)


def batch_label(masks, connectivity=8):
    """(labels int32 [B, H, W], num int32 [B]) of a batch."""
    res = [label(m, connectivity) for m in np.asarray(masks)]
    return np.stack([r[0] for r in res]), np.array([r[1] for r in res], np.int32)


def batch_filter(masks, keep_largest=False, min_size=0, connectivity=8, target=None, ignore=None):
    """(filtered [B, H, W], num int32 [B], counts int64 [B, 3] or None) of a batch."""
    masks = np.asarray(masks)
    res = [filter_mask(m, keep_largest, min_size, connectivity) for m in masks]
    out = np.stack([r[0] for r in res])
    num = np.array([r[1] for r in res], np.int32)
    counts = None if target is None else np.stack([counts_of(o, t, ignore) for o, t in zip(out, np.asarray(target))])
    return out, num, counts


def fixture_cases():
    """The cases of tests/golden/components.npz: dicts with name, mask (uint8 [H, W]) and, per
    connectivity c in (4, 8), scipy's ``labels{c}`` (int32 [H, W]) and ``n{c}``."""
    g = np.load(os.path.join(GOLDEN, "components.npz"))
    masks, out, at, lat = g["mask"], [], 0, {c: 0 for c in CONNECTIVITIES}
    for k, (name, (H, W)) in enumerate(zip(g["names"].tolist(), g["shapes"].tolist())):
        nbytes = (H * W + 7) // 8
        case = dict(name=name, mask=np.unpackbits(masks[at:at + nbytes])[:H * W].reshape(H, W))
        at += nbytes
        for c in CONNECTIVITIES:
            n = int(g[f"n{c}"][k])
            # labels are stored as the values of the foreground pixels in raster order
            lab = np.zeros((H, W), np.int32)
            nfg = int(case["mask"].sum())
            lab[case["mask"] != 0] = g[f"labels{c}"][lat[c]:lat[c] + nfg]
            lat[c] += nfg
            case[f"labels{c}"], case[f"n{c}"] = lab, n
        out.append(case)
    assert at == len(masks) and all(lat[c] == len(g[f"labels{c}"]) for c in CONNECTIVITIES)
    return out
