"""numpy restatement of the volume-level connected-component post-processing (tests only; nothing
but numpy is imported).

A stack of slices ``[N, H, W]`` is cut into volumes of ``depths[v]`` consecutive slices; every volume
is handled on its own.  Per volume, for a mask M (any integer or bool array, foreground M != 0):

    components  the classes of the foreground under 6-connectivity (face neighbours), 18 (faces and
                edges) or 26 (faces, edges and corners): two voxels are neighbours when their
                offset has at most 1 / 2 / 3 non-zero coordinates, each of them +-1; voxels outside
                the volume are background
    labels      0 on the background, 1..n on the components, numbered in raster order (z, y, x) of
                each component's first voxel:
                ``scipy.ndimage.label(M, generate_binary_structure(3, 1, 2 or 3))``
    filter      a component passes when it has >= min_size voxels and, with keep_largest, it is the
                one ``np.argmax(np.bincount(labels.ravel())[1:])`` picks: the largest, equal sizes
                going to the lower label; a passing voxel keeps its own value, every other is 0
    counts      (|P' & T|, |P'|, |T|) over the volume with P' = filtered != 0, T = target > 0,
                voxels whose target equals ``ignore`` left out of all three

``label`` is the classic two-pass algorithm with a union-find over provisional labels.
``tests/golden/components3d.npz`` (make_golden_components3d.py: scipy's labels) pins it.
"""
import itertools
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CONNECTIVITIES = (6, 18, 26)
LEVEL = {6: 1, 18: 2, 26: 3}


def earlier_neighbours(connectivity):
    """The offsets (dz, dy, dx) of the neighbours that come before a voxel in raster order."""
    return [o for o in itertools.product((-1, 0, 1), repeat=3)
            if o < (0, 0, 0) and sum(c != 0 for c in o) <= LEVEL[connectivity]]


def label(volume, connectivity=26):
    """(labels int32 [D, H, W], n) of one volume."""
    if connectivity not in CONNECTIVITIES:
        raise ValueError(connectivity)
    fg = np.asarray(volume) != 0
    D, H, W = fg.shape
    prov = np.zeros((D + 2, H + 2, W + 2), np.int64)             # a background rim: no bounds tests
    parent = [0]

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    before = earlier_neighbours(connectivity)
    voxels = (np.argwhere(fg) + 1).tolist()                      # raster order
    for z, y, x in voxels:
        roots = {find(q) for q in (prov[z + dz, y + dy, x + dx] for dz, dy, dx in before) if q}
        if not roots:
            parent.append(len(parent))
            prov[z, y, x] = len(parent) - 1
        else:
            low = min(roots)                            # the lowest provisional label is the earliest voxel
            prov[z, y, x] = low
            for r in roots:
                parent[r] = low
    out = np.zeros((D, H, W), np.int32)
    number = {}
    for z, y, x in voxels:
        out[z - 1, y - 1, x - 1] = number.setdefault(find(prov[z, y, x]), len(number) + 1)
    return out, len(number)


def filter_volume(volume, keep_largest=False, min_size=0, connectivity=26):
    """(filtered volume, same dtype; n before filtering) of one volume."""
    volume = np.asarray(volume)
    labels, n = label(volume, connectivity)
    sizes = np.bincount(labels.ravel(), minlength=n + 1)
    passes = sizes >= min_size
    passes[0] = False
    if keep_largest and n:
        only = np.zeros_like(passes)
        first = 1 + int(np.argmax(sizes[1:]))
        only[first] = passes[first]
        passes = only
    return np.where(passes[labels], volume, 0).astype(volume.dtype), n


def counts_of(filtered, target, ignore=None):
    """int64 [3] = (|P' & T|, |P'|, |T|) of one volume with stf_predict_mask's rules."""
    filtered, target = np.asarray(filtered), np.asarray(target)
    keep = np.ones(target.shape, bool) if ignore is None else target != ignore
    P, T = (filtered != 0) & keep, (target > 0) & keep
    return np.array([(P & T).sum(), P.sum(), T.sum()], np.int64)


def split(stack, depths):
    """The volumes of a stack: views ``[D_v, H, W]``."""
    stack = np.asarray(stack)
    depths = [stack.shape[0]] if depths is None else list(depths)
    assert sum(depths) == stack.shape[0] and all(d >= 1 for d in depths)
    ends = np.cumsum(depths)
    return [stack[e - d:e] for d, e in zip(depths, ends)]


def stack_label(stack, depths=None, connectivity=26):
    """(labels int32 [N, H, W], num int32 [V]) of a stack of volumes."""
    res = [label(v, connectivity) for v in split(stack, depths)]
    return np.concatenate([r[0] for r in res]), np.array([r[1] for r in res], np.int32)


def stack_filter(stack, depths=None, keep_largest=False, min_size=0, connectivity=26, target=None, ignore=None):
    """(filtered [N, H, W], num int32 [V], counts int64 [V, 3] or None) of a stack of volumes."""
    res = [filter_volume(v, keep_largest, min_size, connectivity) for v in split(stack, depths)]
    out = np.concatenate([r[0] for r in res])
    num = np.array([r[1] for r in res], np.int32)
    counts = None
    if target is not None:
        counts = np.stack([counts_of(o, t, ignore) for o, t in zip(split(out, depths), split(target, depths))])
    return out, num, counts


FLAT = {6: 4, 18: 8, 26: 8}                        # what a connectivity means inside one slice


def depth_one_inputs():
    """[(name, mask uint8 [B, H, W], target int64 [B, H, W] with values 0..2)]: the batches on which a
    stack of depth-1 volumes must equal a batch of images -- one row chunk, three chunks per row, a
    width of exactly one chunk and a single voxel, random at 0.5 and at 0.593, and the 2-D fixture
    cases padded to a common size as one batch."""
    from _components_ref import fixture_cases as cases2d
    rng = np.random.default_rng(77)
    out = []
    for shape in ((6, 5, 70), (3, 9, 130), (4, 3, 64), (1, 1, 1)):
        for fill in (0.5, 0.593):
            out.append(("%dx%dx%d_f%g" % (shape + (fill,)), (rng.random(shape) < fill).astype(np.uint8)))
    cases = cases2d()
    H, W = max(c["mask"].shape[0] for c in cases), max(c["mask"].shape[1] for c in cases)
    batch = np.zeros((len(cases), H, W), np.uint8)
    for b, c in enumerate(cases):
        batch[b, :c["mask"].shape[0], :c["mask"].shape[1]] = c["mask"]
    out.append(("fixture2d", batch))
    return [(name, m, rng.integers(0, 3, m.shape).astype(np.int64)) for name, m in out]


def fixture_cases():
    """The cases of tests/golden/components3d.npz: dicts with name, mask (uint8 [D, H, W]) and, per
    connectivity c in (6, 18, 26), scipy's ``labels{c}`` (int32 [D, H, W]) and ``n{c}``."""
    g = np.load(os.path.join(GOLDEN, "components3d.npz"))
    masks, out, at, lat = g["mask"], [], 0, {c: 0 for c in CONNECTIVITIES}
    for k, (name, (D, H, W)) in enumerate(zip(g["names"].tolist(), g["shapes"].tolist())):
        nbytes = (D * H * W + 7) // 8
        case = dict(name=name, mask=np.unpackbits(masks[at:at + nbytes])[:D * H * W].reshape(D, H, W))
        at += nbytes
        nfg = int(case["mask"].sum())
        for c in CONNECTIVITIES:
            # labels are stored as the values of the foreground voxels in raster order
            lab = np.zeros((D, H, W), np.int32)
            lab[case["mask"] != 0] = g[f"labels{c}"][lat[c]:lat[c] + nfg]
            lat[c] += nfg
            case[f"labels{c}"], case[f"n{c}"] = lab, int(g[f"n{c}"][k])
        out.append(case)
    assert at == len(masks) and all(lat[c] == len(g[f"labels{c}"]) for c in CONNECTIVITIES)
    return out
