"""Volume-level connected-component post-processing on the GPU (the volume kernels of csrc/ccl.hip through the C
entry points and stfunet.predict) against tests/golden/components3d.npz (scipy's labels) and the numpy
restatement of tests/_components3d_ref.py, which tests/test_components3d_cpu.py pins to that fixture.

Everything is an integer, so every comparison is equality, element for element.

The kernel-level tests call the C entry points on buffers with 64 guard bytes on each side and run
every case twice, the buffers (scratch included) prefilled with 0xAA and then 0x55: equal results
show that every output byte is written and that two runs agree bit for bit; the guards must keep
their fill.
"""
import itertools

import numpy as np
import pytest
import torch

import _launch_trace as lt
from _components3d_ref import CONNECTIVITIES, FLAT, LEVEL, depth_one_inputs, fixture_cases, stack_filter, stack_label

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
CASES = fixture_cases()


class Guarded:
    """``nbytes`` of device memory between two guards, everything prefilled with ``fill``."""

    def __init__(self, nbytes, fill):
        self.fill, self.n = fill, nbytes
        self.raw = torch.full((nbytes + 2 * GUARD,), fill, dtype=torch.uint8, device=DEV)
        self.body = self.raw[GUARD:GUARD + nbytes]
        assert self.raw.data_ptr() % 64 == 0

    def guards_intact(self):
        return bool((self.raw[:GUARD] == self.fill).all() and (self.raw[GUARD + self.n:] == self.fill).all())


def _scratch(N, H, W, V, fill):
    from stfunet import _lib
    nbytes = _lib.load().stf_ccl3d_scratch_bytes(N, H, W, V)
    assert nbytes >= 8 * N * H * W and nbytes % 8 == 0
    return Guarded(nbytes, fill)


def _starts(depths, N):
    depths = [N] if depths is None else list(depths)
    host = np.concatenate([[0], np.cumsum(depths)]).astype(np.int32)
    assert host[-1] == N
    return host, torch.from_numpy(host).to(DEV), len(depths)


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def run_label(mask, depths, connectivity, fill):
    from stfunet._lib import call, stream
    N, H, W = mask.shape
    host, starts, V = _starts(depths, N)
    m = _dev(mask, np.uint8)
    labels, num, scratch = Guarded(N * H * W * 4, fill), Guarded(V * 4, fill), _scratch(N, H, W, V, fill)
    call("stf_ccl3d_label", m.data_ptr(), N, H, W, starts.data_ptr(), host.ctypes.data, V, connectivity,
         labels.body.data_ptr(), num.body.data_ptr(), scratch.body.data_ptr(), stream())
    torch.cuda.synchronize()
    assert labels.guards_intact() and num.guards_intact() and scratch.guards_intact()
    return (labels.body.cpu().numpy().view(np.int32).reshape(N, H, W), num.body.cpu().numpy().view(np.int32))


def check_label(mask, connectivity, depths=None):
    """Two runs on differently prefilled buffers agree and equal the numpy oracle."""
    mask = np.asarray(mask, dtype=np.uint8)
    labels, num = run_label(mask, depths, connectivity, 0xAA)
    labels2, num2 = run_label(mask, depths, connectivity, 0x55)
    assert np.array_equal(labels, labels2) and np.array_equal(num, num2)
    ref, ref_num = stack_label(mask, depths, connectivity)
    assert np.array_equal(num, ref_num), (num.tolist(), ref_num.tolist())
    assert np.array_equal(labels, ref)
    return labels, num


def run_filter(mask, depths, connectivity, keep_largest, min_size, target, ignore, fill, want_num=True):
    from stfunet._lib import call, stream
    N, H, W = mask.shape
    host, starts, V = _starts(depths, N)
    m = _dev(mask, np.uint8)
    t = None if target is None else _dev(target, np.int64)
    out, num, scratch = Guarded(N * H * W, fill), Guarded(V * 4, fill), _scratch(N, H, W, V, fill)
    counts = None if target is None else Guarded(V * 24, fill)
    call("stf_ccl3d_filter", m.data_ptr(), None if t is None else t.data_ptr(), N, H, W, starts.data_ptr(),
         host.ctypes.data, V, connectivity, int(keep_largest), min_size, ignore, out.body.data_ptr(),
         None if counts is None else counts.body.data_ptr(), num.body.data_ptr() if want_num else None,
         scratch.body.data_ptr(), stream())
    torch.cuda.synchronize()
    assert out.guards_intact() and num.guards_intact() and scratch.guards_intact()
    assert counts is None or counts.guards_intact()
    assert want_num or bool((num.body == fill).all())
    return (out.body.cpu().numpy().reshape(N, H, W), num.body.cpu().numpy().view(np.int32) if want_num else None,
            None if counts is None else counts.body.cpu().numpy().view(np.int64).reshape(V, 3))


def check_filter(mask, connectivity=26, depths=None, keep_largest=False, min_size=0, target=None, ignore=None,
                 want_num=True):
    mask = np.asarray(mask, dtype=np.uint8)
    if target is not None:
        target = np.asarray(target, dtype=np.int64).reshape(mask.shape)
    ign = -1 if ignore is None else ignore
    first = run_filter(mask, depths, connectivity, keep_largest, min_size, target, ign, 0xAA, want_num)
    second = run_filter(mask, depths, connectivity, keep_largest, min_size, target, ign, 0x55, want_num)
    ref = list(stack_filter(mask, depths, keep_largest, min_size, connectivity, target, ignore))
    if not want_num:
        ref[1] = None                                             # num is optional: not asked for, not written
    for a, b, r in zip(first, second, ref):
        assert (a is None) == (r is None)
        if a is not None:
            assert np.array_equal(a, b) and np.array_equal(a, r), (a.tolist(), r.tolist())
    return first


def _random(shape, density, seed):
    return (np.random.default_rng(seed).random(shape) < density).astype(np.uint8)


# ---------------------------------------------------------------- labels
@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_labels_equal_the_fixture(c):
    for k in CONNECTIVITIES:
        labels, num = check_label(c["mask"], k)
        assert num.tolist() == [c[f"n{k}"]]                      # scipy's own numbers, as committed
        assert np.array_equal(labels, c[f"labels{k}"])


OFFSETS = [o for o in itertools.product((-1, 0, 1), repeat=3) if o != (0, 0, 0)]


@pytest.mark.parametrize("offset", OFFSETS, ids=["%+d%+d%+d" % o for o in OFFSETS])
def test_every_neighbour_offset(offset):
    """Two voxels at c and c + offset, c.x = 63 so that +1 crosses the 64-pixel word seam: joined iff
    the number of non-zero offset coordinates is at most 1 / 2 / 3 for connectivity 6 / 18 / 26."""
    m = np.zeros((3, 3, 66), np.uint8)
    m[1, 1, 63] = 1
    m[1 + offset[0], 1 + offset[1], 63 + offset[2]] = 1
    for k in CONNECTIVITIES:
        _, num = check_label(m, k)
        assert num.tolist() == [1 if sum(o != 0 for o in offset) <= LEVEL[k] else 2]


def test_volumes_never_touch():
    full = np.ones((6, 5, 70), np.uint8)
    for k in CONNECTIVITIES:
        labels, num = check_label(full, k, (1, 3, 2))
        assert num.tolist() == [1, 1, 1] and (labels == 1).all()     # labels restart at 1 per volume
        _, num = check_label(full, k)
        assert num.tolist() == [1]
    # corner contact across the boundary only: one component as one volume under 26, two as two volumes
    m = np.zeros((2, 4, 70), np.uint8)
    m[0, 1, 63] = m[1, 2, 64] = 1
    assert check_label(m, 26)[1].tolist() == [1] and check_label(m, 26, (1, 1))[1].tolist() == [1, 1]
    # specks in every volume: the numbering of one volume does not continue into the next
    s = _random((7, 9, 70), 0.1, 3)
    labels, num = check_label(s, 6, (2, 1, 4))
    assert labels[:2].max() == num[0] and labels[2].max() == num[1] and labels[3:].max() == num[2]


@pytest.mark.parametrize("D,H,W", list(itertools.product((1, 2, 5), (1, 2, 9, 17), (1, 63, 64, 65, 70, 130))))
def test_label_shapes(D, H, W):
    """Single slices, rows and columns, widths below, at and above one and two 64-pixel chunks: empty,
    full and random masks on both sides of the 26- and the 6-neighbour percolation points."""
    masks = [np.zeros((D, H, W), np.uint8), np.ones((D, H, W), np.uint8)]
    masks += [_random((D, H, W), d, 100000 * D + 1000 * H + W + i) for i, d in enumerate((0.05, 0.15, 0.3, 0.5))]
    for k in CONNECTIVITIES:
        for m in masks:
            check_label(m, k)


def _snake(D, H, W):
    """A one-voxel-wide path through every slice: every other row end to end, joined at alternating
    ends; a single voxel in every second slice joins the end of one slice's path to the next one's."""
    assert D % 2 == 1 and H % 4 == 1
    m = np.zeros((D, H, W), np.uint8)
    for z in range(0, D, 2):
        m[z, ::2, :] = 1
        for j, y in enumerate(range(1, H, 2)):
            m[z, y, W - 1 if j % 2 == 0 else 0] = 1
    for j, z in enumerate(range(1, D, 2)):
        y, x = (H - 1, W - 1) if j % 2 == 0 else (0, 0)
        m[z, y, x] = 1
    return m


def test_serpentine_through_every_slice():
    """Deep find chains and roots far from their members, in every orientation."""
    m = _snake(7, 13, 130)
    for k in CONNECTIVITIES:
        for v in (m, m[::-1].copy(), m[:, ::-1].copy(), m[:, :, ::-1].copy(), m[::-1, ::-1, ::-1].copy()):
            _, num = check_label(v, k)
            assert num.tolist() == [1]
        out, num, _ = check_filter(m, k, keep_largest=True, min_size=int(m.sum()))
        assert num.tolist() == [1] and np.array_equal(out, m)
        assert check_filter(m, k, min_size=int(m.sum()) + 1)[0].sum() == 0


def test_area_is_counted_per_run_segment():
    """One component made of runs longer than 64 pixels across three slices (and across chunk seams),
    next to a smaller one: min_size at the exact area keeps it, one more removes it."""
    m = np.zeros((3, 4, 200), np.uint8)
    m[0, 1, 3:140] = 1                                            # 137
    m[1, 1, 100:199] = 1                                          # 99
    m[2, 1, 60:130] = 1                                           # 70
    m[2, 2, 64:128] = 1                                           # 64: exactly one full word
    m[0, 3, 0:128] = 2                                            # 128 in two full words: another component
    area = 137 + 99 + 70 + 64
    for k in CONNECTIVITIES:
        out, num, _ = check_filter(m, k, keep_largest=True)
        assert num.tolist() == [2] and out.sum() == area
        assert check_filter(m, k, min_size=area)[0].sum() == area
        assert check_filter(m, k, min_size=area + 1)[0].sum() == 0
        assert check_filter(m, k, min_size=128)[0].sum() == area + 2 * 128


# ---------------------------------------------------------------- the filter
def test_filter_min_size_applies_before_keep_largest():
    m = np.zeros((4, 6, 80), np.uint8)
    m[0, 0, 0:3] = 1                                              # 3 voxels
    m[1:3, 2:4, 60:70] = 1                                        # 40 voxels over two slices and a seam
    m[3, 5, 79] = 1                                               # 1 voxel
    for k in CONNECTIVITIES:
        assert check_filter(m, k)[0].sum() == 44                  # neither option: the input
        assert check_filter(m, k, min_size=3)[0].sum() == 43      # a size equal to min_size stays
        assert check_filter(m, k, min_size=4)[0].sum() == 40
        assert check_filter(m, k, min_size=41)[0].sum() == 0
        assert check_filter(m, k, min_size=1 << 40)[0].sum() == 0
        assert check_filter(m, k, keep_largest=True, min_size=40)[0].sum() == 40
        out, num, _ = check_filter(m, k, keep_largest=True, min_size=41)
        assert out.sum() == 0 and num.tolist() == [3]             # counted before filtering
    check_filter(m, 18, keep_largest=True, want_num=False)


def test_filter_tie_goes_to_the_earlier_first_voxel():
    tie = next(c for c in CASES if c["name"] == "tie")["mask"]
    for k in CONNECTIVITIES:
        out, num, _ = check_filter(tie, k, keep_largest=True)
        assert num.tolist() == [2] and out[1:3, 6:9, 62:66].all() and out.sum() == 24
    # three components, the two largest equal and in different slices, the first component smaller;
    # the later of the two has the smaller in-slice position
    m = np.zeros((4, 5, 72), np.uint8)
    m[0, 0, 0] = 1
    m[1, 3, 66:70] = 1
    m[2, 0, 0:4] = 1
    m[2, 0, 5] = 1                                                # a fourth one between them
    out, num, _ = check_filter(m, 26, keep_largest=True)
    assert num.tolist() == [4] and out[1, 3, 66:70].all() and out.sum() == 4


def test_filter_keeps_class_ids():
    m = np.zeros((3, 10, 90), np.uint8)
    m[0:2, 2:8, 5:40] = 1
    m[1:3, 2:8, 40:70] = 2                                        # one component of two classes
    m[2, 9, 80:86] = 3
    m[0, 9, 0] = 200
    out, num, _ = check_filter(m, 26, keep_largest=True)
    assert num.tolist() == [3] and np.array_equal(out, np.where(m <= 2, m, 0))
    out, _, _ = check_filter(m, 6, min_size=2)
    assert np.array_equal(out, np.where(m <= 3, m, 0))


def test_filter_counts_with_and_without_ignore_index():
    P = _random((6, 12, 90), 0.2, 22)
    T = _random((6, 12, 90), 0.4, 23).astype(np.int64) * 3
    T[:, :, 70:] = 255
    T[4:, 8:, :] = 255
    for k in CONNECTIVITIES:
        for depths in (None, (2, 4)):
            _, _, with_ignore = check_filter(P, k, depths, keep_largest=True, target=T, ignore=255)
            _, _, plain = check_filter(P, k, depths, keep_largest=True, target=T)
            assert not np.array_equal(with_ignore, plain)         # without ignore a 255 pad is foreground
            check_filter(P, k, depths, min_size=4, target=T, ignore=255)
    check_filter(P, 26, (1, 5), target=T, ignore=255)


def test_filter_on_the_fixture_cases():
    for c in CASES:
        check_filter(c["mask"], 26, keep_largest=True)
        check_filter(c["mask"], 6, min_size=3)
        check_filter(c["mask"], 18, keep_largest=True, min_size=2)


def test_ragged_volumes_in_one_call_equal_single_volume_calls():
    depths = (2, 5, 1)
    m = np.concatenate([_random((d, 11, 70), dens, 50 + i) for i, (d, dens) in enumerate(zip(depths, (0.3, 0.15, 0.5)))])
    T = _random(m.shape, 0.4, 60).astype(np.int64)
    ends = np.cumsum(depths)
    for k in CONNECTIVITIES:
        labels, num = check_label(m, k, depths)
        out, fnum, counts = check_filter(m, k, depths, keep_largest=True, min_size=2, target=T)
        for v, (d, e) in enumerate(zip(depths, ends)):
            one_labels, one_num = run_label(m[e - d:e], None, k, 0xAA)
            assert np.array_equal(labels[e - d:e], one_labels) and num[v] == one_num[0]
            one = run_filter(m[e - d:e], None, k, True, 2, T[e - d:e], -1, 0xAA)
            assert np.array_equal(out[e - d:e], one[0]) and fnum[v] == one[1][0]
            assert np.array_equal(counts[v], one[2][0])


# ---------------------------------------------------------------- one family: depth-1 volumes are images
@pytest.mark.parametrize("name,m,t", depth_one_inputs(), ids=[i[0] for i in depth_one_inputs()])
def test_depth_one_volumes_are_images(name, m, t):
    """The volume instantiation on volumes one slice deep against the image instantiation on the same
    slices, 6 / 18 / 26 against 4 / 8 / 8: labels, num, filtered mask and counts, bit for bit
    (tests/test_components3d_cpu.py shows the same identity for the numpy oracles on these inputs)."""
    from stfunet import connected_components, connected_components_3d, filter_components, filter_components_3d
    d, target = torch.from_numpy(m).to(DEV), torch.from_numpy(t).to(DEV)
    ones = [1] * m.shape[0]
    for k in CONNECTIVITIES:
        l3, n3 = connected_components_3d(d, ones, k)
        l2, n2 = connected_components(d, FLAT[k])
        assert torch.equal(l3, l2) and torch.equal(n3, n2)
        f3, c3 = filter_components_3d(d, ones, True, 3, k, target=target, ignore_index=2)
        f2, c2 = filter_components(d, True, 3, FLAT[k], target=target, ignore_index=2)
        assert torch.equal(f3, f2) and torch.equal(c3, c2)


# ---------------------------------------------------------------- the Python surface
def test_python_surface():
    from stfunet import connected_components, connected_components_3d, filter_components_3d, image_metrics
    depths = (3, 1, 4)
    m = _random((8, 17, 70), 0.2, 13)
    T = _random(m.shape, 0.5, 17).astype(np.int64)
    T[5, :, 50:] = 255
    d = torch.from_numpy(m).to(DEV)
    for k in CONNECTIVITIES:
        ref, ref_num = stack_label(m, depths, k)
        for t in (d, d.bool(), d.long() * 7):
            labels, num = connected_components_3d(t, depths, connectivity=k)
            assert labels.dtype == torch.int32 and num.dtype == torch.int32 and labels.is_cuda and num.is_cuda
            assert np.array_equal(labels.cpu().numpy(), ref) and np.array_equal(num.cpu().numpy(), ref_num)
        want, _, want_counts = stack_filter(m, depths, True, 2, k, T, 255)
        out = filter_components_3d(d, depths, keep_largest=True, min_size=2, connectivity=k)
        assert out.dtype == torch.uint8 and out.is_cuda and np.array_equal(out.cpu().numpy(), want)
        out, counts = filter_components_3d(d.bool(), list(depths), True, 2, k, target=torch.from_numpy(T).int().to(DEV),
                                           ignore_index=255)
        assert counts.dtype == torch.int64 and tuple(counts.shape) == (3, 3)
        assert np.array_equal(out.cpu().numpy(), want) and np.array_equal(counts.cpu().numpy(), want_counts)
        dice, iou = image_metrics(counts)
        assert tuple(dice.shape) == (3,) and dice.dtype == torch.float64
    labels, num = connected_components_3d(d)                       # one volume, 26 neighbours
    ref, ref_num = stack_label(m, None, 26)
    assert np.array_equal(labels.cpu().numpy(), ref) and num.tolist() == ref_num.tolist()
    # depth 1 everywhere: the 2-D labels with 6 -> 4 and 18, 26 -> 8
    for k3, k2 in ((6, 4), (18, 8), (26, 8)):
        l3, n3 = connected_components_3d(d, [1] * 8, k3)
        l2, n2 = connected_components(d, k2)
        assert torch.equal(l3, l2) and torch.equal(n3, n2)
    same = filter_components_3d(d * 5, depths)                     # neither option: the input comes back
    assert torch.equal(same, d * 5) and same.data_ptr() != d.data_ptr()
    empty = torch.zeros(0, 4, 4, dtype=torch.uint8, device=DEV)
    labels, num = connected_components_3d(empty)
    assert tuple(labels.shape) == (0, 4, 4) and tuple(num.shape) == (0,)
    out, counts = filter_components_3d(empty, [], target=torch.zeros(0, 4, 4, dtype=torch.int64, device=DEV))
    assert tuple(out.shape) == (0, 4, 4) and tuple(counts.shape) == (0, 3)


# ---------------------------------------------------------------- the loop over volumes
DEPTHS = (3, 5, 2)


def _pattern():
    """bool [10, 32, 32] in volumes of DEPTHS.  Volume 0: a block through all three slices and a
    speck.  Volume 1: a block through slices 3..6 and, alone in slice 7, a smaller block that touches
    nothing.  Volume 2: a block in slice 8 whose thin top, two voxels, lies in slice 9."""
    p = torch.zeros(10, 32, 32, dtype=torch.bool)
    p[0:3, 4:12, 5:15] = True
    p[1, 28, 2] = True
    p[3:7, 10:20, 8:20] = True
    p[7, 2:6, 24:30] = True
    p[8, 6:14, 6:14] = True
    p[9, 9, 9:11] = True
    return p


class Fixed(torch.nn.Module):
    """A model whose logits are fixed: slice i of the loader gets ``pattern[i]`` as its argmax mask."""
    input_format = "flat_channels"

    def __init__(self, pattern):
        super().__init__()
        self.at = 0
        self.register_buffer("logits", torch.stack([torch.zeros(pattern.shape), pattern.float() * 2 - 1], 1))

    def forward(self, x):
        out = self.logits[self.at:self.at + x.shape[0]]
        self.at = (self.at + x.shape[0]) % self.logits.shape[0]
        return {"out": out}


def _loader(n, batch, targets=True, seed=70):
    T = _random((n, 32, 32), 0.3, seed).astype(np.int64)
    T[:, :, 30:] = 255
    T |= _pattern().numpy()[:n] & (_random((n, 32, 32), 0.8, seed + 1) != 0)
    batches = []
    for a in range(0, n, batch):
        x = torch.zeros(min(batch, n - a), 1, 1, 32, 32)
        batches.append((x, torch.from_numpy(T[a:a + batch])) if targets else x)
    return batches, T


def test_predict_volumes_equals_the_restatement():
    from stfunet import image_metrics, predict_volumes
    from stfunet.predict import predict
    model, dev = Fixed(_pattern()).to(DEV), torch.device(DEV)
    loader, T = _loader(10, 4)
    raw = _pattern().numpy().astype(np.uint8)
    for kw in (dict(keep_largest=True), dict(min_size=3, connectivity=6), dict(keep_largest=True, min_size=200),
               dict(keep_largest=True, connectivity=18, ignore_index=255)):
        opts = {k: v for k, v in kw.items() if k != "ignore_index"}
        res = predict_volumes(model, loader, dev, DEPTHS, keep_masks=True, **kw)
        assert set(res) == {"num", "num_volumes", "dice", "iou", "mean_dice", "mean_iou", "num_components", "masks"}
        assert res["num"] == 10 and res["num_volumes"] == 3
        want, want_num, want_counts = stack_filter(raw, DEPTHS, target=T, ignore=kw.get("ignore_index"), **opts)
        assert [tuple(m.shape) for m in res["masks"]] == [(d, 32, 32) for d in DEPTHS]
        assert all(m.dtype == torch.uint8 and m.is_cuda for m in res["masks"])
        assert np.array_equal(torch.cat(res["masks"]).cpu().numpy(), want)
        nc = res["num_components"]
        assert nc.is_cuda and nc.dtype == torch.int64 and nc.tolist() == want_num.tolist()
        dice, iou = image_metrics(torch.from_numpy(want_counts).to(DEV))
        assert torch.equal(res["dice"], dice) and torch.equal(res["iou"], iou) and tuple(dice.shape) == (3,)
        assert torch.equal(res["mean_dice"], dice.mean()) and torch.equal(res["mean_iou"], iou.mean())
    # the difference the feature exists for: the block alone in slice 7 goes with its volume's largest
    # component kept, and stays when every slice keeps its own largest one
    vol = predict_volumes(model, loader, dev, DEPTHS, keep_largest=True, keep_masks=True)
    per_slice = predict(model, loader, dev, keep_largest=True, keep_masks=True)
    assert not vol["masks"][1][4].any() and torch.cat(per_slice["masks"])[7].sum() == 24
    assert vol["num_components"].tolist() == [2, 2, 1]
    # and the thin top of volume 2 survives a min_size in voxels, but not one per slice
    vol = predict_volumes(model, loader, dev, DEPTHS, min_size=3, keep_masks=True)
    per_slice = predict(model, loader, dev, min_size=3, keep_masks=True)
    assert vol["masks"][2][1].sum() == 2 and not torch.cat(per_slice["masks"])[9].any()
    # without targets: masks and component counts, no metrics
    bare = predict_volumes(model, _loader(10, 4, targets=False)[0], dev, DEPTHS, keep_largest=True, keep_masks=True)
    assert bare["dice"] is None and bare["mean_iou"] is None
    assert np.array_equal(torch.cat(bare["masks"]).cpu().numpy(), stack_filter(raw, DEPTHS, True)[0])


def test_predict_volumes_with_the_options_off_sums_the_slice_counts():
    from stfunet import image_metrics, predict_volumes
    from stfunet.predict import predict
    model, dev = Fixed(_pattern()).to(DEV), torch.device(DEV)
    loader, T = _loader(10, 4)
    raw = _pattern().numpy().astype(np.uint8)
    for ignore in (None, 255):
        res = predict_volumes(model, loader, dev, DEPTHS, ignore_index=ignore, keep_masks=True)
        assert set(res) == {"num", "num_volumes", "dice", "iou", "mean_dice", "mean_iou", "masks"}
        per_slice = predict(model, loader, dev, ignore_index=ignore, keep_masks=True)
        assert np.array_equal(torch.cat(res["masks"]).cpu().numpy(), raw)
        assert torch.equal(torch.cat(res["masks"]), torch.cat(per_slice["masks"]))
        _, _, counts = stack_filter(raw, DEPTHS, target=T, ignore=ignore)
        dice, iou = image_metrics(torch.from_numpy(counts).to(DEV))
        assert torch.equal(res["dice"], dice) and torch.equal(res["iou"], iou)
        assert not torch.equal(res["mean_dice"], per_slice["mean_dice"])     # per case, not per slice
    # the same numbers from predict's own per-slice counts, summed by volume
    from stfunet import predict_masks
    slice_counts = torch.cat([predict_masks(model(x.to(DEV)), target=t.to(DEV))[1] for x, t in loader])
    ends = np.cumsum(DEPTHS)
    summed = torch.stack([slice_counts[e - d:e].sum(0) for d, e in zip(DEPTHS, ends)])
    dice, iou = image_metrics(summed)
    res = predict_volumes(model, loader, dev, DEPTHS)
    assert torch.equal(res["dice"], dice) and torch.equal(res["iou"], iou) and "masks" not in res


def test_predict_volumes_refuses_a_wrong_slice_total():
    from stfunet import predict_volumes
    model, dev = Fixed(_pattern()).to(DEV), torch.device(DEV)
    loader, _ = _loader(10, 4)
    for kw in ({}, dict(keep_largest=True)):
        for bad in ((3, 5, 3), (3, 5, 1), (3, 5), (11,)):
            model.at = 0
            with pytest.raises(ValueError, match="slices"):
                predict_volumes(model, loader, dev, bad, **kw)


def test_one_filter_call_per_flush_and_none_with_the_options_off():
    from stfunet import predict_volumes
    model, dev = Fixed(_pattern()).to(DEV), torch.device(DEV)
    loader, _ = _loader(10, 4)
    raw = _pattern().numpy().astype(np.uint8)

    def traced(depths, **kw):
        model.at = 0
        with lt.tracing() as trace:
            res = predict_volumes(model, loader, dev, depths, keep_masks=True, **kw)
            torch.cuda.synchronize()
            return res, [e if isinstance(e, str) else e[0] for e in trace]

    # batches of 4, 4, 2 slices.  (3, 5, 2): every batch completes one volume.  (1, 1, 2, 5, 1): the
    # first batch completes three volumes in one call, the second none, the third two in one call.
    for depths, flushes in ((DEPTHS, 3), ((1, 1, 2, 5, 1), 2), ((10,), 1)):
        res, got = traced(depths, keep_largest=True)
        assert got.count("stf_ccl3d_filter") == flushes and got.count("stf_predict_mask") == 3
        assert not any(e in ("stf_ccl_filter", "stf_ccl_label", "stf_ccl3d_label") for e in got)
        assert np.array_equal(torch.cat(res["masks"]).cpu().numpy(), stack_filter(raw, depths, True)[0])
        assert [m.shape[0] for m in res["masks"]] == list(depths)
        _, off = traced(depths)
        assert not any("ccl" in e for e in off) and off.count("stf_predict_mask") == 3
