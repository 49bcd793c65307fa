"""Connected-component post-processing on the GPU (csrc/ccl.hip through the C entry points and
stfunet.predict) against tests/golden/components.npz (scipy's labels) and the numpy restatement of
tests/_components_ref.py, which tests/test_components_cpu.py pins to that fixture.

Everything is an integer, so every comparison is equality, element for element.

The kernel-level tests call the C entry points on buffers with 64 guard bytes on each side and run
every case twice, the buffers (scratch included) prefilled with 0xAA and then 0x55: equal results
show that every output byte is written and that two runs agree bit for bit; the guards must keep
their fill.
"""
import ctypes

import numpy as np
import pytest
import torch

import _launch_trace as lt
from _components_ref import batch_filter, batch_label, fixture_cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
EINVAL = 100001
CASES = fixture_cases()
BOTH = (4, 8)


class Guarded:
    """``nbytes`` of device memory between two guards, everything prefilled with ``fill``; the body
    starts ``offset`` bytes past a 64-byte boundary."""

    def __init__(self, nbytes, fill, offset=0):
        self.fill, self.n, self.lead = fill, nbytes, GUARD + offset
        self.raw = torch.full((nbytes + 2 * GUARD + offset,), fill, dtype=torch.uint8, device=DEV)
        self.body = self.raw[self.lead:self.lead + nbytes]
        assert self.raw.data_ptr() % 64 == 0

    def guards_intact(self):
        return bool((self.raw[:self.lead] == self.fill).all() and (self.raw[self.lead + self.n:] == self.fill).all())


def _scratch(B, H, W, fill, offset=0):
    from stfunet import _lib
    nbytes = _lib.load().stf_ccl_scratch_bytes(B, H, W)
    assert nbytes >= 8 * B * H * W
    return Guarded(nbytes, fill, offset)


def _u8(a, offset=0):
    """uint8 device copy of ``a`` whose base address is ``offset`` bytes past an allocation's."""
    flat = torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8)).flatten()
    buf = torch.zeros(flat.numel() + offset, dtype=torch.uint8, device=DEV)
    buf[offset:] = flat.to(DEV)
    return buf[offset:]


def run_label(mask, connectivity, fill=0xAA, mask_offset=0, labels_offset=0):
    from stfunet._lib import call, stream
    B, H, W = mask.shape
    m = _u8(mask, mask_offset)
    labels, num = Guarded(B * H * W * 4, fill, labels_offset), Guarded(B * 4, fill, labels_offset)
    scratch = _scratch(B, H, W, fill)
    call("stf_ccl_label", m.data_ptr(), B, H, W, connectivity, labels.body.data_ptr(), num.body.data_ptr(),
         scratch.body.data_ptr(), stream())
    torch.cuda.synchronize()
    assert labels.guards_intact() and num.guards_intact() and scratch.guards_intact()
    return (labels.body.cpu().numpy().view(np.int32).reshape(B, H, W), num.body.cpu().numpy().view(np.int32))


def check_label(mask, connectivity, **kw):
    """Two runs on differently prefilled buffers agree and equal the numpy oracle."""
    mask = np.asarray(mask, dtype=np.uint8)
    mask = mask[None] if mask.ndim == 2 else mask
    labels, num = run_label(mask, connectivity, 0xAA, **kw)
    labels2, num2 = run_label(mask, connectivity, 0x55, **kw)
    assert np.array_equal(labels, labels2) and np.array_equal(num, num2)
    ref, ref_num = batch_label(mask, connectivity)
    assert np.array_equal(num, ref_num), (num.tolist(), ref_num.tolist())
    assert np.array_equal(labels, ref)
    return labels, num


def run_filter(mask, connectivity=8, keep_largest=False, min_size=0, target=None, ignore=-1, fill=0xAA,
               want_num=True, mask_offset=0):
    from stfunet._lib import call, stream
    B, H, W = mask.shape
    m = _u8(mask, mask_offset)
    t = None if target is None else torch.from_numpy(np.ascontiguousarray(target, dtype=np.int64)).to(DEV)
    out, num, scratch = Guarded(B * H * W, fill, mask_offset), Guarded(B * 4, fill), _scratch(B, H, W, fill)
    counts = None if target is None else Guarded(B * 24, fill)
    call("stf_ccl_filter", m.data_ptr(), None if t is None else t.data_ptr(), B, H, W, connectivity,
         int(keep_largest), min_size, ignore, out.body.data_ptr(), None if counts is None else counts.body.data_ptr(),
         num.body.data_ptr() if want_num else None, scratch.body.data_ptr(), stream())
    torch.cuda.synchronize()
    assert out.guards_intact() and num.guards_intact() and scratch.guards_intact()
    assert counts is None or counts.guards_intact()
    assert want_num or bool((num.body == fill).all())
    return (out.body.cpu().numpy().reshape(B, H, W), num.body.cpu().numpy().view(np.int32) if want_num else None,
            None if counts is None else counts.body.cpu().numpy().view(np.int64).reshape(B, 3))


def check_filter(mask, connectivity=8, keep_largest=False, min_size=0, target=None, ignore=None, **kw):
    mask = np.asarray(mask, dtype=np.uint8)
    mask = mask[None] if mask.ndim == 2 else mask
    if target is not None:
        target = np.asarray(target, dtype=np.int64).reshape(mask.shape)
    ign = -1 if ignore is None else ignore
    first = run_filter(mask, connectivity, keep_largest, min_size, target, ign, 0xFF, **kw)
    second = run_filter(mask, connectivity, keep_largest, min_size, target, ign, 0x55, **kw)
    ref = list(batch_filter(mask, keep_largest, min_size, connectivity, target, ignore))
    if not kw.get("want_num", True):
        ref[1] = None                                             # num is optional: not asked for, not written
    for a, b, r in zip(first, second, ref):
        assert (a is None) == (r is None)
        if a is not None:
            assert np.array_equal(a, b) and np.array_equal(a, r), (a.tolist(), r.tolist())
    return first


def _random(H, W, density, seed):
    return (np.random.default_rng(seed).random((H, W)) < density).astype(np.uint8)


# ---------------------------------------------------------------- labels
@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_labels_equal_the_fixture(c):
    for k in BOTH:
        labels, num = check_label(c["mask"], k)
        assert num.tolist() == [c[f"n{k}"]]                      # scipy's own numbers, as committed
        assert np.array_equal(labels[0], c[f"labels{k}"])


def test_fixture_cases_as_one_batch():
    """All cases padded to a common size as one batch: every image its own answer, no label leaks
    from one image into the next."""
    H, W = max(c["mask"].shape[0] for c in CASES), max(c["mask"].shape[1] for c in CASES)
    batch = np.zeros((len(CASES), H, W), np.uint8)
    for b, c in enumerate(CASES):
        batch[b, :c["mask"].shape[0], :c["mask"].shape[1]] = c["mask"]
    for k in BOTH:
        labels, num = run_label(batch, k)
        for b, c in enumerate(CASES):
            h, w = c["mask"].shape
            assert num[b] == c[f"n{k}"], c["name"]
            assert np.array_equal(labels[b, :h, :w], c[f"labels{k}"]), c["name"]
            assert not labels[b, h:].any() and not labels[b, :, w:].any()


@pytest.mark.parametrize("H,W", [(1, 1), (1, 64), (1, 65), (64, 1), (3, 63), (3, 64), (3, 65), (5, 129), (2, 4096)])
def test_label_seam_shapes(H, W):
    """Below, at and above one 64-pixel chunk, single rows and columns, the widest row: all ones (one
    run across every seam), alternating columns and a random mask."""
    cols = np.zeros((H, W), np.uint8)
    cols[:, ::2] = 1
    for k in BOTH:
        _, num = check_label(np.ones((H, W), np.uint8), k)
        assert num.tolist() == [1]
        _, num = check_label(cols, k)
        assert num.tolist() == [(W + 1) // 2]
        check_label(_random(H, W, 0.55, 1000 * H + W), k)


def test_runs_across_every_chunk_seam():
    """Runs that start and end at every position around the 64-pixel seams, joined from the row above
    or below, straight and by a corner."""
    W = 200
    m = np.zeros((12, W), np.uint8)
    for i, (a, b) in enumerate([(60, 70), (63, 64), (64, 65), (62, 63), (0, 199), (127, 129), (120, 192)]):
        m[i, a:b + 1] = 1
    m[8, 63] = m[9, 64] = m[10, 63] = 1                           # a zigzag over the seam: corners only
    m[11, 127] = m[11, 129] = 1
    m[10, 128] = 1
    for k in BOTH:
        check_label(m, k)
        check_label(m[::-1].copy(), k)
        check_label(m[:, ::-1].copy(), k)


def test_label_misaligned_base_pointers():
    """mask at any byte; labels and num 4-byte aligned are enough."""
    m = _random(19, 68, 0.5, 11)
    for k in BOTH:
        check_label(m, k, mask_offset=1)
        check_label(m, k, mask_offset=3, labels_offset=4)


def test_connected_components_python_surface():
    from stfunet import connected_components
    m = np.stack([_random(17, 70, 0.3, 13), _random(17, 70, 0.6, 14), np.zeros((17, 70), np.uint8)])
    for k in BOTH:
        ref, ref_num = batch_label(m, k)
        for t in (torch.from_numpy(m), torch.from_numpy(m).bool(), torch.from_numpy(m).long() * 7):
            labels, num = connected_components(t.to(DEV), connectivity=k)
            assert labels.dtype == torch.int32 and num.dtype == torch.int32 and labels.is_cuda and num.is_cuda
            assert np.array_equal(labels.cpu().numpy(), ref) and np.array_equal(num.cpu().numpy(), ref_num)
    labels, num = connected_components(torch.from_numpy(m).to(DEV))
    assert np.array_equal(num.cpu().numpy(), batch_label(m, 8)[1])                  # 8 is the default
    labels, num = connected_components(torch.zeros(0, 4, 4, dtype=torch.uint8, device=DEV))
    assert tuple(labels.shape) == (0, 4, 4) and tuple(num.shape) == (0,)


# ---------------------------------------------------------------- the filter
def test_filter_tie_keeps_the_raster_first_component():
    tie = next(c for c in CASES if c["name"] == "tie")["mask"]
    for k in BOTH:
        out, num, _ = check_filter(tie, k, keep_largest=True)
        assert num.tolist() == [2] and out[0, 5:11, 60:64].all() and out.sum() == 24
    m = np.zeros((8, 72), np.uint8)
    m[0, 0] = 1
    m[2:4, 66:69] = 1
    m[3:5, 1:4] = 1
    out, num, _ = check_filter(m, 8, keep_largest=True)
    assert num.tolist() == [3] and out[0, 2:4, 66:69].all() and out.sum() == 6


def test_filter_min_size_and_keep_largest():
    m = np.zeros((9, 80), np.uint8)
    m[0, 0:3] = 1                                                 # area 3
    m[4:6, 60:70] = 1                                             # area 20, over a chunk seam
    m[8, 79] = 1                                                  # area 1
    for k in BOTH:
        assert check_filter(m, k)[0].sum() == 24                  # neither option: the input
        assert check_filter(m, k, min_size=3)[0].sum() == 23      # an area equal to min_size stays
        assert check_filter(m, k, min_size=4)[0].sum() == 20
        assert check_filter(m, k, min_size=20)[0].sum() == 20
        assert check_filter(m, k, min_size=21)[0].sum() == 0      # above every area: empty
        assert check_filter(m, k, min_size=1 << 40)[0].sum() == 0
        assert check_filter(m, k, keep_largest=True, min_size=20)[0].sum() == 20
        out, num, _ = check_filter(m, k, keep_largest=True, min_size=21)
        assert out.sum() == 0 and num.tolist() == [3]             # counted before filtering
    batch = np.stack([m, np.zeros_like(m), np.ones_like(m), m[::-1]])
    out, num, _ = check_filter(batch, 8, keep_largest=True, min_size=2)
    assert num.tolist() == [3, 0, 1, 3] and out[1].sum() == 0 and out[2].all()
    check_filter(batch, 4, keep_largest=True, want_num=False)


def _comb():
    """uint8 [2, 4, 130].  Image 0: a spine over the full width of row 0 (three chunks, both seams)
    with teeth down rows 1..3, one of them across the first seam, and between the teeth of chunk 0 two
    components of their own on rows 2..3 that pass under a short tooth each -- so within one chunk of
    rows 2 and 3 the run segments alternate between the spine's root and another, and row 3 starts
    with a root that is not the spine's.  Image 1: full."""
    m = np.zeros((2, 4, 130), np.uint8)
    m[0, 0, :] = 1
    for x in (40, 62, 63, 64, 65, 66, 100, 129):
        m[0, 1:4, x] = 1                                          # long teeth
    m[0, 1:3, 2] = 1                                              # a tooth that stops above row 3
    m[0, 1, 10] = m[0, 1, 30] = 1                                 # short teeth
    m[0, 3, 5:19] = m[0, 2, 5:8] = m[0, 2, 14:17] = 1             # component A, under the tooth at 10
    m[0, 3, 24:37] = m[0, 2, 24:27] = m[0, 2, 34:37] = 2          # component B, under the tooth at 30
    m[1] = 1
    return m


def test_exact_areas_of_a_comb_across_chunk_seams():
    """The areas compress collects, whether every run segment adds on its own (images) or the
    segments of a chunk's first root are summed in the wave and carried along the row (volumes; the
    form is a compile-time parameter of the one body): min_size at each component's exact area keeps
    it, one more removes it."""
    m = _comb()
    for k in BOTH:
        labels, num = batch_label(m, k)
        assert num.tolist() == [3, 1]
        areas = np.bincount(labels[0].ravel())[1:].tolist()
        assert areas == [int(m[0].astype(bool).sum()) - 20 - 19, 20, 19]     # the spine, A, B
        for a in areas + [4 * 130]:
            kept = check_filter(m, k, min_size=a)[0]
            gone = check_filter(m, k, min_size=a + 1)[0]
            assert kept.astype(bool).sum() - gone.astype(bool).sum() == a
        out, _, _ = check_filter(m, k, keep_largest=True, min_size=areas[0])
        assert np.array_equal(out[0] != 0, labels[0] == 1) and out[1].all()


def test_filter_keeps_class_ids():
    m = np.zeros((20, 90), np.uint8)
    m[2:10, 5:40] = 1
    m[2:10, 40:70] = 2                                            # one component of two classes
    m[15:18, 60:66] = 3
    m[19, 0] = 200
    out, num, _ = check_filter(m, 8, keep_largest=True)
    assert num.tolist() == [3] and np.array_equal(out[0], np.where(m <= 2, m, 0))
    out, _, _ = check_filter(m, 4, min_size=2)
    assert np.array_equal(out[0], np.where(m <= 3, m, 0))


def test_filter_counts_with_and_without_ignore_index():
    P = np.stack([_random(24, 90, 0.45, 22), _random(24, 90, 0.6, 24)])
    T = np.stack([_random(24, 90, 0.4, 23), _random(24, 90, 0.4, 25)]).astype(np.int64) * 3
    T[:, :, 70:] = 255
    T[:, 20:, :] = 255
    for k in BOTH:
        _, _, with_ignore = check_filter(P, k, keep_largest=True, target=T, ignore=255)
        _, _, plain = check_filter(P, k, keep_largest=True, target=T)
        assert not np.array_equal(with_ignore, plain)             # without ignore a 255 pad is foreground
        check_filter(P, k, min_size=4, target=T, ignore=255)
    check_filter(P, 8, target=T, ignore=255)


def test_filter_on_the_fixture_cases():
    for c in CASES:
        check_filter(c["mask"], 8, keep_largest=True)
        check_filter(c["mask"], 4, min_size=3)


def test_filter_misaligned_mask_and_out():
    m = _random(19, 68, 0.5, 12)
    check_filter(m, 8, keep_largest=True, mask_offset=1)
    check_filter(m, 4, min_size=3, mask_offset=7)


def test_filter_components_python_surface():
    from stfunet import filter_components
    m = np.stack([_random(17, 70, 0.45, 15), _random(17, 70, 0.6, 16), np.zeros((17, 70), np.uint8)])
    T = np.stack([_random(17, 70, 0.5, 17 + i) for i in range(3)]).astype(np.int64)
    T[1, :, 50:] = 255
    d = torch.from_numpy(m).to(DEV)
    for k in BOTH:
        ref, _, ref_counts = batch_filter(m, True, 2, k, T, 255)
        out = filter_components(d, keep_largest=True, min_size=2, connectivity=k)
        assert out.dtype == torch.uint8 and out.is_cuda and np.array_equal(out.cpu().numpy(), ref)
        out, counts = filter_components(d.bool(), True, 2, k, target=torch.from_numpy(T).int().to(DEV),
                                        ignore_index=255)
        assert counts.dtype == torch.int64 and tuple(counts.shape) == (3, 3)
        assert np.array_equal(out.cpu().numpy(), ref) and np.array_equal(counts.cpu().numpy(), ref_counts)
    same = filter_components(d * 5)                                # neither option: the input comes back
    assert torch.equal(same, d * 5) and same.data_ptr() != d.data_ptr()
    out, counts = filter_components(torch.zeros(0, 4, 4, dtype=torch.uint8, device=DEV),
                                    target=torch.zeros(0, 4, 4, dtype=torch.int64, device=DEV))
    assert tuple(out.shape) == (0, 4, 4) and tuple(counts.shape) == (0, 3)


# ---------------------------------------------------------------- determinism
def test_percolation_mask_twice_bit_identical():
    from stfunet import connected_components, filter_components
    m = np.stack([_random(128, 128, 0.593, 300 + b) for b in range(8)])
    T = np.stack([_random(128, 128, 0.5, 400 + b) for b in range(8)]).astype(np.int64)
    d, t = torch.from_numpy(m).to(DEV), torch.from_numpy(T).to(DEV)
    for k in BOTH:
        l1, n1 = connected_components(d, k)
        l2, n2 = connected_components(d, k)
        assert torch.equal(l1, l2) and torch.equal(n1, n2)
        f1, c1 = filter_components(d, True, 5, k, target=t)
        f2, c2 = filter_components(d, True, 5, k, target=t)
        assert torch.equal(f1, f2) and torch.equal(c1, c2)
        # the filter recomputed on the host from the device labels
        labels, num = l1.cpu().numpy(), n1.cpu().numpy()
        for b in range(8):
            areas = np.bincount(labels[b].ravel(), minlength=num[b] + 1)[1:]
            first = 1 + int(np.argmax(areas))
            want = np.where((labels[b] == first) & (areas[first - 1] >= 5), m[b], 0)
            assert np.array_equal(f1[b].cpu().numpy(), want)
            assert c1[b].tolist() == [int(((want != 0) & (T[b] > 0)).sum()), int((want != 0).sum()),
                                      int((T[b] > 0).sum())]
    ref, ref_num = batch_label(m[:2], 4)                          # and the labels are the oracle's
    l4, n4 = connected_components(d[:2], 4)
    assert np.array_equal(l4.cpu().numpy(), ref) and np.array_equal(n4.cpu().numpy(), ref_num)


# ---------------------------------------------------------------- refusals
def test_scratch_misaligned_by_four_is_refused_and_untouched():
    from stfunet import _lib
    lib = _lib.load()
    B, H, W = 1, 5, 70
    m = _u8(_random(H, W, 0.5, 1)[None])
    st = ctypes.c_void_p(_lib.stream())
    labels, num, out = Guarded(B * H * W * 4, 0xAA), Guarded(B * 4, 0xAA), Guarded(B * H * W, 0xAA)
    scratch = _scratch(B, H, W, 0xAA, offset=4)
    assert scratch.body.data_ptr() % 8 == 4
    p = lambda g: ctypes.c_void_p(g.body.data_ptr())
    assert lib.stf_ccl_label(ctypes.c_void_p(m.data_ptr()), B, H, W, 8, p(labels), p(num), p(scratch), st) == EINVAL
    assert lib.stf_ccl_filter(ctypes.c_void_p(m.data_ptr()), None, B, H, W, 8, 1, 0, -1, p(out), None, p(num),
                              p(scratch), st) == EINVAL
    torch.cuda.synchronize()
    assert all(bool((g.raw == 0xAA).all()) for g in (labels, num, out, scratch))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_einval_without_a_launch(dtype):
    """Refusals with real device buffers far smaller than the refused sizes: nothing may touch them."""
    from stfunet import _lib
    lib = _lib.load(dtype)
    buf, other = Guarded(4096, 0xAA), Guarded(4096, 0xAA)
    p, q = ctypes.c_void_p(buf.body.data_ptr()), ctypes.c_void_p(other.body.data_ptr())
    st = ctypes.c_void_p(_lib.stream())

    def at(offset):
        return ctypes.c_void_p(other.body.data_ptr() + offset)

    def lab(mask=p, B=1, H=4, W=4, conn=8, labels=q, num=q, scratch=q):
        return lib.stf_ccl_label(mask, B, H, W, conn, labels, num, scratch, st)

    def fil(mask=p, target=q, B=1, H=4, W=4, conn=8, min_size=0, out=q, counts=q, num=q, scratch=q):
        return lib.stf_ccl_filter(mask, target, B, H, W, conn, 1, min_size, -1, out, counts, num, scratch, st)

    assert lab(mask=None) == EINVAL and lab(labels=None) == EINVAL and lab(num=None) == EINVAL
    assert lab(scratch=None) == EINVAL and lab(labels=at(2)) == EINVAL
    assert fil(mask=None) == EINVAL and fil(out=None) == EINVAL and fil(scratch=None) == EINVAL
    assert fil(target=None) == EINVAL and fil(out=p) == EINVAL and fil(min_size=-1) == EINVAL
    assert fil(counts=at(4)) == EINVAL and fil(target=at(4)) == EINVAL
    for f in (lab, fil):
        assert f(conn=0) == EINVAL and f(conn=6) == EINVAL and f(conn=1) == EINVAL
        assert f(B=0) == EINVAL and f(H=0) == EINVAL and f(W=0) == EINVAL
        assert f(H=4097) == EINVAL and f(W=4097) == EINVAL
        assert f(B=128, H=4096, W=4096) == EINVAL and f(B=1 << 19, H=64, W=64) == EINVAL
        assert f(scratch=at(4)) == EINVAL and f(num=at(2)) == EINVAL
    torch.cuda.synchronize()
    assert bool((buf.raw == 0xAA).all()) and bool((other.raw == 0xAA).all())


# ---------------------------------------------------------------- the predict loop
def _pattern():
    """bool [6, 32, 32]: image i holds a block of (6 + i) x 10 pixels and i single-pixel specks."""
    p = torch.zeros(6, 32, 32, dtype=torch.bool)
    for i in range(6):
        p[i, 4:10 + i, 5:15] = True
        for j in range(i):
            p[i, 28, 2 + 4 * j] = True
    return p


class Speckled(torch.nn.Module):
    """A real UNet whose logits get their sign from a fixed pattern: the forward runs on the kernels,
    and the argmax mask of slice i of the loader is ``pattern[i]`` whatever the weights are (the
    canonical weights alone predict foreground everywhere at this size)."""
    input_format = "flat_channels"

    def __init__(self, unet, pattern):
        super().__init__()
        self.unet, self.at = unet, 0
        self.register_buffer("pattern", pattern)

    def forward(self, x):
        out = self.unet(x)["out"]
        p = self.pattern[self.at:self.at + out.shape[0]]
        self.at = (self.at + out.shape[0]) % self.pattern.shape[0]
        mag = (out[:, 1] - out[:, 0]).abs().float() + 1
        return {"out": torch.stack([torch.zeros_like(mag), torch.where(p, mag, -mag)], 1)}


def _unet_and_loader(speckled=False):
    from oracle.cases import dce_case
    from oracle.init import canonical_state_dict
    from stfunet.unet import UNet
    model = UNet(in_channels=8, num_classes=2, base_c=8)
    model.load_state_dict(canonical_state_dict(model.state_dict(), seed=0))
    loader = [dce_case(400 + i, 3, 8, 32, 32) for i in range(2)]
    loader[1][1][1].zero_()                                  # image 4 of 6: an empty target
    if speckled:
        model = Speckled(model, _pattern())
    return model.to(DEV), loader


def _assembled(plain, loader, **kw):
    """The loop's results from its pieces: every kept raw mask through filter_components, the counts
    through image_metrics, the filtered masks through boundary_metrics."""
    from stfunet import boundary_metrics, filter_components, image_metrics
    masks, counts, bm = [], [], []
    for m, (_, t) in zip(plain["masks"], loader):
        f, c = filter_components(m, target=t.to(DEV), **kw)
        masks.append(f)
        counts.append(c)
        bm.append(boundary_metrics(f, t.to(DEV)))
    dice, iou = image_metrics(torch.cat(counts))
    return masks, dice, iou, {k: torch.cat([b[k] for b in bm]) for k in ("hd", "hd95", "assd")}


def test_predict_with_components_equals_the_pieces():
    from stfunet import connected_components
    from stfunet.predict import predict
    model, loader = _unet_and_loader(speckled=True)
    dev = torch.device(DEV)
    plain = predict(model, loader, dev, keep_masks=True, boundary=True)
    raw = torch.cat(plain["masks"])
    assert torch.equal(raw.bool().cpu(), _pattern())
    raw_num = connected_components(raw)[1]
    assert raw_num.tolist() == [1, 2, 3, 4, 5, 6]
    # keep_largest alone drops the specks; with min_size = 80 the blocks of images 0 and 1 go too
    big = 80
    for kw in (dict(keep_largest=True), dict(keep_largest=True, min_size=big)):
        res = predict(model, loader, dev, keep_masks=True, boundary=True, **kw)
        assert set(res) == set(plain) | {"num_components"}
        assert res["num"] == 6
        nc = res["num_components"]
        assert nc.is_cuda and nc.dtype == torch.int64 and tuple(nc.shape) == (6,)
        assert torch.equal(nc, raw_num.to(torch.int64))           # counted before filtering
        ref, ref_num, _ = batch_filter(raw.cpu().numpy(), **kw)
        assert np.array_equal(torch.cat(res["masks"]).cpu().numpy(), ref)
        assert np.array_equal(nc.cpu().numpy(), ref_num)
        masks, dice, iou, bm = _assembled(plain, loader, **kw)
        assert all(torch.equal(a, b) for a, b in zip(res["masks"], masks))
        assert torch.equal(res["dice"], dice) and torch.equal(res["iou"], iou)
        assert torch.equal(res["mean_dice"], dice.mean()) and torch.equal(res["mean_iou"], iou.mean())
        for k in ("hd", "hd95", "assd"):
            assert torch.equal(res[k].nan_to_num(-1), bm[k].nan_to_num(-1))
    assert not torch.equal(res["dice"], plain["dice"])            # the min_size run removed something
    assert not torch.equal(torch.cat(res["masks"]), raw)
    # min_size alone, connectivity 4, a loader without targets
    bare = predict(model, [x for x, _ in loader], dev, keep_masks=True, min_size=big, connectivity=4)
    ref, ref_num, _ = batch_filter(raw.cpu().numpy(), min_size=big, connectivity=4)
    assert bare["dice"] is None and np.array_equal(torch.cat(bare["masks"]).cpu().numpy(), ref)
    assert np.array_equal(bare["num_components"].cpu().numpy(), ref_num)


def test_predict_with_the_options_off_is_unchanged(monkeypatch):
    """With both options off: the keys of the loop without them, the tensors of the loop assembled
    from its pieces, and the same entry points in the same order whether the options are left out or
    spelled out as off -- no component kernel among them.  With an option on, the same sequence with
    one stf_ccl_filter behind every stf_predict_mask.  Eager steps, as the launch-trace fixture
    records them, so every forward shows its launches."""
    monkeypatch.setenv("STF_PLAN", "0")
    from stfunet import image_metrics, predict_masks
    from stfunet.engine import preprocess_input
    from stfunet.predict import predict
    model, loader = _unet_and_loader()
    dev = torch.device(DEV)

    def traced(**kw):
        with lt.tracing() as trace:
            res = predict(model, loader, dev, keep_masks=True, **kw)
            torch.cuda.synchronize()
            return res, list(trace)

    traced()                                                      # one-time work (weight packing) is done
    base, want = traced()
    res, got = traced(keep_largest=False, min_size=0, connectivity=4)
    assert set(res) == set(base) == {"num", "dice", "iou", "mean_dice", "mean_iou", "masks"}
    assert got == want and got.count("stf_predict_mask") == 2
    assert not any("ccl" in (e if isinstance(e, str) else e[0]) for e in got)
    with torch.no_grad():
        pieces = [predict_masks(model(preprocess_input(x, model).to(dev)), target=t.to(dev)) for x, t in loader]
    dice, iou = image_metrics(torch.cat([c for _, c in pieces]))
    for r in (res, base):
        assert torch.equal(r["dice"], dice) and torch.equal(r["iou"], iou)
        assert all(torch.equal(a, m) for a, (m, _) in zip(r["masks"], pieces))
    _, on = traced(keep_largest=True)
    expect = []
    for e in want:
        expect.append(e)
        if e == "stf_predict_mask":
            expect.append("stf_ccl_filter")
    assert on == expect


# ---------------------------------------------------------------- a recorded plan
def test_recorded_plan_replays_to_the_same_bits():
    from stfunet import _lib
    from stfunet._lib import call, stream
    lib = _lib.load()
    B, H, W = 3, 37, 130
    P = np.stack([_random(H, W, d, 41 + i) for i, d in enumerate((0.3, 0.593, 0.0))])
    T = np.stack([_random(H, W, d, 51 + i) for i, d in enumerate((0.05, 0.5, 0.3))]).astype(np.int64)
    m, t = torch.from_numpy(P).to(DEV), torch.from_numpy(T).to(DEV)
    out, counts, num = Guarded(B * H * W, 0xAA), Guarded(B * 24, 0xAA), Guarded(B * 4, 0xAA)
    scratch = _scratch(B, H, W, 0xAA)
    plan = lib.stf_plan_create()
    try:
        assert lib.stf_plan_record(plan) == 0
        try:
            call("stf_ccl_filter", m.data_ptr(), t.data_ptr(), B, H, W, 8, 1, 2, -1, out.body.data_ptr(),
                 counts.body.data_ptr(), num.body.data_ptr(), scratch.body.data_ptr(), stream())
        finally:
            assert lib.stf_plan_stop() == 0
        torch.cuda.synchronize()
        n = lib.stf_plan_size(plan)
        assert n == 6                                        # the counts' memset and five kernels
        first = (out.body.clone(), counts.body.clone(), num.body.clone())
        ref, ref_num, ref_counts = batch_filter(P, True, 2, 8, T)
        assert np.array_equal(first[0].cpu().numpy().reshape(B, H, W), ref)
        assert np.array_equal(first[1].cpu().numpy().view(np.int64).reshape(B, 3), ref_counts)
        assert np.array_equal(first[2].cpu().numpy().view(np.int32), ref_num)
        for fill in (0x55, 0xAA):
            for g in (out, counts, num, scratch):
                g.body.fill_(fill)
            torch.cuda.synchronize()
            assert lib.stf_plan_replay(plan, 0, n, None) == 0
            torch.cuda.synchronize()
            assert all(torch.equal(g.body, f) for g, f in zip((out, counts, num), first))
            assert all(g.guards_intact() for g in (out, counts, num, scratch))
    finally:
        lib.stf_plan_destroy(plan)
