"""Boundary metrics on the GPU (csrc/boundary.hip through the C entry points and stfunet.predict)
against the numpy brute force of tests/_boundary_ref.py, which tests/test_boundary_cpu.py pins to
scipy and to tests/golden/boundary.npz.

* ``stf_edt_sq``: integer equality at every pixel.
* ``stf_boundary_metrics``: border counts equal; HD bit-equal to ``np.sqrt(float(max d2))`` (the
  maximum is an exact integer and sqrt is correctly rounded on both sides); HD95 within 1e-12
  relative (two square roots and one interpolation in double); ASSD within 1e-9 relative (the sums
  of at most 2^20 roots taken in two different fixed orders differ by at most n * 2^-53 relative).

The kernel-level tests call the C entry points on buffers with 64 guard bytes on each side and run
every case twice, the buffers (scratch included) prefilled with 0xAA and then 0x55: equal results
show that every output byte is written and that two runs agree bit for bit; the guards must keep
their fill.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

from _boundary_ref import INT32_MAX, batch_metrics, d2_all, fixture_cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
EINVAL = 100001
CASES = fixture_cases()


class Guarded:
    """``nbytes`` of device memory between two guards, everything prefilled with ``fill``."""

    def __init__(self, nbytes, fill):
        self.fill, self.n = fill, nbytes
        self.raw = torch.full((nbytes + 2 * GUARD,), fill, dtype=torch.uint8, device=DEV)
        self.body = self.raw[GUARD:GUARD + nbytes]

    def guards_intact(self):
        return bool((self.raw[:GUARD] == self.fill).all() and (self.raw[GUARD + self.n:] == self.fill).all())


def _scratch(B, H, W, fill):
    from stfunet import _lib
    nbytes = _lib.load().stf_boundary_scratch_bytes(B, H, W)
    assert nbytes > 0
    return Guarded(nbytes, fill)


def _u8_at_offset(a, offset):
    """uint8 device copy of ``a`` whose base address is ``offset`` bytes past an allocation's."""
    flat = torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8)).flatten()
    buf = torch.zeros(flat.numel() + offset, dtype=torch.uint8, device=DEV)
    buf[offset:] = flat.to(DEV)
    return buf[offset:]


def run_edt(sites, where=None, offset=0, fill=0xAA):
    from stfunet._lib import call, stream
    B, H, W = sites.shape
    s = _u8_at_offset(sites, offset)
    w = None if where is None else _u8_at_offset(where, offset)
    assert s.data_ptr() % 2 == offset % 2
    d2, scratch = Guarded(B * H * W * 4, fill), _scratch(B, H, W, fill)
    call("stf_edt_sq", s.data_ptr(), None if w is None else w.data_ptr(), B, H, W, d2.body.data_ptr(),
         scratch.body.data_ptr(), stream())
    torch.cuda.synchronize()
    assert d2.guards_intact() and scratch.guards_intact()
    return d2.body.view(torch.int32).view(B, H, W).cpu().numpy()


def check_edt(sites, where=None, offset=0):
    sites = np.asarray(sites, dtype=np.uint8)
    if sites.ndim == 2:
        sites = sites[None]
        where = None if where is None else np.asarray(where)[None]
    first = run_edt(sites, where, offset, 0xAA)
    second = run_edt(sites, where, offset, 0x55)
    assert np.array_equal(first, second)
    ref = np.stack([d2_all(s) for s in sites])
    if where is not None:
        ref = np.where(np.asarray(where) != 0, ref, -1)
    assert first.dtype == np.int32 and np.array_equal(first, ref)
    return first


def run_metrics(mask, target, ignore=-1, fill=0xAA):
    from stfunet._lib import call, stream
    B, H, W = mask.shape
    m = torch.from_numpy(np.ascontiguousarray(mask, dtype=np.uint8)).to(DEV)
    t = torch.from_numpy(np.ascontiguousarray(target, dtype=np.int64)).to(DEV)
    out, counts, scratch = Guarded(B * 24, fill), Guarded(B * 16, fill), _scratch(B, H, W, fill)
    call("stf_boundary_metrics", m.data_ptr(), t.data_ptr(), B, H, W, ignore, out.body.data_ptr(),
         counts.body.data_ptr(), scratch.body.data_ptr(), stream())
    torch.cuda.synchronize()
    assert out.guards_intact() and counts.guards_intact() and scratch.guards_intact()
    return (out.body.view(torch.float64).view(B, 3).cpu().numpy(),
            counts.body.view(torch.int64).view(B, 2).cpu().numpy())


def assert_metrics(out, counts, mask, target, ignore=None):
    """Device results of a batch against the brute force, with the bounds of the module docstring."""
    ref, ref_counts, ref_max = batch_metrics(mask, target, ignore)
    print("device", out.tolist(), counts.tolist(), "reference", ref.tolist(), ref_counts.tolist())
    assert np.array_equal(counts, ref_counts)
    for b in range(len(ref)):
        if ref_max[b] is None:
            assert np.isnan(out[b]).all()
            continue
        assert not np.isnan(out[b]).any()
        assert out[b, 0] == np.sqrt(float(ref_max[b])) == ref[b, 0]
        assert abs(out[b, 1] - ref[b, 1]) <= 1e-12 * abs(ref[b, 1])
        assert abs(out[b, 2] - ref[b, 2]) <= 1e-9 * abs(ref[b, 2])


def check_metrics(mask, target, ignore=None):
    mask, target = np.asarray(mask), np.asarray(target)
    if mask.ndim == 2:
        mask, target = mask[None], target[None]
    ign = -1 if ignore is None else ignore
    out, counts = run_metrics(mask, target, ign, 0xAA)
    out2, counts2 = run_metrics(mask, target, ign, 0x55)
    assert np.array_equal(out.view(np.int64), out2.view(np.int64)) and np.array_equal(counts, counts2)
    assert_metrics(out, counts, mask, target, ignore)
    return out, counts


# ---------------------------------------------------------------- the distance transform
@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_edt_fixture_cases(c):
    check_edt(c["T"])
    check_edt(c["border_p"], where=c["T"])


def _random_sites(H, W, density, seed):
    return (np.random.default_rng(seed).random((H, W)) < density).astype(np.uint8)


@pytest.mark.parametrize("H,W", [(1, 1), (1, 130), (130, 1), (3, 64), (65, 63)])
def test_edt_seam_shapes(H, W):
    """Below, at and above one 64-pixel word; W no multiple of the wave; single rows and columns."""
    for k, density in enumerate((0.03, 0.5)):
        s = _random_sites(H, W, density, 100 * H + W + k)
        s[H // 2, W // 2] = 1
        check_edt(s)


def test_edt_image_without_sites():
    d2 = check_edt(np.zeros((7, 70), np.uint8))
    assert (d2 == INT32_MAX).all()
    where = _random_sites(7, 70, 0.5, 1)
    d2 = check_edt(np.zeros((7, 70), np.uint8), where=where)
    assert (d2[0][where != 0] == INT32_MAX).all() and (d2[0][where == 0] == -1).all()


def test_edt_rows_without_sites_between_rows_with_sites():
    s = np.zeros((40, 150), np.uint8)
    s[3] = _random_sites(1, 150, 0.05, 2)[0]
    s[4, 149] = 1
    s[31] = _random_sites(1, 150, 0.3, 3)[0]
    s[39, 0] = 1
    check_edt(s)


def test_edt_all_pixels_sites():
    d2 = check_edt(np.ones((9, 131), np.uint8))
    assert (d2 == 0).all()


def test_edt_sites_in_the_four_corners():
    s = np.zeros((67, 129), np.uint8)
    s[0, 0] = s[0, -1] = s[-1, 0] = s[-1, -1] = 1
    d2 = check_edt(s)
    assert d2[0, 33, 64] == 33 * 33 + 64 * 64


def test_edt_where_mask():
    s = _random_sites(33, 97, 0.02, 4)
    where = _random_sites(33, 97, 0.4, 5)
    d2 = check_edt(s, where=where)
    assert (d2[0][where == 0] == -1).all() and (d2[0][where != 0] >= 0).all()


def test_edt_batch_of_different_images():
    s = np.stack([_random_sites(21, 75, 0.02, 6), np.zeros((21, 75), np.uint8), _random_sites(21, 75, 0.6, 7)])
    d2 = check_edt(s)
    assert (d2[1] == INT32_MAX).all()
    where = np.stack([_random_sites(21, 75, 0.5, 8 + i) for i in range(3)])
    check_edt(s, where=where)


def test_edt_misaligned_base_pointer():
    s = _random_sites(19, 68, 0.05, 11)
    check_edt(s, where=_random_sites(19, 68, 0.7, 12), offset=1)
    check_edt(s, offset=1)


def test_distance_transform_sq_python_surface():
    from stfunet import distance_transform_sq
    s = np.stack([_random_sites(17, 70, 0.04, 13), _random_sites(17, 70, 0.3, 14)])
    ref = np.stack([d2_all(x) for x in s])
    for t in (torch.from_numpy(s), torch.from_numpy(s).bool(), torch.from_numpy(s).long() * 7):
        d2 = distance_transform_sq(t.to(DEV))
        assert d2.dtype == torch.int32 and d2.is_cuda and np.array_equal(d2.cpu().numpy(), ref)
    where = torch.from_numpy(s[::-1].copy()).bool()
    d2 = distance_transform_sq(torch.from_numpy(s).to(DEV), where=where.to(DEV))
    assert np.array_equal(d2.cpu().numpy(), np.where(where.numpy(), ref, -1))
    assert tuple(distance_transform_sq(torch.zeros(0, 4, 4, dtype=torch.uint8, device=DEV)).shape) == (0, 4, 4)


# ---------------------------------------------------------------- the metrics
@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_metrics_fixture_cases(c):
    out, _ = check_metrics(c["P"], c["T"].astype(np.int64))
    if math.isnan(c["hd"]):
        assert np.isnan(out).all()
    else:                                                   # scipy's own numbers, as committed
        assert out[0, 0] == c["hd"]
        assert abs(out[0, 1] - c["hd95"]) <= 1e-12 * abs(c["hd95"])
        assert abs(out[0, 2] - c["assd"]) <= 1e-9 * abs(c["assd"])


def test_metrics_fixture_cases_as_batches():
    """The cases of one shape as one batch: every image its own answer."""
    for shape in {c["P"].shape for c in CASES}:
        group = [c for c in CASES if c["P"].shape == shape]
        check_metrics(np.stack([c["P"] for c in group]), np.stack([c["T"] for c in group]).astype(np.int64))


def test_metrics_checkerboard_every_pixel_is_border():
    yy, xx = np.mgrid[0:18, 0:67]
    board = ((yy + xx) % 2).astype(np.uint8)
    _, counts = check_metrics(board, (1 - board).astype(np.int64))
    assert counts[0].tolist() == [int(board.sum()), int((1 - board).sum())]


def test_metrics_mask_with_a_hole_has_an_inner_border():
    P = np.zeros((40, 70), np.uint8)
    P[5:35, 8:66] = 1
    P[15:25, 30:40] = 0
    T = np.zeros((40, 70), np.int64)
    T[18:22, 33:37] = 1                                    # inside the hole: nearest to the inner border
    out, _ = check_metrics(P, T)
    assert out[0, 0] == np.sqrt(float(13 * 13 + 29 * 29))  # outer corner (5, 65) to the target's (18, 36)


def test_metrics_full_foreground_border_is_the_frame():
    P = np.ones((20, 66), np.uint8)
    T = np.zeros((20, 66), np.int64)
    T[9:12, 30:36] = 1
    _, counts = check_metrics(P, T)
    assert counts[0, 0] == 2 * 20 + 2 * 66 - 4
    check_metrics(P, np.ones((20, 66), np.int64))


def test_metrics_masks_touching_the_image_edge():
    P = np.zeros((30, 64), np.uint8)
    P[0:6, 0:9] = 1
    P[25:30, 60:64] = 1
    T = np.zeros((30, 64), np.int64)
    T[0:30, 63] = 1
    T[29, 0:64] = 1
    check_metrics(P, T)


def test_metrics_one_two_and_three_border_pixels():
    """n = 1 (one side empty: undefined), n = 2 and n = 3: the percentile ranks degenerate."""
    P, T = np.zeros((9, 70), np.uint8), np.zeros((9, 70), np.int64)
    P[2, 3] = 1
    out, counts = check_metrics(P, T)
    assert np.isnan(out).all() and counts[0].tolist() == [1, 0]
    T[6, 66] = 1
    out, _ = check_metrics(P, T)
    d = np.sqrt(float(16 + 63 * 63))
    assert out[0].tolist() == [d, d, d]
    T[2, 4] = 1
    out, _ = check_metrics(P, T)
    assert out[0, 0] == d and abs(out[0, 1] - (1.0 + (d - 1.0) * 0.9)) <= 1e-12 * d


def test_metrics_empty_sides_give_nan_and_keep_the_counts():
    g = _random_sites(15, 80, 0.3, 21)
    e = np.zeros_like(g)
    mask = np.stack([e, g, e, g])
    target = np.stack([g, e, e, g]).astype(np.int64)
    out, counts = check_metrics(mask, target)
    assert np.isnan(out[:3]).all() and (out[3] == 0).all()
    assert counts[0, 0] == 0 and counts[0, 1] > 0 and counts[1, 1] == 0 and counts[2].tolist() == [0, 0]


def test_metrics_ignore_index_on_a_padded_target():
    P = _random_sites(24, 90, 0.4, 22)
    T = _random_sites(24, 90, 0.4, 23).astype(np.int64)
    T[:, 70:] = 255
    T[20:, :] = 255
    out, counts = check_metrics(P, T, ignore=255)
    keep = T != 255
    cleared, _ = check_metrics(P * keep, T * keep)
    assert np.array_equal(out, cleared)
    plain, _ = check_metrics(P, T)                          # without ignore a 255 pad is foreground
    assert not np.array_equal(plain, out)


def test_metrics_far_apart_corners_of_512():
    P, T = np.zeros((512, 512), np.uint8), np.zeros((512, 512), np.int64)
    P[0, 0] = T[511, 511] = 1
    out, counts = check_metrics(P, T)
    d = np.sqrt(float(2 * 511 * 511))
    assert out[0].tolist() == [d, d, d] and counts[0].tolist() == [1, 1]


def test_metrics_one_row_of_4096():
    P, T = np.zeros((1, 4096), np.uint8), np.zeros((1, 4096), np.int64)
    P[0, 0] = T[0, 4095] = 1
    out, _ = check_metrics(P, T)
    assert out[0].tolist() == [4095.0, 4095.0, 4095.0]
    P[0, 4095] = T[0, 0] = 1
    T[0, 2000:2100] = 1
    check_metrics(P, T)


def test_boundary_metrics_python_surface():
    from stfunet import boundary_metrics
    P = np.stack([_random_sites(26, 71, 0.3, 31), np.zeros((26, 71), np.uint8), _random_sites(26, 71, 0.6, 32)])
    T = np.stack([_random_sites(26, 71, 0.3, 33 + i) for i in range(3)]).astype(np.int64)
    T[2, :, 60:] = 255
    for ignore in (None, 255):
        for mask in (torch.from_numpy(P), torch.from_numpy(P).bool(), torch.from_numpy(P).int() * 3):
            res = boundary_metrics(mask.to(DEV), torch.from_numpy(T).int().to(DEV), ignore_index=ignore)
            assert set(res) == {"hd", "hd95", "assd", "border_counts"}
            assert all(res[k].is_cuda and res[k].dtype == torch.float64 and tuple(res[k].shape) == (3,)
                       for k in ("hd", "hd95", "assd"))
            assert res["border_counts"].dtype == torch.int64
            out = torch.stack([res["hd"], res["hd95"], res["assd"]], 1).cpu().numpy()
            assert_metrics(out, res["border_counts"].cpu().numpy(), P, T, ignore)
    scaled = boundary_metrics(torch.from_numpy(P).to(DEV), torch.from_numpy(T).to(DEV), spacing=0.5)
    unit = boundary_metrics(torch.from_numpy(P).to(DEV), torch.from_numpy(T).to(DEV))
    for k in ("hd", "hd95", "assd"):
        assert torch.equal(scaled[k].nan_to_num(-1), (unit[k] * 0.5).nan_to_num(-1))
    empty = boundary_metrics(torch.zeros(0, 5, 5, dtype=torch.uint8, device=DEV),
                             torch.zeros(0, 5, 5, dtype=torch.int64, device=DEV))
    assert tuple(empty["hd"].shape) == (0,) and tuple(empty["border_counts"].shape) == (0, 2)


@pytest.mark.parametrize("B,H,W", [(1, 11, 33), (1, 1, 107), (1, 5, 47), (3, 7, 9)])
def test_python_surface_odd_pixel_counts(B, H, W):
    """12 scratch bytes per pixel: with an odd pixel count the last border-distance row ends on a
    half 8-byte word, and 107 (mod 128) pixels fill the allocator's 512-byte units to the last
    byte.  The scratch the package allocates holds every byte the entry points ask for, and the
    results equal the brute force."""
    from stfunet import boundary_metrics, distance_transform_sq
    from stfunet import predict as P
    assert (B * H * W) % 2 == 1
    mask = np.stack([_random_sites(H, W, 0.5, 61 + b) for b in range(B)])
    mask[:, -1, -2:] = 1                                     # border pixels at the very end of the planes
    target = np.stack([_random_sites(H, W, 0.5, 71 + b) for b in range(B)]).astype(np.int64)
    target[:, -1, -1] = 1
    m, t = torch.from_numpy(mask).to(DEV), torch.from_numpy(target).to(DEV)
    from stfunet import _lib
    scratch = P._boundary_scratch(B, H, W, DEV)
    assert scratch.numel() * scratch.element_size() >= _lib.load().stf_boundary_scratch_bytes(B, H, W)
    assert scratch.numel() * scratch.element_size() >= 256 + 12 * B * H * W
    res = boundary_metrics(m, t)
    out = torch.stack([res["hd"], res["hd95"], res["assd"]], 1).cpu().numpy()
    assert_metrics(out, res["border_counts"].cpu().numpy(), mask, target)
    d2 = distance_transform_sq(m).cpu().numpy()
    assert np.array_equal(d2, np.stack([d2_all(x) for x in mask]))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_einval_without_a_launch(dtype):
    """Refusals with real device buffers far smaller than the refused sizes: nothing may touch them."""
    from stfunet import _lib
    lib = _lib.load(dtype)
    buf = Guarded(4096, 0xAA)
    p = ctypes.c_void_p(buf.body.data_ptr())
    st = ctypes.c_void_p(_lib.stream())

    def bm(mask=p, target=p, B=1, H=4, W=4, out=p, counts=p, scratch=p):
        return lib.stf_boundary_metrics(mask, target, B, H, W, -1, out, counts, scratch, st)

    def edt(sites=p, B=1, H=4, W=4, d2=p, scratch=p):
        return lib.stf_edt_sq(sites, None, B, H, W, d2, scratch, st)

    assert bm(mask=None) == EINVAL and bm(target=None) == EINVAL and bm(out=None) == EINVAL
    assert bm(counts=None) == EINVAL and bm(scratch=None) == EINVAL
    assert edt(sites=None) == EINVAL and edt(d2=None) == EINVAL and edt(scratch=None) == EINVAL
    for f in (bm, edt):
        assert f(B=0) == EINVAL and f(H=0) == EINVAL and f(W=0) == EINVAL
        assert f(H=4097) == EINVAL and f(W=4097) == EINVAL
        assert f(B=128, H=4096, W=4096) == EINVAL and f(B=1 << 19, H=64, W=64) == EINVAL
    torch.cuda.synchronize()
    assert bool((buf.raw == 0xAA).all())


# ---------------------------------------------------------------- the predict loop
def _unet_and_loader():
    from oracle.cases import dce_case
    from oracle.init import canonical_state_dict
    from stfunet.unet import UNet
    model = UNet(in_channels=8, num_classes=2, base_c=8)
    model.load_state_dict(canonical_state_dict(model.state_dict(), seed=0))
    loader = [dce_case(400 + i, 3, 8, 32, 32) for i in range(2)]
    loader[1][1][1].zero_()                                  # image 4 of 6: an empty target
    return model.to(DEV), loader


def test_predict_with_boundary_metrics():
    from stfunet import boundary_metrics
    from stfunet.predict import predict
    model, loader = _unet_and_loader()
    plain = predict(model, loader, torch.device(DEV), keep_masks=True)
    assert set(plain) == {"num", "dice", "iou", "mean_dice", "mean_iou", "masks"}
    assert set(predict(model, loader, torch.device(DEV))) == {"num", "dice", "iou", "mean_dice", "mean_iou"}
    res = predict(model, loader, torch.device(DEV), keep_masks=True, boundary=True, spacing=0.25)
    assert set(res) == set(plain) | {"hd", "hd95", "assd", "mean_hd", "mean_hd95", "mean_assd", "num_boundary"}
    assert res["num"] == 6 and torch.equal(res["dice"], plain["dice"])
    assert all(torch.equal(a, b) for a, b in zip(res["masks"], plain["masks"]))
    P = torch.cat(res["masks"]).cpu().numpy()
    T = torch.cat([t for _, t in loader]).numpy()
    ref, _, ref_max = batch_metrics(P, T)
    assert ref_max[4] is None
    direct = [boundary_metrics(m, t.to(DEV), spacing=0.25) for m, (_, t) in zip(res["masks"], loader)]
    for j, k in enumerate(("hd", "hd95", "assd")):
        v = res[k]
        assert v.is_cuda and v.dtype == torch.float64 and tuple(v.shape) == (6,)
        want = torch.cat([d[k] for d in direct])
        assert torch.equal(v.nan_to_num(-1), want.nan_to_num(-1))
        got = v.cpu().numpy()
        assert np.array_equal(np.isnan(got), np.isnan(ref[:, j])) and np.isnan(got[4])
        ok = ~np.isnan(got)
        assert np.allclose(got[ok], 0.25 * ref[ok, j], rtol=1e-9, atol=0)
        mean = res["mean_" + k]
        assert mean.is_cuda and mean.dim() == 0
        if ok.any():
            assert abs(mean.item() - got[ok].mean()) <= 1e-12 * abs(got[ok].mean())
        else:
            assert math.isnan(mean.item())
    nb = res["num_boundary"]
    assert nb.is_cuda and nb.dim() == 0 and nb.dtype == torch.int64
    assert 2 <= nb.item() == int((~np.isnan(ref[:, 0])).sum()) <= 5     # the means below are over real values
    # no image defined: NaN means, zero count
    none = predict(model, [(x, torch.zeros_like(t)) for x, t in loader], torch.device(DEV), boundary=True)
    assert none["num_boundary"].item() == 0 and math.isnan(none["mean_hd95"].item())
    assert torch.isnan(none["assd"]).all()
    # a loader without targets: the keys are there, empty
    bare = predict(model, [x for x, _ in loader], torch.device(DEV), boundary=True)
    assert bare["hd"] is None and bare["mean_hd"] is None and bare["num_boundary"] is None


def test_predict_boundary_refuses_a_target_of_another_size():
    from stfunet.predict import predict
    model, loader = _unet_and_loader()
    x, t = loader[0]
    with pytest.raises(ValueError, match="does not match"):
        predict(model, [(x, t[:, :16, :16])], torch.device(DEV), boundary=True)


# ---------------------------------------------------------------- a recorded plan
def test_recorded_plan_replays_to_the_same_bits():
    from stfunet import _lib
    from stfunet._lib import call, stream
    lib = _lib.load()
    B, H, W = 3, 37, 130
    P = np.stack([_random_sites(H, W, d, 41 + i) for i, d in enumerate((0.05, 0.5, 0.0))])
    T = np.stack([_random_sites(H, W, d, 51 + i) for i, d in enumerate((0.05, 0.5, 0.3))]).astype(np.int64)
    m, t = torch.from_numpy(P).to(DEV), torch.from_numpy(T).to(DEV)
    out, counts, scratch = Guarded(B * 24, 0xAA), Guarded(B * 16, 0xAA), _scratch(B, H, W, 0xAA)
    plan = lib.stf_plan_create()
    try:
        assert lib.stf_plan_record(plan) == 0
        try:
            call("stf_boundary_metrics", m.data_ptr(), t.data_ptr(), B, H, W, -1, out.body.data_ptr(),
                 counts.body.data_ptr(), scratch.body.data_ptr(), stream())
        finally:
            assert lib.stf_plan_stop() == 0
        torch.cuda.synchronize()
        n = lib.stf_plan_size(plan)
        assert n == 4                                        # the counts' memset and three kernels
        first = (out.body.clone(), counts.body.clone())
        assert_metrics(first[0].view(torch.float64).view(B, 3).cpu().numpy(),
                       first[1].view(torch.int64).view(B, 2).cpu().numpy(), P, T)
        for fill in (0x55, 0xAA):
            for g in (out, counts, scratch):
                g.body.fill_(fill)
            torch.cuda.synchronize()
            assert lib.stf_plan_replay(plan, 0, n, None) == 0
            torch.cuda.synchronize()
            assert torch.equal(out.body, first[0]) and torch.equal(counts.body, first[1])
            assert out.guards_intact() and counts.guards_intact() and scratch.guards_intact()
    finally:
        lib.stf_plan_destroy(plan)
