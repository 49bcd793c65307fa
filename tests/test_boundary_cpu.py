"""CPU checks of the boundary metrics (stfunet.predict.boundary_metrics, csrc/boundary.hip): the
tests' numpy restatement (tests/_boundary_ref.py) against scipy and against the committed fixture,
hand-computed answers, the Python argument checks and the C side's refusals (no kernel launches)."""
import ctypes
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

from _boundary_ref import GOLDEN, batch_metrics, border, d2_all, fixture_cases, metrics

CASES = fixture_cases()
EINVAL = 100001


def _generator():
    spec = importlib.util.spec_from_file_location("make_golden_boundary",
                                                  os.path.join(GOLDEN, "make_golden_boundary.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _close(a, b, rtol):
    return (math.isnan(a) and math.isnan(b)) or abs(a - b) <= rtol * abs(b)


def test_fixture_covers_the_planned_ground():
    shapes = {c["P"].shape for c in CASES}
    assert shapes == {(1, 1), (1, 7), (9, 1), (5, 5), (33, 65), (37, 130)}
    assert len(CASES) == 48 and sum(c["name"].endswith("_dil") for c in CASES) == 24
    assert any(math.isnan(c["hd"]) for c in CASES) and sum(not math.isnan(c["hd"]) for c in CASES) >= 36
    assert any(c["hd"] == 0.0 for c in CASES) and any(c["hd"] > 5 for c in CASES)


def test_fixture_is_what_the_generator_makes():
    gen = _generator()
    made = gen.random_cases()
    assert [n for n, _, _ in made] == [c["name"] for c in CASES]
    for (_, P, T), c in zip(made, CASES):
        assert np.array_equal(P, c["P"]) and np.array_equal(T, c["T"])


def test_restatement_against_scipy():
    """Borders equal, HD bit-equal, HD95 and ASSD within 1e-12 relative (a handful of double
    roundings apart: scipy's percentile and mean take their sums in another order)."""
    pytest.importorskip("scipy")
    gen = _generator()
    for name, P, T in gen.random_cases():
        bp, bt, hd, hd95, assd = gen.scipy_metrics(P, T)
        assert np.array_equal(border(P), bp) and np.array_equal(border(T), bt), name
        rhd, rhd95, rassd, counts, _ = metrics(P, T)
        assert counts == (int(bp.sum()), int(bt.sum()))
        assert (math.isnan(hd) and math.isnan(rhd)) or rhd == hd, name
        assert _close(rhd95, hd95, 1e-12) and _close(rassd, assd, 1e-12), (name, rhd95, hd95, rassd, assd)


def test_restatement_distance_transform_against_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    for c in CASES:
        if not c["border_t"].any():
            assert (d2_all(c["border_t"]) == 2 ** 31 - 1).all()
            continue
        edt = ndi.distance_transform_edt(~c["border_t"])
        assert np.array_equal(np.sqrt(d2_all(c["border_t"]).astype(np.float64)), edt), c["name"]


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_restatement_reproduces_the_fixture(c):
    assert np.array_equal(border(c["P"]), c["border_p"]) and np.array_equal(border(c["T"]), c["border_t"])
    hd, hd95, assd, _, _ = metrics(c["P"], c["T"])
    assert (math.isnan(hd) and math.isnan(c["hd"])) or hd == c["hd"]
    assert _close(hd95, c["hd95"], 1e-12) and _close(assd, c["assd"], 1e-12)


def test_hand_computed_answers():
    # one pixel against one pixel: every distance is theirs
    P, T = np.zeros((6, 9), bool), np.zeros((6, 9), bool)
    P[1, 2] = T[4, 6] = True
    hd, hd95, assd, counts, mx = metrics(P, T)
    assert counts == (1, 1) and mx == 25 and hd == hd95 == assd == 5.0
    # 5x5 full mask (border = the 16 frame pixels) against its centre pixel: frame -> centre is
    # sqrt(dy^2 + dx^2) over the frame (4 corners sqrt 8, 8 at sqrt 5, 4 at 2), centre -> frame is 2
    P, T = np.ones((5, 5), bool), np.zeros((5, 5), bool)
    T[2, 2] = True
    assert border(P).sum() == 16 and not border(P)[1:4, 1:4].any()
    hd, hd95, assd, counts, mx = metrics(P, T)
    assert counts == (16, 1) and mx == 8 and hd == math.sqrt(8)
    s = sorted([2.0] * 5 + [math.sqrt(5)] * 8 + [math.sqrt(8)] * 4)
    r = 0.95 * 16
    assert hd95 == s[15] + (s[16] - s[15]) * (r - 15) == math.sqrt(8)
    frame_mean = (4 * math.sqrt(8) + 8 * math.sqrt(5) + 4 * 2.0) / 16
    assert abs(assd - 0.5 * (frame_mean + 2.0)) < 1e-15
    # identical masks
    g = np.random.default_rng(3).random((12, 17)) < 0.4
    assert metrics(g, g)[:3] == (0.0, 0.0, 0.0)
    # an empty mask on either side, or both
    e = np.zeros((12, 17), bool)
    for a, b in ((e, g), (g, e), (e, e)):
        hd, hd95, assd, counts, mx = metrics(a, b)
        assert math.isnan(hd) and math.isnan(hd95) and math.isnan(assd) and mx is None
        assert counts == (int(border(a).sum()), int(border(b).sum()))
    # ignore: those pixels are background on both sides
    t = g.astype(np.int64)
    t[:, 10:] = 255
    out, counts, _ = batch_metrics(np.ones((1, 12, 17), np.uint8), t[None], ignore=255)
    keep = t != 255
    assert metrics(keep, (t > 0) & keep)[:3] == tuple(out[0]) and counts[0, 0] == border(keep).sum()


def test_python_argument_checks():
    """The checks that precede any launch: host tensors raise RuntimeError, a bad spacing or bad
    shapes ValueError."""
    import stfunet
    from stfunet import predict as P
    assert stfunet.boundary_metrics is P.boundary_metrics
    assert stfunet.distance_transform_sq is P.distance_transform_sq
    m, t = torch.zeros(2, 4, 5, dtype=torch.uint8), torch.zeros(2, 4, 5, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.boundary_metrics(m, t)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.boundary_metrics(m.bool(), t.int(), ignore_index=255, spacing=0.7)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.distance_transform_sq(m)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.distance_transform_sq(m, where=m)
    with pytest.raises(ValueError, match="does not match"):
        P.boundary_metrics(m, torch.zeros(2, 4, 6, dtype=torch.int64))
    with pytest.raises(ValueError, match="does not match"):
        P.distance_transform_sq(m, where=torch.zeros(2, 5, 4, dtype=torch.uint8))
    with pytest.raises(ValueError, match=r"\[B, H, W\]"):
        P.boundary_metrics(m[0], t[0])
    for bad in (0.0, -1.0, float("nan"), float("inf"), "1", None, True):
        with pytest.raises(ValueError, match="spacing"):
            P.boundary_metrics(m, t, spacing=bad)
    with pytest.raises(ValueError, match="4096"):
        P.boundary_metrics(torch.zeros(1, 1, 4097, dtype=torch.uint8), torch.zeros(1, 1, 4097, dtype=torch.int64))
    with pytest.raises(ValueError, match="4096"):
        P.distance_transform_sq(torch.zeros(1, 4097, 1, dtype=torch.uint8))
    with pytest.raises(ValueError, match="4096"):
        P.distance_transform_sq(torch.zeros(1, 0, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="2\\^31"):      # an expanded view: no memory behind it
        P.distance_transform_sq(torch.zeros(1, 1, 1, dtype=torch.uint8).expand(128, 4096, 4096))
    with pytest.raises(ValueError, match="integer"):
        P.boundary_metrics(m.float(), t)
    with pytest.raises(ValueError, match="integer"):
        P.boundary_metrics(m, t.float())
    # the full transform of a large image is refused unless `where` takes the cost on (views: no memory)
    big = torch.zeros(1, 1, 1, dtype=torch.uint8).expand(1, 2048, 2048)
    assert 2048 ** 3 > P.MAX_FULL_SCAN == 1 << 32
    with pytest.raises(ValueError, match="where"):
        P.distance_transform_sq(big)
    with pytest.raises(ValueError, match="where"):
        P.distance_transform_sq(torch.zeros(1, 1, 1, dtype=torch.uint8).expand(257, 256, 256))
    with pytest.raises(RuntimeError, match="no CPU fallback"):        # at the bound: on to the device check
        P.distance_transform_sq(torch.zeros(1, 1, 1, dtype=torch.uint8).expand(256, 256, 256))
    with pytest.raises(TypeError):
        P.predict(torch.nn.Identity(), [], "cpu", boundry=True)
    # predict checks spacing before it runs anything, targets or not; without the flag it is not looked at
    for bad in (0.0, -2.0, float("nan"), float("inf"), "1", None):
        with pytest.raises(ValueError, match="spacing"):
            P.predict(torch.nn.Identity(), [], "cpu", boundary=True, spacing=bad)
    assert P.predict(torch.nn.Identity(), [], "cpu", spacing=0.0)["num"] == 0
    res = P.predict(torch.nn.Identity(), [], "cpu")
    assert set(res) == {"num", "dice", "iou", "mean_dice", "mean_iou"}
    res = P.predict(torch.nn.Identity(), [], "cpu", boundary=True)
    assert set(res) == {"num", "dice", "iou", "mean_dice", "mean_iou", "hd", "hd95", "assd", "mean_hd",
                        "mean_hd95", "mean_assd", "num_boundary"}
    assert res["hd"] is None and res["num_boundary"] is None


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_library_refuses_bad_arguments_without_launch(dtype):
    """STF_EINVAL with fake non-null pointers: nothing is launched or dereferenced."""
    from stfunet import _lib
    lib = _lib.load(dtype)
    fake = ctypes.c_void_p(1 << 20)

    def bm(mask=fake, target=fake, B=2, H=8, W=8, out=fake, counts=fake, scratch=fake):
        return lib.stf_boundary_metrics(mask, target, B, H, W, -1, out, counts, scratch, None)

    def edt(sites=fake, where=None, B=2, H=8, W=8, d2=fake, scratch=fake):
        return lib.stf_edt_sq(sites, where, B, H, W, d2, scratch, None)

    assert bm(mask=None) == EINVAL and bm(target=None) == EINVAL and bm(out=None) == EINVAL
    assert bm(counts=None) == EINVAL and bm(scratch=None) == EINVAL
    assert edt(sites=None) == EINVAL and edt(d2=None) == EINVAL and edt(scratch=None) == EINVAL
    for f in (bm, edt):
        assert f(B=0) == EINVAL and f(H=0) == EINVAL and f(W=0) == EINVAL and f(B=-1) == EINVAL
        assert f(H=4097) == EINVAL and f(W=4097) == EINVAL
        assert f(B=128, H=4096, W=4096) == EINVAL                     # B * H * W = 2^31
        assert f(B=1 << 30, H=2, W=1) == EINVAL
    assert bm(scratch=ctypes.c_void_p((1 << 20) + 4)) == EINVAL and edt(d2=ctypes.c_void_p((1 << 20) + 2)) == EINVAL
    sb = lib.stf_boundary_scratch_bytes
    assert sb(0, 8, 8) == 0 and sb(1, 0, 8) == 0 and sb(1, 8, 4097) == 0 and sb(128, 4096, 4096) == 0
    # per-image site counts (256-byte rounded), two int32 and two uint16 planes per pixel, the sum
    # rounded up to whole 8-byte words (12 bytes per pixel: an odd pixel count ends on a half word)
    assert sb(1, 1, 1) == 256 + 16 and sb(3, 5, 7) == 256 + 12 * 105 + 4 and sb(17, 8, 8) == 512 + 12 * 17 * 64
    assert sb(1, 11, 33) == 256 + 12 * 363 + 4 and sb(1, 1, 107) == 1544
    assert all(sb(1, 1, w) % 8 == 0 and sb(1, 1, w) >= 256 + 12 * w for w in range(1, 300))
    assert sb(64, 256, 256) == 1024 + 12 * 64 * 256 * 256
    assert sb(127, 4096, 4096) == 2048 + 12 * 127 * 4096 * 4096      # beyond 32 bits: size_t
