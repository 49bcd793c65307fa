"""Lesion confidence and FROC on the GPU (the FROC passes of csrc/ccl.hip through the C entry points and
stfunet.predict) against tests/golden/froc.npz (scipy's labels) and the numpy restatement of
tests/_froc_ref.py, which tests/test_froc_cpu.py pins to that fixture and to cases counted by hand.

Everything is an integer, so every comparison is equality, element for element.

The kernel-level tests call the C entry points on buffers with 64 guard bytes on each side and run
every case twice, the buffers (scratch included) prefilled with 0xAA and then with 0xFF: equal results
show that every output byte is written, that nothing is read before it is written and that two runs
agree bit for bit; the guards must keep their fill.
"""
import itertools

import numpy as np
import pytest
import torch

import _froc_ref as ref
import _launch_trace as lt

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
FIXTURE = ref.fixture()
EINVAL = 100001
SOURCES = {"softmax": 0, "sigmoid": 1, "probs": 2}


class Guarded:
    """``nbytes`` of device memory between two guards, everything prefilled with ``fill``."""

    def __init__(self, nbytes, fill):
        self.fill, self.n = fill, nbytes
        self.raw = torch.full((nbytes + 2 * GUARD,), fill, dtype=torch.uint8, device=DEV)
        self.body = self.raw[GUARD:GUARD + nbytes]
        assert self.raw.data_ptr() % 64 == 0

    def guards_intact(self):
        return bool((self.raw[:GUARD] == self.fill).all() and (self.raw[GUARD + self.n:] == self.fill).all())

    def ptr(self):
        return self.body.data_ptr() if self.n else None


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def run(mask, scores, target, depths, connectivity, bins=256, min_overlap=0.0, max_lesions=64, ignore=None,
        fill=0xAA, source="probs", channel=0):
    """One call of stf_froc3d (``depths`` a sequence) or stf_froc (``depths`` None: per image) on guarded
    buffers: (summary int64 [V, 4], table int64 [V, 2, max_lesions, 3], hist int64 [V, 3, bins + 1]).
    ``scores`` is [N, H, W] or [N, K, H, W]."""
    from stfunet import _lib
    N, H, W = mask.shape
    V = N if depths is None else len(depths)
    scores = scores[:, None] if scores.ndim == 3 else scores
    K = scores.shape[1]
    m, s, t = _dev(mask, np.uint8), _dev(scores, np.float32), _dev(target, np.int64)
    nbytes = _lib.load().stf_froc_scratch_bytes(N, H, W, V, bins)
    assert nbytes >= 36 * N * H * W and nbytes % 8 == 0
    summary, table = Guarded(V * 32, fill), Guarded(V * max_lesions * 48, fill)
    hist, scratch = Guarded(V * 3 * (bins + 1) * 8, fill), Guarded(nbytes, fill)
    head = (m.data_ptr(), s.data_ptr(), K, SOURCES[source], channel, t.data_ptr(), N, H, W)
    tail = (connectivity, float(min_overlap), max_lesions, -1 if ignore is None else ignore, bins, summary.ptr(),
            table.ptr(), hist.ptr(), scratch.ptr(), _lib.stream())
    if depths is None:
        _lib.call("stf_froc", *head, *tail)
    else:
        host = np.concatenate([[0], np.cumsum(depths)]).astype(np.int32)
        assert host[-1] == N
        starts = torch.from_numpy(host).to(DEV)
        _lib.call("stf_froc3d", *head, starts.data_ptr(), host.ctypes.data, V, *tail)
    torch.cuda.synchronize()
    assert all(b.guards_intact() for b in (summary, table, hist, scratch))
    return (summary.body.cpu().numpy().view(np.int64).reshape(V, 4),
            table.body.cpu().numpy().view(np.int64).reshape(V, 2, max_lesions, 3),
            hist.body.cpu().numpy().view(np.int64).reshape(V, 3, bins + 1))


def check(mask, scores, target, depths, connectivity, bins=256, min_overlap=0.0, max_lesions=64, ignore=None,
          want=None):
    """Two runs, the second on buffers (scratch included) poisoned with 0xFF, agree byte for byte and
    equal the restatement (and ``want``, the fixture's entry, when given); the summary is
    stf_lesion_metrics' and the sides of hist sum to what it says."""
    from test_lesions_gpu import run as lesion_run
    mask, target = np.asarray(mask, np.uint8), np.asarray(target, np.int64)
    scores = np.asarray(scores, np.float32)
    args = (bins, min_overlap, max_lesions, ignore)
    first = run(mask, scores, target, depths, connectivity, *args, fill=0xAA)
    second = run(mask, scores, target, depths, connectivity, *args, fill=0xFF)
    if depths is None:
        expect = ref.image_froc(mask, scores, target, bins, connectivity, min_overlap, max_lesions, ignore)
    else:
        expect = ref.stack_froc(mask, scores, target, depths, bins, connectivity, min_overlap, max_lesions, ignore)
    for a, b, r in zip(first, second, expect):
        assert a.tobytes() == b.tobytes()
        assert np.array_equal(a, r), (a.tolist(), r.tolist())
    if want is not None:
        assert all(np.array_equal(a, w) for a, w in zip(first, want))
    summary, table, hist = first
    plain = lesion_run(mask, target, depths, connectivity, min_overlap, max_lesions, ignore)
    assert summary.tobytes() == plain[0].tobytes() and np.array_equal(table[..., :2], plain[1])
    assert np.array_equal(hist.sum(-1), np.stack([summary[:, 2] - summary[:, 3], summary[:, 0], summary[:, 3]], 1))
    return first


def _random(shape, density, seed):
    return (np.random.default_rng(seed).random(shape) < density).astype(np.uint8)


def _scores(shape, bins, seed):
    return ref.dyadic_scores(np.random.default_rng(seed), shape, bins)


# ---------------------------------------------------------------- the named cases
@pytest.mark.parametrize("name", list(FIXTURE))
def test_cases_equal_the_fixture_and_the_restatement(name):
    c, want = FIXTURE[name]
    args = (c["bins"], c["min_overlap"], c["max_lesions"], c["ignore"], want)
    check(c["mask"], c["scores"], c["target"], c["depths"], c["connectivity"], *args)
    if all(d == 1 for d in c["depths"]):                           # the image entry point on the same slices
        check(c["mask"], c["scores"], c["target"], None, ref.FLAT[c["connectivity"]], *args)


def test_detected_at_zero_is_matched_target_without_an_overlap_floor():
    """min_overlap = 0 and every candidate voxel in a row >= 1: a lesion is reached iff it is matched."""
    from stfunet import froc_curves, lesion_scores_3d
    m, t = _random((6, 5, 70), 0.3, 61), _random((6, 5, 70), 0.3, 62).astype(np.int64)
    s = np.maximum(_scores(m.shape, 64, 63), np.float32(1 / 128))
    res = lesion_scores_3d(_dev(m, np.uint8), _dev(s, np.float32), _dev(t, np.int64), (1, 3, 2), bins=64)
    curve = froc_curves(res["froc_hist"])
    assert int(curve["detected"][0]) == int(res["matched_target"].sum()) > 0
    assert int(curve["matched"][0]) == int(res["matched_pred"].sum())
    assert int(curve["false_findings"][0]) == int((res["n_pred"] - res["matched_pred"]).sum())
    want = ref.curves(ref.stack_froc(m, s, t, (1, 3, 2), 64)[2])
    assert np.array_equal(curve["sensitivity"].cpu().numpy(), want["sensitivity"])
    assert np.array_equal(curve["sensitivity_at"].cpu().numpy(), want["sensitivity_at"])
    assert curve["cpm"].is_cuda and abs(float(curve["cpm"]) - want["cpm"]) <= 2.0 ** -49


# ---------------------------------------------------------------- shapes
@pytest.mark.parametrize("D,H,W", list(itertools.product((1, 2, 3), (1, 2, 5), (1, 63, 64, 65, 130))))
def test_shapes_across_the_chunk_seam(D, H, W):
    seed = 100 * D + 10 * H + W
    m, t = _random((D, H, W), 0.5, seed), _random((D, H, W), 0.5, 7 + seed)
    s = _scores((D, H, W), 16, 13 + seed)
    for k in (6, 26):
        check(m, s, t, [D], k, 16, 0.5, 8)
    check(m, s, t, None, 8, 16, 0.25, 8)


@pytest.mark.parametrize("W", (1, 63, 64, 65, 130))
def test_ragged_depths_in_one_call(W):
    m, t = _random((6, 5, W), 0.5, W), _random((6, 5, W), 0.5, W + 1)
    check(m, _scores(m.shape, 256, W + 2), t, (1, 3, 2), 18, 256, 0.25, 16)


@pytest.mark.parametrize("where", ((0, 0), (0, 63), (0, 64), (0, 129), (2, 5)))
def test_one_peak_in_a_candidate_as_wide_as_the_slice(where):
    """The largest score of a candidate of full rows sits at one voxel: the carried maximum, the skipped
    atomic and the flush at the row's end each have to deliver it."""
    m, t = np.ones((1, 3, 130), np.uint8), np.zeros((1, 3, 130), np.int64)
    t[0, 1, 100:110] = 1
    s = np.full(m.shape, 0.25, np.float32)
    s[0][where] = 0.75
    for depths, k in (([1], 26), (None, 8)):
        summary, table, hist = check(m, s, t, depths, k, 256, 0.0, 4)
        assert table[0, 1, 0].tolist() == [390, 10, 192] and table[0, 0, 0].tolist() == [10, 10, 192]
        assert hist[0, 1, 192] == 1 and hist[0, 2, 192] == 1 and hist.sum() == 2


# ---------------------------------------------------------------- the row rule is stf_score_hist's
@pytest.mark.parametrize("source,K", [(s, k) for s in ("softmax", "sigmoid", "probs") for k in (1, 2, 3, 16)])
def test_isolated_voxels_tie_the_rows_to_score_histogram(source, K):
    """A checkerboard mask at connectivity 4 / 6 on an empty target: every candidate is one voxel and a
    false finding, so side 0 is the score histogram of the masked voxels, whatever expf does."""
    from stfunet import lesion_scores, lesion_scores_3d, score_histogram
    rng = np.random.default_rng(K + 20 * SOURCES[source])
    N, H, W = 3, 6, 66                                              # H W % 4 == 0: the quad path
    zz, yy, xx = np.mgrid[0:N, 0:H, 0:W]
    board = torch.from_numpy(((zz + yy + xx) % 2 == 0).astype(np.uint8)).to(DEV)
    logits = torch.from_numpy((rng.standard_normal((N, K, H, W)) * 3).astype(np.float32)).to(DEV)
    zero = torch.zeros((N, H, W), dtype=torch.int64, device=DEV)
    channel = K - 1
    for scores, mask in ((logits, board), (logits[:, :, :, :65].contiguous(), board[:, :, :65].contiguous())):
        t = zero[:, :, :mask.shape[2]]
        want = score_histogram(scores, mask.long(), source, channel, 64)[:, 1]
        got = lesion_scores(mask, scores, t, source, channel, 64, connectivity=4)["froc_hist"]
        assert torch.equal(got[:, 0], want) and int(got[:, 1:].sum()) == 0
        got = lesion_scores_3d(mask, scores, t, None, source, channel, 64, connectivity=6)["froc_hist"]
        assert torch.equal(got[0, 0], want.sum(0)) and int(got[:, 1:].sum()) == 0


# ---------------------------------------------------------------- connectivity, determinism
def test_every_connectivity_and_depth_one_volumes_are_images():
    m, t = _random((4, 5, 70), 0.4, 21), _random((4, 5, 70), 0.4, 22) * 2
    t[2, :, 30] = 255
    s = _scores(m.shape, 256, 23)
    for k in (6, 18, 26):
        check(m, s, t, (2, 2), k, 256, 0.5, 32, 255)
        vol = check(m, s, t, (1, 1, 1, 1), k, 256, 0.5, 32, 255)
        img = check(m, s, t, None, ref.FLAT[k], 256, 0.5, 32, 255)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(vol, img))
    four, eight = check(m, s, t, None, 4), check(m, s, t, None, 8)
    assert not np.array_equal(four[2], eight[2])                   # the two are told apart by this input


def test_a_volume_alone_equals_the_volume_inside_a_ragged_stack():
    m, t = _random((6, 5, 130), 0.45, 31), _random((6, 5, 130), 0.45, 32)
    s = _scores(m.shape, 4096, 33)
    depths = (1, 3, 2)
    stack = check(m, s, t, depths, 26, 4096, 0.5, 16)
    at = 0
    for v, d in enumerate(depths):
        alone = check(m[at:at + d], s[at:at + d], t[at:at + d], [d], 26, 4096, 0.5, 16)
        assert all(a.tobytes() == b[v:v + 1].tobytes() for a, b in zip(alone, stack))
        at += d


@pytest.mark.parametrize("cap", (0, 1, 3))
def test_a_cut_table_leaves_the_summary_and_the_histogram_complete(cap):
    m, t = _random((6, 5, 65), 0.3, 41), _random((6, 5, 65), 0.3, 42)
    s = _scores(m.shape, 16, 43)
    full = check(m, s, t, (1, 3, 2), 6, 16, 0.25, 128)
    assert 3 < full[0][:, [0, 2]].min() and full[0][:, [0, 2]].max() <= 128    # 128 rows hold all, 3 cut every table
    cut = check(m, s, t, (1, 3, 2), 6, 16, 0.25, cap)
    assert np.array_equal(cut[0], full[0]) and np.array_equal(cut[2], full[2])
    assert np.array_equal(cut[1], full[1][:, :, :cap])


# ---------------------------------------------------------------- the Python surface
def test_python_surface():
    from stfunet import lesion_metrics, lesion_metrics_3d, lesion_scores, lesion_scores_3d
    m, T = _random((6, 9, 70), 0.3, 51), _random((6, 9, 70), 0.3, 52).astype(np.int64) * 3
    T[4, :, 20:24] = 255
    S = _scores(m.shape, 256, 53)
    d, t, s = torch.from_numpy(m).to(DEV), torch.from_numpy(T).to(DEV), torch.from_numpy(S).to(DEV)
    keys = {"n_target", "matched_target", "n_pred", "matched_pred", "sensitivity", "precision", "lesions", "froc_hist"}

    def same(res, plain, want, cap):
        assert set(res) == (keys if cap else keys - {"lesions"})
        assert all(v.is_cuda for v in res.values())
        for k in ("n_target", "matched_target", "n_pred", "matched_pred", "sensitivity", "precision"):
            assert res[k].dtype == plain[k].dtype
            assert np.array_equal(res[k].cpu().numpy(), plain[k].cpu().numpy(), equal_nan=True)
        assert res["froc_hist"].dtype == torch.int64 and np.array_equal(res["froc_hist"].cpu().numpy(), want[2])
        if cap:
            assert res["lesions"].dtype == torch.int64 and np.array_equal(res["lesions"].cpu().numpy(), want[1])

    for mask in (d, d.bool(), d.long() * 7):
        same(lesion_scores(mask, s, t.int(), ignore_index=255), lesion_metrics(mask, t, ignore_index=255),
             ref.image_froc(m, S, T, 256, 8, 0.0, 64, 255), 64)
        same(lesion_scores_3d(mask, {"out": s.double()}, t, (1, 3, 2), ignore_index=255),
             lesion_metrics_3d(mask, t, (1, 3, 2), ignore_index=255),
             ref.stack_froc(m, S, T, (1, 3, 2), 256, 26, 0.0, 64, 255), 64)
    two = torch.stack((1 - s, s), 1)                                # the plane is chosen by channel
    same(lesion_scores(d, two, t, "probs", 1, 16, 4, 0.5, 3), lesion_metrics(d, t, 4, 0.5, 3),
         ref.image_froc(m, S, T, 16, 4, 0.5, 3), 3)
    same(lesion_scores_3d(d, two, t, None, "probs", 1, 2, 6, 1.0, 0), lesion_metrics_3d(d, t, None, 6, 1.0, 0),
         ref.stack_froc(m, S, T, None, 2, 6, 1.0, 0), 0)
    empty = torch.zeros(0, 4, 4, dtype=torch.uint8, device=DEV)
    res = lesion_scores(empty, empty.float(), empty.long())
    assert tuple(res["froc_hist"].shape) == (0, 3, 257) and tuple(res["lesions"].shape) == (0, 2, 64, 3)
    res = lesion_scores_3d(empty, empty.float(), empty.long(), [], bins=16)
    assert tuple(res["froc_hist"].shape) == (0, 3, 17)


# ---------------------------------------------------------------- the C ABI's refusals
def test_c_abi_refusals_leave_the_outputs_untouched():
    from stfunet import _lib
    lib = _lib.load()
    N, H, W, V, cap, bins, K = 4, 5, 70, 2, 8, 16, 2
    m, t = _dev(_random((N, H, W), 0.3, 71), np.uint8), _dev(_random((N, H, W), 0.3, 72), np.int64)
    sc = _dev(np.random.default_rng(73).random((N, K, H, W)), np.float32)
    host = np.array([0, 1, 4], np.int32)
    starts = torch.from_numpy(host).to(DEV)
    summary, table = Guarded(N * 32, 0xAA), Guarded(N * cap * 48, 0xAA)
    hist = Guarded(N * 3 * (bins + 1) * 8, 0xAA)
    scratch = Guarded(lib.stf_froc_scratch_bytes(N, H, W, N, bins), 0xAA)
    s = _lib.stream()
    good2 = dict(mask=m.data_ptr(), src=sc.data_ptr(), K=K, source=0, channel=1, target=t.data_ptr(), B=N, H=H, W=W,
                 connectivity=8, min_overlap=0.5, max_lesions=cap, ignore=-1, bins=bins, summary=summary.ptr(),
                 table=table.ptr(), hist=hist.ptr(), scratch=scratch.ptr())
    good3 = dict(good2, connectivity=26, starts_dev=starts.data_ptr(), starts_host=host.ctypes.data, V=V)

    def call2(**kw):
        a = dict(good2, **kw)
        return lib.stf_froc(a["mask"], a["src"], a["K"], a["source"], a["channel"], a["target"], a["B"], a["H"], a["W"],
                            a["connectivity"], a["min_overlap"], a["max_lesions"], a["ignore"], a["bins"],
                            a["summary"], a["table"], a["hist"], a["scratch"], s)

    def call3(**kw):
        a = dict(good3, **kw)
        return lib.stf_froc3d(a["mask"], a["src"], a["K"], a["source"], a["channel"], a["target"], a["B"], a["H"],
                              a["W"], a["starts_dev"], a["starts_host"], a["V"], a["connectivity"], a["min_overlap"],
                              a["max_lesions"], a["ignore"], a["bins"], a["summary"], a["table"], a["hist"],
                              a["scratch"], s)

    shared = [dict(mask=None), dict(src=None), dict(target=None), dict(summary=None), dict(table=None),
              dict(hist=None), dict(scratch=None),
              dict(B=0), dict(H=0), dict(W=0), dict(H=4097), dict(W=4097), dict(B=1 << 20, H=64, W=64),
              dict(min_overlap=-0.01), dict(min_overlap=1.01), dict(min_overlap=float("nan")), dict(max_lesions=-1),
              dict(K=0), dict(K=17), dict(channel=-1), dict(channel=2), dict(source=-1), dict(source=3),
              dict(bins=0), dict(bins=1), dict(bins=3), dict(bins=48), dict(bins=8192), dict(bins=-16),
              dict(summary=summary.ptr() + 4), dict(table=table.ptr() + 4), dict(hist=hist.ptr() + 4),
              dict(scratch=scratch.ptr() + 4), dict(target=t.data_ptr() + 4), dict(src=sc.data_ptr() + 2)]
    for kw in shared + [dict(connectivity=c) for c in (0, 6, 26, -8)]:
        assert call2(**kw) == EINVAL, kw
    bad_starts = [np.array(b, np.int32) for b in ([1, 2, 4], [0, 2, 3], [0, 0, 4], [0, 4, 4], [0, 3, 2])]
    for kw in (shared + [dict(connectivity=c) for c in (0, 4, 8, 27)] + [dict(starts_dev=None), dict(starts_host=None)]
               + [dict(V=0), dict(V=5), dict(starts_dev=starts.data_ptr() + 2)]
               + [dict(starts_host=b.ctypes.data) for b in bad_starts]):
        assert call3(**kw) == EINVAL, kw
    torch.cuda.synchronize()
    for buf in (summary, table, hist, scratch):
        assert bool((buf.raw == 0xAA).all())
    assert call2() == 0 and call3() == 0 and call3(max_lesions=0, table=None) == 0   # and the good calls are taken
    torch.cuda.synchronize()
    assert all(b.guards_intact() for b in (summary, table, hist, scratch))


# ---------------------------------------------------------------- the predict loops
def _unet_and_loader():
    from oracle.cases import dce_case
    from oracle.init import canonical_state_dict
    from stfunet.unet import UNet
    model = UNet(in_channels=8, num_classes=2, base_c=16)
    model.load_state_dict(canonical_state_dict(model.state_dict(), seed=0))
    loader = [dce_case(500 + i, 3, 8, 32, 32) for i in range(2)]
    loader[1][1][1].zero_()                                        # image 4 of 6: an empty target
    loader[0][1][0, :, 28:] = 255
    return model.to(DEV), loader


def _loop_agrees(res, want, cases):
    summary, table, hist = want
    assert res["froc_hist"].is_cuda and res["froc_hist"].dtype == torch.int64
    assert np.array_equal(res["froc_hist"].cpu().numpy(), hist)
    assert np.array_equal(res["lesion_scores"].cpu().numpy(), table)
    curve = ref.curves(hist, cases)
    assert set(res["froc"]) == set(curve)
    for k, w in curve.items():
        if k == "cpm":
            assert np.isnan(w) == bool(res["froc"][k].isnan()) and not abs(float(res["froc"][k]) - w) > 2.0 ** -49
        else:
            assert np.array_equal(res["froc"][k].cpu().numpy(), w, equal_nan=True), k


def test_predict_loops_report_the_restatement_on_the_masks_and_scores_they_report():
    from stfunet import predict_volumes
    from stfunet.predict import predict, predict_tta
    model, loader = _unet_and_loader()
    T = torch.cat([t for _, t in loader]).numpy()
    dev, depths = torch.device(DEV), (1, 3, 2)
    views = ("none", "w")
    # under tta the loop's score is the mean probability it keeps in `probs`: the restatement reads the same numbers
    for kw in (dict(), dict(froc_overlap=0.5, froc_bins=16, connectivity=4, ignore_index=255),
               dict(keep_largest=True, min_size=3, froc_overlap=0.25, ignore_index=255)):
        res = predict_tta(model, loader, dev, tta=views, keep_probs=True, froc=True, keep_masks=True, **kw)
        masks = torch.cat(res["masks"]).cpu().numpy()
        probs = torch.cat(res["probs"])[:, 1].cpu().numpy()
        want = ref.image_froc(masks, probs, T, kw.get("froc_bins", 256), kw.get("connectivity", 8),
                              kw.get("froc_overlap", 0.0), 64, kw.get("ignore_index"))
        _loop_agrees(res, want, len(T))
        assert want[0][:, 2].sum() > 0                              # the model predicts something
    # without tta the score is the softmax of the logits: take it from tta_probabilities' one-view mean, whose
    # arithmetic is the same (probs.h), so the rows agree bit for bit
    from stfunet import tta_probabilities
    plain = predict_tta(model, loader, dev, tta=None, froc=True, keep_masks=True, froc_overlap=0.25)
    masks = torch.cat(plain["masks"]).cpu().numpy()
    from stfunet.engine import preprocess_input
    with torch.no_grad():
        probs = torch.cat([tta_probabilities(model.eval(), preprocess_input(x, model).to(dev), ("none",))
                           for x, _ in loader])[:, 1].cpu().numpy()
    _loop_agrees(plain, ref.image_froc(masks, probs, T, 256, 8, 0.25, 64), len(T))
    vol = predict_volumes(model, loader, dev, depths, froc=True, keep_masks=True, froc_overlap=0.25,
                          keep_largest=True, ignore_index=255)
    masks = torch.cat(vol["masks"]).cpu().numpy()
    _loop_agrees(vol, ref.stack_froc(masks, probs, T, depths, 256, 26, 0.25, 64, 255), len(depths))
    # off by default: no key, and the default result's keys are what they were
    base = predict(model, loader, dev, keep_masks=True)
    assert set(base) == {"num", "dice", "iou", "mean_dice", "mean_iou", "masks"}
    assert set(predict_volumes(model, loader, dev, depths)) == {"num", "num_volumes", "dice", "iou", "mean_dice",
                                                                 "mean_iou"}
    bare = predict_tta(model, [x for x, _ in loader], dev, tta=None, froc=True)
    assert bare["froc_hist"] is None and bare["froc"] is None and bare["lesion_scores"] is None


def test_one_froc_call_per_flush_and_none_by_default():
    from stfunet import predict_volumes
    from stfunet.predict import predict, predict_tta
    model, loader = _unet_and_loader()
    dev = torch.device(DEV)

    def traced(fn, *args, **kw):
        with lt.tracing() as trace:
            fn(model, loader, dev, *args, **kw)
            torch.cuda.synchronize()
            return [e if isinstance(e, str) else e[0] for e in trace]

    got = traced(predict_tta, tta=None, froc=True)
    assert got.count("stf_froc") == len(loader) and "stf_froc3d" not in got
    assert not any("ccl" in e or "lesion" in e or "score_hist" in e for e in got)
    assert not any("froc" in e for e in traced(predict))
    assert not any("froc" in e for e in traced(predict_tta, tta=None, lesions=True, curves=True))
    for depths, flushes in (((1, 3, 2), 2), ((3, 3), 2), ((6,), 1), ((1, 1, 1, 1, 1, 1), 2)):
        got = traced(predict_volumes, depths, froc=True)
        assert got.count("stf_froc3d") == flushes and "stf_froc" not in got
        assert not any("ccl" in e or "lesion" in e for e in got)
        got = traced(predict_volumes, depths, froc=True, keep_largest=True)
        assert got.count("stf_froc3d") == flushes and got.count("stf_ccl3d_filter") == flushes
        assert not any("froc" in e for e in traced(predict_volumes, depths, lesions=True, curves=True))
