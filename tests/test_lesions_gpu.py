"""Lesion-level detection metrics on the GPU (the lesion kernels of csrc/ccl.hip through the C entry points
and stfunet.predict) against tests/golden/lesions.npz (scipy's labels) and the numpy restatement of
tests/_lesion_ref.py, which tests/test_lesions_cpu.py pins to that fixture.

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

import _launch_trace as lt
import _lesion_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
CASES = ref.cases()
FIXTURE = ref.fixture()
EINVAL = 100001


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


def run(mask, target, depths, connectivity, min_overlap=0.0, max_lesions=64, ignore=None, fill=0xAA):
    """One call of stf_lesion3d_metrics (``depths`` a sequence) or stf_lesion_metrics (``depths`` None:
    per image) on guarded buffers: (summary int64 [V, 4], table int64 [V, 2, max_lesions, 2])."""
    from stfunet import _lib
    N, H, W = mask.shape
    V = N if depths is None else len(depths)
    m, t = _dev(mask, np.uint8), _dev(target, np.int64)
    nbytes = _lib.load().stf_lesion_scratch_bytes(N, H, W, V)
    assert nbytes >= 26 * N * H * W and nbytes % 8 == 0
    summary, table, scratch = Guarded(V * 32, fill), Guarded(V * max_lesions * 32, fill), Guarded(nbytes, fill)
    tail = (connectivity, float(min_overlap), max_lesions, -1 if ignore is None else ignore, summary.ptr(),
            table.ptr(), scratch.ptr(), _lib.stream())
    if depths is None:
        _lib.call("stf_lesion_metrics", m.data_ptr(), t.data_ptr(), N, H, W, *tail)
    else:
        host = np.concatenate([[0], np.cumsum(depths)]).astype(np.int32)
        assert host[-1] == N
        starts = torch.from_numpy(host).to(DEV)
        _lib.call("stf_lesion3d_metrics", m.data_ptr(), t.data_ptr(), N, H, W, starts.data_ptr(), host.ctypes.data,
                  V, *tail)
    torch.cuda.synchronize()
    assert summary.guards_intact() and table.guards_intact() and scratch.guards_intact()
    return (summary.body.cpu().numpy().view(np.int64).reshape(V, 4),
            table.body.cpu().numpy().view(np.int64).reshape(V, 2, max_lesions, 2))


def check(mask, target, depths, connectivity, min_overlap=0.0, max_lesions=64, ignore=None, want=None):
    """Two runs, the second on buffers (scratch included) poisoned with 0xFF, agree byte for byte and
    equal the restatement (and ``want``, the fixture's entry, when given)."""
    mask, target = np.asarray(mask, np.uint8), np.asarray(target, np.int64)
    first = run(mask, target, depths, connectivity, min_overlap, max_lesions, ignore, 0xAA)
    second = run(mask, target, depths, connectivity, min_overlap, max_lesions, ignore, 0xFF)
    if depths is None:
        expect = ref.image_metrics(mask, target, connectivity, min_overlap, max_lesions, ignore)
    else:
        expect = ref.stack_metrics(mask, target, depths, connectivity, min_overlap, max_lesions, ignore)
    for a, b, r in zip(first, second, expect):
        assert a.tobytes() == b.tobytes()
        assert np.array_equal(a, r), (a.tolist(), r.tolist())
    if want is not None:
        assert np.array_equal(first[0], want[0]) and np.array_equal(first[1], want[1])
    return first


def _random(shape, density, seed):
    return (np.random.default_rng(seed).random(shape) < density).astype(np.uint8)


# ---------------------------------------------------------------- the named cases
@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_cases_equal_the_fixture_and_the_restatement(c):
    """Runs, topology, thresholds at exact equality, ignore_index, the table's capacity, ragged depths."""
    args = (c["min_overlap"], c["max_lesions"], c["ignore"], FIXTURE[c["name"]])
    check(c["mask"], c["target"], c["depths"], c["connectivity"], *args)
    if all(d == 1 for d in c["depths"]):                           # the image entry point on the same slices
        check(c["mask"], c["target"], None, ref.FLAT[c["connectivity"]], *args)


def test_empty_sides_give_nan_ratios():
    from stfunet import lesion_metrics_3d
    by_name = {c["name"]: c for c in CASES}
    for name, sens_nan, prec_nan in (("empty_prediction", False, True), ("empty_target", True, False),
                                     ("both_empty", True, True), ("identical", False, False)):
        c = by_name[name]
        res = lesion_metrics_3d(_dev(c["mask"], np.uint8), _dev(c["target"], np.int64), c["depths"],
                                c["connectivity"])
        assert bool(torch.isnan(res["sensitivity"]).all()) == sens_nan
        assert bool(torch.isnan(res["precision"]).all()) == prec_nan
        want = ref.ratios(FIXTURE[name][0])
        assert np.array_equal(res["sensitivity"].cpu().numpy(), want[0], equal_nan=True)
        assert np.array_equal(res["precision"].cpu().numpy(), want[1], equal_nan=True)


# ---------------------------------------------------------------- shapes
@pytest.mark.parametrize("D,H,W", list(itertools.product((1, 2, 3), (1, 2, 5), (1, 63, 64, 65, 130))))
def test_shapes_across_the_chunk_seam(D, H, W):
    m, t = _random((D, H, W), 0.45, 100 * D + 10 * H + W), _random((D, H, W), 0.45, 7 + 100 * D + 10 * H + W)
    for k in (6, 26):
        check(m, t, [D], k, 0.5, 8)
    check(m, t, None, 8, 0.25, 8)


@pytest.mark.parametrize("W", (1, 63, 64, 65, 130))
def test_ragged_depths_in_one_call(W):
    m, t = _random((6, 5, W), 0.4, W), _random((6, 5, W), 0.4, W + 1)
    check(m, t, (1, 3, 2), 18, 0.25, 16)


# ---------------------------------------------------------------- connectivity
def test_every_connectivity_and_depth_one_volumes_are_images():
    m, t = _random((4, 5, 70), 0.35, 21), _random((4, 5, 70), 0.35, 22) * 2
    t[2, :, 30] = 255
    for k in (6, 18, 26):
        check(m, t, (2, 2), k, 0.5, 32, 255)
        vol = check(m, t, (1, 1, 1, 1), k, 0.5, 32, 255)
        img = check(m, t, None, ref.FLAT[k], 0.5, 32, 255)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(vol, img))
    four, eight = check(m, t, None, 4), check(m, t, None, 8)
    assert not np.array_equal(four[0], eight[0])                   # the two are told apart by this input


# ---------------------------------------------------------------- determinism
def test_a_volume_alone_equals_the_volume_inside_a_ragged_stack():
    m, t = _random((6, 5, 130), 0.4, 31), _random((6, 5, 130), 0.4, 32)
    depths = (1, 3, 2)
    stack = check(m, t, depths, 26, 0.5, 16)
    at = 0
    for v, d in enumerate(depths):
        alone = check(m[at:at + d], t[at:at + d], [d], 26, 0.5, 16)
        assert alone[0].tobytes() == stack[0][v:v + 1].tobytes()
        assert alone[1].tobytes() == stack[1][v:v + 1].tobytes()
        at += d


# ---------------------------------------------------------------- the Python surface
def test_python_surface():
    from stfunet import lesion_metrics, lesion_metrics_3d
    m, T = _random((6, 9, 70), 0.3, 41), _random((6, 9, 70), 0.3, 42).astype(np.int64) * 3
    T[4, :, 20:24] = 255
    d, t = torch.from_numpy(m).to(DEV), torch.from_numpy(T).to(DEV)
    keys = {"n_target", "matched_target", "n_pred", "matched_pred", "sensitivity", "precision", "lesions"}

    def same(res, want, cap):
        assert set(res) == (keys if cap else keys - {"lesions"})
        assert all(v.is_cuda for v in res.values())
        cols = torch.stack([res[k] for k in ("n_target", "matched_target", "n_pred", "matched_pred")], 1)
        assert cols.dtype == torch.int64 and np.array_equal(cols.cpu().numpy(), want[0])
        sens, prec = ref.ratios(want[0])
        assert res["sensitivity"].dtype == torch.float64 and res["precision"].dtype == torch.float64
        assert np.array_equal(res["sensitivity"].cpu().numpy(), sens, equal_nan=True)
        assert np.array_equal(res["precision"].cpu().numpy(), prec, equal_nan=True)
        if cap:
            assert res["lesions"].dtype == torch.int64 and np.array_equal(res["lesions"].cpu().numpy(), want[1])

    for mask in (d, d.bool(), d.long() * 7):
        same(lesion_metrics(mask, t.int(), ignore_index=255), ref.image_metrics(m, T, 8, 0.0, 64, 255), 64)
        same(lesion_metrics_3d(mask, t, (1, 3, 2), ignore_index=255), ref.stack_metrics(m, T, (1, 3, 2), 26, 0.0, 64, 255),
             64)
    same(lesion_metrics(d, t, 4, 0.5, 3), ref.image_metrics(m, T, 4, 0.5, 3), 3)
    same(lesion_metrics_3d(d, t, None, 6, 1.0, 0), ref.stack_metrics(m, T, None, 6, 1.0, 0), 0)
    same(lesion_metrics_3d(d, t, [2, 4], 18, 0.25, 200, ignore_index=-1), ref.stack_metrics(m, T, (2, 4), 18, 0.25, 200),
         200)
    empty = torch.zeros(0, 4, 4, dtype=torch.uint8, device=DEV)
    res = lesion_metrics(empty, empty.long())
    assert tuple(res["n_target"].shape) == (0,) and tuple(res["lesions"].shape) == (0, 2, 64, 2)
    res = lesion_metrics_3d(empty, empty.long(), [])
    assert tuple(res["sensitivity"].shape) == (0,)


# ---------------------------------------------------------------- the C ABI's refusals
def test_c_abi_refusals_leave_the_outputs_untouched():
    from stfunet import _lib
    lib = _lib.load()
    N, H, W, V, cap = 4, 5, 70, 2, 8
    m, t = _dev(_random((N, H, W), 0.3, 51), np.uint8), _dev(_random((N, H, W), 0.3, 52), np.int64)
    host = np.array([0, 1, 4], np.int32)
    starts = torch.from_numpy(host).to(DEV)
    summary, table = Guarded(N * 32, 0xAA), Guarded(N * cap * 32, 0xAA)
    scratch = Guarded(lib.stf_lesion_scratch_bytes(N, H, W, N), 0xAA)
    s = _lib.stream()
    good2 = dict(mask=m.data_ptr(), target=t.data_ptr(), B=N, H=H, W=W, connectivity=8, min_overlap=0.5,
                 max_lesions=cap, ignore=-1, summary=summary.ptr(), table=table.ptr(), scratch=scratch.ptr())
    good3 = dict(good2, connectivity=26, starts_dev=starts.data_ptr(), starts_host=host.ctypes.data, V=V)

    def call2(**kw):
        a = dict(good2, **kw)
        return lib.stf_lesion_metrics(a["mask"], a["target"], a["B"], a["H"], a["W"], a["connectivity"],
                                      a["min_overlap"], a["max_lesions"], a["ignore"], a["summary"], a["table"],
                                      a["scratch"], s)

    def call3(**kw):
        a = dict(good3, **kw)
        return lib.stf_lesion3d_metrics(a["mask"], a["target"], a["B"], a["H"], a["W"], a["starts_dev"],
                                        a["starts_host"], a["V"], a["connectivity"], a["min_overlap"],
                                        a["max_lesions"], a["ignore"], a["summary"], a["table"], a["scratch"], s)

    shared = [dict(mask=None), dict(target=None), dict(summary=None), dict(table=None), dict(scratch=None),
              dict(B=0), dict(H=0), dict(W=0), dict(H=4097), dict(W=4097), dict(B=1 << 20, H=64, W=64),
              dict(min_overlap=-0.01), dict(min_overlap=1.01), dict(min_overlap=float("nan")), dict(max_lesions=-1),
              dict(summary=summary.ptr() + 4), dict(table=table.ptr() + 4), dict(scratch=scratch.ptr() + 4),
              dict(target=t.data_ptr() + 4)]
    for kw in shared + [dict(connectivity=c) for c in (0, 6, 26, -8)]:
        assert call2(**kw) == EINVAL, kw
    bad_starts = [np.array(b, np.int32) for b in ([1, 2, 4], [0, 2, 3], [0, 0, 4], [0, 4, 4], [0, 3, 2])]
    for kw in (shared + [dict(connectivity=c) for c in (0, 4, 8, 27)] + [dict(starts_dev=None), dict(starts_host=None)]
               + [dict(V=0), dict(V=5), dict(starts_dev=starts.data_ptr() + 2)]
               + [dict(starts_host=b.ctypes.data) for b in bad_starts]):
        assert call3(**kw) == EINVAL, kw
    torch.cuda.synchronize()
    for buf in (summary, table, scratch):
        assert bool((buf.raw == 0xAA).all())
    assert call2() == 0 and call3() == 0 and call3(max_lesions=0, table=None) == 0   # and the good calls are taken
    torch.cuda.synchronize()
    assert summary.guards_intact() and table.guards_intact() and scratch.guards_intact()


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


def _pooled(res, want, per):
    counts = res["lesion_counts"]
    assert counts.is_cuda and counts.dtype == torch.int64 and np.array_equal(counts.cpu().numpy(), want)
    tot = want.sum(0).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        sens, prec = tot[1] / tot[0], tot[3] / tot[2]
    assert np.array_equal(res["lesion_sensitivity"].cpu().numpy(), sens, equal_nan=True)
    assert np.array_equal(res["lesion_precision"].cpu().numpy(), prec, equal_nan=True)
    false = want[:, 2] - want[:, 3]
    assert res["false_findings"].tolist() == false.tolist()
    assert float(res["false_findings_per_" + per]) == false.astype(np.float64).mean()


def test_predict_reports_the_restatement_on_the_masks_it_reports():
    from stfunet.predict import predict, predict_tta
    model, loader = _unet_and_loader()

    def plain_loop(*args, **kw):                                   # predict's loop; its own parameter list is pinned
        return predict_tta(*args, tta=None, **kw)

    T = torch.cat([t for _, t in loader]).numpy()
    dev = torch.device(DEV)
    for kw in (dict(), dict(lesion_overlap=0.5, connectivity=4, ignore_index=255),
               dict(keep_largest=True, min_size=3, lesion_overlap=0.25, ignore_index=255)):
        res = plain_loop(model, loader, dev, lesions=True, keep_masks=True, **kw)
        masks = torch.cat(res["masks"]).cpu().numpy()
        want = ref.image_metrics(masks, T, kw.get("connectivity", 8), kw.get("lesion_overlap", 0.0), 0,
                                 kw.get("ignore_index"))[0]
        _pooled(res, want, "image")
        assert want[:, 2].sum() > 0                                 # the model predicts something
    plain = predict(model, loader, dev, keep_masks=True)
    assert not any("lesion" in k or "false" in k for k in plain)
    tta = predict_tta(model, loader, dev, tta=("none", "w"), lesions=True, keep_masks=True)
    _pooled(tta, ref.image_metrics(torch.cat(tta["masks"]).cpu().numpy(), T, 8, 0.0, 0)[0], "image")
    bare = plain_loop(model, [x for x, _ in loader], dev, lesions=True)
    assert bare["lesion_counts"] is None and bare["lesion_precision"] is None


def test_predict_volumes_reports_the_restatement_on_the_masks_it_reports():
    from stfunet import predict_volumes
    model, loader = _unet_and_loader()
    T = torch.cat([t for _, t in loader]).numpy()
    dev, depths = torch.device(DEV), (1, 3, 2)
    for kw in (dict(), dict(lesion_overlap=0.5, connectivity=6, ignore_index=255),
               dict(keep_largest=True, min_size=3, lesion_overlap=0.25, ignore_index=255, boundary=True)):
        res = predict_volumes(model, loader, dev, depths, lesions=True, keep_masks=True, **kw)
        masks = torch.cat(res["masks"]).cpu().numpy()
        want = ref.stack_metrics(masks, T, depths, kw.get("connectivity", 26), kw.get("lesion_overlap", 0.0), 0,
                                 kw.get("ignore_index"))[0]
        _pooled(res, want, "case")
    plain = predict_volumes(model, loader, dev, depths)
    assert not any("lesion" in k or "false" in k for k in plain)


def test_one_lesion_call_per_flush_and_none_by_default():
    from stfunet import predict_volumes
    from stfunet.predict import predict, predict_tta
    model, loader = _unet_and_loader()
    dev = torch.device(DEV)

    def traced(fn, *args, **kw):
        with lt.tracing() as trace:
            fn(model, loader, dev, *args, **kw)
            torch.cuda.synchronize()
            return [e if isinstance(e, str) else e[0] for e in trace]

    got = traced(predict_tta, tta=None, lesions=True)
    assert got.count("stf_lesion_metrics") == len(loader) and "stf_lesion3d_metrics" not in got
    assert not any("ccl" in e for e in got)
    assert not any("lesion" in e for e in traced(predict))
    assert not any("lesion" in e for e in traced(predict, keep_largest=True, boundary=True))
    # batches of 3 slices.  (1, 3, 2): the first batch completes one volume, the second two in one call.
    for depths, flushes in (((1, 3, 2), 2), ((3, 3), 2), ((6,), 1), ((1, 1, 1, 1, 1, 1), 2)):
        got = traced(predict_volumes, depths, lesions=True)
        assert got.count("stf_lesion3d_metrics") == flushes and "stf_lesion_metrics" not in got
        assert not any("ccl" in e for e in got)
        got = traced(predict_volumes, depths, lesions=True, keep_largest=True)
        assert got.count("stf_lesion3d_metrics") == flushes and got.count("stf_ccl3d_filter") == flushes
        assert not any("lesion" in e for e in traced(predict_volumes, depths))
        assert not any("lesion" in e for e in traced(predict_volumes, depths, keep_largest=True, boundary=True))
