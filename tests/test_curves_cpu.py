"""Score histograms and threshold curves without a device: the numpy restatement (tests/_curves_ref.py)
against tests/golden/curves.npz (rows by counting thresholds in float64; scikit-learn's AUROC and average
precision), the row rule's edge cases and its threshold identity, the declared and exported symbols, and
the Python argument refusals, which all come before anything touches a device."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _curves_ref as ref

CASES = ref.cases()
FIXTURE = ref.fixture()


def test_the_fixture_holds_every_case():
    assert list(FIXTURE) == [c["name"] for c in CASES] and len(set(FIXTURE)) == len(CASES)
    assert os.path.getsize(os.path.join(ref.GOLDEN, "curves.npz")) < 64 * 1024


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_the_restatement_reproduces_the_fixture(c):
    hist = ref.histogram(c["scores"], c["target"], c["bins"], c["positive"], c["ignore"])
    want, auroc, ap = FIXTURE[c["name"]]
    N = c["scores"].shape[0]
    assert hist.shape == (N, 2, c["bins"] + 1) and hist.dtype == np.int64
    assert np.array_equal(hist.sum(0), want)
    kept = c["target"] != c["ignore"] if c["ignore"] is not None else np.ones(c["target"].shape, bool)
    assert hist.sum() == kept.sum()
    got = ref.curves(hist.sum(0))
    if np.isnan(auroc):
        assert np.isnan(got["auroc"]) and np.isnan(got["average_precision"])
    else:
        assert abs(got["auroc"] - auroc) <= 1e-12 and abs(got["average_precision"] - ap) <= 1e-12


def test_the_cases_say_what_their_names_say():
    f = FIXTURE
    assert np.isnan(f["all_negative"][1]) and np.isnan(f["all_positive"][2])
    assert f["all_negative"][0][1].sum() == 0 and f["all_positive"][0][0].sum() == 0
    assert f["separable"][1] == 1.0 and f["separable"][2] == 1.0
    h = f["trained_like"][0]
    assert h[:, [0, -1]].sum() > 0.9 * h.sum()                       # the end rows hold nearly everything
    assert 0.5 < f["uniform_b256"][1] < 1.0
    c = ref.curves(f["separable"][0])
    assert c["best_threshold"] == 2 / 16 and c["best_dice"] > 0.999   # first maximum: the lowest threshold
    assert f["ignore_255"][0].sum() == 2 * 9 * 11 - 9


@pytest.mark.parametrize("bins", ref.BINS)
def test_row_rule_edges(bins):
    e = ref.edge_scores(bins)
    r = ref.rows(e, bins)
    n = bins + 1
    assert r[:n].tolist() == list(range(n))                            # j / bins is the top of row j
    assert r[n:2 * n].tolist() == list(range(n))                       # just below: still row j (below 0: row 0)
    assert r[2 * n:3 * n].tolist() == list(range(1, n)) + [bins]       # just above: the next row, capped
    assert r[3 * n:].tolist() == ref.special_rows(bins)
    assert r.min() == 0 and r.max() == bins


@pytest.mark.parametrize("bins", ref.BINS)
def test_rows_above_j_are_the_scores_above_j_over_bins(bins):
    rng = np.random.default_rng(bins)
    p = np.concatenate([ref.edge_scores(bins), rng.random(4096).astype(np.float32)])
    p = p[~(p > 1)]                                                   # the identity is stated for p <= 1 (NaN stays)
    r = ref.rows(p, bins)
    for j in range(bins + 1):
        with np.errstate(invalid="ignore"):
            assert np.array_equal(r > j, p > np.float32(j / bins)), j


def test_curves_of_a_hand_table():
    # bins 2: rows 0, 1, 2.  negatives (3, 1, 0), positives (1, 1, 2)
    c = ref.curves(np.array([[3, 1, 0], [1, 1, 2]]), cal_groups=2, smooth=0.0)
    assert c["tp"].tolist() == [3, 2, 0] and c["fp"].tolist() == [1, 0, 0]
    assert c["fn"].tolist() == [1, 2, 4] and c["tn"].tolist() == [3, 4, 4]
    assert c["dice"][0] == 6 / 8 and c["iou"][0] == 3 / 5
    # ROC points (1,1), (1/4, 3/4), (0, 1/2), (0, 0): area = 3/4 * 7/8 + 1/4 * 5/8
    assert abs(c["auroc"] - (0.75 * 0.875 + 0.25 * 0.625)) < 1e-15
    # rows descending: k=2 R=1/2 P=1; k=1 R=3/4 P=3/4; k=0 R=1 P=1/2
    assert abs(c["average_precision"] - (0.5 + 0.25 * 0.75 + 0.25 * 0.5)) < 1e-15
    # groups: rows {0, 1} and {2}; confidences 0, 0.25, 0.75
    assert c["reliability"][:, 0].tolist() == [6, 2]
    assert c["reliability"][0, 1] == (2 * 0.25) / 6 and c["reliability"][0, 2] == 2 / 6
    assert c["reliability"][1].tolist() == [2, 0.75, 1.0]
    assert abs(c["ece"] - (6 * abs(2 / 6 - 0.5 / 6) + 2 * 0.25) / 8) < 1e-15


def test_symbols_are_declared_and_exported():
    import stfunet
    from stfunet import _lib
    from stfunet import predict as P
    for name in ("score_histogram", "threshold_curves"):
        assert name in stfunet.__all__ and getattr(stfunet, name) is getattr(P, name)
    assert stfunet.__all__ == sorted(stfunet.__all__)
    header = open(os.path.join(os.path.dirname(ref.GOLDEN), "..", "include", "stfunet.h")).read()
    assert re.findall(r"\b(stf_score[0-9a-z_]*)\s*\(", header) == ["stf_score_hist"]
    assert "stf_score_hist" in _lib.EXPORTED
    c_int, c_int64, P_ = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
    assert _lib._SIGS["stf_score_hist"] == (c_int, [P_] + [c_int] * 6 + [P_, c_int64, c_int64, c_int, P_, P_])
    for dtype in (torch.bfloat16, torch.float16):
        lib = _lib.load(dtype)
        assert hasattr(lib, "stf_score_hist") and lib.stf_abi_version() == 17


def test_c_abi_refusals_need_no_device():
    from stfunet import _lib
    lib = _lib.load()
    fake = ctypes.c_void_p(1 << 20)
    good = dict(src=fake, N=2, K=3, H=4, W=5, source=0, channel=1, target=fake, positive=-1, ignore=-1, bins=16,
                hist=fake)

    def call(**kw):
        a = dict(good, **kw)
        return lib.stf_score_hist(a["src"], a["N"], a["K"], a["H"], a["W"], a["source"], a["channel"], a["target"],
                                  a["positive"], a["ignore"], a["bins"], a["hist"], None)

    bad = [dict(bins=b) for b in (3, 8192, 0, 1, -16, 24)] + [dict(K=17), dict(K=0), dict(channel=3), dict(channel=-1),
           dict(src=None), dict(target=None), dict(hist=None), dict(source=3), dict(source=-1), dict(N=0), dict(H=0),
           dict(W=0), dict(H=4097), dict(W=4097), dict(N=1 << 20, H=64, W=64),
           dict(target=ctypes.c_void_p((1 << 20) + 4)), dict(hist=ctypes.c_void_p((1 << 20) + 4)),
           dict(src=ctypes.c_void_p((1 << 20) + 2))]
    for kw in bad:
        assert call(**kw) == 100001, kw


def test_python_argument_refusals():
    from stfunet import predict as P
    s = torch.zeros(4, 3, 8, 8)
    t = torch.zeros(4, 8, 8, dtype=torch.int64)
    ident = torch.nn.Identity()
    for bad in (3, 8192, 0, 1, 256.0, "256", None, True):
        with pytest.raises(ValueError, match="bins"):
            P.score_histogram(s, t, bins=bad)
        with pytest.raises(ValueError, match="bins"):
            P.predict_tta(ident, [], "cpu", tta=None, curves=True, curve_bins=bad)
        with pytest.raises(ValueError, match="bins"):
            P.predict_tta(ident, [], "cpu", curves=True, curve_bins=bad)
        with pytest.raises(ValueError, match="bins"):
            P.predict_volumes(ident, [], "cpu", [], curves=True, curve_bins=bad)
    for bad in (-1, 1.0, "1", None, True):
        with pytest.raises(ValueError, match="curve_channel"):
            P.predict_tta(ident, [], "cpu", tta=None, curves=True, curve_channel=bad)
        with pytest.raises(ValueError, match="curve_channel"):
            P.predict_volumes(ident, [], "cpu", [], curves=True, curve_channel=bad)
    for bad in (3, -1, 1.0, None, True):
        with pytest.raises(ValueError, match="channel"):
            P.score_histogram(s, t, channel=bad)
    with pytest.raises(ValueError, match="source"):
        P.score_histogram(s, t, source="logits")
    for bad in (-1, 1.0, "1", True):
        with pytest.raises(ValueError, match="positive"):
            P.score_histogram(s, t, positive=bad)
    for bad in (1.0, "255", True):
        with pytest.raises(ValueError, match="ignore_index"):
            P.score_histogram(s, t, ignore_index=bad)
    with pytest.raises(ValueError, match="planes"):
        P.score_histogram(torch.zeros(4, 17, 8, 8), t)
    with pytest.raises(ValueError, match=r"\[N, K, H, W\]"):
        P.score_histogram(s[0, 0], t)
    with pytest.raises(ValueError, match="floating-point"):
        P.score_histogram(s.long(), t)
    with pytest.raises(ValueError, match="does not match"):
        P.score_histogram(s, t[:3])
    with pytest.raises(ValueError, match="integer tensor"):
        P.score_histogram(s, t.float())
    for bad in ([3], [2, 3], [0, 4], [4.0], 4, "4", True):
        with pytest.raises(ValueError, match="depths"):
            P.score_histogram(s, t, depths=bad)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.score_histogram(s, t, "softmax", 2, 16, 1, 255, [1, 3])      # every check passed: only the device is missing
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.score_histogram(s[:, 0], t)
    # the curve options are not looked at while curves is off: the loops run as they always did
    assert "score_hist" not in P.predict_tta(ident, [], "cpu", tta=None, curve_bins=7)
    assert "score_hist" not in P.predict_volumes(ident, [], "cpu", [], curve_bins=7)
    for res in (P.predict_tta(ident, [], "cpu", tta=None, curves=True), P.predict_volumes(ident, [], "cpu", [], curves=True)):
        assert all(res[k] is None for k in P.CURVE_KEYS)


def test_threshold_curves_on_the_host_equal_the_restatement():
    """threshold_curves is torch ops on whatever device the table is on: checked here on the host."""
    from stfunet import threshold_curves
    for c in CASES:
        hist = ref.histogram(c["scores"], c["target"], c["bins"], c["positive"], c["ignore"])
        for table, groups in ((hist.sum(0), 2), (hist, 1 if c["bins"] == 2 else 16)):
            got = threshold_curves(torch.from_numpy(table), cal_groups=groups)
            wants = [ref.curves(h, groups) for h in (table if table.ndim == 3 else table[None])]
            for k in got:
                g = got[k].numpy()
                if k == "thresholds":
                    assert np.array_equal(g, wants[0][k])
                    continue
                g = g if table.ndim == 3 else g[None]
                w = np.stack([np.asarray(x[k]) for x in wants])
                assert g.shape == w.shape, k
                if k in ("tp", "fp", "fn", "tn"):
                    assert got[k].dtype == torch.int64 and np.array_equal(g, w), k
                elif k in ("dice", "iou", "best_threshold", "best_dice"):
                    assert np.array_equal(g, w), k                   # elementwise float64: the same bits
                else:
                    assert got[k].dtype == torch.float64
                    assert np.allclose(g, w, rtol=0, atol=1e-12, equal_nan=True), k
                    assert np.array_equal(np.isnan(g), np.isnan(w)), k
    for bad in (3, 0, -1, 2.0, None, True, 32):
        with pytest.raises(ValueError, match="cal_groups"):
            threshold_curves(torch.zeros(2, 17, dtype=torch.int64), cal_groups=bad)
    with pytest.raises(ValueError, match="bins"):
        threshold_curves(torch.zeros(2, 16, dtype=torch.int64))
    with pytest.raises(ValueError, match=r"\[..., 2, bins \+ 1\]"):
        threshold_curves(torch.zeros(3, 17, dtype=torch.int64))
    with pytest.raises(ValueError, match="integer tensor"):
        threshold_curves(torch.zeros(2, 17))
