"""Lesion confidence and FROC without a GPU: the numpy restatement of tests/_froc_ref.py against cases
counted by hand and against tests/golden/froc.npz (scipy's labels), ``froc_curves`` on host tensors
against the restatement, the declared and exported symbols, and every Python-side refusal, which must
come before the library is touched.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _froc_ref as ref

FIXTURE = ref.fixture()


# ---------------------------------------------------------------- the restatement
def test_cases_counted_by_hand():
    got = {name: ref.run_case(c) for name, c in ref.hand_cases().items()}

    def rows_of(hist):
        return [{int(r): int(n) for r, n in enumerate(side) if n} for side in hist]

    # two candidates (conf 128 and 192) on one lesion: it takes the larger; no false finding
    s, t, h = got["two_on_one"]
    assert s.tolist() == [[1, 1, 2, 2]]
    assert t[0, 1, :2].tolist() == [[6, 3, 128], [32, 10, 192]] and t[0, 0, 0].tolist() == [150, 13, 192]
    assert rows_of(h[0]) == [{}, {192: 1}, {128: 1, 192: 1}]
    # one candidate on two lesions: its confidence (160, found outside both) goes to both
    s, t, h = got["one_on_two"]
    assert s.tolist() == [[2, 2, 1, 1]]
    assert t[0, 0, :2].tolist() == [[8, 2, 160], [12, 3, 160]] and t[0, 1, 0].tolist() == [59, 5, 160]
    assert rows_of(h[0]) == [{}, {160: 2}, {160: 1}]
    # min_overlap 0.5: both candidates graze a lesion and fail (1 of 8, 2 of 10), so both are false findings
    # and both lesions keep det 0 -- also the second, which the target-side rule still counts (2 of 4)
    s, t, h = got["grazing"]
    assert s.tolist() == [[2, 1, 2, 0]]
    assert t[0, 0, :2].tolist() == [[8, 1, 0], [4, 2, 0]] and t[0, 1, :2].tolist() == [[8, 1, 128], [10, 2, 256]]
    assert rows_of(h[0]) == [{128: 1, 256: 1}, {0: 2}, {}]
    # 0, -0, a negative, NaN and -inf: conf 0, and a matched candidate of conf 0 leaves det at 0
    s, t, h = got["zero_conf"]
    assert s.tolist() == [[1, 1, 1, 1]] and t[0, :, 0].tolist() == [[4, 3, 0], [5, 3, 0]]
    assert rows_of(h[0]) == [{}, {0: 1}, {0: 1}]
    # +inf and 1.5 land in row bins = 16
    s, t, h = got["above_one"]
    assert t[0, 1, :2, 2].tolist() == [16, 16] and t[0, 0, :2, 2].tolist() == [16, 16]
    assert rows_of(h[0]) == [{}, {16: 2}, {16: 2}]
    # the ignored column cuts the candidate: 3..63 (conf 192, on the lesion) and 65..66 (conf 128, a false finding)
    s, t, h = got["ignore_splits"]
    assert s.tolist() == [[1, 1, 2, 1]]
    assert t[0, 1, :2].tolist() == [[61, 25, 192], [2, 0, 128]] and t[0, 0, 0].tolist() == [25, 25, 192]
    assert rows_of(h[0]) == [{128: 1}, {192: 1}, {192: 1}]


@pytest.mark.parametrize("name", list(FIXTURE))
def test_restatement_equals_the_fixture(name):
    c, want = FIXTURE[name]
    got = ref.run_case(c)
    for a, b in zip(got, want):
        assert a.dtype == np.int64 and np.array_equal(a, b)
    summary, table, hist = got
    assert np.array_equal(hist.sum(-1), np.stack([summary[:, 2] - summary[:, 3], summary[:, 0], summary[:, 3]], 1))
    assert table.shape[2:] == (c["max_lesions"], 3)


def test_fixture_holds_the_cases():
    made = {c["name"]: c for c in ref.cases()}
    assert list(made) == list(FIXTURE)
    for name, (c, _) in FIXTURE.items():
        for k in ("mask", "scores", "target"):
            assert np.array_equal(c[k], made[name][k], equal_nan=(k == "scores"))
        assert all(c[k] == made[name][k] for k in ("depths", "bins", "connectivity", "min_overlap", "max_lesions",
                                                    "ignore"))
        s = c["scores"][np.isfinite(c["scores"])].astype(np.float64) * 2 * c["bins"]
        assert np.array_equal(s, np.round(s))                       # row edges and midpoints only


# ---------------------------------------------------------------- froc_curves on the host
def _same(got, want):
    assert set(got) == set(want)
    for k, w in want.items():
        g = got[k]
        assert not g.is_cuda
        assert g.dtype == (torch.int64 if np.asarray(w).dtype == np.int64 else torch.float64), k
        if k == "cpm":
            # the mean of at most 8 values in [0, 1]: the two libraries add in different orders, each sum is
            # within 7 roundings of half an ulp of a number below 8 of the exact one: 8 * 2^-52 covers both
            assert np.array_equal(np.isnan(g.numpy()), np.isnan(w)) and not abs(float(g) - float(w)) > 2.0 ** -49, k
            continue
        assert np.array_equal(g.numpy(), w, equal_nan=True), k


def _hist(rng, bins, scale=5):
    return rng.integers(0, scale, (3, bins + 1)).astype(np.int64)


@pytest.mark.parametrize("bins", (2, 16, 256, 4096))
def test_froc_curves_equal_the_restatement(bins):
    from stfunet import froc_curves
    rng = np.random.default_rng(bins)
    h = _hist(rng, bins)
    res = froc_curves(torch.from_numpy(h))
    _same(res, ref.curves(h))
    for k in ("detected", "false_findings", "matched"):
        assert bool((res[k][1:] <= res[k][:-1]).all()) and int(res[k][-1]) == 0
    assert int(res["detected"][0]) == h[1, 1:].sum() and int(res["n_lesions"]) == h[1].sum()
    _same(froc_curves(torch.from_numpy(h), cases=7, rates=(0, 0.5, 3)), ref.curves(h, 7, (0, 0.5, 3)))
    _same(froc_curves(torch.from_numpy(h.astype(np.int32)), cases=2.5), ref.curves(h, 2.5))
    stack = np.stack([_hist(rng, bins) for _ in range(5)])
    pooled = froc_curves(torch.from_numpy(stack))
    _same(pooled, ref.curves(stack))
    _same(pooled, ref.curves(stack.sum(0), 5))                      # pooling equals summing first
    _same(froc_curves(torch.from_numpy(stack), cases=3), ref.curves(stack.sum(0), 3))


def test_sensitivity_at_a_rate_hit_exactly_and_one_just_missed():
    from stfunet import froc_curves
    h = np.zeros((3, 5), np.int64)
    h[0] = [0, 3, 2, 1, 0]                               # false findings above j: 6, 3, 1, 0, 0
    h[1] = [1, 1, 1, 1, 0]                               # detected above j:       3, 2, 1, 0, 0 of 4
    h[2] = [0, 1, 1, 1, 0]
    res = froc_curves(torch.from_numpy(h), cases=2, rates=(3, 1.5, 1.49, 0.5, 0.49, 0))
    assert res["false_findings"].tolist() == [6, 3, 1, 0, 0]
    # 6 <= 3 * 2 at j = 0; 3 <= 1.5 * 2 exactly at j = 1; 2.98 misses it: j = 2; 1 <= 0.5 * 2 at j = 2; then j = 3
    assert res["sensitivity_at"].tolist() == [0.75, 0.5, 0.25, 0.25, 0.0, 0.0]
    assert float(res["cpm"]) == np.mean([0.75, 0.5, 0.25, 0.25, 0.0, 0.0])
    assert res["fp_per_case"].tolist() == [3.0, 1.5, 0.5, 0.0, 0.0]
    assert res["precision"].tolist() == [3 / 9, 2 / 5, 1 / 2, 1.0, 1.0]       # 1 where nothing is predicted
    _same(res, ref.curves(h, 2, (3, 1.5, 1.49, 0.5, 0.49, 0)))


def test_no_lesions_is_nan():
    from stfunet import froc_curves
    h = np.zeros((3, 17), np.int64)
    h[0, 3] = 2
    res = froc_curves(torch.from_numpy(h))
    assert bool(torch.isnan(res["sensitivity"]).all() and torch.isnan(res["sensitivity_at"]).all())
    assert bool(torch.isnan(res["cpm"])) and int(res["n_lesions"]) == 0
    _same(res, ref.curves(h))


def test_froc_curves_refusals():
    from stfunet import froc_curves
    good = torch.zeros(3, 17, dtype=torch.int64)
    for bad in (torch.zeros(2, 17, dtype=torch.int64), torch.zeros(17, dtype=torch.int64),
                torch.zeros(1, 1, 3, 17, dtype=torch.int64), torch.zeros(3, 2, dtype=torch.int64)):
        with pytest.raises(ValueError, match="hist must be"):
            froc_curves(bad)
    with pytest.raises(ValueError, match="integer tensor"):
        froc_curves(good.double())
    with pytest.raises(ValueError, match="bins"):
        froc_curves(torch.zeros(3, 13, dtype=torch.int64))
    for bad in (0, -1, "2", True, float("nan")):
        with pytest.raises(ValueError, match="cases"):
            froc_curves(good, cases=bad)
    with pytest.raises(ValueError, match="cases"):
        froc_curves(torch.zeros(0, 3, 17, dtype=torch.int64))
    for bad in ((), (-1,), ("1",), 3, (True,)):
        with pytest.raises(ValueError, match="rates"):
            froc_curves(good, rates=bad)


# ---------------------------------------------------------------- the surface
def test_symbols_are_declared_and_exported():
    import stfunet
    from stfunet import _lib
    from stfunet import predict as P
    for name in ("lesion_scores", "lesion_scores_3d", "froc_curves"):
        assert name in stfunet.__all__ and getattr(stfunet, name) is getattr(P, name)
    assert stfunet.__all__ == sorted(stfunet.__all__)
    names = {"stf_froc_scratch_bytes", "stf_froc", "stf_froc3d"}
    header = open(os.path.join(os.path.dirname(ref.GOLDEN), "..", "include", "stfunet.h")).read()
    assert set(re.findall(r"\b(stf_froc[0-9a-z_]*)\s*\(", header)) == names <= set(_lib.EXPORTED)
    c_int, c_int64, P_ = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
    head = [P_, P_, c_int, c_int, c_int, P_, c_int, c_int, c_int]
    tail = [c_int, ctypes.c_double, c_int, c_int64, c_int, P_, P_, P_, P_, P_]
    assert _lib._SIGS["stf_froc_scratch_bytes"] == (ctypes.c_size_t, [c_int] * 5)
    assert _lib._SIGS["stf_froc"] == (c_int, head + tail)
    assert _lib._SIGS["stf_froc3d"] == (c_int, head + [P_, P_, c_int] + tail)
    lib = _lib.load()
    assert all(hasattr(lib, s) for s in names)
    assert lib.stf_abi_version() == 17


def test_scratch_bytes():
    from stfunet import _lib
    lib = _lib.load()
    for N, H, W, V in ((1, 1, 1, 1), (6, 5, 65, 3), (6, 5, 65, 6), (128, 256, 256, 8)):
        for bins in (2, 256, 4096):
            nbytes = lib.stf_froc_scratch_bytes(N, H, W, V, bins)
            assert nbytes % 8 == 0 and 36 * N * H * W <= nbytes <= 36 * N * H * W + 8 * V + 16 * N + 3 * 256 + 16
    for bad in ((0, 4, 4, 1, 256), (2, 0, 4, 1, 256), (2, 4, 0, 1, 256), (2, 4097, 4, 1, 256), (2, 4, 4097, 1, 256),
                (2, 4, 4, 0, 256), (2, 4, 4, 3, 256), (1 << 15, 256, 256, 1, 256), (2, 4, 4, 1, 0), (2, 4, 4, 1, 1),
                (2, 4, 4, 1, 3), (2, 4, 4, 1, 8192), (2, 4, 4, 1, -256)):
        assert lib.stf_froc_scratch_bytes(*bad) == 0


def test_python_argument_refusals(monkeypatch):
    from stfunet import _lib
    from stfunet import predict as P

    def touched(*a, **k):
        raise AssertionError("the library was touched before the arguments were refused")

    monkeypatch.setattr(P, "call", touched)
    monkeypatch.setattr(P, "load", touched)
    monkeypatch.setattr(_lib, "call", touched)
    m = torch.zeros(4, 8, 8, dtype=torch.uint8)
    t = torch.zeros(4, 8, 8, dtype=torch.int64)
    s = torch.zeros(4, 2, 8, 8)
    ident = torch.nn.Identity()
    both = (P.lesion_scores, P.lesion_scores_3d)
    for f in both:
        for bad in (0, 1, 3, 100, 8192, -256, 256.0, "256", None, True):
            with pytest.raises(ValueError, match="bins must be a power of two"):
                f(m, s, t, bins=bad)
        for bad in (-1, 2, 1.0, "0", None, True):
            with pytest.raises(ValueError, match="channel"):
                f(m, s, t, channel=bad)
        for bad in ("logits", 0, None):
            with pytest.raises(ValueError, match="unknown source"):
                f(m, s, t, source=bad)
        for bad in (s[:3], s[:, :, :7], torch.zeros(4, 2, 8, 9), torch.zeros(3, 8, 8)):
            with pytest.raises(ValueError, match="do not match the mask"):
                f(m, bad, t)
        for bad in (torch.zeros(8, 8), torch.zeros(4, 1, 2, 8, 8)):
            with pytest.raises(ValueError, match=r"scores must be \[N, K, H, W\]"):
                f(m, bad, t)
        with pytest.raises(ValueError, match="floating-point"):
            f(m, s.long(), t)
        with pytest.raises(ValueError, match="planes are supported"):
            f(m, torch.zeros(4, 17, 8, 8), t)
        with pytest.raises(ValueError, match="does not match"):
            f(m, s, t[:3])
        with pytest.raises(ValueError, match="integer tensor"):
            f(m, s, t.float())
        for bad in (-0.01, 1.01, float("nan"), "0.5", None, True):
            with pytest.raises(ValueError, match="min_overlap"):
                f(m, s, t, min_overlap=bad)
        for bad in (-1, 1.0, None, True, (1 << 20) + 1):
            with pytest.raises(ValueError, match="max_lesions"):
                f(m, s, t, max_lesions=bad)
        with pytest.raises(RuntimeError, match="no CPU fallback"):       # host tensors, everything else in order
            f(m, s, t)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            f(m, s[:, 0], t, source="sigmoid", bins=2)
    for bad in (0, 6, 26, "8", None, True):
        with pytest.raises(ValueError, match="connectivity"):
            P.lesion_scores(m, s, t, connectivity=bad)
    for bad in (0, 4, 8, "26", None, True):
        with pytest.raises(ValueError, match="connectivity"):
            P.lesion_scores_3d(m, s, t, connectivity=bad)
    for bad in ([3], [2, 3], [0, 4], [4.0], 4, "4", True):
        with pytest.raises(ValueError, match="depths"):
            P.lesion_scores_3d(m, s, t, depths=bad)
    # the loops check their options before the first batch
    for bad in (0, 3, 8192, None):
        with pytest.raises(ValueError, match="bins"):
            P.predict_tta(ident, [], "cpu", tta=None, froc=True, froc_bins=bad)
        with pytest.raises(ValueError, match="bins"):
            P.predict_volumes(ident, [], "cpu", [], froc=True, froc_bins=bad)
    for bad in (-0.01, 1.01, float("nan"), None):
        with pytest.raises(ValueError, match="min_overlap"):
            P.predict_tta(ident, [], "cpu", froc=True, froc_overlap=bad)
        with pytest.raises(ValueError, match="min_overlap"):
            P.predict_volumes(ident, [], "cpu", [], froc=True, froc_overlap=bad)
    for bad in (-1, 1.0, None):
        with pytest.raises(ValueError, match="curve_channel"):
            P.predict_tta(ident, [], "cpu", tta=None, froc=True, curve_channel=bad)
        with pytest.raises(ValueError, match="curve_channel"):
            P.predict_volumes(ident, [], "cpu", [], froc=True, curve_channel=bad)
    # off: the options are not looked at, and an empty loader gives the keys as None when on
    assert "froc" not in P.predict_tta(ident, [], "cpu", tta=None, froc=False, froc_bins=3)
    res = P.predict_tta(ident, [], "cpu", tta=None, froc=True)
    assert res["froc_hist"] is None and res["froc"] is None and res["lesion_scores"] is None
    res = P.predict_volumes(ident, [], "cpu", [], froc=True)
    assert res["froc_hist"] is None and res["froc"] is None and res["lesion_scores"] is None
