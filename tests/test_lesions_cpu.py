"""Lesion-level detection metrics without a device: the numpy restatement (tests/_lesion_ref.py) against
tests/golden/lesions.npz (scipy's labels), the declared and exported symbols, and the Python argument
refusals, which all come before anything touches a device."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _lesion_ref as ref

CASES = ref.cases()
FIXTURE = ref.fixture()


def test_the_fixture_holds_every_case():
    assert list(FIXTURE) == [c["name"] for c in CASES] and len(set(FIXTURE)) == len(CASES)
    assert os.path.getsize(os.path.join(ref.GOLDEN, "lesions.npz")) < 64 * 1024


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_the_restatement_reproduces_the_fixture(c):
    summary, table = ref.stack_metrics(c["mask"], c["target"], c["depths"], c["connectivity"], c["min_overlap"],
                                       c["max_lesions"], c["ignore"])
    want_summary, want_table = FIXTURE[c["name"]]
    V = len(c["depths"])
    assert summary.shape == (V, 4) and table.shape == (V, 2, c["max_lesions"], 2)
    assert summary.dtype == np.int64 and table.dtype == np.int64
    assert np.array_equal(summary, want_summary) and np.array_equal(table, want_table)
    if all(d == 1 for d in c["depths"]):                           # an image is a volume one slice deep
        flat = ref.image_metrics(c["mask"], c["target"], ref.FLAT[c["connectivity"]], c["min_overlap"],
                                 c["max_lesions"], c["ignore"])
        assert np.array_equal(flat[0], want_summary) and np.array_equal(flat[1], want_table)


def test_the_cases_say_what_their_names_say():
    s = {name: v[0] for name, v in FIXTURE.items()}
    t = {name: v[1] for name, v in FIXTURE.items()}
    assert s["bridge"].tolist() == [[2, 2, 1, 1]]
    assert s["two_hits"].tolist() == [[1, 1, 3, 2]]
    assert s["edge_touch"].tolist() == [[2, 0, 3, 0]] and s["corner_touch"].tolist() == [[2, 0, 2, 0]]
    assert (s["identical"][:, 0] == s["identical"][:, 1]).all() and (s["identical"][:, 0] == s["identical"][:, 2]).all()
    assert (s["disjoint"][:, [1, 3]] == 0).all() and (s["disjoint"][:, [0, 2]] > 0).all()
    assert (s["empty_prediction"][:, 1:] == 0).all() and s["empty_prediction"][0, 0] > 0
    assert (s["empty_target"][:, [0, 1, 3]] == 0).all() and s["empty_target"][0, 2] > 0
    assert s["both_empty"].tolist() == [[0, 0, 0, 0]]
    sens, prec = ref.ratios(s["both_empty"])
    assert np.isnan(sens).all() and np.isnan(prec).all()
    sens, prec = ref.ratios(s["empty_prediction"])
    assert sens.tolist() == [0.0] and np.isnan(prec).all()
    assert s["seam_run"].tolist() == [[2, 2, 3, 2]] and t["seam_run"][0, 0, :2].tolist() == [[10, 3], [10, 3]]
    assert s["one_voxel_runs"].tolist() == [[65, 2, 33, 2]]
    for name, n in (("checkerboard_image", 256), ("checkerboard_volume", 512)):
        # the target is the whole board; the prediction changes to the other colour at column 40, where
        # the two colours meet edge to edge in every other row
        assert s[name][0, 0] == n and s[name][0, 2] == n - n // 64 and t[name].shape[2] == 64 < n - n // 64
        assert 0 < s[name][0, 1] < n
    # six lesions with hit / area = 4/8, 3/8, 2/8, 1/8, 8/8, 4/4 and predictions 4/4, 3/3, 2/4, 1/4, 8/8, 4/8
    assert s["overlap_0.25"].tolist() == [[6, 5, 6, 6]]
    assert s["overlap_0.5"].tolist() == [[6, 3, 6, 5]]
    assert s["overlap_1"].tolist() == [[6, 2, 6, 3]]
    # the ignored column cuts the long row on either side; the ignored voxels are in no area
    assert s["ignore_none"].tolist() == [[1, 1, 1, 1], [1, 1, 1, 1]]
    assert s["ignore_255"].tolist() == [[2, 2, 2, 2], [1, 0, 1, 0]]
    assert t["ignore_255"][0, 0, :2].tolist() == [[59, 59], [4, 2]]
    assert t["ignore_255"][0, 1, :2].tolist() == [[61, 59], [2, 2]]
    assert t["ignore_255"][1, 0, 0].tolist() == [15, 0] and t["ignore_255"][1, 1, 0].tolist() == [15, 0]
    n = int(s["capacity_equal"][:, [0, 2]].max())
    assert [t["capacity_" + k].shape[2] for k in ("below", "equal", "above", "none")] == [n - 1, n, n + 3, 0]
    assert all(np.array_equal(s["capacity_" + k], s["capacity_equal"]) for k in ("below", "above", "none"))
    assert np.array_equal(t["capacity_below"], t["capacity_above"][:, :, :n - 1])
    assert (t["capacity_above"][:, :, n:] == 0).all()


def test_symbols_are_declared_and_exported():
    import stfunet
    from stfunet import _lib
    from stfunet import predict as P
    for name in ("lesion_metrics", "lesion_metrics_3d"):
        assert name in stfunet.__all__ and getattr(stfunet, name) is getattr(P, name)
    assert stfunet.__all__ == sorted(stfunet.__all__)
    names = {"stf_lesion_scratch_bytes", "stf_lesion_metrics", "stf_lesion3d_metrics"}
    header = open(os.path.join(os.path.dirname(ref.GOLDEN), "..", "include", "stfunet.h")).read()
    assert set(re.findall(r"\b(stf_lesion[0-9a-z_]*)\s*\(", header)) == names <= set(_lib.EXPORTED)
    c_int, c_int64, P_ = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
    tail = [c_int, ctypes.c_double, c_int, c_int64, P_, P_, P_, P_]
    assert _lib._SIGS["stf_lesion_scratch_bytes"] == (ctypes.c_size_t, [c_int] * 4)
    assert _lib._SIGS["stf_lesion_metrics"] == (c_int, [P_, P_, c_int, c_int, c_int] + tail)
    assert _lib._SIGS["stf_lesion3d_metrics"] == (c_int, [P_, P_, c_int, c_int, c_int, P_, P_, c_int] + tail)
    lib = _lib.load()
    assert all(hasattr(lib, s) for s in names)
    assert lib.stf_abi_version() == 17


def test_scratch_bytes():
    from stfunet import _lib
    lib = _lib.load()
    for N, H, W, V in ((1, 1, 1, 1), (6, 5, 65, 3), (6, 5, 65, 6), (128, 256, 256, 8)):
        nbytes = lib.stf_lesion_scratch_bytes(N, H, W, V)
        assert nbytes % 8 == 0 and 26 * N * H * W <= nbytes <= 26 * N * H * W + 8 * V + 16 * N + 3 * 256 + 16
    for bad in ((0, 4, 4, 1), (2, 0, 4, 1), (2, 4, 0, 1), (2, 4097, 4, 1), (2, 4, 4097, 1), (2, 4, 4, 0), (2, 4, 4, 3),
                (1 << 15, 256, 256, 1)):
        assert lib.stf_lesion_scratch_bytes(*bad) == 0


def test_python_argument_refusals():
    from stfunet import predict as P
    m = torch.zeros(4, 8, 8, dtype=torch.uint8)
    t = torch.zeros(4, 8, 8, dtype=torch.int64)
    ident = torch.nn.Identity()
    for bad in (-0.01, 1.01, float("nan"), float("inf"), "0.5", None, True, [0.5]):
        with pytest.raises(ValueError, match="min_overlap"):
            P.lesion_metrics(m, t, min_overlap=bad)
        with pytest.raises(ValueError, match="min_overlap"):
            P.lesion_metrics_3d(m, t, min_overlap=bad)
        with pytest.raises(ValueError, match="min_overlap"):
            P.predict_tta(ident, [], "cpu", tta=None, lesions=True, lesion_overlap=bad)
        with pytest.raises(ValueError, match="min_overlap"):
            P.predict_volumes(ident, [], "cpu", [], lesions=True, lesion_overlap=bad)
        with pytest.raises(ValueError, match="min_overlap"):
            P.predict_tta(ident, [], "cpu", lesions=True, lesion_overlap=bad)
    for bad in (-1, 1.0, "3", None, True, (1 << 20) + 1):
        for f in (P.lesion_metrics, P.lesion_metrics_3d):
            with pytest.raises(ValueError, match="max_lesions"):
                f(m, t, max_lesions=bad)
    for bad in (0, 6, 26, "8", None, True):
        with pytest.raises(ValueError, match="connectivity"):
            P.lesion_metrics(m, t, connectivity=bad)
    for bad in (0, 4, 8, "26", None, True):
        with pytest.raises(ValueError, match="connectivity"):
            P.lesion_metrics_3d(m, t, connectivity=bad)
    for bad in ([3], [2, 3], [0, 4], [4.0], 4, "4", True):
        with pytest.raises(ValueError, match="depths"):
            P.lesion_metrics_3d(m, t, depths=bad)
    for f in (P.lesion_metrics, P.lesion_metrics_3d):
        with pytest.raises(ValueError, match="does not match"):
            f(m, t[:3])
        with pytest.raises(ValueError, match="integer tensor"):
            f(m, t.float())
        with pytest.raises(ValueError, match="bool or an integer"):
            f(m.float(), t)
        with pytest.raises(ValueError, match=r"\[B, H, W\]"):
            f(m[0], t[0])
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            f(m, t)                                               # every check passed: only the device is missing
    # lesion_overlap is not looked at while lesions is off: the loops run as they always did
    assert "lesion_counts" not in P.predict_tta(ident, [], "cpu", tta=None, lesion_overlap=7)
    assert "lesion_counts" not in P.predict_volumes(ident, [], "cpu", [], lesion_overlap=7)
    res = P.predict_tta(ident, [], "cpu", tta=None, lesions=True)
    assert res["lesion_counts"] is None and res["false_findings_per_image"] is None
    res = P.predict_volumes(ident, [], "cpu", [], lesions=True)
    assert res["lesion_sensitivity"] is None and res["false_findings_per_case"] is None
