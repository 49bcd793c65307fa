"""CPU checks of the per-volume boundary metrics (stfunet.predict.boundary_metrics_3d, the volume
kernels of csrc/boundary.hip): the tests' numpy restatement (tests/_boundary3d_ref.py) against scipy
and against the committed fixture bit for bit, hand-computed answers, the Python argument checks
(every form of ``spacing``, every rejection), the result keys of ``predict_volumes(boundary=True)``
and the C side's refusals (no kernel launches)."""
import ctypes
import importlib.util
import math
import os
import re

import numpy as np
import pytest
import torch

from _boundary3d_ref import GOLDEN, border3, d2_all3, fixture_cases, fixture_spacings, metrics3, stack_metrics

CASES = fixture_cases()
EINVAL = 100001
SPACINGS = [(1.0, 1.0, 1.0), (2.5, 0.75, 0.75), (3.0, 0.5, 0.625), (2.2, 0.7, 0.7), (1.3, 0.9, 0.65)]


def _generator():
    spec = importlib.util.spec_from_file_location("make_golden_boundary3d",
                                                  os.path.join(GOLDEN, "make_golden_boundary3d.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _same(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == b


def test_fixture_covers_the_planned_ground():
    assert {c["P"].shape for c in CASES} == {(1, 40, 66), (2, 33, 65), (5, 20, 70), (12, 24, 40), (4, 37, 130)}
    assert len(CASES) == 12 and fixture_spacings() == [(1.0, 1.0, 1.0), (2.5, 0.75, 0.75)]
    assert sum(math.isnan(c["metrics"][0, 0]) for c in CASES) == 2
    for c in CASES:                                         # border voxels in the hundreds, brute force stays quick
        assert c["border_t"].sum() <= 400 and c["border_p"].sum() <= 400
    assert os.path.getsize(os.path.join(GOLDEN, "boundary3d.npz")) < 16384


def test_fixture_is_what_the_generator_makes():
    gen = _generator()
    made = gen.random_cases()
    assert [n for n, _, _ in made] == [c["name"] for c in CASES]
    assert [tuple(s) for s in gen.SPACINGS] == fixture_spacings()
    for (_, P, T), c in zip(made, CASES):
        assert np.array_equal(P, c["P"]) and np.array_equal(T, c["T"])


def test_restatement_equals_scipy_bit_for_bit():
    """Borders equal; HD, HD95 and ASSD the same float64 at five spacings, exact and generic."""
    pytest.importorskip("scipy")
    gen = _generator()
    for name, P, T in gen.random_cases():
        for sp in SPACINGS:
            bp, bt, hd, hd95, assd = gen.scipy_metrics(P, T, sp)
            assert np.array_equal(border3(P), bp) and np.array_equal(border3(T), bt), name
            rhd, rhd95, rassd, counts, _ = metrics3(P, T, sp)
            assert counts == (int(bp.sum()), int(bt.sum()))
            assert _same(rhd, hd) and _same(rhd95, hd95) and _same(rassd, assd), (name, sp)


def test_restatement_distance_transform_equals_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    for c in CASES[:8]:
        for sp in SPACINGS[1:4]:
            edt = ndi.distance_transform_edt(~c["border_t"], sampling=sp)
            assert np.array_equal(np.sqrt(d2_all3(c["border_t"], sp)), edt), (c["name"], sp)
    assert np.isinf(d2_all3(np.zeros((2, 3, 4)), (1, 1, 1))).all()


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_restatement_reproduces_the_fixture(c):
    assert np.array_equal(border3(c["P"]), c["border_p"]) and np.array_equal(border3(c["T"]), c["border_t"])
    for k, sp in enumerate(fixture_spacings()):
        hd, hd95, assd, _, _ = metrics3(c["P"], c["T"], sp)
        assert _same(hd, c["metrics"][k, 0]) and _same(hd95, c["metrics"][k, 1]) and _same(assd, c["metrics"][k, 2])


def test_hand_computed_answers():
    # one voxel against one voxel
    P, T = np.zeros((4, 6, 9), bool), np.zeros((4, 6, 9), bool)
    P[0, 1, 2] = T[2, 4, 6] = True
    hd, hd95, assd, counts, mx = metrics3(P, T, (2.5, 0.75, 0.75))
    assert counts == (1, 1) and mx == 25.0 + 2.25 * 0.25 * 9 + 9.0 and hd == hd95 == assd == math.sqrt(mx)
    # a volume one slice deep: every foreground voxel is a border voxel (the 2-D metric keeps the frame only)
    full = np.ones((1, 5, 5), bool)
    assert border3(full).sum() == 25
    # 3x5x5 full: the border is everything but the 3x3 core of the middle slice
    cube = np.ones((3, 5, 5), bool)
    assert border3(cube).sum() == 75 - 9 and not border3(cube)[1, 1:4, 1:4].any()
    # identical masks
    g = np.random.default_rng(3).random((3, 8, 11)) < 0.4
    assert metrics3(g, g, (3, 0.5, 0.625))[:3] == (0.0, 0.0, 0.0)
    # an empty mask on either side, or both
    e = np.zeros_like(g)
    for a, b in ((e, g), (g, e), (e, e)):
        hd, hd95, assd, counts, mx = metrics3(a, b)
        assert math.isnan(hd) and math.isnan(hd95) and math.isnan(assd) and mx is None
    # volumes in a stack never see each other; ignore: those voxels are background on both sides
    t = np.concatenate([g, g]).astype(np.int64)
    t[:, :, 8:] = 255
    out, counts, _ = stack_metrics(np.ones((6, 8, 11), np.uint8), t, [3, 3], [(1, 1, 1), (2, 1, 1)], ignore=255)
    keep = t[:3] != 255
    assert metrics3(keep, (t[:3] > 0) & keep)[:3] == tuple(out[0]) and counts[0, 0] == border3(keep).sum()
    assert metrics3(keep, (t[:3] > 0) & keep, (2, 1, 1))[:3] == tuple(out[1])


def test_names_are_exported():
    import stfunet
    from stfunet import _lib
    from stfunet import predict as P
    for name in ("boundary_metrics_3d", "distance_transform_3d"):
        assert name in stfunet.__all__ and getattr(stfunet, name) is getattr(P, name)
    assert stfunet.__all__ == sorted(stfunet.__all__)
    header = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "stfunet.h")).read()
    names = {"stf_boundary3d_scratch_bytes", "stf_boundary3d_metrics", "stf_edt3d_sq"}
    assert set(re.findall(r"\b(stf_(?:boundary3d|edt3d)_[a-z_]+)\s*\(", header)) == names <= set(_lib.EXPORTED)
    assert "Not here: boundary metrics" not in P.predict_volumes.__doc__


def test_spacing_forms():
    from stfunet.predict import _check_spacing_3d as f
    assert f(1.5, 2) == [[1.5] * 3] * 2 and f(2, 1) == [[2.0] * 3] and f(np.float32(0.5), 1) == [[0.5] * 3]
    assert f((3, 0.5, 0.625), 2) == [[3.0, 0.5, 0.625]] * 2 and f([3, 0.5, 0.625], 3) == [[3.0, 0.5, 0.625]] * 3
    assert f(np.array([1.0, 2.0, 3.0]), 2) == [[1.0, 2.0, 3.0]] * 2 and f(torch.tensor([1.0, 2.0, 3.0]), 1) == [[1.0, 2.0, 3.0]]
    rows = [[2.5, 0.75, 0.75], [1.0, 1.0, 1.0]]
    assert f(rows, 2) == rows and f(tuple(map(tuple, rows)), 2) == rows and f(np.array(rows), 2) == rows
    assert f(torch.tensor(rows, dtype=torch.float64), 2) == rows and f(torch.tensor(rows), 2) == rows
    three = [[1.0, 2.0, 3.0], [4.0, 5.0, 6.0], [7.0, 8.0, 9.0]]
    assert f(three, 3) == three and f(1.0, 0) == []
    for bad in (0.0, -1.0, float("nan"), float("inf"), "1", None, True, (1, 2), (1, 2, 3, 4), (1, 0, 1), (1, -2, 1),
                (1, float("nan"), 1), (1, float("inf"), 1), (1, "2", 1), (1, True, 1), [[1, 1, 1]], [[1, 1, 1]] * 3,
                [[1, 1], [1, 1]], [[1, 1, 1], [1, 0, 1]], [[1, 1, 1], "abc"], [[1, 1, 1], None], [[1, 1, 1], 5],
                torch.ones(2, 2), torch.ones(3, 3), torch.ones(2, 3, 1), torch.tensor(1.0), torch.zeros(2, 3),
                torch.ones(2, 3, dtype=torch.bool), np.ones((2, 2)), {"sz": 1}):
        with pytest.raises(ValueError, match="spacing"):
            f(bad, 2)


def test_python_argument_checks():
    """The checks that precede any launch: a bad spacing, depths or shape ValueError, host tensors RuntimeError."""
    from stfunet import predict as P
    m, t = torch.zeros(4, 5, 6, dtype=torch.uint8), torch.zeros(4, 5, 6, dtype=torch.int64)
    ident = torch.nn.Identity()
    for ok in (dict(), dict(depths=[1, 3]), dict(depths=[1, 3], spacing=[(1, 2, 3), (4, 5, 6)]), dict(spacing=(3, 1, 1)),
               dict(spacing=0.7, ignore_index=255), dict(depths=(4,), spacing=torch.ones(1, 3))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            P.boundary_metrics_3d(m, t, **ok)
        ok.pop("ignore_index", None)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            P.distance_transform_3d(m, **ok)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.boundary_metrics_3d(m.bool(), t.int())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.distance_transform_3d(m, where=m)
    for bad in (0.0, -1.0, float("nan"), "1", None, True, (1, 2), [[1, 1, 1]] * 3, (1, 0, 1)):
        with pytest.raises(ValueError, match="spacing"):
            P.boundary_metrics_3d(m, t, depths=[2, 2], spacing=bad)
        with pytest.raises(ValueError, match="spacing"):
            P.distance_transform_3d(m, depths=[2, 2], spacing=bad)
        with pytest.raises(ValueError, match="spacing"):
            P.predict_volumes(ident, [], "cpu", [2, 2], boundary=True, spacing=bad)
    for bad in ([True, 3], [2.0, 2], [0, 4], [3], [2, 3], [], 4, "4", [None]):
        with pytest.raises(ValueError, match="depths"):
            P.boundary_metrics_3d(m, t, depths=bad)
        with pytest.raises(ValueError, match="depths"):
            P.distance_transform_3d(m, depths=bad)
    with pytest.raises(ValueError, match="does not match"):
        P.boundary_metrics_3d(m, torch.zeros(4, 5, 7, dtype=torch.int64))
    with pytest.raises(ValueError, match="does not match"):
        P.distance_transform_3d(m, where=torch.zeros(4, 6, 5, dtype=torch.uint8))
    with pytest.raises(ValueError, match=r"\[B, H, W\]"):
        P.boundary_metrics_3d(m[0], t[0])
    with pytest.raises(ValueError, match="integer"):
        P.boundary_metrics_3d(m.float(), t)
    with pytest.raises(ValueError, match="integer"):
        P.boundary_metrics_3d(m, t.float())
    with pytest.raises(ValueError, match="integer"):
        P.distance_transform_3d(m.float())
    with pytest.raises(ValueError, match="4096"):
        P.boundary_metrics_3d(torch.zeros(1, 1, 4097, dtype=torch.uint8), torch.zeros(1, 1, 4097, dtype=torch.int64))
    with pytest.raises(ValueError, match="2\\^31"):          # an expanded view: no memory behind it
        P.distance_transform_3d(torch.zeros(1, 1, 1, dtype=torch.uint8).expand(128, 4096, 4096))
    # the full transform of a large stack is refused unless `where` takes the cost on (views: no memory)
    big = torch.zeros(1, 1, 1, dtype=torch.uint8).expand(64, 512, 512)
    assert 64 * 512 * 512 * (512 + 64) > P.MAX_FULL_SCAN
    with pytest.raises(ValueError, match="where"):
        P.distance_transform_3d(big)
    with pytest.raises(RuntimeError, match="no CPU fallback"):        # eight shallow volumes: below the bound
        P.distance_transform_3d(torch.zeros(1, 1, 1, dtype=torch.uint8).expand(64, 256, 256), depths=[8] * 8)


def test_predict_volumes_boundary_keys_and_none_rules():
    from stfunet import predict as P
    ident = torch.nn.Identity()
    base = {"num", "num_volumes", "dice", "iou", "mean_dice", "mean_iou"}
    extra = {"hd", "hd95", "assd", "mean_hd", "mean_hd95", "mean_assd", "num_boundary"}
    assert set(P.predict_volumes(ident, [], "cpu", [])) == base
    assert set(P.predict_volumes(ident, [], "cpu", [], boundary=False, spacing="not looked at")) == base
    res = P.predict_volumes(ident, [], "cpu", [], boundary=True, spacing=(2.5, 0.75, 0.75))
    assert set(res) == base | extra and all(res[k] is None for k in extra)
    res = P.predict_volumes(ident, [], "cpu", [], boundary=True, keep_largest=True, keep_masks=True)
    assert set(res) == base | extra | {"num_components", "masks"}
    with pytest.raises(ValueError, match="slices"):
        P.predict_volumes(ident, [], "cpu", [2, 3], boundary=True, spacing=[(1, 1, 1), (2, 1, 1)])
    with pytest.raises(TypeError):
        P.predict_volumes(ident, [], "cpu", [], boundry=True)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_library_refuses_bad_arguments_without_launch(dtype):
    """STF_EINVAL with fake non-null device pointers: nothing is launched or dereferenced.  Only the
    host copy of the volume table is real, because the entry points read it."""
    from stfunet import _lib
    lib = _lib.load(dtype)
    fake = ctypes.c_void_p(1 << 20)
    good = (ctypes.c_int32 * 3)(0, 3, 4)

    def bm(mask=fake, target=fake, N=4, H=8, W=8, sd=fake, sh=good, V=2, sp=fake, out=fake, counts=fake, scratch=fake):
        return lib.stf_boundary3d_metrics(mask, target, N, H, W, sd, sh, V, sp, -1, out, counts, scratch, None)

    def edt(sites=fake, N=4, H=8, W=8, sd=fake, sh=good, V=2, sp=fake, d2=fake, scratch=fake):
        return lib.stf_edt3d_sq(sites, None, N, H, W, sd, sh, V, sp, d2, scratch, None)

    for kw in ("mask", "target", "sd", "sh", "sp", "out", "counts", "scratch"):
        assert bm(**{kw: None}) == EINVAL, kw
    for kw in ("sites", "sd", "sh", "sp", "d2", "scratch"):
        assert edt(**{kw: None}) == EINVAL, kw
    at = lambda off: ctypes.c_void_p((1 << 20) + off)
    assert bm(out=at(4)) == EINVAL and bm(counts=at(4)) == EINVAL and bm(target=at(4)) == EINVAL
    assert bm(sp=at(4)) == EINVAL and bm(scratch=at(4)) == EINVAL and bm(sd=at(2)) == EINVAL
    assert edt(d2=at(4)) == EINVAL and edt(scratch=at(2)) == EINVAL and edt(sp=at(1)) == EINVAL
    for f in (bm, edt):
        for bad in ((1, 3, 4), (0, 4, 4), (0, 0, 4), (0, 3, 5), (0, 3, 3), (0, 4, 3)):
            assert f(sh=(ctypes.c_int32 * 3)(*bad)) == EINVAL, bad
        assert f(N=0) == EINVAL and f(H=0) == EINVAL and f(W=0) == EINVAL and f(V=0) == EINVAL and f(V=5) == EINVAL
        assert f(H=4097) == EINVAL and f(W=4097) == EINVAL and f(N=-1) == EINVAL
        assert f(N=128, H=4096, W=4096) == EINVAL                     # N * H * W = 2^31
    sb = lib.stf_boundary3d_scratch_bytes
    assert sb(0, 8, 8, 1) == 0 and sb(1, 0, 8, 1) == 0 and sb(1, 8, 4097, 1) == 0 and sb(128, 4096, 4096, 1) == 0
    assert sb(4, 8, 8, 0) == 0 and sb(4, 8, 8, 5) == 0
    # counts, unit partials and flags each 256-byte rounded; 16 + 8 + 4 bytes per voxel
    assert sb(4, 8, 8, 2) == 256 + 256 + 256 + 28 * 256
    assert sb(1, 1, 1, 1) == 256 + 256 + 256 + 32 and sb(1, 1, 3, 1) == 768 + 28 * 3 + 4
    n = 128 * 256 * 256
    assert sb(128, 256, 256, 8) == 256 + 128 * 32 * 2 * 16 + 1536 + 28 * n
    assert all(sb(1, 1, w, 1) % 8 == 0 and sb(1, 1, w, 1) >= 768 + 28 * w for w in range(1, 200))
