"""Volume-level connected-component post-processing without a GPU: the numpy restatement
(tests/_components3d_ref.py) against the scipy-generated fixture tests/golden/components3d.npz and
against the 2-D restatement on depth-1 volumes, ``volume_order`` on a temporary tree, and the argument
checks of the Python surface and of the C entry points (which refuse before they launch, so fake
pointers are enough)."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import _components_ref as ref2d
from _components3d_ref import (CONNECTIVITIES, FLAT, GOLDEN, counts_of, depth_one_inputs, earlier_neighbours,
                               filter_volume, fixture_cases, label, stack_filter, stack_label)
from _dataset_util import make_tree

CASES = fixture_cases()
EINVAL = 100001


def _generator():
    spec = importlib.util.spec_from_file_location("make_golden_components3d",
                                                  os.path.join(GOLDEN, "make_golden_components3d.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_fixture_covers_the_planned_ground():
    by = {c["name"]: c for c in CASES}
    assert len(CASES) == 19 and os.path.getsize(os.path.join(GOLDEN, "components3d.npz")) < 64 * 1024
    assert [len(earlier_neighbours(c)) for c in CONNECTIVITIES] == [3, 9, 13]
    for shape in ((5, 17, 33), (7, 19, 70)):
        for d in ("050", "150", "300", "500"):
            assert by["rand_%dx%dx%d_d%s" % (shape + (d,))]["mask"].shape == shape
    assert [by["space_diagonal"][f"n{c}"] for c in CONNECTIVITIES] == [8, 8, 1]
    assert [by["face_diagonal"][f"n{c}"] for c in CONNECTIVITIES] == [8, 1, 1]
    assert [by["checkerboard"][f"n{c}"] for c in CONNECTIVITIES] == [792, 1, 1]
    for name in ("serpentine", "bridge", "full"):
        assert all(by[name][f"n{c}"] == 1 for c in CONNECTIVITIES)
    assert by["serpentine"]["mask"].sum() > 1000                   # one chain through every slice
    assert all(by[name][f"n{c}"] == 2 for name in ("tie", "shell_core") for c in CONNECTIVITIES)
    assert by["single_slice"]["mask"].shape[0] == 1
    assert not by["empty"]["mask"].any() and all(by["empty"][f"n{c}"] == 0 for c in CONNECTIVITIES)


def test_fixture_is_what_the_generator_makes():
    made = _generator().cases()
    assert [n for n, _ in made] == [c["name"] for c in CASES]
    for (_, m), c in zip(made, CASES):
        assert np.array_equal(m, c["mask"])


def test_fixture_labels_are_scipys():
    pytest.importorskip("scipy")
    gen = _generator()
    for c in CASES:
        for k in CONNECTIVITIES:
            labels, n = gen.scipy_label(c["mask"], k)
            assert n == c[f"n{k}"] and np.array_equal(labels, c[f"labels{k}"]), (c["name"], k)


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_restatement_reproduces_the_fixture(c):
    for k in CONNECTIVITIES:
        labels, n = label(c["mask"], k)
        assert labels.dtype == np.int32 and n == c[f"n{k}"]
        assert np.array_equal(labels, c[f"labels{k}"]), k


def test_depth_one_volumes_are_the_2d_labels():
    """Every slice its own volume: the 2-D restatement with 6 -> 4 and 18, 26 -> 8, labels and filter."""
    rng = np.random.default_rng(5)
    stack = (rng.random((6, 19, 70)) < np.array([0.2, 0.4, 0.5, 0.593, 0.8, 0.0])[:, None, None]).astype(np.uint8)
    target = (rng.random(stack.shape) < 0.4).astype(np.int64)
    target[:, :, 60:] = 255
    for k in CONNECTIVITIES:
        labels, num = stack_label(stack, [1] * 6, k)
        want, want_num = ref2d.batch_label(stack, FLAT[k])
        assert np.array_equal(labels, want) and np.array_equal(num, want_num)
        got = stack_filter(stack, [1] * 6, True, 3, k, target, 255)
        want = ref2d.batch_filter(stack, True, 3, FLAT[k], target, 255)
        assert all(np.array_equal(a, b) for a, b in zip(got, want))
    for c in ref2d.fixture_cases()[:4]:
        for k in CONNECTIVITIES:
            labels, n = label(c["mask"][None], k)
            assert n == c[f"n{FLAT[k]}"] and np.array_equal(labels[0], c[f"labels{FLAT[k]}"])


@pytest.mark.parametrize("name,m,t", depth_one_inputs(), ids=[i[0] for i in depth_one_inputs()])
def test_depth_one_volumes_are_images_for_the_restatements(name, m, t):
    """The premise of the GPU test of the same name, for the oracles alone and on its inputs: a stack of
    depth-1 volumes under 6 / 18 / 26 is the batch of its slices under 4 / 8 / 8, labels, num, filtered
    mask and counts."""
    ones = [1] * m.shape[0]
    for k in CONNECTIVITIES:
        labels, num = stack_label(m, ones, k)
        want, want_num = ref2d.batch_label(m, FLAT[k])
        assert np.array_equal(labels, want) and np.array_equal(num, want_num)
        got = stack_filter(m, ones, True, 3, k, t, 2)
        want = ref2d.batch_filter(m, True, 3, FLAT[k], t, 2)
        assert all(np.array_equal(a, b) for a, b in zip(got, want))


def test_volumes_never_touch():
    full = np.ones((6, 4, 5), np.uint8)
    for k in CONNECTIVITIES:
        labels, num = stack_label(full, (1, 3, 2), k)
        assert num.tolist() == [1, 1, 1] and (labels == 1).all()
        assert stack_label(full, None, k)[1].tolist() == [1]


def test_filter_rules():
    m = np.zeros((4, 6, 12), np.uint8)
    m[0, 0, 0:3] = 1                                              # 3 voxels
    m[1:3, 2:4, 4:6] = 2                                          # 8 voxels over two slices
    m[3, 5, 4:12] = 3                                             # 8 voxels in one slice: the later tie
    m[3, 0, 0] = 4                                                # 1 voxel
    assert filter_volume(m, min_size=3)[0].sum() == 3 + 16 + 24
    assert np.array_equal(filter_volume(m, min_size=4)[0], np.where((m == 2) | (m == 3), m, 0))
    out, n = filter_volume(m, keep_largest=True)
    assert n == 4 and np.array_equal(out, np.where(m == 2, m, 0))  # the tie goes to the earlier first voxel
    assert filter_volume(m, keep_largest=True, min_size=8)[0].sum() == 16
    assert filter_volume(m, keep_largest=True, min_size=9)[0].sum() == 0    # min_size applies first
    out, n = filter_volume(m)
    assert n == 4 and np.array_equal(out, m)
    t = np.where(m > 0, 1, 0).astype(np.int64)
    t[3] = 255
    out, num, counts = stack_filter(m, (2, 2), keep_largest=True, target=t, ignore=255)
    # volume 0: the 4 voxels of the block in slice 1; volume 1: its 8-voxel row wins, all ignored
    assert num.tolist() == [2, 3] and counts.tolist() == [[4, 4, 7], [0, 0, 4]]
    assert counts_of(m, t).tolist() == [int((m > 0).sum()), int((m > 0).sum()), int((t > 0).sum())]


# ---------------------------------------------------------------- volume_order
def _rename_slices(root, patient, names):
    """Rename slice files 0.png, 1.png, ... of one patient to ``names`` in every folder that has them."""
    base = os.path.join(root, "seg", "training")
    for kind in ("images", "labels"):
        pdir = os.path.join(base, kind, patient)
        for seq in os.listdir(pdir):
            present = [k for k in range(len(names)) if os.path.exists(os.path.join(pdir, seq, f"{k}.png"))]
            for k in present:                                      # two steps: a new name may be an old one
                os.rename(os.path.join(pdir, seq, f"{k}.png"), os.path.join(pdir, seq, f"old{k}"))
            for k in present:
                os.rename(os.path.join(pdir, seq, f"old{k}"), os.path.join(pdir, seq, names[k]))


def test_volume_order_groups_patients_and_sorts_slices_naturally(tmp_path):
    from stfunet.dataset import DriveDataset, volume_order
    root = str(tmp_path)
    make_tree(root, n_patients=2, slices=4, size=(8, 8), pk=False)
    _rename_slices(root, "P000", ["10.png", "2.png", "slice_3.png", "1.png"])
    _rename_slices(root, "P001", ["b12.png", "b9.png", "b100.png", "a.png"])    # its last label is missing
    ds = DriveDataset(root, "train")
    assert len(ds) == 7

    def names(indices):
        return [os.path.basename(ds.patient_data[i]["image_paths"][0]) for i in indices]

    # whatever order the directory scan gave, and with the two patients interleaved
    order = [5, 0, 3, 1, 6, 2, 4]
    ds.patient_data = [ds.patient_data[i] for i in order]
    first = ds.patient_data[0]["patient_id"]
    indices, depths, patients = volume_order(ds)
    assert sorted(indices) == list(range(7)) and sum(depths) == 7
    assert patients == [first, "P001" if first == "P000" else "P000"]
    want = {"P000": ["1.png", "2.png", "10.png", "slice_3.png"], "P001": ["b9.png", "b12.png", "b100.png"]}
    at = 0
    for p, d in zip(patients, depths):
        got = indices[at:at + d]
        assert all(ds.patient_data[i]["patient_id"] == p for i in got)
        assert names(got) == want[p]
        at += d
    assert depths == [len(want[p]) for p in patients]
    sub = torch.utils.data.Subset(ds, indices)
    assert len(sub) == 7 and sub[0][0].shape[-2:] == (8, 8)
    empty = DriveDataset(root, "train")
    empty.patient_data = []
    assert volume_order(empty) == ([], [], [])


# ---------------------------------------------------------------- the Python surface
def test_names_are_exported():
    import stfunet
    from stfunet import predict as P
    for name in ("connected_components_3d", "filter_components_3d", "predict_volumes"):
        assert name in stfunet.__all__ and getattr(stfunet, name) is getattr(P, name)
    assert stfunet.__all__ == sorted(stfunet.__all__)
    from stfunet import _lib
    for s in ("stf_ccl3d_scratch_bytes", "stf_ccl3d_label", "stf_ccl3d_filter"):
        assert s in _lib.EXPORTED
    header = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "stfunet.h")).read()
    assert set(re.findall(r"\b(stf_ccl3d_[a-z_]+)\s*\(", header)) == {s for s in _lib.EXPORTED if "ccl3d" in s}


def test_python_argument_checks():
    from stfunet import predict as P
    m = torch.zeros(4, 8, 8, dtype=torch.uint8)
    ident = torch.nn.Identity()
    for bad in (0, 4, 8, 7, "26", None, 26.5, True):
        with pytest.raises(ValueError, match="connectivity"):
            P.connected_components_3d(m, connectivity=bad)
        with pytest.raises(ValueError, match="connectivity"):
            P.filter_components_3d(m, connectivity=bad)
        with pytest.raises(ValueError, match="connectivity"):
            P.predict_volumes(ident, [], "cpu", [], connectivity=bad)
    for bad in (-1, 1.0, 2.5, "3", None, True, False, 1 << 63):
        with pytest.raises(ValueError, match="min_size"):
            P.filter_components_3d(m, min_size=bad)
        with pytest.raises(ValueError, match="min_size"):
            P.predict_volumes(ident, [], "cpu", [], min_size=bad)
    for bad in ([True, 3], [2.0, 2], [0, 4], [4, 0], [-1, 5], [3], [2, 3], [], 4, 4.0, "4", ["4"], [None], True):
        for f in (P.connected_components_3d, P.filter_components_3d):
            with pytest.raises(ValueError, match="depths"):
                f(m, depths=bad)
    for bad in ([True], [2.0], [0], [1, -1], 4, "4", None):
        with pytest.raises(ValueError, match="depths"):
            P.predict_volumes(ident, [], "cpu", bad)
    for f in (P.connected_components_3d, P.filter_components_3d):
        with pytest.raises(ValueError, match="integer"):
            f(m.float())
        with pytest.raises(ValueError, match=r"\[B, H, W\]"):
            f(m[0])
        with pytest.raises(ValueError, match="4096"):
            f(torch.zeros(1, 1, 4097, dtype=torch.uint8))
        with pytest.raises(ValueError, match="2\\^31"):           # an expanded view: no memory behind it
            f(torch.zeros(1, 1, 1, dtype=torch.uint8).expand(128, 4096, 4096))
        for ok in (None, [4], (1, 3), [np.int64(2), 2], np.array([1, 1, 2])):
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                f(m, depths=ok)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            f(m.bool(), connectivity=6)
    with pytest.raises(ValueError, match="does not match"):
        P.filter_components_3d(m, target=torch.zeros(4, 8, 9, dtype=torch.int64))
    with pytest.raises(ValueError, match="integer"):
        P.filter_components_3d(m, target=torch.zeros(4, 8, 8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.filter_components_3d(m, target=torch.zeros(4, 8, 8, dtype=torch.int64), min_size=np.int64(3))
    with pytest.raises(ValueError, match="rule"):
        P.predict_volumes(ident, [], "cpu", [], rule="softmax")
    with pytest.raises(ValueError, match="view"):
        P.predict_volumes(ident, [], "cpu", [], tta=("diag",))
    with pytest.raises(TypeError):                                # the options are keyword-only
        P.predict_volumes(ident, [], "cpu", [], True)
    # an empty loader: the slice total must still match, and the key appears with the options only
    with pytest.raises(ValueError, match="slices"):
        P.predict_volumes(ident, [], "cpu", [2, 3])
    base = {"num", "num_volumes", "dice", "iou", "mean_dice", "mean_iou"}
    res = P.predict_volumes(ident, [], "cpu", [])
    assert set(res) == base and res["num"] == 0 and res["num_volumes"] == 0 and res["dice"] is None
    res = P.predict_volumes(ident, [], "cpu", [], keep_largest=True, keep_masks=True)
    assert set(res) == base | {"num_components", "masks"} and res["num_components"] is None and res["masks"] == []


# ---------------------------------------------------------------- the C entry points
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_library_refuses_bad_arguments_without_launch(dtype):
    """STF_EINVAL with fake non-null device pointers: nothing is launched or dereferenced.  Only the
    host copy of the volume table is real, because the entry points read it."""
    from stfunet import _lib
    lib = _lib.load(dtype)
    fake, other = ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 21)

    def at(offset):
        return ctypes.c_void_p((1 << 21) + offset)

    def table(*values):
        return (ctypes.c_int32 * len(values))(*values)

    good = table(0, 1, 4)

    def lab(mask=fake, N=4, H=8, W=8, sdev=other, shost=good, V=2, conn=26, labels=other, num=other, scratch=other):
        return lib.stf_ccl3d_label(mask, N, H, W, sdev, shost, V, conn, labels, num, scratch, None)

    def fil(mask=fake, target=other, N=4, H=8, W=8, sdev=other, shost=good, V=2, conn=26, keep=1, min_size=0,
            out=other, counts=other, num=other, scratch=other):
        return lib.stf_ccl3d_filter(mask, target, N, H, W, sdev, shost, V, conn, keep, min_size, -1, out, counts, num,
                                    scratch, None)

    assert lab(mask=None) == EINVAL and lab(labels=None) == EINVAL and lab(num=None) == EINVAL
    assert lab(scratch=None) == EINVAL
    assert fil(mask=None) == EINVAL and fil(out=None) == EINVAL and fil(scratch=None) == EINVAL
    assert fil(target=None) == EINVAL                              # counts without target
    assert fil(out=fake) == EINVAL                                 # out == mask
    assert fil(min_size=-1) == EINVAL
    for f in (lab, fil):
        assert f(sdev=None) == EINVAL and f(shost=None) == EINVAL
        assert all(f(conn=c) == EINVAL for c in (0, 1, 3, 4, 8, 7, 27, -26))
        assert f(N=0) == EINVAL and f(H=0) == EINVAL and f(W=0) == EINVAL and f(N=-1) == EINVAL
        assert f(H=4097) == EINVAL and f(W=4097) == EINVAL
        assert f(N=128, H=4096, W=4096, shost=table(0, 1, 128)) == EINVAL      # N * H * W = 2^31
        assert f(N=1 << 30, H=2, W=1, shost=table(0, 1, 1 << 30)) == EINVAL
        assert f(V=0) == EINVAL and f(V=-1) == EINVAL
        assert f(V=5, shost=table(0, 1, 2, 3, 4, 4)) == EINVAL                 # more volumes than slices
        assert f(shost=table(1, 2, 4)) == EINVAL                               # does not start at 0
        assert f(shost=table(0, 1, 3)) == EINVAL and f(shost=table(0, 1, 5)) == EINVAL     # does not end at N
        assert f(shost=table(0, 0, 4)) == EINVAL and f(shost=table(0, 4, 4)) == EINVAL     # an empty volume
        assert f(V=3, shost=table(0, 3, 2, 4)) == EINVAL                       # descending
        assert f(shost=table(0, -1, 4)) == EINVAL
        assert f(scratch=at(4)) == EINVAL and f(num=at(2)) == EINVAL and f(sdev=at(2)) == EINVAL
    assert lab(labels=at(2)) == EINVAL
    assert fil(counts=at(4)) == EINVAL and fil(target=at(4)) == EINVAL


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_scratch_bytes_at_and_beyond_the_limits(dtype):
    from stfunet import _lib
    sb = _lib.load(dtype).stf_ccl3d_scratch_bytes
    assert sb(0, 8, 8, 1) == 0 and sb(1, 0, 8, 1) == 0 and sb(1, 8, 0, 1) == 0 and sb(1, 8, 4097, 1) == 0
    assert sb(1, 4097, 8, 1) == 0 and sb(128, 4096, 4096, 1) == 0 and sb(-1, 8, 8, 1) == 0
    assert sb(4, 8, 8, 0) == 0 and sb(4, 8, 8, -1) == 0 and sb(4, 8, 8, 5) == 0
    # the selected roots (int32 per volume), the root counts (int32 per slice) and the best keys
    # (8 bytes per slice), each 256-byte rounded, and two int32 planes
    assert sb(1, 1, 1, 1) == 3 * 256 + 8 and sb(3, 5, 7, 2) == 3 * 256 + 8 * 105
    assert sb(65, 8, 8, 65) == 512 + 512 + 768 + 8 * 65 * 64
    assert sb(128, 256, 256, 8) == 256 + 512 + 1024 + 8 * 128 * 256 * 256
    assert sb(1, 4096, 4096, 1) == 3 * 256 + 8 * 4096 * 4096
    assert sb(127, 4096, 4096, 127) == 512 + 512 + 1024 + 8 * 127 * 4096 * 4096      # beyond 32 bits: size_t
    assert all(sb(n, h, w, v) % 8 == 0 for n, h, w, v in ((3, 3, 3, 1), (7, 1, 1, 7), (5, 9, 11, 2)))
