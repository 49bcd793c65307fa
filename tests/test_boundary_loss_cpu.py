"""Boundary loss without a GPU: the tests' restatement against brute force and a hand-computed case, the
closed-form gradient against autograd, every ValueError of the Python surface, and the new entry points
in the header, the binding and both libraries."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

from _boundary_loss_ref import (abs_loss, blobs, boundary_loss_ref, closed_form_grad, padded, sdf_brute, sdf_ref)
from conftest import REPO

NEW = ("stf_sdf_scratch_bytes", "stf_sdf", "stf_bloss_scratch_floats", "stf_bloss_fwd", "stf_bloss_bwd")
EINVAL = 100001


@pytest.mark.parametrize("N,K,H,W", [(1, 2, 1, 1), (2, 2, 1, 9), (1, 2, 7, 1), (2, 3, 6, 11), (1, 4, 9, 8)])
@pytest.mark.parametrize("density", [0.02, 0.5, 0.97])
def test_sdf_ref_against_brute_force(N, K, H, W, density):
    t = blobs(N, K, H, W, density, seed=H * W + K).numpy()
    assert np.array_equal(sdf_ref(t, K).view(np.uint32), sdf_brute(t, K).view(np.uint32))
    p = padded(N, K, H, W, seed=H + W).numpy()
    assert np.array_equal(sdf_ref(p, K, 255).view(np.uint32), sdf_brute(p, K, 255).view(np.uint32))


def test_sdf_ref_values_by_hand():
    t = np.zeros((1, 5, 5), np.int64)
    t[0, 1:4, 1:4] = 1
    phi = sdf_ref(t, 2)[0, 0]
    assert phi[2, 2] == -1 and phi[1, 1] == 0 and phi[1, 2] == 0          # centre, innermost border
    assert phi[0, 2] == 1 and phi[0, 0] == np.float32(np.sqrt(2.0))       # outside: at least 1
    assert (phi[t[0] == 0] >= 1).all() and (phi[t[0] == 1] <= 0).all()


def test_empty_and_full_are_zero():
    t = np.zeros((2, 4, 6), np.int64)
    t[1] = 1
    assert not sdf_ref(t, 2).any()                       # class 1 empty in image 0, full in image 1
    t[1, 0, 0] = 255                                     # one ignored pixel: class 1 is no longer the whole image
    phi = sdf_ref(t, 2, 255)
    assert not phi[0].any() and phi[1, 0, 0, 0] == 1 and phi[1, 0, 0, 1] == 0 and phi[1, 0, 3, 5] == np.float32(
        1.0 - np.sqrt(34.0))
    # an ignored value that nothing declares is just another non-class value: the same map
    assert np.array_equal(sdf_ref(t, 2, 255), sdf_ref(t, 2, None))


@pytest.mark.parametrize("K", [2, 5])
@pytest.mark.parametrize("ignore", [-100, 255])
def test_closed_form_gradient_is_autograd(K, ignore):
    g = torch.Generator().manual_seed(K)
    logits = torch.randn(2, K, 6, 7, generator=g) * 3
    t = padded(2, K, 6, 7, seed=3) if ignore >= 0 else blobs(2, K, 6, 7, 0.5, seed=3)
    phi = sdf_ref(t.numpy(), K, ignore)
    _, auto = boundary_loss_ref(logits, t, phi, ignore)
    closed = closed_form_grad(logits, t, phi, ignore)
    assert (auto - closed).abs().max().item() < 1e-14
    if ignore >= 0:
        assert (closed.permute(0, 2, 3, 1)[t == ignore] == 0).all()


def test_loss_by_hand_1x3():
    # target 0 1 0: phi = (1, 0, 1); logits chosen so that p_1 = (1/4, 1/2, 3/4)
    t = torch.tensor([[[0, 1, 0]]])
    phi = sdf_ref(t.numpy(), 2)
    assert phi.reshape(-1).tolist() == [1.0, 0.0, 1.0]
    p1 = torch.tensor([0.25, 0.5, 0.75], dtype=torch.float64)
    logits = torch.stack([torch.zeros(3, dtype=torch.float64), torch.log(p1 / (1 - p1))]).reshape(1, 2, 1, 3)
    loss, _ = boundary_loss_ref(logits, t, phi)
    assert abs(loss - (0.25 + 0.75) / 3) < 1e-15
    assert abs(abs_loss(logits, t, phi) - 1.0 / 3) < 1e-15
    # the middle pixel ignored: M = 2
    t2 = torch.tensor([[[0, 255, 0]]])
    loss2, _ = boundary_loss_ref(logits, t2, np.ones((1, 1, 1, 3), np.float32), 255)
    assert abs(loss2 - (0.25 + 0.75) / 2) < 1e-15


@pytest.mark.parametrize("bad", [-0.5, float("nan"), float("inf"), "x", None])
def test_boundary_weight_must_be_finite_and_non_negative(bad):
    from stfunet import boundary_criterion, engine
    from stfunet.loss import ce_dice_boundary_loss
    x, t = torch.zeros(1, 2, 4, 4), torch.zeros(1, 4, 4, dtype=torch.long)
    with pytest.raises(ValueError, match="boundary_weight"):
        boundary_criterion({"out": x}, t, boundary_weight=bad)
    with pytest.raises(ValueError, match="boundary_weight"):
        ce_dice_boundary_loss(x, t, boundary_weight=bad)
    with pytest.raises(ValueError, match="boundary_weight"):       # the loop hands it on before any step runs
        engine.train_one_epoch(torch.nn.Identity(), None, [(x, t)], torch.device("cpu"), 0, 2, boundary_weight=bad)


def test_a_single_class_has_no_boundary_term():
    from stfunet import boundary_criterion, boundary_loss
    from stfunet.loss import ce_dice_boundary_loss
    x, t = torch.zeros(1, 1, 4, 4), torch.zeros(1, 4, 4, dtype=torch.long)
    with pytest.raises(ValueError, match="boundary_weight"):
        boundary_criterion({"out": x}, t, num_classes=1, boundary_weight=0.1)
    with pytest.raises(ValueError, match="boundary_weight"):
        ce_dice_boundary_loss(x, t, boundary_weight=0.1)
    with pytest.raises(ValueError, match="foreground"):
        boundary_loss(x, t)
    # weight 0 with one class is the criterion as it was: it reaches the device guard
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        boundary_criterion({"out": x}, t, num_classes=1, boundary_weight=0.0)


def test_other_value_errors():
    from stfunet import boundary_loss, signed_distance_maps
    from stfunet.loss import ce_dice_boundary_loss
    x, t = torch.zeros(1, 3, 4, 4), torch.zeros(1, 4, 4, dtype=torch.long)
    for K in (1, 17):
        with pytest.raises(ValueError, match="num_classes"):
            signed_distance_maps(t, K)
    with pytest.raises(ValueError, match=r"\[N, H, W\]"):
        signed_distance_maps(t[0], 2)
    with pytest.raises(ValueError, match="integer"):
        signed_distance_maps(t.float(), 2)
    with pytest.raises(ValueError, match="4096"):
        signed_distance_maps(torch.zeros(1, 1, 4097, dtype=torch.long), 2)
    with pytest.raises(ValueError, match="2\\^31"):
        signed_distance_maps(torch.zeros(1, 1, 1, dtype=torch.int8).expand(9, 4096, 4096), 16)
    with pytest.raises(ValueError, match="class id"):
        boundary_loss(x, t, ignore_index=1)
    for bad in (torch.zeros(1, 3, 4, 4), torch.zeros(1, 2, 4, 5), torch.zeros(1, 2, 4, 4, dtype=torch.float64), 3.0):
        with pytest.raises(ValueError, match="dist"):
            boundary_loss(x, t, dist=bad)
        with pytest.raises(ValueError, match="dist"):
            ce_dice_boundary_loss(x, t, boundary_weight=0.1, dist=bad)


def test_valid_values_reach_the_device_guard():
    from stfunet import boundary_criterion, boundary_loss, signed_distance_maps
    x, t = torch.zeros(1, 2, 4, 4), torch.zeros(1, 4, 4, dtype=torch.long)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        boundary_criterion({"out": x}, t, boundary_weight=0.01)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        boundary_loss(x, t, dist=torch.zeros(1, 1, 4, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        signed_distance_maps(t, 2, ignore_index=255)


def test_signatures_and_exports():
    import stfunet
    from stfunet import engine
    from stfunet.loss import ce_dice_boundary_loss, ce_dice_loss
    assert {"boundary_criterion", "boundary_loss", "signed_distance_maps"} <= set(stfunet.__all__)
    # criterion's parameters, then the weight; criterion and ce_dice_loss keep theirs
    ps = inspect.signature(stfunet.boundary_criterion).parameters
    assert list(ps) == list(inspect.signature(stfunet.criterion).parameters) + ["boundary_weight"]
    assert ps["boundary_weight"].default == 0.0 and "boundary_weight" not in inspect.signature(ce_dice_loss).parameters
    ps = inspect.signature(ce_dice_boundary_loss).parameters
    assert list(ps) == list(inspect.signature(ce_dice_loss).parameters) + ["boundary_weight", "dist"]
    assert ps["boundary_weight"].default == 0.0
    assert ps["dist"].default is None
    par = inspect.signature(engine.train_one_epoch).parameters["boundary_weight"]
    assert par.kind is inspect.Parameter.KEYWORD_ONLY and par.default == 0.0
    assert list(inspect.signature(stfunet.signed_distance_maps).parameters) == ["target", "num_classes",
                                                                                  "ignore_index"]
    assert list(inspect.signature(stfunet.boundary_loss).parameters) == ["logits", "target", "ignore_index", "dist"]


def test_entry_points_in_header_binding_and_libraries():
    import ctypes
    from stfunet import _lib
    header = open(os.path.join(REPO, "include", "stfunet.h")).read()
    for s in NEW:
        assert re.search(r"\b%s\s*\(" % s, header), s
        assert s in _lib.EXPORTED
    i, P, f = ctypes.c_int, ctypes.c_void_p, ctypes.c_float
    assert _lib._SIGS["stf_sdf_scratch_bytes"] == (ctypes.c_size_t, [i, i, i, i])
    assert _lib._SIGS["stf_sdf"] == (i, [P, i, i, i, i, ctypes.c_int64, P, P, P])
    assert _lib._SIGS["stf_bloss_fwd"] == (i, [P, P, P, i, i, i, i, i, f, P, P, P])
    assert _lib._SIGS["stf_bloss_bwd"] == (i, [P, P, P, i, i, i, i, i, f, P, P, P, P])
    for dtype in (torch.bfloat16, torch.float16):
        lib = _lib.load(dtype)
        assert all(hasattr(lib, s) for s in NEW)
        assert lib.stf_abi_version() == 17


def test_library_rejects_bad_arguments_without_launch():
    import ctypes
    from stfunet import _lib
    lib = _lib.load()
    fake = ctypes.c_void_p(1 << 20)          # fake non-null pointers: nothing runs
    assert lib.stf_sdf_scratch_bytes(1, 4097, 4, 2) == 0 and lib.stf_sdf_scratch_bytes(1, 4, 4, 1) == 0
    assert lib.stf_sdf_scratch_bytes(1, 4, 4, 17) == 0 and lib.stf_sdf_scratch_bytes(9, 4096, 4096, 16) == 0
    n = 2 * 3 * 5 * 7                                      # counts (256-B rounded), stack, two g planes
    assert lib.stf_sdf_scratch_bytes(2, 5, 7, 4) == 256 + n * 8 + n * 4
    assert lib.stf_sdf(fake, 1, 4, 4, 1, -1, fake, fake, None) == EINVAL
    assert lib.stf_sdf(fake, 1, 4, 4097, 2, -1, fake, fake, None) == EINVAL
    assert lib.stf_sdf(None, 1, 4, 4, 2, -1, fake, fake, None) == EINVAL
    assert lib.stf_sdf(fake, 1, 4, 4, 2, -1, fake, ctypes.c_void_p((1 << 20) + 4), None) == EINVAL
    assert lib.stf_bloss_scratch_floats(3) == 2 + 3 * 64 * 2 and lib.stf_bloss_scratch_floats(0) == 0
    fwd = lambda K, ign, a: lib.stf_bloss_fwd(fake, fake, fake, 1, 4, 4, K, ign, a, fake, fake, None)  # noqa
    bwd = lambda K, ign, a: lib.stf_bloss_bwd(fake, fake, fake, 1, 4, 4, K, ign, a, fake, fake, fake, None)  # noqa
    for fn in (fwd, bwd):
        assert fn(1, -100, 1.0) == EINVAL        # no foreground class
        assert fn(17, -100, 1.0) == EINVAL
        assert fn(2, 1, 1.0) == EINVAL           # ignore is a class id
        assert fn(2, 255, -1.0) == EINVAL
        assert fn(2, 255, float("nan")) == EINVAL
    assert lib.stf_bloss_fwd(fake, fake, None, 1, 4, 4, 2, 255, 1.0, fake, fake, None) == EINVAL
    assert lib.stf_bloss_bwd(fake, fake, fake, 1, 4, 4, 2, 255, 1.0, fake, None, fake, None) == EINVAL
