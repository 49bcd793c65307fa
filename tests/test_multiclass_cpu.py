"""Five to sixteen classes on the CPU: the many-class entry points' surface and argument checks
(no kernel launches), the class limit of ``criterion`` and of the model constructors, the tests'
float64 restatement against the reference-generated ``multiclass.npz``, the K = 6 state_dict
against the reference module's, and the oracle functions the GPU tests lean on at K > 2."""
import ctypes
import json
import os
import re

import pytest
import torch

from _criterion_ref import ref_loss_and_grad
from _multiclass import MC_ENTRIES
from conftest import GOLDEN, REPO

EINVAL = 100001
NEW = ["stf_head_mc_fwd", "stf_head_mc_bwd", "stf_loss_mc_scratch_floats", "stf_loss_mc_fwd", "stf_loss_mc_bwd"]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_new_symbols_declared_and_exported(dtype):
    from stfunet import _lib
    header = open(os.path.join(REPO, "include", "stfunet.h")).read()
    lib = _lib.load(dtype)
    for s in NEW:
        assert re.search(r"\b%s\s*\(" % s, header), s
        assert s in _lib.EXPORTED and hasattr(lib, s), s
    assert lib.stf_abi_version() == 17


def test_fixture_covers_the_option_grid():
    got = {(e["logits"].shape[1], e["weight"] is not None, e["dice"], e["ignore_index"]) for e in MC_ENTRIES}
    want = {(k, w, d, i) for k in (5, 7, 16) for w in (False, True) for d in (False, True) for i in (-100, 255)}
    assert got == want and len(MC_ENTRIES) == 24
    for e in MC_ENTRIES:
        K = e["logits"].shape[1]
        assert e["logits"].shape == (3, K, 7, 9)
        if e["weight"] is not None:
            assert e["weight"].shape == (K,)
        t = e["target"]
        if e["ignore_index"] == 255:
            assert (t[0, :, 6:] == 255).all() and (t[0, :, :6] != 255).all()
            assert (t[1, 5:] == 255).all() and (t[1, :5] != 255).all() and (t[2] == 255).all()
        else:
            assert t.min() >= 0 and t.max() < K


@pytest.mark.parametrize("e", MC_ENTRIES, ids=[e["name"] for e in MC_ENTRIES])
def test_restatement_equals_reference(e):
    loss, grad = ref_loss_and_grad(e["logits"], e["target"], e["weight"], e["ignore_index"], e["dice"])
    print(e["name"], "loss", loss, "ref", e["loss"], "max |dgrad|", (grad - e["grad"].double()).abs().max().item())
    assert abs(loss - e["loss"]) < 1e-6 * max(1.0, abs(e["loss"]))       # the fixture's loss is an fp32 value
    assert (grad - e["grad"].double()).abs().max().item() < 1e-6
    if e["ignore_index"] >= 0:
        assert (e["grad"].permute(0, 2, 3, 1)[e["target"] == e["ignore_index"]] == 0).all()


def test_library_rejects_bad_many_class_arguments_without_launch():
    from stfunet import _lib
    for dtype in (torch.bfloat16, torch.float16):
        lib = _lib.load(dtype)
        fake = ctypes.c_void_p(1 << 20)          # fake non-null pointers: nothing runs
        lfwd = lambda K, ign, w=None, lg=fake: lib.stf_loss_mc_fwd(lg, fake, 1, 4, 4, K, w, ign, 1, fake, fake,  # noqa
                                                                   None)
        lbwd = lambda K, ign, w=None, lg=fake: lib.stf_loss_mc_bwd(lg, fake, 1, 4, 4, K, w, ign, 1, fake, fake,  # noqa
                                                                   fake, None)
        for f in (lfwd, lbwd):
            assert f(0, 255) == EINVAL           # classes outside 1..16
            assert f(17, 255, fake) == EINVAL
            assert f(-3, -100) == EINVAL
            assert f(6, 5) == EINVAL             # ignore_index is a class id
            assert f(6, 0, fake) == EINVAL
            assert f(16, 15) == EINVAL
            assert f(6, 255, None, None) == EINVAL     # a NULL required pointer
        hfwd = lambda C, K, y=fake: lib.stf_head_mc_fwd(y, 1, 4, 4, C, fake, fake, fake, fake, K, fake, None)  # noqa
        hbwd = lambda C, K, y=fake: lib.stf_head_mc_bwd(fake, y, 1, 4, 4, C, fake, fake, fake, fake, fake, K,  # noqa
                                                        fake, fake, fake, fake, fake, None)
        for f in (hfwd, hbwd):
            assert f(64, 0) == EINVAL and f(64, 17) == EINVAL
            for C in (12, 20, 24, 1024, 0):      # not 8 * a power of two up to 512: head_ok refuses
                assert f(C, 6) == EINVAL, C
            assert f(64, 6, None) == EINVAL
        # the 32-bit unit index: 2^31 units (and the grid strides past the end) are refused up front
        assert lib.stf_head_mc_fwd(fake, 1 << 13, 512, 512, 64, fake, fake, fake, fake, 6, fake, None) == EINVAL
        assert lib.stf_head_mc_bwd(fake, fake, 1 << 13, 512, 512, 64, fake, fake, fake, fake, fake, 6, fake, fake,
                                   fake, fake, fake, None) == EINVAL
        assert lib.stf_loss_mc_fwd(fake, fake, 65536, 4, 4, 6, None, -100, 1, fake, fake, None) == EINVAL


def test_scratch_floats_formula():
    from stfunet import _lib
    lib = _lib.load()
    for N, K in ((1, 1), (3, 5), (65, 16), (2, 9)):
        assert lib.stf_loss_mc_scratch_floats(N, K) == N * K * 3 + 2 + N * 64 * (3 * K + 2)
        if K <= 4:
            assert lib.stf_loss_mc_scratch_floats(N, K) == lib.stf_loss_opt_scratch_floats(N, K)
    assert lib.stf_loss_mc_scratch_floats(3, 0) == 0 and lib.stf_loss_mc_scratch_floats(3, 17) == 0


def test_seventeen_classes_are_refused_up_front():
    from stfunet import STFLSTMUNet, UNet, criterion
    from stfunet.loss import ce_dice_loss
    x, t = torch.zeros(1, 17, 4, 4), torch.zeros(1, 4, 4, dtype=torch.long)
    with pytest.raises(ValueError, match="16"):
        criterion({"out": x}, t, num_classes=17)
    with pytest.raises(ValueError, match="16"):
        ce_dice_loss(x, t)
    with pytest.raises(ValueError, match="16"):
        UNet(8, 17, 8)
    with pytest.raises(ValueError, match="16"):
        STFLSTMUNet(num_classes=17, time_steps=2)
    # sixteen build; a CPU tensor reaches the device guard (no eager fallback)
    assert UNet(8, 16, 8).out_conv.out_channels == 16
    assert STFLSTMUNet(num_classes=16, time_steps=2).final.out_channels == 16
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        criterion({"out": x[:, :16]}, t, num_classes=16, loss_weight=[1.0] * 16, ignore_index=255)


def test_k6_state_dict_matches_reference_module():
    from stfunet import UNet
    with open(os.path.join(GOLDEN, "multiclass_keys.json")) as f:
        ref = json.load(f)
    m = UNet(8, 6, 8)
    got = [[k, list(v.shape)] for k, v in m.state_dict().items()]
    assert got == ref["unet_in8_k6_c8"] and len(got) == 136
    assert sum(p.numel() for p in m.parameters()) == ref["param_count"]
    assert ["out_conv.weight", [6, 8, 1, 1]] in got and ["out_conv.bias", [6]] in got


def test_oracle_takes_many_classes_unchanged():
    """The GPU tests compare K = 6 / K = 5 models with oracle.unet / oracle.stf / oracle.loss: those
    take the class count from the state dict / ``num_classes`` without change, and oracle.loss agrees
    with the restatement (which the fixture pins to the reference) at K = 6."""
    from oracle import loss as o_loss, stf as o_stf, unet as o_unet, unet_bf16 as o_unet16
    from oracle.init import canonical_state_dict
    from stfunet import STFLSTMUNet, UNet
    g = torch.Generator().manual_seed(5)
    sd = canonical_state_dict(UNet(8, 6, 8).state_dict(), seed=0)
    x = torch.randn(1, 8, 32, 32, generator=g)
    t = torch.randint(0, 6, (1, 32, 32), generator=g)
    with torch.no_grad():
        out = o_unet.forward({k: v.clone() for k, v in sd.items()}, x, training=True)["out"]
        emu = o_unet16.forward({k: v.clone() for k, v in sd.items()}, x, training=True)["out"]
    assert out.shape == (1, 6, 32, 32) and emu.shape == out.shape
    ref, _ = ref_loss_and_grad(out, t)
    assert abs(o_loss.criterion(out, t, num_classes=6).item() - ref) < 1e-5
    sd5 = canonical_state_dict(STFLSTMUNet(num_classes=5, time_steps=2).state_dict(), seed=0)
    with torch.no_grad():
        out5 = o_stf.forward(sd5, torch.randn(1, 2, 1, 32, 32, generator=g), False)["out"]
    assert out5.shape == (1, 5, 16, 16)
