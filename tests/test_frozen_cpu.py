"""Frozen-parameter training, the parts that need no GPU: the freeze map (stfunet/program.py) is a
pure function of the parameters' ``requires_grad`` flags and ``want_dx``, checked per block against
hand-written expectations, and ``FlatParams`` reports the first trainable flat offset."""
import pytest
import torch


def _freeze(model, names):
    for n in names:
        model.get_submodule(n).requires_grad_(False)


ENCODER = ("conv1", "bn1", "layer1", "layer2", "layer3", "layer4")
STF_LAYERS = [f"layer{k}.{b}" for k, n in ((1, 3), (2, 4), (3, 6), (4, 3)) for b in range(n)]
STF_DECODER = [f"decoder{n}.{b}" for n in (4, 3, 2) for b in ("up", "fusion", "res_conv")]
STF_TAIL = STF_DECODER + ["upconv1", "final_res", "final"]


def _stf(pk=False):
    from stfunet import STFLSTMUNet
    return STFLSTMUNet(time_steps=3, use_pk_maps=pk)


def _unet():
    from stfunet import UNet
    return UNet(in_channels=3, base_c=8)


def _as_dict(fm):
    return {n: (w, d) for n, w, d in fm.key}


def test_freeze_map_pure_function():
    """A diamond: c reads a and b.  need_din follows trainable predecessors, transitively, and the input
    counts as one only with want_dx; a block with nothing trainable above it needs no input gradient."""
    from stfunet.program import freeze_map
    blocks = (("a", ("x",)), ("b", ("a",)), ("c", ("a", "b")), ("d", ("c",)))
    fm = freeze_map(blocks, dict(a=False, b=True, c=False, d=True))
    assert _as_dict(fm) == dict(a=(False, False), b=(True, False), c=(False, True), d=(True, True))
    assert fm.runs("b") and fm.runs("c") and not fm.runs("a")
    fm_dx = freeze_map(blocks, dict(a=False, b=True, c=False, d=True), want_dx=True)
    assert _as_dict(fm_dx) == dict(a=(False, True), b=(True, True), c=(False, True), d=(True, True))
    assert fm == freeze_map(blocks, dict(a=0, b=1, c=0, d=1)) and hash(fm) != hash(fm_dx)
    with pytest.raises(AttributeError):
        fm.key = ()


def test_stf_all_trainable():
    m = _stf()
    fm = _as_dict(m.program.freeze_map())
    assert list(fm) == ["stem"] + STF_LAYERS[:3] + ["lstm1"] + STF_LAYERS[3:7] + ["lstm2"] + STF_LAYERS[7:13] + \
        ["lstm3"] + STF_LAYERS[13:] + ["lstm4"] + STF_TAIL
    assert fm.pop("stem") == (True, False)             # the input gradient only on request
    assert all(v == (True, True) for v in fm.values())
    assert _as_dict(m.program.freeze_map(want_dx=True))["stem"] == (True, True)


def test_stf_encoder_frozen():
    m = _stf()
    _freeze(m, ENCODER)
    fm = _as_dict(m.program.freeze_map())
    for n in ["stem"] + STF_LAYERS:
        assert fm[n] == (False, False), n
    for k in (1, 2, 3, 4):
        assert fm[f"lstm{k}"] == (True, False)         # trainable, nothing upstream: the no-dx backward
    for n in STF_TAIL:
        assert fm[n] == (True, True), n
    fm = _as_dict(m.program.freeze_map(want_dx=True))  # the input gradient goes through the frozen encoder
    for n in ["stem"] + STF_LAYERS:
        assert fm[n] == (False, True), n
    assert fm["lstm1"] == (True, True)


def test_stf_encoder_frozen_pk():
    m = _stf(pk=True)
    _freeze(m, ENCODER)
    fm = _as_dict(m.program.freeze_map())
    for k in (1, 2, 3, 4):
        assert fm[f"pk_fusion{k}"] == (True, False)    # its wgrad from de[k], no dpk dgrad
        assert fm[f"lstm{k}"] == (True, True)          # d x_t feeds pk_fusion's weight gradient
    assert fm["layer4.2"] == (False, False)
    fm = _as_dict(m.program.freeze_map(want_dx=True))  # the PK maps are part of the input
    assert fm["pk_fusion2"] == (True, True) and fm["layer1.0"] == (False, True)


def test_stf_head_only():
    m = _stf()
    m.requires_grad_(False)
    m.final.requires_grad_(True)
    fm = _as_dict(m.program.freeze_map())
    assert fm.pop("final") == (True, False)
    assert all(v == (False, False) for v in fm.values())


def test_stf_decoder_frozen():
    m = _stf()
    _freeze(m, ("decoder4", "decoder3", "decoder2", "upconv1", "final_res", "final"))
    fm = _as_dict(m.program.freeze_map())
    for n in STF_TAIL:
        assert fm[n] == (False, True), n
    assert fm["lstm3"] == (True, True) and fm["layer1.0"] == (True, True) and fm["stem"] == (True, False)


def test_stf_middle_block_and_partial_freeze():
    m = _stf()
    _freeze(m, ("layer2.1",))
    fm = _as_dict(m.program.freeze_map())
    assert fm.pop("layer2.1") == (False, True) and fm.pop("stem") == (True, False)
    assert all(v == (True, True) for v in fm.values())
    # a partly frozen block counts as trainable; a stem with only bn1 trainable too
    m = _stf()
    _freeze(m, ENCODER)
    m.layer3[2].bn2.bias.requires_grad_(True)
    m.bn1.weight.requires_grad_(True)
    fm = _as_dict(m.program.freeze_map())
    assert fm["stem"] == (True, False) and fm["layer1.0"] == (False, True) and fm["layer3.1"] == (False, True)
    assert fm["layer3.2"] == (True, True) and fm["layer3.3"] == (False, True) and fm["layer4.0"] == (False, True)
    assert fm["lstm1"] == (True, True)


def test_stf_lowest_trainable_block_ends_the_backward():
    m = _stf()
    _freeze(m, ENCODER)
    m.layer4.requires_grad_(True)
    fm = _as_dict(m.program.freeze_map())
    assert fm["layer4.0"] == (True, False) and fm["layer4.1"] == (True, True) and fm["layer3.5"] == (False, False)
    assert fm["lstm3"] == (True, False) and fm["lstm4"] == (True, True)


def test_unet_patterns():
    m = _unet()
    fm = _as_dict(m.program.freeze_map())
    assert list(fm) == ["enc1", "enc2", "enc3", "enc4", "bottleneck", "up4", "dec4", "up3", "dec3", "up2", "dec2",
                        "up1", "dec1", "out_conv"]
    assert fm.pop("enc1") == (True, False) and all(v == (True, True) for v in fm.values())
    _freeze(m, ("enc1", "enc2", "enc3", "enc4"))
    fm = _as_dict(m.program.freeze_map())
    for n in ("enc1", "enc2", "enc3", "enc4"):
        assert fm[n] == (False, False), n
    assert fm["bottleneck"] == (True, False) and fm["up4"] == (True, True) and fm["dec4"] == (True, True)
    assert _as_dict(m.program.freeze_map(want_dx=True))["enc1"] == (False, True)
    m = _unet()
    m.requires_grad_(False)
    m.out_conv.requires_grad_(True)
    fm = _as_dict(m.program.freeze_map())
    assert fm.pop("out_conv") == (True, False) and all(v == (False, False) for v in fm.values())
    m = _unet()
    _freeze(m, ("enc3",))
    fm = _as_dict(m.program.freeze_map())
    assert fm["enc3"] == (False, True) and fm["enc2"] == (True, True) and fm["enc4"] == (True, True)
    m = _unet()
    _freeze(m, ("up4", "dec4", "up3", "dec3", "up2", "dec2", "up1", "dec1", "out_conv"))
    fm = _as_dict(m.program.freeze_map())
    assert fm["dec1"] == (False, True) and fm["up4"] == (False, True) and fm["bottleneck"] == (True, True)


def test_freeze_map_follows_flags_and_is_cached():
    m = _stf()
    prog = m.program
    a = prog.freeze_map()
    assert prog.freeze_map() is a
    _freeze(m, ENCODER)
    b = prog.freeze_map()
    assert b != a and b.key != a.key
    m.requires_grad_(True)
    assert prog.freeze_map() is a


def test_first_trainable_offset():
    m = _stf()
    flat = m.program.flat
    assert flat.first_trainable_offset() == 0
    _freeze(m, ENCODER)
    lo = flat.first_trainable_offset()
    first = m.lstm1.weight_ih_l0
    assert lo == flat.offsets[flat.index[id(first)]] and 0 < lo < flat.numel
    assert lo == sum((p.numel() + 3) // 4 * 4 for n, p in m.named_parameters()
                     if n.startswith(("conv1.", "bn1.", "layer")))
    m.requires_grad_(False)
    assert flat.first_trainable_offset() == flat.numel
    assert flat.requires_grad_flags() == (False,) * len(flat.params)
    assert torch.is_tensor(first)
