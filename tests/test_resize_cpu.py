"""CPU checks of the full-resolution output option (no kernel launches): the ``output_size``
keyword of ``STFLSTMUNet``, its unchanged ``state_dict``, and the resize entry points' declarations."""
import json
import os
import re

import pytest
import torch

from conftest import GOLDEN, REPO

ENTRY_POINTS = ("stf_resize_bilinear_fwd", "stf_resize_bilinear_bwd")


def test_output_size_keyword():
    import inspect
    from stfunet import STFLSTMUNet
    par = inspect.signature(STFLSTMUNet.__init__).parameters["output_size"]
    assert par.kind is inspect.Parameter.KEYWORD_ONLY and par.default == "half"
    assert STFLSTMUNet(1, 2, time_steps=3).output_size == "half"
    assert STFLSTMUNet(1, 2, time_steps=3, output_size="input").output_size == "input"
    with pytest.raises(ValueError, match="output_size"):
        STFLSTMUNet(1, 2, time_steps=3, output_size="full")
    with pytest.raises(TypeError):
        STFLSTMUNet(1, 2, 3, False, 3, "input")            # keyword-only


@pytest.mark.parametrize("pk", [False, True], ids=["plain", "pk"])
def test_state_dict_unchanged_by_output_size(pk):
    from stfunet import STFLSTMUNet
    keys = json.load(open(os.path.join(GOLDEN, "state_dict_keys.json")))["stf_t8_pk" if pk else "stf_t8"]
    m = STFLSTMUNet(1, 2, time_steps=3, use_pk_maps=pk, output_size="input")
    sd = m.state_dict()
    assert list(sd.keys()) == [k for k, _ in keys]
    for k, shp in keys:
        assert list(sd[k].shape) == list(shp), k
    half = STFLSTMUNet(1, 2, time_steps=3, use_pk_maps=pk)
    assert list(half.state_dict().keys()) == list(sd.keys())
    assert len(list(m.buffers())) == len(list(half.buffers()))


def test_entry_points_declared():
    import ctypes
    from stfunet import _lib
    header = open(os.path.join(REPO, "include", "stfunet.h")).read()
    for name in ENTRY_POINTS:
        assert name in _lib.EXPORTED
        res, args = _lib._SIGS[name]
        assert res is ctypes.c_int and len(args) == 8
        assert re.search(r"\bint\s+" + name + r"\s*\(const float\*", header), name
        for dt in (torch.bfloat16, torch.float16):         # built into both libraries
            assert hasattr(_lib.load(dt), name)


def test_upsample_logits_refuses_host_tensors():
    import stfunet
    assert "upsample_logits" in stfunet.__all__
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        stfunet.upsample_logits(torch.zeros(1, 2, 4, 4), (8, 8))
