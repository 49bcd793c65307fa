"""Capture of the eager launch sequence of one training step, shared by
tests/test_launch_trace_gpu.py and tests/golden/make_golden_launch_trace.py.

A trace is the ordered list of C-ABI entry points the step reaches through ``stfunet._lib.call``.
``stf_igemm`` and ``stf_wgrad`` entries also carry their ``ConvGeom`` fields and the output-channel
count; pointers and everything derived from the device (grids, tile counts, split counts,
workspace sizes) are left out.  ``stf_wgrad_plan`` is a host-side size query that the process
asks once per geometry, not a launch: it is left out too, so a trace does not depend on what ran
earlier in the process.
"""
import contextlib
import os

import torch

GEOM = ("N", "Hs", "Ws", "Cs", "src_cstride", "Hd", "Wd", "R", "S", "stride", "pad", "transposed")
CASES = ("unet", "stf", "stf_pk")


@contextlib.contextmanager
def tracing(dtype=torch.bfloat16):
    """Pre-fill the entry-point table ``call`` looks names up in with recording wrappers around
    the loaded library's functions; the table is put back as it was on exit."""
    from stfunet import _lib
    lib = _lib.load(dtype)
    table = _lib._FNS.setdefault(dtype, {})
    before = dict(table)
    trace = []

    def wrap(name, fn):
        if name in ("stf_igemm", "stf_wgrad"):
            def traced(args, stream):
                a = args._obj
                trace.append([name] + [getattr(a.g, f) for f in GEOM] + [a.Nout])
                return fn(args, stream)
        elif name == "stf_wgrad_plan":
            return fn
        else:
            def traced(*args):
                trace.append(name)
                return fn(*args)
        return traced
    table.update({name: wrap(name, getattr(lib, name)) for name in _lib.EXPORTED})
    try:
        yield trace
    finally:
        table.clear()
        table.update(before)


def _case(which):
    from stfunet import STFLSTMUNet, UNet
    from stfunet.synthetic import dce_batch
    torch.manual_seed(0)
    if which == "unet":
        model = UNet(in_channels=3, num_classes=2, base_c=8)
        x = dce_batch(2, 3, 32, 32, seed=11, device="cuda")[0].flatten(1, 2)
    else:
        pk = which == "stf_pk"
        model = STFLSTMUNet(in_channels=1, num_classes=2, time_steps=3, use_pk_maps=pk)
        x = dce_batch(1, 3, 32, 32, seed=11, device="cuda", pk_channels=3 if pk else 0)[0]
    return model.cuda().train(), x


def capture(which):
    """The trace of one eager training step (forward and backward) of case ``which``."""
    model, x = _case(which)
    prev = os.environ.get("STF_PLAN")
    os.environ["STF_PLAN"] = "0"
    try:
        with tracing() as trace:
            out = model(x)["out"]
            out.square().mean().backward()
            torch.cuda.synchronize()
    finally:
        if prev is None:
            del os.environ["STF_PLAN"]
        else:
            os.environ["STF_PLAN"] = prev
    return trace
