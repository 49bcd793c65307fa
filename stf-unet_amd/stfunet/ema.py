"""Exponential moving average of a model's weights, kept on the device.

``WeightEMA(model)`` holds ONE fp32 shadow buffer ``[parameters | float buffers]`` next to the model.
``update()`` after every optimizer step is one ``stf_ema_update`` launch over a segment table
(parameters and BatchNorm running statistics together; the weight is a host scalar, nothing is
read back); ``swap()`` / ``with ema.averaged():`` exchange the average into the model's OWN storage
with one ``stf_ema_swap`` launch, so the average is evaluated by the same program, the same pack
cache and the same recorded launch plan (all keyed on addresses, which do not change), and exchanged
back.  The semantics are ``torch.optim.swa_utils.AveragedModel(model,
multi_avg_fn=get_ema_multi_avg_fn(decay), use_buffers=True).update_parameters(model)`` called once
after every ``optimizer.step()`` -- a step the GradScaler or a non-finite clip norm skipped included:
the parameters did not move and the average still relaxes toward them.

For a ``stfunet`` model the parameter region has exactly ``model.program.flat``'s layout (padding
included) and is ONE segment over the whole flat buffer: the padding is zero on both sides and stays
zero.  Every floating-point buffer is a segment of its own at a 4-aligned offset; integer buffers
(``num_batches_tracked``) are neither averaged nor stored, a state dict takes them from the model.
"""
import contextlib
import ctypes
from collections import namedtuple

import numpy as np
import torch

from ._lib import EmaSeg, call, stream


def _align4(n):
    return (n + 3) & ~3


def decay_at(n, decay, warmup=False):
    """The decay of the update after ``n`` earlier ones: ``decay``, or under ``warmup``
    ``min(decay, (1 + n) / (10 + n))`` (timm's ModelEmaV3 schedule)."""
    return min(decay, (1 + n) / (10 + n)) if warmup else decay


def ema_weight(n, decay, warmup=False):
    """``w`` of update ``n`` (0-based) as the kernel gets it: 1 for the first (a copy), else
    ``float32(1 - decay_n)``."""
    return 1.0 if n == 0 else float(np.float32(1.0 - decay_at(n, decay, warmup)))


EmaLayout = namedtuple("EmaLayout", "segs param_offsets buffer_offsets total")
EmaLayout.__doc__ = """``segs``: ``[(model address, shadow offset, length), ...]`` in elements, what the
entry points take; ``param_offsets`` / ``buffer_offsets``: where each parameter / buffer lives in the
shadow; ``total``: the shadow's size in elements (a multiple of 4)."""


def ema_segments(param_ptrs, param_numels, buffer_ptrs=(), buffer_numels=(), flat_offsets=None):
    """The shadow layout and segment table of a model, from addresses and sizes alone.

    ``flat_offsets=None``: every parameter is a segment of its own, at the next 4-aligned offset.
    ``flat_offsets`` (``FlatParams.offsets``): the parameters are slices of one flat buffer, parameter
    ``i`` at element ``flat_offsets[i]`` of it; the region keeps that layout and is ONE segment over the
    whole buffer, padding included.  Buffers follow, each a segment of its own at a 4-aligned offset."""
    segs, off = [], 0
    if flat_offsets is not None and len(param_ptrs):
        base = param_ptrs[0] - 4 * flat_offsets[0]
        if any(p != base + 4 * o for p, o in zip(param_ptrs, flat_offsets)):
            raise ValueError("the parameters are not slices of one flat buffer at flat_offsets")
        if any(o % 4 or o + n > o2 for o, n, o2 in zip(flat_offsets, param_numels, flat_offsets[1:])):
            raise ValueError("flat_offsets must be multiples of 4 and must not overlap")
        poffs = list(flat_offsets)
        off = _align4(flat_offsets[-1] + param_numels[-1])
        segs.append((base, 0, off))
    else:
        poffs = []
        for p, n in zip(param_ptrs, param_numels):
            poffs.append(off)
            segs.append((p, off, n))
            off += _align4(n)
    boffs = []
    for p, n in zip(buffer_ptrs, buffer_numels):
        boffs.append(off)
        segs.append((p, off, n))
        off += _align4(n)
    return EmaLayout(segs, poffs, boffs, off)


class _Table:
    """A segment table as the entry points take it: on the device and the same entries on the host."""

    def __init__(self, segs, device):
        self.count = len(segs)
        self.host = (EmaSeg * max(self.count, 1))(*[EmaSeg(p, o, n) for p, o, n in segs])
        self.hptr = ctypes.addressof(self.host)
        self.dev = torch.frombuffer(bytearray(bytes(self.host)), dtype=torch.uint8).to(device)
        self.dptr = self.dev.data_ptr()


class WeightEMA:
    def __init__(self, model, decay=0.999, warmup=False, buffers=True):
        decay = float(decay)
        if not 0.0 <= decay <= 1.0:
            raise ValueError(f"decay must be in [0, 1], not {decay}")
        self.model = model
        self.decay = decay
        self.warmup = bool(warmup)
        self.buffers = bool(buffers)
        self.num_updates = 0
        self._swapped = False
        self._params = list(model.parameters())
        self._bufs = [b for b in model.buffers() if b.is_floating_point()] if buffers else []
        tensors = self._params + self._bufs
        if not tensors:
            raise ValueError("the model has no floating-point state to average")
        if not all(t.is_cuda for t in tensors):
            raise RuntimeError("stfunet.WeightEMA runs on the gfx950 kernels only: move the model to a ROCm device "
                               "first (no CPU fallback)")
        prog = getattr(model, "program", None)
        self._flat = getattr(prog, "flat", None)
        if self._flat is not None and not self._flat.owns(self._params):
            self._flat = None
        self._key = None
        self._table = None
        self.shadow = None
        self._tab()

    # ------------------------------------------------------------------ table
    def _tab(self):
        """The segment table for the model's current addresses; rebuilt (and the shadow moved to the
        model's device) when they changed, e.g. after ``.to()`` re-laid the flat buffer."""
        if self._flat is not None:
            self._flat.ensure()
            key = [self._flat.data.data_ptr()]
        else:
            key = list(map(torch.Tensor.data_ptr, self._params))
        key += map(torch.Tensor.data_ptr, self._bufs)
        if key == self._key:
            return self._table
        bad = [t for t in ([] if self._flat is not None else self._params) + self._bufs
               if t.dtype != torch.float32 or not t.is_contiguous()]
        if bad:
            raise ValueError("stfunet.WeightEMA averages contiguous fp32 parameters and buffers only (found "
                             f"{bad[0].dtype}, contiguous={bad[0].is_contiguous()})")
        pptrs = list(map(torch.Tensor.data_ptr, self._params))
        lay = ema_segments(pptrs, [p.numel() for p in self._params], [b.data_ptr() for b in self._bufs],
                           [b.numel() for b in self._bufs],
                           self._flat.offsets if self._flat is not None else None)
        dev = (self._params + self._bufs)[0].device
        if self.shadow is None:
            self.shadow = torch.zeros(lay.total, dtype=torch.float32, device=dev)
        elif self.shadow.device != dev:
            self.shadow = self.shadow.to(dev)
        assert self.shadow.numel() == lay.total
        self.layout = lay
        self._slots = {id(t): (o, t.numel()) for t, o in zip(self._params, lay.param_offsets)}
        self._slots.update({id(t): (o, t.numel()) for t, o in zip(self._bufs, lay.buffer_offsets)})
        self._table = _Table(lay.segs, dev)
        self._key = key
        return self._table

    # ------------------------------------------------------------------ update / swap
    def update(self):
        """One step of the average, after ``optimizer.step()``: the first call copies the model, every
        later one is ``shadow += w (model - shadow)`` with ``w = float32(1 - decay_n)``.  One launch, no
        host synchronisation."""
        if self._swapped:
            raise RuntimeError("WeightEMA.update() while the average is swapped into the model (inside averaged())")
        t = self._tab()
        w = ema_weight(self.num_updates, self.decay, self.warmup)
        call("stf_ema_update", self.shadow.data_ptr(), t.dptr, t.hptr, t.count, w, stream())
        self.num_updates += 1

    def swap(self):
        """Exchange model and shadow in place (one launch).  Addresses do not change: the launch plan,
        the pack cache, the optimizer's flat views and data-parallel buckets stay valid; the next
        forward repacks the 16-bit weights as every forward does."""
        t = self._tab()
        call("stf_ema_swap", self.shadow.data_ptr(), t.dptr, t.hptr, t.count, stream())
        self._swapped = not self._swapped

    @contextlib.contextmanager
    def averaged(self):
        """The model holds the average inside the block and its own weights again after it, also
        when the block raises."""
        self.swap()
        try:
            yield self.model
        finally:
            self.swap()

    # ------------------------------------------------------------------ state
    def _view(self, t):
        off, n = self._slots[id(t)]
        return self.shadow[off:off + n].view(t.shape)

    def _shadow_dict(self, clone):
        """The model's ``state_dict()`` keys in its order: averaged entries from the shadow, everything
        else (integer buffers; float buffers under ``buffers=False``) from the model."""
        if self._swapped:
            raise RuntimeError("WeightEMA state while the average is swapped into the model (inside averaged())")
        self._tab()
        out = {}
        for k, v in self.model.state_dict(keep_vars=True).items():
            src = self._view(v) if id(v) in self._slots else v.detach()
            out[k] = src.clone() if clone else src
        return out

    def state_dict(self):
        return {"decay": self.decay, "warmup": self.warmup, "num_updates": self.num_updates,
                "shadow": self._shadow_dict(clone=True)}

    def load_state_dict(self, sd):
        if self._swapped:
            raise RuntimeError("WeightEMA.load_state_dict() while the average is swapped into the model")
        self._tab()
        shadow = sd["shadow"]
        mine = self.model.state_dict(keep_vars=True)
        missing = [k for k, v in mine.items() if id(v) in self._slots and k not in shadow]
        if missing:
            raise KeyError(f"WeightEMA.load_state_dict: missing shadow entries {missing[:3]}...")
        for k, v in mine.items():
            if id(v) in self._slots:
                self._view(v).copy_(shadow[k])
        self.decay = float(sd["decay"])
        self.warmup = bool(sd["warmup"])
        self.num_updates = int(sd["num_updates"])

    @torch.no_grad()
    def copy_to(self, model):
        """Write the average into ``model`` (this one or another of the same architecture); the
        shadow stays as it is."""
        model.load_state_dict(self._shadow_dict(clone=False), strict=True)
