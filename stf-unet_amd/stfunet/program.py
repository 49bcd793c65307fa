"""What ``UNetProgram`` (unet.py) and ``STFProgram`` (stf_lstm_unet.py) share.

  * ``Program``: the base of both -- the model's packed weights, flat parameters, plan runtime,
    the data-parallel ``grad_ready_hook`` and the input-gradient handshake; ``forward`` /
    ``backward`` run the subclass's ``_forward`` / ``_backward`` schedule with the program's
    ``PackCache`` active.
  * ``StepFunction``: the one ``torch.autograd.Function`` both models go through, and
    ``run_step``, the tail of both ``nn.Module.forward``s.
  * ``conv_bn`` and ``conv_pair_backward``: the forward step and the backward core that the
    block programs (``DoubleConvProgram``, ``ResBlockProgram``) are built from.
  * ``Saved``: the attribute bag a forward keeps for its backward.
  * ``freeze_map`` / ``FreezeMap``: which blocks' parameter gradients and input gradients a
    step needs, from the parameters' ``requires_grad`` flags (frozen-parameter training).
"""
from collections import namedtuple

import torch

from . import _lib, nhwc
from .flat import FlatParams
from .nhwc import Feat, new_feat
from .plan import StepRuntime


class Saved:
    pass


# ------------------------------------------------------------------ freeze map
Need = namedtuple("Need", "need_w need_din")
Need.__doc__ = """What a step's backward needs of one block.  ``need_w``: at least one of the block's
parameters requires grad (a partly frozen block counts as trainable); ``need_din``: something
upstream of the block in the dataflow is trainable, or the input gradient is wanted."""


class FreezeMap:
    """Immutable ``block name -> Need`` of one step; ``key`` (hashable) joins the plan signatures."""
    __slots__ = ("_need", "key")

    def __init__(self, items):
        object.__setattr__(self, "key", tuple((n, bool(w), bool(d)) for n, w, d in items))
        object.__setattr__(self, "_need", {n: Need(w, d) for n, w, d in self.key})

    def __setattr__(self, *a):
        raise AttributeError("FreezeMap is immutable")

    def __getitem__(self, name):
        return self._need[name]

    def runs(self, name):
        """Does the block's backward run at all (it produces a gradient somebody reads)?"""
        n = self._need[name]
        return n.need_w or n.need_din

    def names(self):
        return [n for n, _, _ in self.key]

    def __eq__(self, other):
        return isinstance(other, FreezeMap) and self.key == other.key

    def __hash__(self):
        return hash(self.key)


def freeze_map(blocks, trainable, want_dx=False):
    """The freeze map of a dataflow graph: a pure function of the flags.

    ``blocks``: ``(name, predecessors)`` in forward (topological) order, a predecessor being an
    earlier block's name or ``"x"``, the model input; ``trainable``: ``name -> bool`` (any of the
    block's parameters requires grad).  ``need_din`` of a block: one of its predecessors is
    trainable or itself needs an input gradient; the input counts as trainable iff ``want_dx``."""
    wants = {"x": bool(want_dx)}
    items = []
    for name, preds in blocks:
        din = any(wants[p] for p in preds)
        w = bool(trainable[name])
        items.append((name, w, din))
        wants[name] = w or din
    return FreezeMap(items)


# ------------------------------------------------------------------ block steps
def conv_bn(src: Feat, conv, bn, R, stride, pad, training=None, groups=1):
    """conv (+bias, +BN partial sums in the epilogue) -> bn_finalize: returns the raw conv output
    and its BNState.  The apply pass (bn_act) is the caller's: what it writes differs per block.
    ``training=None`` (the model programs): the BatchNorm's mode is its own ``bn.training``, so a
    frozen encoder put in ``.eval()`` inside a training model normalises with, and leaves alone,
    its running statistics."""
    if training is None:
        training = bn.training
    C, dev = conv.out_channels, src.buf.device
    y = new_feat(src.N, (src.H - 1) // stride + 1, (src.W - 1) // stride + 1, C, dev)
    bias = conv.bias.detach() if conv.bias is not None else None
    stats, tiles = nhwc.igemm(src, nhwc.pack_weight(conv.weight, 0, src.C), C, y, R, R, stride, pad, bias=bias,
                              want_stats=training, groups=groups)
    return y, nhwc.bn_finalize(stats, tiles, bn, y.M, training, groups)


def conv_pair_backward(s, gv, dy2: Feat, conv1, bn1, conv2, stride=1, dbias1=None, need_w=True):
    """Backward core of relu(bn1(conv1 src)) -> conv2, from ``dy2`` (grad w.r.t. conv2's raw output;
    the caller ran bn2's backward) to dy1 (w.r.t. conv1's raw output), which it returns: conv2's
    weight gradient, its dgrad, bn1's backward, conv1's weight gradient.  The input gradient is
    the caller's (padding, shortcut and accumulation differ per block).  ``s``: the forward's
    ``src``, ``y1``, ``bn1``, ``a1``; ``dbias1``: conv1's bias gradient view, if it has a bias.
    ``need_w=False`` (a frozen block on the way to a trainable one): the two weight gradients
    are not launched; bn1's dgamma / dbeta fall out of the BN backward that runs anyway."""
    if need_w:
        nhwc.wgrad(dy2, s.a1, 3, 3, 1, 1, gv(conv2.weight))
    da1 = new_feat(s.a1.N, s.a1.H, s.a1.W, conv2.in_channels, s.a1.buf.device)
    # dgrad of conv2 also reduces BN1's backward sums (fused epilogue)
    part, tiles = nhwc.conv_dgrad(dy2, conv2.weight, da1, 3, 3, 1, 1, bnr=(s.y1, s.bn1, True))
    del dy2
    dy1 = nhwc.bn_backward_fused(da1, s.y1, s.bn1, bn1, part, tiles, gv(bn1.weight), gv(bn1.bias), dbias=dbias1)
    del da1
    cin = conv1.in_channels
    if not need_w:
        return dy1
    if s.src.C == cin:
        nhwc.wgrad(dy1, s.src, 3, 3, stride, 1, gv(conv1.weight))
    else:   # zero-padded input channels (in_channels % 8 != 0): drop the padded columns
        nhwc.wgrad_padded(dy1, s.src, 3, 3, stride, 1, gv(conv1.weight), cin)
    return dy1


# ------------------------------------------------------------------ program base
class Program:
    """Base of the two models' programs.  A subclass builds its block programs and writes the
    ``_forward(x, training, need_bwd) -> (logits, saved)`` and ``_backward(S, dlogits)``
    schedules; ``StepRuntime`` (plan.py) records and replays them through ``forward`` / ``backward``."""

    def __init__(self, model):
        self.m = model
        self.packs = nhwc.PackCache()
        self.flat = FlatParams(model)
        # grad_ready_hook(begin, deps): flat-gradient elements [begin, numel) are final once the
        # current stream's work and the streams ``deps`` have run.  Backward finishes blocks in
        # exactly the reverse of registration (= flat) order, so the finished gradients always
        # form a suffix of the flat buffer (DDP buckets).
        self.grad_ready_hook = None
        # set by StepFunction for the backward in flight: also leave d(loss)/d(input) in ``dx``
        self.want_dx = False
        self.dx = None
        # the step's freeze map (set by run_step / StepFunction before the forward; the forward
        # leaves it in its saved state for the backward): None = everything trainable
        self.fmap = None
        self._graph_idx = None
        self._fmaps = {}
        self.runtime = StepRuntime(self)

    def graph(self):
        """The model's blocks as the schedules visit them: ``(name, modules, predecessors)`` in
        forward order (``freeze_map``); written by the subclass."""
        raise NotImplementedError

    def freeze_map(self, want_dx=False, flags=None):
        """The freeze map for the parameters' current ``requires_grad`` flags (or ``flags``, in
        flat order): cached per (flags, want_dx), one tuple of flags and a lookup per step."""
        if flags is None:
            flags = self.flat.requires_grad_flags()
        key = (flags, bool(want_dx))
        fm = self._fmaps.get(key)
        if fm is None:
            if self._graph_idx is None:
                index = self.flat.index
                self._graph_idx = [(name, tuple(index[id(p)] for mod in mods for p in mod.parameters()), preds)
                                   for name, mods, preds in self.graph()]
            if len(self._fmaps) > 64:
                self._fmaps.clear()
            fm = self._fmaps[key] = freeze_map([(n, pr) for n, _, pr in self._graph_idx],
                                               {n: any(flags[i] for i in idx) for n, idx, _ in self._graph_idx},
                                               want_dx)
        return fm

    def step_map(self):
        """The freeze map the schedule in flight follows: ``fmap`` as ``run_step`` set it, or (a
        direct call of ``forward``) everything trainable and the input gradient wanted."""
        if self.fmap is not None:
            return self.fmap
        return self.freeze_map(True, (True,) * len(self.flat.params))

    def forward(self, x, training, need_bwd):
        """Refresh the packed weights (one launch) and run the forward schedule.  ``training`` is the
        model's flag (what the plan runtime gates on); every BatchNorm runs in its own mode."""
        self.packs.refresh()
        nhwc.ACTIVE_PACKS = self.packs
        try:
            return self._forward(x, training, need_bwd)
        finally:
            nhwc.ACTIVE_PACKS = None

    def backward(self, S, dlogits):
        nhwc.ACTIVE_PACKS = self.packs
        try:
            return self._backward(S, dlogits)
        finally:
            nhwc.ACTIVE_PACKS = None

    def _done(self, module, deps):
        """The gradients of ``module`` and of everything after it in flat order are final once the
        current stream's work and the streams ``deps`` have run: tell the hook."""
        if self.grad_ready_hook is not None:
            first = next(module.parameters())
            self.grad_ready_hook(self.flat.offsets[self.flat.index[id(first)]], deps)


# ------------------------------------------------------------------ autograd
class StepFunction(torch.autograd.Function):
    """``res``: (logits, saved state) of the plan-cached forward ``run_step`` already enqueued: the
    GPU starts on the step while autograd processes the parameter inputs of this call (~160 for
    the STF model, ~100 us of host time at every synced step boundary); or None (input
    gradients: the eager forward runs here)."""
    @staticmethod
    def forward(ctx, x, prog, storage, res, *params):
        ctx.need_dx = ctx.needs_input_grad[0]
        if res is not None:
            logits, saved = res
            prog.runtime.own(saved, ctx)
        else:
            flags = tuple(ctx.needs_input_grad[4:])
            need_bwd = True in flags or ctx.need_dx
            prog.fmap = prog.freeze_map(ctx.need_dx, flags) if need_bwd else None
            try:
                with _lib.storage(storage):
                    logits, saved = prog.forward(x, prog.m.training, need_bwd)
            finally:
                prog.fmap = None
        ctx.storage = storage
        ctx.prog = prog
        ctx.saved = saved
        return logits.detach()        # the plan's static logits: a fresh tensor object per step

    @staticmethod
    def backward(ctx, dlogits):
        prog = ctx.prog
        dlogits = dlogits.float().contiguous()     # autocast / GradScaler callers: any float dtype
        prog.flat.fresh_grad()
        prog.want_dx, prog.dx = ctx.need_dx, None
        try:
            with _lib.storage(ctx.storage):
                prog.runtime.backward(ctx.saved, dlogits)
        finally:
            prog.want_dx = False
        ctx.saved = None
        if prog.grad_ready_hook is not None:
            prog.grad_ready_hook(0, ())
        dx, prog.dx = prog.dx, None
        return (dx, None, None, None, *prog.flat.grad_views())


def run_step(model, x):
    """What both models' ``forward`` end in: ``model.program``'s step on ``x`` -> ``{"out": logits}``.

    With an input that requires grad (the reference's autograd returns d(loss)/d(x)) the eager
    forward runs inside ``StepFunction`` and the programs' backward leaves the input gradient in
    ``prog.dx``; otherwise the forward goes through the plan runtime here, ahead of autograd's
    per-parameter bookkeeping."""
    if not x.is_cuda:
        raise RuntimeError(f"stfunet.{type(model).__name__} runs on the gfx950 HIP kernels only; move the model "
                           "and input to a ROCm device (no CPU fallback)")
    prog = model.program
    prog.flat.ensure()
    storage = _lib.storage_for(model.storage_dtype)
    grad = torch.is_grad_enabled()
    res = None
    if not (grad and x.requires_grad):
        flags = prog.flat.requires_grad_flags()
        need_bwd = grad and True in flags
        # which blocks' backward this step will run: the forward keeps state for those only, and
        # the map is part of the plan signature (a toggled flag re-records)
        prog.fmap = prog.freeze_map(False, flags) if need_bwd else None
        try:
            with _lib.storage(storage), torch.no_grad():   # (as inside autograd.Function.forward)
                res = prog.runtime.forward(x, model.training, need_bwd)   # launched before autograd's bookkeeping
        finally:
            prog.fmap = None
    return {"out": StepFunction.apply(x, prog, storage, res, *prog.flat.params)}
