"""Drop-in ``UNet`` (reference ``src/unet.py:5-57``) running on gfx950 kernels.

Surface kept from the reference: class attribute ``input_format =
"flat_channels"`` (read by ``preprocess_input``, train_and_eval.py:9-22), the
constructor ``UNet(in_channels=8, num_classes=2, base_c=64)``, the module tree
(``enc1..4``, ``pool``, ``bottleneck``, ``up1..4``, ``dec1..4``, ``out_conv``; each
DoubleConv an ``nn.Sequential(Conv2d, BatchNorm2d, ReLU, Conv2d, BatchNorm2d,
ReLU)``) and therefore the 136 ``state_dict`` keys and PyTorch's default init,
and ``forward(x) -> {"out": logits}`` with logits [B, classes, H, W] fp32.

What runs is not those modules' forward: ``forward`` hands the input and every
parameter to ``program.run_step`` (the autograd function, the plan runtime and the
``Program`` base are in program.py), which runs ``UNetProgram``'s explicit schedule over
NHWC bf16 buffers:

  forward, per DoubleConv (src/unet.py:10-18):
    igemm conv3x3 (+bias, +BN partial sums) -> bn_finalize -> bn_act
    igemm conv3x3 (+bias, +BN partial sums) -> bn_finalize -> bn_act writing
        the skip half of the level's concat buffer and the 2x2-pooled input of
        the next level in one pass (Down = MaxPool2d(2), src/unet.py:25,41-45)
  Up (src/unet.py:28-35,47-54): igemm with a ConvTranspose2d(2,2) scatter
        epilogue writes the other half of the concat buffer: no torch.cat
  OutConv (src/unet.py:37,56): fused with dec1's last BN+ReLU in stf_head_fwd
  backward: the mirror schedule, gradients written into one flat fp32 buffer.
"""

import torch
import torch.nn as nn

from . import nhwc
from .nhwc import Feat, new_feat
from .program import Program, Saved as _Saved, conv_bn, conv_pair_backward, run_step


def _double_conv(cin, cout):
    # src/unet.py:10-18 -- module indices 0/1/3/4 are the state_dict contract
    return nn.Sequential(nn.Conv2d(cin, cout, 3, padding=1), nn.BatchNorm2d(cout), nn.ReLU(inplace=True),
                         nn.Conv2d(cout, cout, 3, padding=1), nn.BatchNorm2d(cout), nn.ReLU(inplace=True))


def _cpad(c):
    return (c + 7) // 8 * 8


class DoubleConvProgram:
    """Forward/backward schedule of one DoubleConv block on NHWC buffers."""

    def __init__(self, blk, name=""):
        self.blk = blk
        self.cout = blk[0].out_channels
        self.name = name

    def forward(self, src: Feat, training, need_bwd, out: Feat = None, pooled: Feat = None):
        with nhwc.timed_block(f"{self.name}.fwd"):
            return self._forward(src, training, need_bwd, out, pooled)

    def backward(self, s, grads, need_dsrc, dz: Feat = None, dpool: Feat = None, dy2: Feat = None,
                 dsrc_stats=False, need_w=True):
        with nhwc.timed_block(f"{self.name}.bwd"):
            return self._backward(s, grads, need_dsrc, dz, dpool, dy2, dsrc_stats, need_w)

    def _forward(self, src: Feat, training, need_bwd, out: Feat = None, pooled: Feat = None):
        conv1, bn1, conv2, bn2 = self.blk[0], self.blk[1], self.blk[3], self.blk[4]
        C, dev = self.cout, src.buf.device
        s = _Saved()
        s.src = src
        y1, s.bn1 = conv_bn(src, conv1, bn1, 3, 1, 1)
        a1 = new_feat(src.N, src.H, src.W, C, dev)
        nhwc.bn_act(y1, s.bn1, a1)
        y2, s.bn2 = conv_bn(a1, conv2, bn2, 3, 1, 1)
        if out is not None:
            nhwc.bn_act(y2, s.bn2, out, pooled=pooled)
        s.y1, s.a1, s.y2 = y1, a1, y2
        return s if need_bwd else None

    def _backward(self, s, grads, need_dsrc, dz: Feat = None, dpool: Feat = None, dy2: Feat = None,
                  dsrc_stats=False, need_w=True):
        """Either (dz and/or dpool) w.r.t. the block output, or dy2 (grad w.r.t.
        the raw second conv output, when the BN backward was fused upstream).  ``dsrc_stats``:
        return (dsrc, statistics rows, tiles) -- the per-tile column sums of the stored input
        gradient (a decoder block's concat gradient: the up-conv's bias gradient, no extra pass).
        ``need_w=False``: a frozen block that only passes the gradient on (no weight gradients)."""
        conv1, bn1, conv2, bn2 = self.blk[0], self.blk[1], self.blk[3], self.blk[4]
        gv = grads.grad_view
        if dy2 is None:
            dy2 = nhwc.bn_backward(s.y2, s.bn2, bn2, gv(bn2.weight), gv(bn2.bias), dz=dz, dpool=dpool,
                                   dbias=gv(conv2.bias))
        dy1 = conv_pair_backward(s, gv, dy2, conv1, bn1, conv2, dbias1=gv(conv1.bias), need_w=need_w)
        if not need_dsrc:
            return None
        dsrc = new_feat(s.src.N, s.src.H, s.src.W, s.src.C, s.src.buf.device)
        w1 = conv1.weight
        if s.src.C != w1.shape[1]:
            # zero-padded input channels (in_channels % 8 != 0): the weight padded the same way, so the
            # padded channels' gradient is computed and dropped by the caller
            w1 = nhwc.pad_weight(w1, s.src.C)
        st, tiles = nhwc.conv_dgrad(dy1, w1, dsrc, 3, 3, 1, 1, cache=w1 is conv1.weight, want_stats=dsrc_stats)
        return (dsrc, st, tiles) if dsrc_stats else dsrc


class UNetProgram(Program):
    def __init__(self, model):
        super().__init__(model)
        self.levels = [DoubleConvProgram(b, f"enc{i}") for i, b in
                       enumerate((model.enc1, model.enc2, model.enc3, model.enc4), start=1)]
        self.bott = DoubleConvProgram(model.bottleneck, "bottleneck")
        self.ups = [model.up4, model.up3, model.up2, model.up1]
        self.decs = [DoubleConvProgram(b, f"dec{i}") for i, b in
                     zip((4, 3, 2, 1), (model.dec4, model.dec3, model.dec2, model.dec1))]

    def graph(self):
        m = self.m
        g = [("enc1", (m.enc1,), ("x",))]
        g += [(f"enc{i}", (getattr(m, f"enc{i}"),), (f"enc{i - 1}",)) for i in (2, 3, 4)]
        g.append(("bottleneck", (m.bottleneck,), ("enc4",)))
        below = "bottleneck"
        for i in (4, 3, 2, 1):
            g.append((f"up{i}", (getattr(m, f"up{i}"),), (below,)))
            g.append((f"dec{i}", (getattr(m, f"dec{i}"),), (f"up{i}", f"enc{i}")))
            below = f"dec{i}"
        g.append(("out_conv", (m.out_conv,), ("dec1",)))
        return g

    def _done(self, module):
        # (with weight gradients on a side stream, the bucket waits for that stream too)
        super()._done(module, (nhwc.WGRAD_STREAM,) if nhwc.WGRAD_STREAM is not None else ())

    # Program.backward as it is: weight gradients stay on the current stream here: a side stream
    # (as in the STF program) measured +1.2 / -0.3..-3.8 % at cfg2 (full / one-per-CU grid, round 5) and
    # makes every concurrent kernel's duration a shared-machine number; the variant was removed

    # ------------------------------------------------------------------ forward
    def _forward(self, x, training, need_bwd):
        m = self.m
        nhwc._NBT_PENDING.clear()
        N, _, H, W = x.shape
        assert H % 16 == 0 and W % 16 == 0, "UNet needs H, W divisible by 16 (four 2x2 pools)"
        dev = x.device
        S = _Saved()
        # the freeze map: a block whose backward will not run keeps no state (y1, a1, y2)
        fm = S.fmap = self.step_map()
        src = nhwc.pack_input(x, _cpad(m.in_channels))
        S.enc, S.cats = [], []
        h, w = H, W
        for lvl in self.levels:
            C = lvl.cout
            cat = new_feat(N, h, w, 2 * C, dev)
            pooled = new_feat(N, h // 2, w // 2, C, dev)
            S.enc.append(lvl.forward(src, training, need_bwd and fm.runs(lvl.name), out=cat.slice(C, C),
                                     pooled=pooled))
            S.cats.append(cat)
            src = pooled
            h, w = h // 2, w // 2
        Cb = self.bott.cout
        a_b = new_feat(N, h, w, Cb, dev)
        S.bott = self.bott.forward(src, training, need_bwd and fm.runs("bottleneck"), out=a_b)
        cur = a_b
        S.dec, S.dec_in = [], []
        for i, (up, dec) in enumerate(zip(self.ups, self.decs)):
            cat = S.cats[3 - i]
            Clo = dec.cout
            wt = nhwc.pack_weight(up.weight, 2)
            nhwc.igemm(cur, wt, 4 * Clo, cat.slice(0, Clo), 1, 1, 1, 0, bias=up.bias.detach(), scatter2x2=True)
            S.dec_in.append(cur if fm[f"up{4 - i}"].need_w else None)     # (the up-conv's weight gradient)
            last = i == 3
            if not last:
                out = new_feat(cat.N, cat.H, cat.W, Clo, dev)
                S.dec.append(dec.forward(cat, training, need_bwd and fm.runs(dec.name), out=out))
                cur = out
            else:
                s = dec.forward(cat, training, True)
                if not fm.runs(dec.name):          # the head's backward reads y2 and its BN state only
                    s.src = s.y1 = s.a1 = None
                S.dec.append(s)
        # OutConv fused with dec1's last BN+ReLU
        s = S.dec[-1]
        K = m.out_conv.out_channels
        logits = nhwc.empty((N, K, H, W), torch.float32, dev)
        S.head_w = nhwc.head_fwd(s.y2, s.bn2, m.out_conv, logits)
        S.cats = None                  # (a block that runs its backward holds its own source)
        if not need_bwd:
            S.enc = S.dec = None
        nhwc.flush_batches_tracked()
        return logits, (S if need_bwd else None)

    # ------------------------------------------------------------------ backward
    def _backward(self, S, dlogits):
        m = self.m
        gv = self.flat.grad_view
        dev = dlogits.device
        dlogits = dlogits.contiguous().float()
        # The freeze map decides per block: weight gradients only where a parameter is trainable
        # (need_w), the input gradient only where something upstream still wants it (need_din); a
        # block with neither is not run, so the backward ends at the lowest trainable block
        fm = S.fmap
        # head + dec1's last BN+ReLU
        s = S.dec[-1]
        g, bnp, tiles = nhwc.head_bwd(dlogits, s.y2, s.bn2, S.head_w, gv(m.out_conv.weight), gv(m.out_conv.bias))
        dec1 = self.decs[3]
        dcats = [None] * 4
        if fm.runs("dec1"):
            dy2 = nhwc.bn_backward_from_partial(g, s.y2, s.bn2, dec1.blk[4], bnp, tiles, gv(dec1.blk[4].weight),
                                                gv(dec1.blk[4].bias), gv(dec1.blk[3].bias))
            # the concat gradient of each decoder block comes with the per-tile column sums of what its
            # dgrad stored (statistics epilogue): the up-conv's bias gradient is their up-half fold
            dcats[0] = dec1.backward(s, self.flat, fm["dec1"].need_din, dy2=dy2, dsrc_stats=True,
                                     need_w=fm["dec1"].need_w)
        self._done(dec1.blk)
        # decoder levels 2..4 and the up-convs, deepest last
        for i in (3, 2, 1, 0):                       # index into self.ups / S.dec_in (up1 is i=3)
            up, nu = self.ups[i], fm[f"up{4 - i}"]
            dsrc = None
            if dcats[3 - i] is not None:
                dcat, cst, ctiles = dcats[3 - i]
                dcats[3 - i] = dcat
                Clo = self.decs[i].cout
                dup = dcat.slice(0, Clo)
                if nu.need_w:
                    nhwc.wgrad(S.dec_in[i], dup, 2, 2, 2, 0, gv(up.weight))
                    nhwc.stat_sums(cst, ctiles, dcat.C, 0, Clo, gv(up.bias))       # (= channel_sum(dup))
                if nu.need_din:
                    dsrc = new_feat(dcat.N, dcat.H // 2, dcat.W // 2, up.in_channels, dev)
                    nhwc.igemm(dup, nhwc.pack_weight(up.weight, 3), dsrc.C, dsrc, 2, 2, 2, 0)
            self._done(up)
            if i > 0:
                dec = self.decs[i - 1]
                if fm.runs(dec.name):            # (then the up-conv above it needed its input gradient)
                    dcats[4 - i] = dec.backward(S.dec[i - 1], self.flat, fm[dec.name].need_din, dz=dsrc,
                                                dsrc_stats=True, need_w=fm[dec.name].need_w)
                self._done(dec.blk)
            else:
                d_b = dsrc
        dpool = None
        if fm.runs("bottleneck"):
            dpool = self.bott.backward(S.bott, self.flat, fm["bottleneck"].need_din, dz=d_b,
                                       need_w=fm["bottleneck"].need_w)
        self._done(self.bott.blk)
        for j in (3, 2, 1, 0):
            lvl = self.levels[j]
            C = lvl.cout
            if fm.runs(lvl.name):
                dskip = dcats[j].slice(C, C)
                dpool = lvl.backward(S.enc[j], self.flat, fm[lvl.name].need_din, dz=dskip, dpool=dpool,
                                     need_w=fm[lvl.name].need_w)
            dcats[j] = None
            self._done(lvl.blk)
        if self.want_dx:     # enc1's input gradient, NHWC 16-bit -> the input's [N, C, H, W] fp32
            self.dx = dpool.dense()[:, : m.in_channels].contiguous()


class UNet(nn.Module):
    input_format = "flat_channels"  # [B, T*C, H, W], train_and_eval.py:12-14

    def __init__(self, in_channels=8, num_classes=2, base_c=64):
        super().__init__()
        nhwc.check_num_classes(num_classes)
        self.in_channels = in_channels
        self.enc1 = _double_conv(in_channels, base_c)
        self.enc2 = _double_conv(base_c, base_c * 2)
        self.enc3 = _double_conv(base_c * 2, base_c * 4)
        self.enc4 = _double_conv(base_c * 4, base_c * 8)
        self.pool = nn.MaxPool2d(2)
        self.bottleneck = _double_conv(base_c * 8, base_c * 16)
        self.up4 = nn.ConvTranspose2d(base_c * 16, base_c * 8, kernel_size=2, stride=2)
        self.dec4 = _double_conv(base_c * 16, base_c * 8)
        self.up3 = nn.ConvTranspose2d(base_c * 8, base_c * 4, kernel_size=2, stride=2)
        self.dec3 = _double_conv(base_c * 8, base_c * 4)
        self.up2 = nn.ConvTranspose2d(base_c * 4, base_c * 2, kernel_size=2, stride=2)
        self.dec2 = _double_conv(base_c * 4, base_c * 2)
        self.up1 = nn.ConvTranspose2d(base_c * 2, base_c, kernel_size=2, stride=2)
        self.dec1 = _double_conv(base_c * 2, base_c)
        self.out_conv = nn.Conv2d(base_c, num_classes, kernel_size=1)
        self._program = None
        # 16-bit activation storage: None = bf16, or fp16 under autocast(float16) (the
        # reference's --amp); torch.bfloat16 / torch.float16 force one (_lib.storage_for)
        self.storage_dtype = None

    @property
    def program(self):
        if self._program is None:
            self._program = UNetProgram(self)
        return self._program

    def forward(self, x):
        return run_step(self, x)
