"""One launch signature (at least) for every implicit-GEMM variant an unforced launch can select.

TABLE maps each name of test_igemm_routes_cpu.REACHABLE to signatures in the field order of
tests/golden/make_golden_routes.FIELDS, so make_golden_routes.query answers for them.  Every
signature is the smallest shape found (with the host-only queries on 256 CUs) that selects its
variant and still has the edges the kernel can get wrong: more than one tile or workgroup, a ragged
last tile, a source or destination that is a channel slice of a wider buffer.  The three halo tiles
that do not defer have a second signature whose workgroups walk three (group, slice) keys each,
which is where their statistics fold differs from the deferred form.

The eight register-staged variants without SMALLC are only selected by a source of 4 GiB or more
(SRC_4GIB: a 32-channel slice of a 65536-channel buffer, nine 64 x 64 images, 4.5 GiB; the last
image lies wholly past byte offset 2^32).  DST_4GIB lists launches whose *destination* is such a
buffer while the source is small, one per kernel family that would take them were the destination
small, with the kernel each must run instead; BNR_Y_4GIB is a BN-backward-fused launch whose y is.

tests/test_igemm_variants_cpu.py checks this table against the router without a GPU;
tests/test_igemm_variants_gpu.py runs every entry against a float64 reference.
"""
import importlib.util
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_golden_routes",
                                               os.path.join(_HERE, "golden", "make_golden_routes.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)
sig, FIELDS = gen.sig, gen.FIELDS

DMA_A, DMA_B, DMA_C = "128, 128, 2, 2, 32, 4", "256, 128, 4, 2, 64, 3", "256, 256, 2, 4, 64, 2"
DMA_D, DMA_E = "512, 64, 8, 1, 64, 2", "256, 64, 4, 1, 32, 4"
REG_R, REG_S = "128, 128, 2, 2", "256, 64, 4, 1"
WIDE_CS = 65536                     # channel stride of the 4.5 GiB buffers: 9 * 64 * 64 * 65536 * 2 bytes


def _halo(pw, v):
    return f"conv3x3_halo_kernel<16, {pw}, 8, 2, 0, {v}>"


def _dma(tile, v, c8="false"):
    return f"igemm_dma_kernel<{tile}, {v}, {c8}>"


def _reg(tile, v, epi=0):
    return f"igemm_kernel<{tile}, {v}, {epi}>"


TABLE = {
    # 8-channel network input into the skip half of a concat buffer; three statistics groups
    "conv3x3_c8_kernel": [sig(3, 20, 36, 8, 64, bias=1, stats=1, groups=3, dcs=80)],
    # four 8 x 8 images per tile, two groups of four images, slice source, accumulate
    "conv3x3_halo4_kernel<0>": [sig(8, 8, 8, 32, 64, bias=1, stats=1, groups=2, scs=40, acc=1)],
    # wide kernel: ragged 16 x 32 tiles, two chunks
    "conv3x3_wide_kernel<2, false>": [sig(2, 20, 40, 64, 128, bias=1, stats=1, groups=2, scs=72, dcs=136)],
    "conv3x3_wide_kernel<1, false>": [sig(2, 20, 40, 32, 128, acc=1)],
    "conv3x3_wide_kernel<1, true>": [sig(2, 20, 40, 32, 128, bnr=1, groups=2)],
    # two 16 x 16 images per tile
    "conv3x3_halo2_kernel<2, false, false>": [sig(4, 16, 16, 32, 64, bias=1, stats=1, groups=2, dcs=72)],
    "conv3x3_halo2_kernel<1, false, false>": [sig(2, 16, 16, 32, 320, bias=1)],
    "conv3x3_halo2_kernel<1, true, false>": [sig(2, 16, 16, 32, 320, bnr=1)],
    # single-image 16 x 16 tiles; not deferring: one tile per statistics group
    _halo(16, "2, false, false"): [sig(3, 16, 16, 32, 64, bias=1, stats=1, groups=3),
                                   sig(520, 16, 16, 32, 64, bias=1, stats=1, groups=520)],
    _halo(16, "2, false, true"): [sig(2, 20, 24, 32, 128, bias=1, stats=1, groups=2, scs=40)],
    _halo(16, "1, false, true"): [sig(2, 20, 24, 64, 64, dcs=72, acc=1)],
    _halo(16, "1, true, false"): [sig(3, 16, 16, 32, 64, bnr=1, groups=3),
                                  sig(520, 16, 16, 32, 64, bnr=1, groups=520)],
    _halo(16, "1, true, true"): [sig(2, 20, 24, 32, 64, bnr=1, groups=2)],
    # single-image 16 x 32 tiles
    _halo(32, "2, false, false"): [sig(3, 16, 32, 32, 64, bias=1, stats=1, groups=3),
                                   sig(520, 16, 32, 32, 64, bias=1, stats=1, groups=520)],
    _halo(32, "2, false, true"): [sig(2, 20, 40, 32, 64, bias=1, stats=1, groups=2, scs=40)],
    _halo(32, "1, false, true"): [sig(2, 20, 40, 64, 64, dcs=72, acc=1)],
    _halo(32, "1, true, false"): [sig(3, 16, 32, 32, 64, bnr=1, groups=3),
                                  sig(520, 16, 32, 32, 64, bnr=1, groups=520)],
    _halo(32, "1, true, true"): [sig(2, 20, 40, 32, 64, bnr=1, groups=2)],
    # linear DMA kernels, 128 x 128 tile: plain, the two LSTM epilogues, ConvT 2x2 scatter, transposed
    _dma(DMA_A, "false, false, 0"): [sig(3, 9, 11, 32, 96, R=1, bias=1, stats=1, groups=3, scs=40, dcs=104)],
    _dma(DMA_A, "false, false, 1"): [sig(3, 9, 11, 64, 128, R=1, bias=1, lstm=1, dcs=64)],
    _dma(DMA_A, "false, false, 2"): [sig(3, 9, 11, 64, 128, R=1, bias=1, lstm=2, dcs=64)],
    _dma(DMA_A, "false, true, 0"): [sig(2, 9, 11, 96, 4 * 48, R=1, bias=1, scatter=1, dcs=96)],
    _dma(DMA_A, "true, false, 0"): [sig(2, 8, 9, 64, 128, stride=2, tr=1, bias=1, Hd=15, Wd=17)],
    # 256 x 64 tile
    _dma(DMA_E, "false, false, 0"): [sig(3, 9, 11, 32, 64, bias=1, stats=1, groups=3, scs=40, dcs=72)],
    _dma(DMA_E, "false, true, 0"): [sig(2, 9, 11, 32, 4 * 16, R=1, bias=1, scatter=1, dcs=32)],
    _dma(DMA_E, "true, false, 0"): [sig(3, 5, 6, 64, 32, stride=2, tr=1, acc=1, Hd=9, Wd=11)],
    # 8-channel sources on the linear kernels
    _dma(DMA_A, "false, false, 0", "true"): [sig(3, 9, 11, 8, 128, bias=1, stats=1, groups=3, dcs=136)],
    _dma(DMA_E, "false, false, 0", "true"): [sig(3, 9, 11, 8, 64, R=1, bias=1, dcs=72)],
    # 256 x 128, 256 x 256 (fills the chip: ceil(M / 256) * ceil(Nout / 256) >= 240), 512 x 64
    _dma(DMA_B, "false, false, 0"): [sig(3, 9, 11, 64, 128, R=1, bias=1, stats=1, groups=3, scs=72, dcs=136)],
    _dma(DMA_B, "false, true, 0"): [sig(3, 9, 11, 64, 4 * 32, R=1, bias=1, scatter=1, dcs=40)],
    _dma(DMA_C, "false, false, 0"): [sig(30, 32, 32, 64, 512, R=1, bias=1, stats=1, groups=2, scs=72, dcs=520)],
    _dma(DMA_C, "false, true, 0"): [sig(30, 32, 32, 64, 4 * 128, R=1, bias=1, scatter=1, dcs=136)],
    _dma(DMA_D, "false, false, 0"): [sig(3, 9, 11, 64, 64, R=1, bias=1, stats=1, groups=3, acc=1)],
    _dma(DMA_D, "false, true, 0"): [sig(3, 9, 11, 64, 4 * 16, R=1, bias=1, scatter=1, dcs=24)],
    # register-staged, Cs not a multiple of 32 (the STF PK-fusion 1x1 convs, C + 8 channels, and their dgrads)
    _reg(REG_R, "true, false, false"): [sig(3, 9, 11, 72, 128, R=1, bias=1, stats=1, groups=3, scs=80, dcs=136),
                                        sig(2, 9, 11, 48, 96, acc=1)],
    _reg(REG_R, "true, true, false"): [sig(2, 8, 9, 48, 128, stride=2, tr=1, bias=1, Hd=15, Wd=17)],
    _reg(REG_R, "true, false, true"): [sig(2, 9, 11, 48, 4 * 32, R=1, bias=1, scatter=1, dcs=40)],
    _reg(REG_S, "true, false, false"): [sig(3, 9, 11, 72, 64, R=1, bias=1, stats=1, groups=3, scs=80, dcs=72),
                                        sig(2, 9, 11, 48, 48, acc=1)],
    _reg(REG_S, "true, true, false"): [sig(3, 5, 6, 48, 48, stride=2, tr=1, acc=1, Hd=9, Wd=11)],
    _reg(REG_S, "true, false, true"): [sig(2, 9, 11, 48, 4 * 16, R=1, bias=1, scatter=1, dcs=24)],
}

# Sources of 4 GiB or more: the 64-bit-addressing fallback, SMALLC = false
SRC_4GIB = {
    _reg(REG_R, "false, false, false"): [sig(9, 64, 64, 32, 128, bias=1, stats=1, groups=3, scs=WIDE_CS)],
    _reg(REG_R, "false, true, false"): [sig(9, 64, 64, 32, 128, stride=2, tr=1, bias=1, scs=WIDE_CS)],
    _reg(REG_R, "false, false, true"): [sig(9, 64, 64, 32, 4 * 32, R=1, bias=1, scatter=1, scs=WIDE_CS)],
    _reg(REG_S, "false, false, false"): [sig(9, 64, 64, 32, 64, bias=1, stats=1, groups=3, scs=WIDE_CS)],
    _reg(REG_S, "false, true, false"): [sig(9, 64, 64, 32, 32, stride=2, tr=1, acc=1, scs=WIDE_CS)],
    _reg(REG_S, "false, false, true"): [sig(9, 64, 64, 32, 4 * 16, R=1, bias=1, scatter=1, scs=WIDE_CS)],
    _reg(REG_R, "false, false, false", 1): [sig(9, 64, 64, 64, 128, R=1, bias=1, lstm=1, scs=WIDE_CS, dcs=WIDE_CS)],
    _reg(REG_R, "false, false, false", 2): [sig(9, 64, 64, 64, 128, R=1, bias=1, lstm=2, scs=WIDE_CS, dcs=WIDE_CS)],
}
TABLE.update(SRC_4GIB)

# Destinations of 4 GiB or more (source small): (the family a small destination selects, signature,
# the kernel that must run).  The tile kernels address the destination through a 32-bit buffer
# descriptor, so the router sends these to the linear kernels, whose stores take 64-bit addresses.
_E, _D = _dma(DMA_E, "false, false, 0"), _dma(DMA_D, "false, false, 0")
DST_4GIB = [
    ("halo 16x32 forward", sig(9, 64, 64, 32, 64, bias=1, stats=1, groups=3, dcs=WIDE_CS), _E),
    ("halo 16x32 dgrad", sig(9, 64, 64, 64, 64, dcs=WIDE_CS, acc=1), _D),
    ("halo 16x32 bnr", sig(9, 64, 64, 32, 64, bnr=1, groups=3, dcs=WIDE_CS), _E),
    ("halo 16x16 forward", sig(9, 256, 16, 32, 64, bias=1, stats=1, groups=3, dcs=WIDE_CS), _E),
    ("halo 16x16 dgrad", sig(9, 256, 16, 32, 64, dcs=WIDE_CS), _E),
    ("halo 16x16 bnr", sig(9, 256, 16, 32, 64, bnr=1, groups=3, dcs=WIDE_CS), _E),
    ("wide", sig(9, 64, 64, 32, 128, bias=1, stats=1, groups=3, dcs=WIDE_CS), _dma(DMA_A, "false, false, 0")),
    ("two-image tiles", sig(144, 16, 16, 32, 64, bias=1, stats=1, groups=3, dcs=WIDE_CS), _E),
    ("four-image 8x8 tiles", sig(576, 8, 8, 32, 64, bias=1, stats=1, groups=3, dcs=WIDE_CS), _E),
    ("8-channel input", sig(9, 64, 64, 8, 64, bias=1, stats=1, groups=3, dcs=WIDE_CS),
     _dma(DMA_E, "false, false, 0", "true")),
    ("linear DMA tile", sig(9, 64, 64, 64, 128, R=1, bias=1, stats=1, groups=3, dcs=WIDE_CS),
     _dma(DMA_B, "false, false, 0")),
    ("split-K", sig(9, 64, 64, 1024, 64, R=1, bias=1, stats=1, groups=3, dcs=WIDE_CS), _D),
]
# the kernel each DST_4GIB signature selects when its destination is dense (dcs = the output channels)
DST_4GIB_SMALL = [_halo(32, "2, false, true"), _halo(32, "1, false, true"), _halo(32, "1, true, true"),
                  _halo(16, "2, false, true"), _halo(16, "1, false, true"), _halo(16, "1, true, true"),
                  "conv3x3_wide_kernel<2, false>", "conv3x3_halo2_kernel<2, false, false>", "conv3x3_halo4_kernel<0>",
                  "conv3x3_c8_kernel", _dma(DMA_B, "false, false, 0"), _dma(DMA_D, "false, false, 0")]

# A BN-backward-fused dgrad whose y (not dz) is the 4.5 GiB buffer: (signature, y channel stride, kernel)
BNR_Y_4GIB = (sig(9, 64, 64, 32, 64, bnr=1, groups=3), WIDE_CS, _dma(DMA_E, "false, false, 0"))

LIMIT = 64 << 20                    # bytes: no source or destination outside the 4 GiB cases is larger


def fields(s):
    return dict(zip(FIELDS, s))


def src_bytes(s):
    d = fields(s)
    return d["N"] * d["Hs"] * d["Ws"] * d["scs"] * 2


def dst_bytes(s):
    d = fields(s)
    return d["N"] * d["Hd"] * d["Wd"] * (4 if d["scatter"] else 1) * d["dcs"] * 2


def cases():
    """(name, signature) of every table entry outside the 4 GiB cases."""
    return [(n, s) for n, sigs in TABLE.items() if n not in SRC_4GIB for s in sigs]
