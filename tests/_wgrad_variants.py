"""One launch signature (at least) for every kernel stf_wgrad can select, and what each is there for.

TABLE maps each name stf_wgrad_kernel_name returns to cases (signature, properties).  A signature is
the tuple FIELDS: x is [N, Hs, Ws] pixels of Cs channels at channel xoff of xcs-wide rows, dy is
[N, Hd, Wd] pixels of Nout channels at channel dyoff of dycs-wide rows, and grid_blocks is the
workgroup budget the caller passes (0 inline, the CU count on the side stream).  The shapes are the
smallest found (with plan() below, a port of csrc/wgrad.hip's planner) that still have the edges the
kernel can get wrong; the properties name those edges and tests/test_wgrad_variants_cpu.py checks each
against stf_wgrad_plan, so a planner change that moves a case off its edge fails there:

  single   one split                         ragged   generic kernels: two or more splits, and the last
  many     more than eight splits (the                chunk is neither a whole chunk nor whole K steps
           generic reduce kernel)            multi    tile kernels: a split walks two or more pixel tiles
  short    tile kernels: the last split      images   fused 3x3: a split's run of tiles crosses tile
           has fewer tiles than the others            columns and an image boundary
  grid     grid_blocks changes the number    tiles    pixel tiles ragged at the bottom and the right
           of splits relative to 0           low      an image lower than one pixel tile
  rows     Nout is no multiple of 64         blocks   more than one 64-block of both Nout and Cs
  slices   x or dy starts at a channel       cus      grid_blocks is the MI355X's CU count
           offset of a wider buffer

WIDE_4GIB lists one launch per family in which one operand is a slice of a 4.5 GiB buffer (channel
stride 65536, nine 64 x 64 images, as _igemm_variants.SRC_4GIB; the last image lies wholly past byte
offset 2^32).  tests/test_wgrad_variants_gpu.py runs every entry against float64.
"""
from _igemm_variants import LIMIT, WIDE_CS          # noqa: F401  (LIMIT: re-exported for the tests)

FIELDS = ("N", "Hs", "Ws", "Cs", "xcs", "xoff", "Hd", "Wd", "R", "stride", "pad", "Nout", "dycs", "dyoff",
          "grid_blocks")
CUS = 256                                           # compute units of an MI355X


def sig(N, Hs, Ws, Cs, Nout, R=3, stride=1, pad=None, xcs=None, xoff=0, dycs=None, dyoff=0, gb=0):
    """Signature of a conv weight gradient; pad defaults to R // 2, the strides to dense rows."""
    pad = R // 2 if pad is None else pad
    Hd, Wd = (Hs + 2 * pad - R) // stride + 1, (Ws + 2 * pad - R) // stride + 1
    return (N, Hs, Ws, Cs, xcs or Cs + xoff, xoff, Hd, Wd, R, stride, pad, Nout, dycs or Nout + dyoff, dyoff, gb)


def convt(N, Hd, Wd, Cs, Nout, **kw):
    """ConvTranspose2d(2, 2) weight gradient: dy is the small [Hd, Wd] grid, x the 2x larger tensor."""
    return sig(N, 2 * Hd, 2 * Wd, Cs, Nout, R=2, stride=2, pad=0, **kw)


def case(props, s):
    return (s, frozenset(props.split()))


def fields(s):
    return dict(zip(FIELDS, s))


C8 = "wgrad3x3_c8_kernel"
F16, F8 = "wgrad3x3_kernel<16, 0>", "wgrad3x3_kernel<8, 0>"
T16_2, T8_2, T16_1, T8_1 = ("wgrad2x2s2_kernel<16, 2>", "wgrad2x2s2_kernel<8, 2>", "wgrad2x2s2_kernel<16, 1>",
                            "wgrad2x2s2_kernel<8, 1>")
G128, G64 = "wgrad_kernel<128, 128, 32, false>", "wgrad_kernel<64, 64, 64, false>"
GEN96, GEN64 = "wgrad_kernel<64, 96, 64, true>", "wgrad_kernel<64, 64, 64, true>"

TABLE = {
    # 8-channel input, 16 x 16 pixel tiles, one slab per workgroup
    C8: [
        case("many tiles", sig(3, 37, 21, 8, 64)),                         # 18 tiles, 18 workgroups
        case("multi short grid tiles", sig(3, 37, 21, 8, 64, gb=5)),       # 5 splits of 4 tiles, the last of 2
        case("multi grid slices", sig(2, 12, 40, 8, 64, dycs=192, dyoff=64, gb=4)),        # 3 splits of 2 tiles
        case("single multi grid tiles", sig(1, 20, 20, 8, 64, gb=1)),      # one workgroup walks all 4 tiles
        case("", sig(1, 16, 32, 8, 64)),                                   # 2 splits
        case("tiles", sig(2, 30, 31, 8, 64)),                              # 8 splits
        case("many multi grid cus tiles", sig(3, 150, 150, 8, 64, gb=CUS)),  # 300 tiles: 150 splits, not 300
    ],
    # fused 3x3, 4 x 16 pixel tiles
    F16: [
        case("many tiles", sig(3, 21, 37, 64, 64)),                        # 54 tiles, 14 splits of 4
        case("multi images grid tiles", sig(3, 21, 37, 64, 64, gb=2)),     # 2 splits of 27 tiles, 18 per image
        case("multi short grid tiles slices", sig(3, 21, 37, 64, 64, xcs=136, xoff=64, dycs=80, dyoff=8, gb=5)),
        case("single low", sig(2, 3, 20, 64, 64)),                         # 3 rows: less than one 4-row tile
        case("blocks tiles slices", sig(2, 9, 17, 128, 192, xcs=192, xoff=64, dycs=200, dyoff=8)),   # 3 splits
        case("tiles", sig(2, 14, 50, 64, 64)),                             # 32 tiles, 8 splits
        case("many multi grid cus blocks tiles", sig(4, 21, 37, 256, 256, gb=CUS)),   # 15 splits of 5, not 18 of 4
    ],
    # fused 3x3, 8 x 8 pixel tiles (8 <= W < 16)
    F8: [
        case("multi tiles slices", sig(3, 12, 9, 64, 128, dycs=192, dyoff=64)),          # 3 splits, one per image
        case("multi images grid tiles", sig(3, 12, 9, 64, 64, gb=2)),      # 2 splits of 6 tiles, 4 per image
        case("single", sig(1, 8, 8, 128, 128)),                            # the single-tile 1 x 8 x 8
        case("multi low", sig(3, 5, 9, 64, 64)),                           # 5 rows: less than one 8-row tile
        case("many blocks tiles", sig(9, 15, 15, 128, 128)),               # 36 tiles, 9 splits
        case("multi short grid blocks tiles", sig(9, 15, 15, 128, 128, gb=20)),        # 5 splits of 8, the last of 4
        case("tiles slices", sig(8, 15, 14, 64, 64, xcs=72, xoff=8)),      # 8 splits
    ],
    # ConvT 2x2, 128 dy channels per block (Nout >= 256)
    T16_2: [
        case("multi tiles slices", convt(2, 7, 17, 64, 256, xcs=128, xoff=64, dycs=264, dyoff=8)),   # 2 splits
        case("many multi grid cus blocks", convt(5, 20, 48, 256, 512, gb=CUS)),        # 15 splits of 5, not 19 of 4
    ],
    T8_2: [
        case("multi short grid tiles", convt(5, 9, 12, 64, 256, gb=6)),    # 20 tiles: 3 splits of 7, 7 and 6
        case("single", convt(1, 8, 8, 64, 256)),
    ],
    # ConvT 2x2, 64 dy channels per block
    T16_1: [
        case("multi tiles", convt(3, 5, 20, 64, 128)),                     # 12 tiles, 3 splits
        case("many multi tiles", convt(4, 10, 40, 64, 64)),                # 36 tiles, 9 splits
        case("multi short grid tiles", convt(4, 10, 40, 64, 64, gb=8)),    # 8 splits of 5, the last of 1
        case("multi short grid tiles slices", convt(4, 10, 40, 64, 64, xcs=72, xoff=8, gb=5)),   # 5 splits of 8
    ],
    T8_1: [
        case("multi blocks tiles slices", convt(2, 9, 12, 128, 128, xcs=192, xoff=64, dycs=136, dyoff=8)),  # 2 splits
        case("single multi grid tiles", convt(2, 9, 12, 128, 64, gb=2)),
    ],
    # 128 x 128 tile, 32-pixel K steps: 1x1 convs and stride-2 3x3 at 128-multiples of channels
    G128: [
        case("ragged", sig(3, 9, 11, 128, 128, R=1)),                      # 297 pixels: 3 splits of 128
        case("single", sig(2, 13, 16, 128, 256, R=1, stride=2)),           # 1x1 / stride 2: 13 x 16 -> 7 x 8
        case("ragged", sig(2, 15, 17, 128, 128, stride=2)),                # 3x3 / stride 2: 144 pixels, 2 x 96
        case("many", sig(4, 32, 33, 128, 128, R=1)),                       # 33 splits
        case("ragged slices", sig(2, 15, 20, 128, 128, R=1, xcs=264, xoff=8, dycs=136, dyoff=8)),   # 5 splits
        case("ragged", sig(2, 20, 25, 256, 128, R=1)),                     # 8 splits
    ],
    # 64 x 64 tile, 64-pixel K steps
    G64: [
        case("ragged rows", sig(3, 9, 11, 64, 96, R=1)),                   # Nout 96: half of the second row block
        case("single rows", sig(2, 15, 17, 64, 72, stride=2)),             # 3x3 / stride 2 from odd sizes
        case("ragged", sig(5, 9, 7, 64, 64)),                              # 3x3 / stride 1 at W = 7
        case("ragged slices", convt(12, 5, 7, 64, 128, xcs=72, xoff=8)),   # ConvT-shaped 2x2 at Wd = 7
        case("single", convt(3, 5, 7, 192, 64)),
        case("many ragged", sig(4, 24, 25, 64, 64, R=1)),                  # 10 splits
    ],
    # 96-column block: 64 < R * S * Cs <= 96
    GEN96: [
        case("ragged", sig(3, 9, 11, 8, 128)),                             # Cs 8 3x3 beside the c8 kernel: Nout 128
        case("ragged slices", sig(3, 9, 11, 8, 64, xcs=16, xoff=8)),       # ... and a strided source
        case("single slices", sig(2, 9, 11, 72, 64, R=1, xcs=80, xoff=8)),  # PK fusion: 72 of 80 channels
        case("ragged rows slices", sig(3, 20, 20, 72, 40, R=1, dycs=48, dyoff=8)),    # 5 splits
    ],
    # 64-column blocks that straddle taps; the last one ragged
    GEN64: [
        case("ragged rows", sig(3, 9, 11, 16, 8, R=1)),                    # one quarter-filled block, Nout 8
        case("ragged rows", sig(3, 10, 11, 32, 32)),                       # 288 columns: blocks span taps
        case("single slices", sig(2, 9, 11, 136, 64, R=1, xcs=144, xoff=8)),    # 136 columns: 64 + 64 + 8
        case("single", sig(2, 18, 20, 8, 64, R=7, stride=2)),              # the STF stem: 392 columns
        case("ragged", sig(3, 25, 27, 16, 64, R=1)),                       # 8 splits
        case("ragged rows", sig(3, 17, 15, 24, 72, R=1)),                  # 3 splits
    ],
}

# One operand a slice of a 4.5 GiB buffer: x for the 128-wide generic, fused 3x3 and ConvT kernels, dy
# for the c8 kernel (whose source must be dense); the other operand is small.
WIDE_4GIB = {
    G128: sig(9, 64, 64, 128, 128, R=1, xcs=WIDE_CS, xoff=8),
    F16: sig(9, 64, 64, 64, 64, xcs=WIDE_CS, xoff=8),
    T16_1: convt(9, 32, 32, 64, 64, xcs=WIDE_CS, xoff=8),
    C8: sig(9, 64, 64, 8, 64, dycs=WIDE_CS, dyoff=8),
}
FUSED = (C8, F16, F8, T16_2, T8_2, T16_1, T8_1)     # the kernels whose plan follows grid_blocks


def cases():
    """(name, signature, properties) of every table entry."""
    return [(n, s, p) for n, cs in TABLE.items() for s, p in cs]


def case_id(name, s):
    d = fields(s)
    short = name.replace("wgrad", "").replace("_kernel", "").replace(" ", "").strip("_")
    return (f"{short}-{d['N']}x{d['Hs']}x{d['Ws']}x{d['Cs']}-{d['Nout']}-r{d['R']}s{d['stride']}"
            f"-g{d['grid_blocks']}-{d['xoff']}.{d['dyoff']}")


def x_bytes(s):
    d = fields(s)
    return d["N"] * d["Hs"] * d["Ws"] * d["xcs"] * 2


def dy_bytes(s):
    d = fields(s)
    return d["N"] * d["Hd"] * d["Wd"] * d["dycs"] * 2


def plan(s):
    """csrc/wgrad.hip's route_of restated: the kernel family, its split count and chunk (pixel tiles per
    split for the tile kernels, pixels for the generic ones), and the tiling the properties speak of."""
    d = fields(s)
    N, Hd, Wd, Cs, Nout, R, gb = d["N"], d["Hd"], d["Wd"], d["Cs"], d["Nout"], d["R"], d["grid_blocks"]
    same = d["stride"] == 1 and d["pad"] == 1 and R == 3 and (Hd, Wd) == (d["Hs"], d["Ws"])
    ceil = lambda a, b: -(-a // b)                                                    # noqa: E731
    if same and Cs == 8 and d["xcs"] == 8 and Nout == 64:
        ty, tx = ceil(Hd, 16), ceil(Wd, 16)
        nt = N * ty * tx
        chunk = ceil(nt, min(nt, gb or 512))
        return dict(kind="c8", splits=ceil(nt, chunk), chunk=chunk, nt=nt, ty=ty, tx=tx, ph=16, pw=16)
    f3 = same and Nout % 64 == 0 and Cs % 64 == 0 and Wd >= 8
    f2 = (R == 2 and d["stride"] == 2 and d["pad"] == 0 and (d["Hs"], d["Ws"]) == (2 * Hd, 2 * Wd)
          and Nout % 64 == 0 and Cs % 64 == 0 and Wd >= 8)
    if f3 or f2:
        pw = 16 if Wd >= 16 else 8
        ph = 64 // pw
        ty, tx = ceil(Hd, ph), ceil(Wd, pw)
        nt = N * ty * tx
        nb = 2 if (f2 and not f3 and Nout % 128 == 0 and Nout >= 256) else 1
        blocks = Nout // (64 * nb) * (Cs // 64)
        want = max(1, min(ceil(gb or 512, blocks), (nt + 3) // 4))
        chunk = ceil(nt, want)
        return dict(kind="3x3" if f3 else "2x2", splits=ceil(nt, chunk), chunk=chunk, nt=nt, ty=ty, tx=tx, ph=ph,
                    pw=pw)
    M, rsc = N * Hd * Wd, R * R * Cs
    big = Nout % 128 == 0 and Cs % 128 == 0
    bm, bkp = (128, 32) if big else (64, 64)
    cblocks = 1 if (Cs % 64 and 64 < rsc <= 96) else ceil(rsc, bm)
    want = max(1, min(ceil(512 if big else 2048, ceil(Nout, bm) * cblocks), ceil(M, 4 * bkp)))
    chunk = ceil(ceil(M, want), bkp) * bkp
    return dict(kind="generic", splits=ceil(M, chunk), chunk=chunk, M=M, bkp=bkp)
