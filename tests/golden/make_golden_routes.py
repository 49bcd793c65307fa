"""Pin the implicit-GEMM routes: which kernel stf_igemm launches and what its size queries answer.

    STF_LIB=<parent build>/libstfunet_hip.so python tests/golden/make_golden_routes.py --commit <hash>

writes tests/golden/igemm_routes.json: for every launch signature below, the kernel name
(stf_igemm_kernel_name, as the profiler prints it), the statistics tiles, the BN-backward tiles
and the split-K workspace bytes with the statistics pointer unset and set.  The fixture is the
measure of "the routes did not change" for tests/test_igemm_routes_cpu.py, so it is written from
the build of the commit *before* a change to the route selection, never from the code under test.
The queries launch nothing; without a GPU the library assumes 256 CUs, the MI355X's count.

The signatures come from the two models' layer tables (channel counts and resolutions), in the
forms the layer programs launch them (stfunet/unet.py, stfunet/stf_lstm_unet.py, nhwc.conv_dgrad),
plus the small shapes of tests/test_surface_cpu.py and tests/test_kernels_gpu.py.
"""
import argparse
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "igemm_routes.json")

FIELDS = ("N", "Hs", "Ws", "Cs", "scs", "Hd", "Wd", "R", "S", "stride", "pad", "transposed", "Nout", "dcs",
          "bias", "scatter", "groups", "acc", "lstm", "bnr", "stats", "dst_low")
RESULTS = ("name", "stat_tiles", "bnr_tiles", "ws_unset", "ws_set")


def sig(N, H, W, Cs, Nout, R=3, stride=1, pad=None, tr=0, scs=None, dcs=None, Hd=None, Wd=None, bias=0, scatter=0,
        groups=1, acc=0, lstm=0, bnr=0, stats=0, dst_low=0):
    """One launch signature; H, W are the source's, the destination's default to the conv's output size."""
    pad = R // 2 if pad is None else pad
    if Hd is None:
        Hd, Wd = (H, W) if stride == 1 else ((2 * H, 2 * W) if tr else ((H - 1) // stride + 1, (W - 1) // stride + 1))
    return (N, H, W, Cs, scs or Cs, Hd, Wd, R, R, stride, pad, tr, Nout, dcs or (Nout // 4 if scatter else Nout),
            bias, scatter, groups, acc, lstm, bnr, stats, dst_low)


def conv3x3_forms(N, H, W, cin, cout, groups=1, scs=None, dcs=None):
    """A 3x3 / stride 1 layer as the layer programs run it: forward with statistics (and the eval
    forward without), plain dgrad (also accumulating), dgrad with the fused BN-backward reduce,
    dgrad with statistics."""
    out = [sig(N, H, W, cin, cout, bias=1, stats=1, groups=groups, scs=scs, dcs=dcs),
           sig(N, H, W, cin, cout, bias=1, groups=groups, scs=scs, dcs=dcs),
           sig(N, H, W, cin, cout, stats=1, groups=groups, scs=scs, dcs=dcs)]
    if cin % 8 == 0:
        out += [sig(N, H, W, cout, cin), sig(N, H, W, cout, cin, acc=1),
                sig(N, H, W, cout, cin, bnr=1, groups=groups), sig(N, H, W, cout, cin, stats=1)]
    return out


def unet_signatures(N=64, HW=256, in_c=8, base=64):
    """UNet (stfunet/unet.py): four encoder levels + bottleneck of two 3x3 convs each, four
    ConvT 2x2 + double-conv decoder levels.  Encoder conv2 writes the skip half of the concat."""
    s = []
    ch = [base << i for i in range(5)]
    cin, h = in_c, HW
    for lvl, c in enumerate(ch):
        s += conv3x3_forms(N, h, h, cin, c)
        s += conv3x3_forms(N, h, h, c, c, dcs=2 * c if lvl < 4 else None)
        cin, h = c, h // 2
    h = HW >> 4
    for lvl in (3, 2, 1, 0):
        chi, clo = ch[lvl + 1], ch[lvl]
        s.append(sig(N, h, h, chi, 4 * clo, R=1, bias=1, scatter=1, dcs=2 * clo))            # ConvT scatter
        s.append(sig(N, 2 * h, 2 * h, clo, chi, R=2, stride=2, pad=0, scs=2 * clo, Hd=h, Wd=h))  # its gather
        h *= 2
        s += conv3x3_forms(N, h, h, 2 * clo, clo)
        s += conv3x3_forms(N, h, h, clo, clo)
    return s


def stf_signatures(B, T, HW):
    """STFLSTMUNet (stfunet/stf_lstm_unet.py): ResNet-style encoder over N = B * T frames with one
    statistics group per time step, a per-pixel LSTM per scale, three ConvT 3x3 / stride 2 decoder
    blocks, the last up-convolution and the final residual block."""
    s = []
    N, h = B * T, HW // 4
    ch = (64, 128, 256, 512)
    cin = 64
    for li, c in enumerate(ch):
        st = 1 if li == 0 else 2
        ho = h // st
        if st == 2:
            for R in (3, 1):
                s += [sig(N, h, h, cin, c, R=R, stride=2, stats=1, groups=T), sig(N, h, h, cin, c, R=R, stride=2)]
                for acc in (0, 1):                                  # transposed dgrads
                    s.append(sig(N, ho, ho, c, cin, R=R, stride=2, tr=1, acc=acc))
            s += conv3x3_forms(N, ho, ho, c, c, groups=T)[:3]
            s.append(sig(N, ho, ho, c, c, bnr=1, groups=T))
        else:
            s += conv3x3_forms(N, ho, ho, c, c, groups=T)
        s += [sig(N, ho, ho, c, c, acc=1)]
        # PK-map fusion 1x1 (C + 8 channels in), and its dgrad
        s += [sig(N, ho, ho, c + 8, c, R=1, bias=1, dcs=2 * c), sig(N, ho, ho, c, c + 8, R=1)]
        # LSTM steps over B * ho * ho pixels: forward cell, backward recompute, dh, hoisted dx, [dx | dh]
        s += [sig(B, ho, ho, 2 * c, 4 * c, R=1, bias=1, lstm=1, dcs=2 * c),
              sig(B, ho, ho, 2 * c, 4 * c, R=1, bias=1, lstm=2, dcs=2 * c),
              sig(B, ho, ho, 4 * c, c, R=1, dcs=2 * c), sig(N, ho, ho, 4 * c, c, R=1, dcs=2 * c),
              sig(B, ho, ho, 4 * c, 2 * c, R=1)]
        cin, h = c, ho
    # decoder blocks (batch B): ConvT 3x3 / stride 2 into the concat, 1x1 fusion, residual block
    for c in (512, 256, 128):
        co = c // 2
        s += [sig(B, h, h, c, co, stride=2, tr=1, bias=1, dcs=c), sig(B, h, h, c, co, stride=2, tr=1, bias=1),
              sig(B, 2 * h, 2 * h, co, c, stride=2, scs=c), sig(B, 2 * h, 2 * h, co, c, stride=2)]
        h *= 2
        s += [sig(B, h, h, c, co, R=1, bias=1), sig(B, h, h, co, c, R=1)]
        s += conv3x3_forms(B, h, h, co, co)
    s += [sig(B, h, h, 64, 64, stride=2, tr=1, bias=1), sig(B, 2 * h, 2 * h, 64, 64, stride=2)]
    s += conv3x3_forms(B, 2 * h, 2 * h, 64, 64)
    return s


def small_signatures():
    """tests/test_surface_cpu.py's query shapes and the smallest shapes of each case of
    tests/test_kernels_gpu.py (there as launches; here their routes)."""
    s = []
    for N, Hs, Ws, Cs, Hd, Wd, R, S, st, pad, tr, nout, groups in [
            (64, 256, 256, 64, 256, 256, 3, 3, 1, 1, 0, 64, 1), (64, 16, 16, 512, 16, 16, 3, 3, 1, 1, 0, 1024, 1),
            (128, 8, 8, 512, 8, 8, 3, 3, 1, 1, 0, 512, 8), (128, 16, 16, 256, 8, 8, 3, 3, 2, 1, 0, 512, 8),
            (16, 8, 8, 512, 16, 16, 3, 3, 2, 1, 1, 256, 1), (64, 256, 256, 8, 256, 256, 3, 3, 1, 1, 0, 64, 1)]:
        for stats, bnr in ((0, 0), (1, 0), (0, 1)):
            s.append(sig(N, Hs, Ws, Cs, nout, R=R, stride=st, pad=pad, tr=tr, Hd=Hd, Wd=Wd, groups=groups,
                         stats=stats, bnr=bnr))
    for N, H, W, Cs, nout, groups in [(128, 16, 16, 256, 256, 8), (4, 16, 16, 64, 128, 2), (3, 16, 16, 64, 64, 3),
                                      (128, 8, 8, 512, 512, 8), (8, 8, 8, 256, 128, 2), (6, 8, 8, 256, 128, 2),
                                      (64, 32, 32, 512, 512, 1)]:
        s += [sig(N, H, W, Cs, nout, groups=groups, stats=st) for st in (0, 1)]
    # test_conv_forward_stats_and_dgrad (W = H + 2) and its transposed dgrad
    for cin, cout, H, st, R in [(64, 128, 16, 1, 3), (8, 64, 32, 1, 3), (8, 64, 20, 2, 7), (8, 128, 18, 1, 3),
                                (128, 64, 16, 1, 3), (64, 128, 16, 2, 3), (64, 128, 16, 2, 1), (32, 32, 8, 1, 3),
                                (256, 512, 8, 1, 3)]:
        Ho, Wo = (H - 1) // st + 1, (H + 1) // st + 1
        s += [sig(2, H, H + 2, cin, cout, R=R, stride=st, bias=1, stats=1, Hd=Ho, Wd=Wo),
              sig(2, Ho, Wo, cout, cin, R=R, stride=st, tr=1, Hd=H, Wd=H + 2)]
    # test_strided_dgrad_parity_classes
    for n, cin, cout, H, W, R, acc in [(2, 64, 128, 15, 17, 3, 0), (4, 128, 256, 32, 32, 3, 1),
                                       (2, 64, 128, 13, 16, 1, 0), (2, 256, 64, 8, 9, 1, 1), (3, 32, 64, 9, 11, 3, 0)]:
        s.append(sig(n, (H - 1) // 2 + 1, (W - 1) // 2 + 1, cout, cin, R=R, stride=2, tr=1, acc=acc, Hd=H, Wd=W))
    # test_conv3x3_halo (+ W just under / at 32, Nout 64 / 128 / 256 / 320, Cs not a multiple of 32,
    # an odd number of 16 x 16 images, N not a multiple of 4 at 8 x 8)
    halo = [(2, 64, 64, 37, 70, 1, 0, 64), (4, 128, 128, 64, 64, 2, 0, 192), (2, 32, 128, 20, 96, 1, 1, 32),
            (1, 96, 64, 64, 80, 1, 0, 96), (4, 64, 128, 16, 16, 2, 0, 64), (2, 128, 64, 21, 24, 1, 1, 128),
            (6, 256, 256, 16, 16, 3, 1, 320), (3, 64, 64, 16, 16, 3, 0, 64), (16, 512, 512, 8, 8, 4, 0, 512),
            (8, 256, 128, 8, 8, 2, 1, 320), (2, 128, 256, 37, 70, 1, 0, 128), (4, 256, 128, 32, 64, 2, 1, 320),
            (3, 64, 384, 40, 33, 3, 0, 64), (4, 1024, 512, 16, 16, 2, 0, 1024)]
    halo += [(2, 64, nout, 16, W, 1, 0, 64) for W in (31, 32) for nout in (64, 128, 256, 320)]
    halo += [(2, 64, nout, 16, 16, 1, 0, 64) for nout in (256, 320)]
    halo += [(2, 48, 64, 16, 32, 1, 0, 48), (2, 40, 128, 8, 8, 1, 0, 40), (6, 64, 64, 16, 16, 2, 0, 64),
             (6, 256, 512, 16, 16, 2, 0, 256), (6, 256, 128, 8, 8, 2, 0, 256), (8, 256, 128, 8, 8, 4, 0, 256)]
    for n, cin, cout, H, W, groups, acc, xcs in halo:
        s += [sig(n, H, W, cin, cout, bias=1, stats=1, groups=groups, acc=acc, scs=xcs),
              sig(n, H, W, cin, cout, bias=1, groups=groups, acc=acc, scs=xcs),
              sig(n, H, W, cout, cin), sig(n, H, W, cout, cin, bnr=1, groups=groups),
              sig(n, H, W, cout, cin, bnr=1, groups=groups, acc=1), sig(n, H, W, cout, cin, stats=1)]
    # test_conv3x3_8channel_input: wider destination; and a destination that is not 16-byte aligned
    for n, H, W, groups, dcs in [(6, 20, 36, 3, 64), (4, 64, 64, 2, 96), (2, 16, 16, 1, 64)]:
        s += [sig(n, H, W, 8, 64, bias=1, stats=1, groups=groups, dcs=dcs),
              sig(n, H, W, 8, 64, bias=1, stats=1, groups=groups, dcs=dcs, dst_low=8),
              sig(n, H, W, 8, 64, bias=1, stats=1, groups=groups, dcs=68)]
    s += [sig(2, 16, 16, 8, 128, bias=1, stats=1), sig(2, 16, 16, 8, 64, R=1, bias=1), sig(2, 16, 16, 8, 64, acc=1)]
    # test_conv_splitk; with a misaligned destination the split-K fold is not taken
    for n, cin, cout, H, W, R, groups, acc in [(16, 512, 512, 8, 8, 3, 8, 0), (4, 2048, 1024, 8, 8, 1, 1, 0),
                                               (8, 256, 256, 8, 12, 3, 2, 1)]:
        s += [sig(n, H, W, cin, cout, R=R, bias=1, stats=1, groups=groups, acc=acc),
              sig(n, H, W, cin, cout, R=R, bias=1, groups=groups, acc=acc, dst_low=8, dcs=cout + 4)]
    # test_conv_into_concat_slice, test_convT2x2_fwd_dgrad_wgrad, test_convT3x3_s2_gather, smoke()'s base_c = 8
    s.append(sig(2, 8, 8, 64, 32, scs=72, dcs=96))
    for cin, cout, h in [(128, 64, 8), (1024, 512, 4), (64, 32, 16), (256, 128, 8)]:
        s += [sig(2, h, h, cin, 4 * cout, R=1, bias=1, scatter=1, dcs=2 * cout),
              sig(2, 2 * h, 2 * h, cout, cin, R=2, stride=2, pad=0, Hd=h, Wd=h)]
    s += [sig(2, 8, 8, 128, 64, stride=2, tr=1, bias=1), sig(2, 16, 16, 64, 128, stride=2)]
    s += unet_signatures(1, 32, 8, 8)
    return s


def edge_signatures():
    """Routes no model layer above takes but a launch can: the halo tiles that do not defer (one
    image per statistics group and many items per workgroup), ConvT scatters on the 128 x 128 and
    512 x 64 tiles, and the register-staged kernel in every form -- Cs not a multiple of 32, or a
    source past the 4 GiB buffer descriptor (64 x 256 x 256 x 512)."""
    s = [sig(1024, 32, 32, 64, 64, bias=1, stats=1, groups=1024), sig(1024, 32, 32, 64, 64, bnr=1, groups=1024),
         sig(2, 8, 8, 96, 4 * 48, R=1, bias=1, scatter=1), sig(2, 16, 16, 64, 4 * 16, R=1, bias=1, scatter=1)]
    for nout in (48, 128):
        s += [sig(2, 8, 8, 48, nout, stride=2, tr=1), sig(2, 8, 8, 48, nout, R=1, scatter=1), sig(2, 8, 8, 48, nout)]
    for nout in (64, 128):
        s += [sig(64, 256, 256, 512, nout), sig(64, 256, 256, 512, nout, R=1, scatter=1),
              sig(64, 128, 128, 2048, nout, stride=2, tr=1)]
    s += [sig(64, 256, 256, 512, 1024, R=1, bias=1, lstm=lstm) for lstm in (1, 2)]
    return s


def signatures():
    s = unet_signatures() + small_signatures() + edge_signatures()
    for B, T, HW in ((16, 8, 256), (16, 16, 256), (4, 32, 512)):     # bench cfg3, cfg4, cfg5
        s += stf_signatures(B, T, HW)
    return sorted(set(s))


def query(lib, s):
    """The recorded answers for one signature from a loaded library (host-only calls)."""
    from stfunet import _lib
    d = dict(zip(FIELDS, s))
    fake = 1 << 32                                         # the queries read no memory
    g = _lib.ConvGeom(d["N"], d["Hs"], d["Ws"], d["Cs"], d["scs"], d["Hd"], d["Wd"], d["R"], d["S"], d["stride"],
                      d["pad"], d["transposed"])
    M = d["N"] * d["Hd"] * d["Wd"]
    a = _lib.IgemmArgs(g, fake, 2 * fake, d["Nout"], 3 * fake + d["dst_low"], d["dcs"], fake if d["bias"] else None,
                       None, d["scatter"], M // d["groups"] if d["groups"] > 1 else 0, d["acc"], None)
    if d["lstm"]:
        epi = _lib.LstmEpi(fake, fake, fake, d["dcs"], None, int(d["lstm"] == 2), fake, d["dcs"], fake, fake, fake)
        a.lstm = ctypes.pointer(epi)
    if d["bnr"]:
        bnr = _lib.BnrEpi(4 * fake, d["Nout"], fake, fake, fake, fake, 1, fake)
        a.bnr = ctypes.pointer(bnr)
    r = ctypes.byref(a)
    unset = (lib.stf_igemm_stat_tiles(r), lib.stf_igemm_bnr_tiles(r), lib.stf_igemm_ws_bytes(r))
    name_unset = lib.stf_igemm_kernel_name(r).decode()
    a.stats = 5 * fake
    name = lib.stf_igemm_kernel_name(r).decode() if d["stats"] else name_unset
    return [name, unset[0], unset[1], unset[2], lib.stf_igemm_ws_bytes(r)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="hash of the commit whose build is loaded (STF_LIB)")
    args = ap.parse_args()
    for p in (REPO, os.path.join(REPO, "stf-unet_amd")):
        sys.path.insert(0, p)
    import torch
    from stfunet import _lib
    sigs = signatures()
    rows = [query(_lib.load(torch.bfloat16), s) for s in sigs]
    assert rows == [query(_lib.load(torch.float16), s) for s in sigs], "the two storage builds disagree"
    with open(OUT, "w") as f:
        f.write('{"commit": "%s", "cus": 256,\n "fields": %s,\n "results": %s,\n "routes": [\n' %
                (args.commit, json.dumps(FIELDS), json.dumps(RESULTS)))
        f.write(",\n".join("  " + json.dumps([list(s), r]) for s, r in zip(sigs, rows)))
        f.write("\n ]}\n")
    names = sorted({r[0] for r in rows})
    print(f"{len(sigs)} signatures, {len(names)} kernel names from {_lib.LIB_PATH}")
    for n in names:
        print("  ", n)


if __name__ == "__main__":
    main()
