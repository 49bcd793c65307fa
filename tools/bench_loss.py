"""Loss-kernel pair timing at the cfg2 shape (64 x 2 x 256 x 256 logits): the option entry points
(stf_loss_opt_fwd + stf_loss_opt_bwd, the OPT=true kernels: class weights, ignore_index 255, Dice
on) against the default pair (stf_loss_fwd + stf_loss_bwd, OPT=false) on the same logits and
target, and once more on a target with a padded band of 255; interleaved in one process, HIP
events over --reps launches per round after warm-up.

    python tools/bench_loss.py [--base-lib PATH] [--reps 100] [--rounds 7] [--out FILE]

--base-lib: another build of the library (e.g. the parent commit's libstfunet_hip.so).  Its
default pair and its option pair are timed in the same rounds beside this tree's, so each pair
is compared like for like against the base build's own round-to-round spread.  Prints per-round
times, then one JSON line with the medians, minima and spreads (us per fwd + bwd pair) and the
ratios.

    python tools/bench_loss.py --classes 4,8,16 [--channels 64] [--base-lib PATH] [--out FILE]

--classes: the four full-resolution passes of the many-class kernels instead (stf_loss_mc_fwd, stf_loss_mc_bwd,
stf_head_mc_fwd, stf_head_mc_bwd) at the shape's N, H, W and --channels head inputs, one JSON line per class
count with us per launch and TB/s on algorithmic bytes (loss fwd 4K+8, loss bwd 8K+8, head fwd 2C+4K, head bwd
4C+4K bytes per pixel).  For K <= 4 the templated siblings (stf_loss_fwd/bwd, stf_head_fwd/bwd; of --base-lib
when given) are timed in the same rounds and the line carries the four mc / sibling ratios.

    python tools/bench_loss.py --focal [--classes 8] [--out FILE]

--focal: the focal / Tversky pair (stf_loss_ft_fwd + stf_loss_ft_bwd, gamma = 2, (alpha, beta) = (0.3, 0.7)) against
the option pair of the same build on the same logits, target (a W/8 band of 255) and class weights, interleaved:
stf_loss_opt_* at the shape's K <= 4, stf_loss_mc_* for each count of --classes.  One JSON line per class count
with us per launch, TB/s on the same byte model (fwd 4K+8, bwd 8K+8 bytes per pixel) and the ft / option ratios.

    python tools/bench_loss.py --pair mc|ft --base-lib PATH [--shape 64,8,256,256] [--out FILE]

--pair: the many-class (stf_loss_mc_*) or the focal / Tversky (stf_loss_ft_*, gamma = 2, (0.3, 0.7)) fwd + bwd pair
of --base-lib's build and of this tree's on the same inputs (class weights, a W/8 band of 255), in turn inside each
round.  One JSON line with every round's times, the medians, each build's own spread and new / base.

    python tools/bench_loss.py --boundary [--base-lib PATH] [--out FILE]

--boundary: the boundary loss at 64 x 2 x 256 x 256 and 16 x 2 x 512 x 512 on lesion-like targets (one ellipse
of 0.5-2 % of the pixels per image, every eighth image empty), one JSON line per shape.  The map: stf_sdf
against the route the build of --base-lib (default: this one) has to it, stf_edt_sq with where = ones twice per
class (sites = G, sites = not G) on site masks made beforehand, the select / sqrt glue left out; in turn
inside each round, with the base route's own spread.  The term: stf_bloss_fwd + stf_bloss_bwd, and the default
criterion pair with and without them."""
import argparse
import ctypes
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "stf-unet_amd")]
import torch  # noqa: E402
from stfunet import _lib  # noqa: E402
from stfunet._lib import stream  # noqa: E402
from stfunet.nhwc import _p  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--base-lib", default=None)
ap.add_argument("--reps", type=int, default=100)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--shape", default="64,2,256,256")
ap.add_argument("--out", default=None)
ap.add_argument("--classes", default=None, help="comma-separated class counts: time the many-class passes")
ap.add_argument("--channels", type=int, default=64)
ap.add_argument("--focal", action="store_true", help="time the focal / Tversky pair against the option pair")
ap.add_argument("--pair", choices=("mc", "ft"), default=None,
                help="A/B of the many-class or the focal / Tversky pair against --base-lib's")
ap.add_argument("--boundary", action="store_true", help="time the boundary loss's maps and term")
args = ap.parse_args()

N, K, H, W = (int(v) for v in args.shape.split(","))
dev = "cuda"
lib = _lib.load()
base = lib
if args.base_lib:
    base = ctypes.CDLL(os.path.abspath(args.base_lib))
    for name in ("stf_loss_scratch_floats", "stf_loss_fwd", "stf_loss_bwd", "stf_loss_opt_scratch_floats",
                 "stf_loss_opt_fwd", "stf_loss_opt_bwd"):
        getattr(base, name).restype, getattr(base, name).argtypes = _lib._SIGS[name]


def focal_passes(K):
    """Median us per launch of the option pair (opt for K <= 4, else mc) and of the focal / Tversky pair."""
    sib = "opt" if K <= 4 else "mc"
    gen = torch.Generator(device=dev).manual_seed(K)
    x = torch.randn(N, K, H, W, device=dev, generator=gen) * 2
    t = (torch.rand(N, H, W, device=dev, generator=gen) > 0.9).long() * (K - 1)
    t[:, :, W - W // 8:] = 255                           # a collate-padded band
    w = torch.linspace(0.5, 2.0, K, device=dev)
    trm = torch.empty(lib.stf_loss_ft_scratch_floats(N, K), device=dev)
    out1, one, dx = torch.empty(1, device=dev), torch.ones(1, device=dev), torch.empty_like(x)
    head, ft = (_p(x), _p(t), N, H, W, K, _p(w), 255, 1), (2.0, 0.3, 0.7)
    sfwd, sbwd = getattr(lib, f"stf_loss_{sib}_fwd"), getattr(lib, f"stf_loss_{sib}_bwd")
    passes = {      # fwd first: it writes the terms the bwd reads
        "fwd": (lambda: sfwd(*head, _p(trm), _p(out1), stream()),
                lambda: lib.stf_loss_ft_fwd(*head, *ft, _p(trm), _p(out1), stream()), 4 * K + 8),
        "bwd": (lambda: sbwd(*head, _p(trm), _p(one), _p(dx), stream()),
                lambda: lib.stf_loss_ft_bwd(*head, *ft, _p(trm), _p(one), _p(dx), stream()), 8 * K + 8),
    }

    def timeit(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            rc = fn()
        e1.record()
        torch.cuda.synchronize()
        if rc != 0:
            raise RuntimeError(f"launch failed: {rc}")
        return e0.elapsed_time(e1) / args.reps * 1e3

    P = N * H * W
    res = {"shape": [N, K, H, W], "reps": args.reps, "rounds": args.rounds, "option_pair": f"stf_loss_{sib}",
           "gamma": ft[0], "tversky": ft[1:]}
    for name, (old, new, bpp) in passes.items():
        for fn in (old, new, old, new):
            timeit(fn)
        times = [[timeit(old), timeit(new)] for _ in range(args.rounds)]
        o, m = statistics.median(r[0] for r in times), statistics.median(r[1] for r in times)
        res[name] = {"option_us": o, "option_min_us": min(r[0] for r in times), "option_TBps": bpp * P / o * 1e-6,
                     "ft_us": m, "ft_min_us": min(r[1] for r in times), "ft_TBps": bpp * P / m * 1e-6,
                     "ft_over_option": m / o}
    res["pair"] = {"option_us": res["fwd"]["option_us"] + res["bwd"]["option_us"],
                   "ft_us": res["fwd"]["ft_us"] + res["bwd"]["ft_us"]}
    res["pair"]["ft_over_option"] = res["pair"]["ft_us"] / res["pair"]["option_us"]
    return res


def many_class_passes(K):
    """Median us per launch of the four passes at K classes, mc and (K <= 4) templated sibling, interleaved."""
    C, P = args.channels, N * H * W
    gen = torch.Generator(device=dev).manual_seed(K)
    x = torch.randn(N, K, H, W, device=dev, generator=gen) * 2
    t = torch.randint(0, K, (N, H, W), device=dev, generator=gen)
    y = torch.randn(P * C, device=dev, generator=gen).to(torch.bfloat16)
    vec = [torch.rand(C, device=dev, generator=gen) + 0.5 for _ in range(4)]       # scale, shift, mean, invstd
    w, b = torch.randn(K * C, device=dev, generator=gen) / 8, torch.randn(K, device=dev, generator=gen)
    trm = torch.empty(lib.stf_loss_mc_scratch_floats(N, K), device=dev)
    out1, one, dx = torch.empty(1, device=dev), torch.ones(1, device=dev), torch.empty_like(x)
    tiles = lib.stf_head_tiles(N, H, W, C)
    gout = torch.empty(P * C, device=dev, dtype=torch.bfloat16)
    bnp, hp = torch.empty(tiles * 2 * C, device=dev), torch.empty((tiles + 1) * K * (C + 1), device=dev)
    dw, db = torch.empty(K * C, device=dev), torch.empty(K, device=dev)
    sc, sh, mu, iv = (_p(v) for v in vec)
    head_b = (_p(dx), _p(y), N, H, W, C, sc, sh, mu, iv, _p(w), K, _p(gout), _p(bnp), _p(hp), _p(dw), _p(db))
    passes = {
        "loss_fwd": (lambda: lib.stf_loss_mc_fwd(_p(x), _p(t), N, H, W, K, None, -100, 1, _p(trm), _p(out1), stream()),
                     lambda: base.stf_loss_fwd(_p(x), _p(t), N, H, W, K, _p(trm), _p(out1), stream()), 4 * K + 8),
        "loss_bwd": (lambda: lib.stf_loss_mc_bwd(_p(x), _p(t), N, H, W, K, None, -100, 1, _p(trm), _p(one), _p(dx),
                                                 stream()),
                     lambda: base.stf_loss_bwd(_p(x), _p(t), N, H, W, K, _p(trm), _p(one), _p(dx), stream()),
                     8 * K + 8),
        "head_fwd": (lambda: lib.stf_head_mc_fwd(_p(y), N, H, W, C, sc, sh, _p(w), _p(b), K, _p(x), stream()),
                     lambda: base.stf_head_fwd(_p(y), N, H, W, C, sc, sh, _p(w), _p(b), K, _p(x), stream()),
                     2 * C + 4 * K),
        "head_bwd": (lambda: lib.stf_head_mc_bwd(*head_b, stream()), lambda: base.stf_head_bwd(*head_b, stream()),
                     4 * C + 4 * K),
    }

    def timeit(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            rc = fn()
        e1.record()
        torch.cuda.synchronize()
        if rc != 0:
            raise RuntimeError(f"launch failed: {rc}")
        return e0.elapsed_time(e1) / args.reps * 1e3

    sib = K <= 4
    res = {"shape": [N, K, H, W], "channels": C, "reps": args.reps, "rounds": args.rounds,
           "base_lib": args.base_lib or "in-tree"}
    for name, (mc, old, bpp) in passes.items():      # loss_fwd first: it writes the terms loss_bwd reads
        fns = [mc, old] if sib else [mc]
        for fn in fns:
            timeit(fn)
        times = [[timeit(fn) for fn in fns] for _ in range(args.rounds)]
        m = statistics.median(r[0] for r in times)
        res[name] = {"mc_us": m, "mc_min_us": min(r[0] for r in times), "TBps": bpp * P / m * 1e-6}
        if sib:
            o = statistics.median(r[1] for r in times)
            res[name].update({"sibling_us": o, "sibling_min_us": min(r[1] for r in times), "mc_over_sibling": m / o})
    return res


def pair_ab(fam):
    """The fwd + bwd pair of stf_loss_<fam>_* (mc or ft) of the base build and of this tree, in turn inside
    each round: medians, each build's own round-to-round spread (max - min) / median, and new / base."""
    gen = torch.Generator(device=dev).manual_seed(K)
    x = torch.randn(N, K, H, W, device=dev, generator=gen) * 2
    t = (torch.rand(N, H, W, device=dev, generator=gen) > 0.9).long() * (K - 1)
    t[:, :, W - W // 8:] = 255                           # a collate-padded band
    w = torch.linspace(0.5, 2.0, K, device=dev)
    trm = torch.empty(lib.stf_loss_mc_scratch_floats(N, K), device=dev)
    out1, one, dx = torch.empty(1, device=dev), torch.ones(1, device=dev), torch.empty_like(x)
    opts = (_p(x), _p(t), N, H, W, K, _p(w), 255, 1) + ((2.0, 0.3, 0.7) if fam == "ft" else ())

    def pair_on(l):
        fwd, bwd = getattr(l, f"stf_loss_{fam}_fwd"), getattr(l, f"stf_loss_{fam}_bwd")

        def run():
            rc = fwd(*opts, _p(trm), _p(out1), stream()) or bwd(*opts, _p(trm), _p(one), _p(dx), stream())
            if rc != 0:
                raise RuntimeError(f"launch failed: {rc}")
        return run

    def timeit(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.reps * 1e3

    old, new = pair_on(base), pair_on(lib)
    for fn in (old, new, old, new):
        timeit(fn)
    times = [[timeit(old), timeit(new)] for _ in range(args.rounds)]
    tb, tn = [r[0] for r in times], [r[1] for r in times]
    mb, mn = statistics.median(tb), statistics.median(tn)
    return {"pair": f"stf_loss_{fam}", "shape": [N, K, H, W], "reps": args.reps, "rounds": args.rounds,
            "base_lib": args.base_lib, "base_us": tb, "new_us": tn,
            "base_pair_us": {"median": mb, "min": min(tb), "spread": (max(tb) - min(tb)) / mb},
            "new_pair_us": {"median": mn, "min": min(tn), "spread": (max(tn) - min(tn)) / mn},
            "new_over_base": mn / mb}


def lesion_targets(n, h, w, seed):
    """One ellipse of 0.5-2 % of the pixels per image, anywhere inside it; every eighth image empty."""
    g = torch.Generator().manual_seed(seed)
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    t = torch.zeros(n, h, w, dtype=torch.long)
    for i in range(n):
        if i % 8 == 7:
            continue
        area = (0.005 + 0.015 * torch.rand(1, generator=g).item()) * h * w
        ratio = 0.5 + torch.rand(1, generator=g).item()
        a = (area / 3.141592653589793 * ratio) ** 0.5
        b = area / 3.141592653589793 / a
        cy = a + (h - 2 * a) * torch.rand(1, generator=g).item()
        cx = b + (w - 2 * b) * torch.rand(1, generator=g).item()
        t[i] = ((((ys - cy) / a) ** 2 + ((xs - cx) / b) ** 2) <= 1).long()
    return t


def boundary_leg(n, k, h, w):
    from stfunet import _lib as L
    t = lesion_targets(n, h, w, 7 * h + n).to(dev)
    gen = torch.Generator(device=dev).manual_seed(h)
    x = torch.randn(n, k, h, w, device=dev, generator=gen) * 2
    phi = torch.empty(n, k - 1, h, w, device=dev)
    scr = torch.empty((lib.stf_sdf_scratch_bytes(n, h, w, k) + 7) // 8, dtype=torch.int64, device=dev)
    sites = [(t == c).to(torch.uint8) for c in range(1, k)]
    sites += [1 - m for m in sites]
    ones = torch.ones(n, h, w, dtype=torch.uint8, device=dev)
    d2 = torch.empty(n, h, w, dtype=torch.int32, device=dev)
    for name in ("stf_boundary_scratch_bytes", "stf_edt_sq"):
        getattr(base, name).restype, getattr(base, name).argtypes = L._SIGS[name]
    escr = torch.empty((base.stf_boundary_scratch_bytes(n, h, w) + 7) // 8, dtype=torch.int64, device=dev)
    trm = torch.empty(lib.stf_loss_scratch_floats(n, k), device=dev)
    part = torch.empty(lib.stf_bloss_scratch_floats(n), device=dev)
    out1, one, dx = torch.zeros(1, device=dev), torch.ones(1, device=dev), torch.zeros_like(x)

    def chk(rc):
        if rc != 0:
            raise RuntimeError(f"launch failed: {rc}")

    def sdf():
        chk(lib.stf_sdf(_p(t), n, h, w, k, -1, _p(phi), _p(scr), stream()))

    def edt_route():
        for m in sites:
            chk(base.stf_edt_sq(_p(m), _p(ones), n, h, w, _p(d2), _p(escr), stream()))

    def term():
        chk(lib.stf_bloss_fwd(_p(x), _p(t), _p(phi), n, h, w, k, -100, 0.01, _p(part), _p(out1), stream()))
        chk(lib.stf_bloss_bwd(_p(x), _p(t), _p(phi), n, h, w, k, -100, 0.01, _p(one), _p(part) + 4, _p(dx), stream()))

    def crit():
        chk(base.stf_loss_fwd(_p(x), _p(t), n, h, w, k, _p(trm), _p(out1), stream()))
        chk(base.stf_loss_bwd(_p(x), _p(t), n, h, w, k, _p(trm), _p(one), _p(dx), stream()))

    def crit_boundary():
        chk(lib.stf_loss_fwd(_p(x), _p(t), n, h, w, k, _p(trm), _p(out1), stream()))
        sdf()
        chk(lib.stf_bloss_fwd(_p(x), _p(t), _p(phi), n, h, w, k, -100, 0.01, _p(part), _p(out1), stream()))
        chk(lib.stf_loss_bwd(_p(x), _p(t), n, h, w, k, _p(trm), _p(one), _p(dx), stream()))
        chk(lib.stf_bloss_bwd(_p(x), _p(t), _p(phi), n, h, w, k, -100, 0.01, _p(one), _p(part) + 4, _p(dx), stream()))

    def timeit(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps * 1e3

    fns = {"sdf_us": sdf, "edt_route_us": edt_route, "term_pair_us": term, "criterion_us": crit,
           "criterion_boundary_us": crit_boundary}
    reps = max(1, args.reps // 5)
    for fn in fns.values():
        timeit(fn, 3)
    rounds = {key: [] for key in fns}
    for _ in range(args.rounds):
        for key, fn in fns.items():
            rounds[key].append(timeit(fn, reps))
    res = {"shape": [n, k, h, w], "reps": reps, "rounds": args.rounds, "base_lib": args.base_lib or "in-tree",
           "build": L.build_info(), "foreground_fraction": (t > 0).float().mean().item()}
    for key, v in rounds.items():
        med = statistics.median(v)
        res[key] = {"median": med, "min": min(v), "spread": (max(v) - min(v)) / med, "rounds": v}
    res["sdf_over_edt_route"] = res["sdf_us"]["median"] / res["edt_route_us"]["median"]
    res["sdf_ns_per_pixel"] = res["sdf_us"]["median"] * 1e3 / (n * h * w)
    res["boundary_added_us"] = res["criterion_boundary_us"]["median"] - res["criterion_us"]["median"]
    return res


if args.boundary:
    lines = [json.dumps(boundary_leg(*shape)) for shape in ((64, 2, 256, 256), (16, 2, 512, 512))]
    print("\n".join(lines))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    sys.exit(0)

if args.pair:
    if not args.base_lib:
        sys.exit("--pair needs --base-lib")
    for name in (f"stf_loss_{args.pair}_fwd", f"stf_loss_{args.pair}_bwd"):
        getattr(base, name).restype, getattr(base, name).argtypes = _lib._SIGS[name]
    line = json.dumps(pair_ab(args.pair))
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    sys.exit(0)

if args.focal:
    lines =[json.dumps(focal_passes(int(k))) for k in (args.classes.split(",") if args.classes else [K])]
    print("\n".join(lines))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    sys.exit(0)

if args.classes:
    for name in ("stf_head_fwd", "stf_head_bwd"):
        getattr(base, name).restype, getattr(base, name).argtypes = _lib._SIGS[name]
    lines = [json.dumps(many_class_passes(int(k))) for k in args.classes.split(",")]
    print("\n".join(lines))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    sys.exit(0)

g = torch.Generator(device=dev).manual_seed(0)
logits = torch.randn(N, K, H, W, device=dev, generator=g) * 2
target = (torch.rand(N, H, W, device=dev, generator=g) > 0.9).long()
padded = target.clone()
padded[:, :, W - W // 8:] = 255                       # a collate-padded band
weight = torch.linspace(0.5, 2.0, K, device=dev)
terms = torch.empty(max(lib.stf_loss_opt_scratch_floats(N, K), base.stf_loss_opt_scratch_floats(N, K)), device=dev)
loss, go, dl = torch.empty(1, device=dev), torch.ones(1, device=dev), torch.empty_like(logits)


def check(rc):
    if rc != 0:
        raise RuntimeError(f"launch failed: {rc}")


def default_on(l):
    s = stream()
    check(l.stf_loss_fwd(_p(logits), _p(target), N, H, W, K, _p(terms), _p(loss), s))
    check(l.stf_loss_bwd(_p(logits), _p(target), N, H, W, K, _p(terms), _p(go), _p(dl), s))


def opt_on(l, t):
    s = stream()
    check(l.stf_loss_opt_fwd(_p(logits), _p(t), N, H, W, K, _p(weight), 255, 1, _p(terms), _p(loss), s))
    check(l.stf_loss_opt_bwd(_p(logits), _p(t), N, H, W, K, _p(weight), 255, 1, _p(terms), _p(go), _p(dl), s))


def base_pair():
    default_on(base)


def opt_pair():            # the default pair's own target: like for like
    opt_on(lib, target)


def opt_pair_padded():     # a W/8 band of 255, as a collated mixed-size batch has
    opt_on(lib, padded)


# with --base-lib: this tree's default pair and the base build's option pair, for the per-pair A/B
EXTRA = {"new_default_pair_us": lambda: default_on(lib), "base_option_pair_us": lambda: opt_on(base, target)}


def timeit(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / args.reps * 1e3     # us per pair


extra = EXTRA if args.base_lib else {}
for fn in (base_pair, opt_pair, opt_pair_padded, *extra.values()):
    for _ in range(20):
        fn()
torch.cuda.synchronize()
tb, to, tp, tx = [], [], [], {k: [] for k in extra}
for r in range(args.rounds):
    tb.append(timeit(base_pair))
    to.append(timeit(opt_pair))
    tp.append(timeit(opt_pair_padded))
    for k, fn in extra.items():
        tx[k].append(timeit(fn))
    print(f"round {r}: default pair {tb[-1]:8.2f} us   option pair {to[-1]:8.2f} us   "
          f"option pair, padded target {tp[-1]:8.2f} us" +
          "".join(f"   {k[:-3].replace('_', ' ')} {v[-1]:8.2f} us" for k, v in tx.items()), flush=True)
res = {"shape": [N, K, H, W], "reps": args.reps, "rounds": args.rounds, "base_lib": args.base_lib or "in-tree",
       "default_pair_us": {"median": statistics.median(tb), "min": min(tb)},
       "option_pair_us": {"median": statistics.median(to), "min": min(to)},
       "option_pair_padded_us": {"median": statistics.median(tp), "min": min(tp)},
       "ratio_median": statistics.median(to) / statistics.median(tb)}
if extra:           # new / base per pair, and the base build's own spread (max - min) / median over the rounds
    def spread(t):
        return (max(t) - min(t)) / statistics.median(t)
    res.update({k: {"median": statistics.median(v), "min": min(v), "spread": spread(v)} for k, v in tx.items()})
    res["default_pair_us"]["spread"] = spread(tb)
    res["option_pair_us"]["spread"] = spread(to)
    res["default_new_over_base"] = statistics.median(tx["new_default_pair_us"]) / statistics.median(tb)
    res["option_new_over_base"] = statistics.median(to) / statistics.median(tx["base_option_pair_us"])
line = json.dumps(res)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
