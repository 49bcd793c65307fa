"""Inference outputs at cfg2's output (64 x 2 x 256^2 logits, the shown frame a strided view of the
64 x 8 x 256^2 input): mask + per-image counts + Dice / IoU + overlay on the gfx950 kernels
(stfunet.predict, csrc/predict.hip) against the same results from the torch op sequence of the
reference's test.py:168-169, :71, merge_images and compute_metrics on the same GPU tensors --
once vectorised over the batch and once slice by slice, as the reference's batch-size-1 loop runs it.

The three are timed in turn inside every round (interleaved, same process), with device events
around ``--iters`` calls; the median round is reported.  Bytes: ``algorithmic`` counts every input
and output once (logits, int64 target, frame, mask, overlay); ``moved`` adds what the two-launch
overlay reads again (the frame for the blend after the min / max pass, the mask).  Prints one JSON
line.

    python tools/bench_predict.py [--rule argmax|sigmoid] [--batch 64] [--size 256] [--rounds 7] [--iters 20]

``--boundary`` measures ``stfunet.boundary_metrics`` (csrc/boundary.hip) instead, on two synthetic
mask regimes at the same shape: ``overlap`` (a blob against itself moved by a few pixels: the column
scan ends after a few rows) and ``far_apart`` (two small blobs in opposite corners: every border
pixel scans most of its column, the bad case).  For scale, the same round times ``predict_masks``
with counts (one kernel) and ``overlay`` (two kernels) on the same shape.  Where scipy imports, the
host computation a user would otherwise run (mask to the host, ``binary_erosion``,
``distance_transform_edt``, ``np.percentile`` per slice) is timed on ``--host-images`` images of
each regime.  Prints one JSON line.

``--components`` measures the connected-component post-processing (csrc/ccl.hip) at the same shape on
three inputs: ``realistic`` (one disc per image plus scattered specks), ``percolation`` (a random
mask at density 0.593, the site-percolation threshold: the most merging) and ``checkerboard`` under
connectivity 4 (the most components, no merging).  Per input: ``connected_components``
(stf_ccl_label), ``filter_components`` with a target and ``keep_largest`` (stf_ccl_filter), and for
scale ``boundary_metrics`` on the same mask; once ``predict_masks`` with counts; and the ``predict``
loop (UNet, two batches) with the options off and on.  Prints one JSON line.

``--components3d`` measures the volume-level post-processing (csrc/ccl.hip, volumes) on the same three inputs
stacked as ``--batch`` slices (128 for the record) in 1 and in 8 volumes: ``connected_components_3d``
(stf_ccl3d_label) and ``filter_components_3d`` with a target and ``keep_largest`` (stf_ccl3d_filter) at
connectivity 26 (6 for the checkerboard), next to the 2-D ``connected_components`` /
``filter_components`` on the same slices in the same rounds.  Prints one JSON line.

``--boundary3d`` measures the per-volume boundary metrics (csrc/boundary.hip, volumes) on ``--batch``
slices (128 for the record) cut into 8 volumes, each holding one lesion-sized ellipsoid per side
(``overlap``: the prediction a few voxels off the target; ``far_apart``: in opposite corners), at
spacing (2.5, 0.75, 0.75): ``boundary_metrics_3d`` per call, every launch of one call as the
difference of two replays of a recorded plan (entries 0..i and 0..i-1), ``filter_components_3d``
with ``keep_largest`` on the same volumes for scale, the host computation (scipy on one volume, copy
included) and the ``predict_volumes`` loop (UNet) without and with ``boundary=True``.  Prints one
JSON line.

``--tta`` measures the work mirror test-time augmentation adds around the forwards (csrc/tta.hip) at
the same shape: ``flip_planes`` of the 64 x 8 x 256^2 input per view, and ``stf_tta_accumulate`` on
64 x K x 256^2 logits for K = 2 and 16 (a middle view: K planes read, K planes read and written; the
sigmoid rule: one plane read, one read and written), each as achieved GB/s against those bytes, with
``predict_masks`` (K planes read, one byte written per pixel) in the same rounds for scale.  Then the
``predict_tta`` loop (UNet, one batch, four views) against four plain forwards of the same batch.
Prints one JSON line.

``--lesions`` measures the lesion-level detection metrics (csrc/ccl.hip, the lesion kernels) on the inputs
of ``--components3d`` stacked as ``--batch`` slices (128 for the record) in 1 and in 8 volumes, the target
being the same kind of mask moved by three voxels: ``lesion_metrics_3d`` per call next to what a user
had to do at least without it, two ``connected_components_3d`` calls (one per side, the labels then
still to be copied and looped over on the host), in the same rounds; ``form`` is one elementwise pass
over the same tensors for scale.  Prints one JSON line.

``--froc`` measures lesion confidence and FROC (csrc/ccl.hip, the FROC passes) on the ``--lesions`` inputs with
trained-like scores whose cut at 0.5 is the mask (97 % of the voxels at 0 or 1), against its two yardsticks in
the same interleaved rounds: ``lesion_metrics_3d`` on the same masks and ``score_histogram`` at 256 bins on the
same scores; the ratio reported is froc / (lesions + score_hist).

``--curves`` measures the score histogram (csrc/curves.hip) at the same shape against its yardstick,
``stf_predict_threshold`` with targets on the same tensors (the same 12 bytes read per pixel, and a
mask byte written), both through the C entry points on preallocated outputs and interleaved in every
round, on two score distributions: ``uniform`` and ``trained`` (97 % of the pixels in rows 0 and bins).
Further legs say where the time goes: ``zeros`` (every pixel in row 0: no LDS atomic at all), bins 16 and
4096, the softmax (K = 2) and sigmoid sources, and ``threshold_curves`` of the 64 tables (torch ops).
Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "stf-unet_amd")]
import torch  # noqa: E402

from stfunet import image_metrics, overlay, predict_masks  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rule", default="argmax", choices=["argmax", "sigmoid"])
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--size", type=int, default=256)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--boundary", action="store_true", help="measure boundary_metrics instead")
ap.add_argument("--components", action="store_true", help="measure the connected-component kernels instead")
ap.add_argument("--components3d", action="store_true", help="measure the volume-level component kernels instead")
ap.add_argument("--boundary3d", action="store_true", help="measure the per-volume boundary metrics instead")
ap.add_argument("--lesions", action="store_true", help="measure the lesion-level detection metrics instead")
ap.add_argument("--froc", action="store_true", help="measure lesion confidence and FROC instead")
ap.add_argument("--tta", action="store_true", help="measure the test-time-augmentation kernels instead")
ap.add_argument("--curves", action="store_true", help="measure the score histogram and the curves instead")
ap.add_argument("--host-images", type=int, default=8, help="images per regime of the scipy host timing")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_predict.py measures on the GPU: no ROCm device found")

B, K, H, W = args.batch, 2, args.size, args.size
COLOR, ALPHA, PAINT, SMOOTH = (0, 255, 0), 0.5, 0, 1e-5
torch.manual_seed(0)
logits = torch.randn(B, K, H, W, device="cuda") * 2
target = (torch.rand(B, H, W, device="cuda") < 0.3).long()
inputs = torch.randn(B, 8, H, W, device="cuda")
frames = inputs[:, 0]                                   # the shown frame: a view, batch stride 8 * H * W
color_t = torch.tensor(COLOR, dtype=torch.float32, device="cuda")


def device_path():
    mask, counts = predict_masks(logits, args.rule, 0, 0.5, target=target)
    dice, iou = image_metrics(counts, SMOOTH)
    return mask, dice, iou, overlay(frames, mask, COLOR, ALPHA, PAINT)


def _torch_slices(x, t, f):
    """test.py:168-169 / train_and_eval.py:331, compute_metrics, test.py:71-76 and merge_images on
    device tensors with a leading batch dimension (1 for the slice-by-slice run)."""
    if args.rule == "sigmoid":
        pred = torch.sigmoid(x[:, 0]) > 0.5
    else:
        pred = x.argmax(1) > 0
    tb = t > 0
    inter = (pred & tb).flatten(1).sum(1).double()
    p, g = pred.flatten(1).sum(1).double(), tb.flatten(1).sum(1).double()
    dice = (2 * inter + SMOOTH) / (p + g + SMOOTH)
    iou = (inter + SMOOTH) / (p + g - inter + SMOOTH)
    mn, mx = f.amin((1, 2), keepdim=True), f.amax((1, 2), keepdim=True)
    gray = ((f - mn) / (mx - mn + 1e-8) * 255).to(torch.uint8)
    painted = pred == bool(PAINT)
    blend = (gray.float().unsqueeze(-1) * (1 - ALPHA) + color_t * ALPHA).to(torch.uint8)
    pic = torch.where(painted.unsqueeze(-1), blend, gray.unsqueeze(-1).expand(-1, -1, -1, 3))
    return pred.to(torch.uint8), dice, iou, pic


def torch_batched():
    return _torch_slices(logits, target, frames)


def torch_per_slice():
    out = [_torch_slices(logits[b:b + 1], target[b:b + 1], frames[b:b + 1]) for b in range(B)]
    return tuple(torch.cat(v) for v in zip(*out))


def blobs(regime):
    """(mask uint8, target int64) [B, H, W]: one disk per image and side, seeded."""
    g = torch.Generator().manual_seed(1 if regime == "overlap" else 2)
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    P, T = torch.zeros(B, H, W, dtype=torch.uint8), torch.zeros(B, H, W, dtype=torch.int64)
    for b in range(B):
        if regime == "overlap":
            r = int(torch.randint(H // 12, H // 6, (1,), generator=g))
            cy, cx = (int(v) for v in torch.randint(H // 4, 3 * H // 4, (2,), generator=g))
            dy, dx = (int(v) for v in torch.randint(-4, 5, (2,), generator=g))
            py, px, ty, tx = cy + dy, cx + dx, cy, cx
        else:
            r = max(2, H // 20)
            oy, ox = (int(v) for v in torch.randint(0, H // 16 + 1, (2,), generator=g))
            py, px, ty, tx = r + oy, r + ox, H - 1 - r - oy, W - 1 - r - ox
        P[b] = ((yy - py) ** 2 + (xx - px) ** 2 <= r * r).to(torch.uint8)
        T[b] = ((yy - ty) ** 2 + (xx - tx) ** 2 <= r * r).long()
    return P, T


def scipy_host_us(P, T, n):
    """us per image of the host computation on n images, the device-to-host copy included; None without scipy."""
    try:
        import numpy as np
        from scipy.ndimage import binary_erosion, distance_transform_edt, generate_binary_structure
    except ImportError:
        return None
    import time
    cross = generate_binary_structure(2, 1)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for b in range(n):
        p, t = P[b].cpu().numpy().astype(bool), T[b].cpu().numpy() > 0
        bp, bt = p ^ binary_erosion(p, cross), t ^ binary_erosion(t, cross)
        if bp.any() and bt.any():
            a, c = distance_transform_edt(~bt)[bp], distance_transform_edt(~bp)[bt]
            _ = max(a.max(), c.max()), np.percentile(np.hstack((a, c)), 95), (a.mean() + c.mean()) / 2
    return (time.perf_counter() - t0) * 1e6 / n


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters           # us per call


def component_masks():
    """{name: (mask uint8, target int64, connectivity)} [B, H, W], seeded."""
    g = torch.Generator().manual_seed(3)
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    P, T = torch.zeros(B, H, W, dtype=torch.uint8), torch.zeros(B, H, W, dtype=torch.int64)
    for b in range(B):
        r = int(torch.randint(H // 12, H // 6, (1,), generator=g))
        cy, cx = (int(v) for v in torch.randint(H // 4, 3 * H // 4, (2,), generator=g))
        dy, dx = (int(v) for v in torch.randint(-4, 5, (2,), generator=g))
        P[b] = ((yy - cy - dy) ** 2 + (xx - cx - dx) ** 2 <= r * r).to(torch.uint8)
        T[b] = ((yy - cy) ** 2 + (xx - cx) ** 2 <= r * r).long()
        sy, sx = torch.randint(0, H - 1, (40,), generator=g), torch.randint(0, W - 1, (40,), generator=g)
        P[b, sy, sx] = 1                                   # 40 specks: single pixels, half of them 2 x 2
        P[b, sy[:20] + 1, sx[:20]] = P[b, sy[:20], sx[:20] + 1] = P[b, sy[:20] + 1, sx[:20] + 1] = 1
    perc = (torch.rand(B, H, W, generator=g) < 0.593).to(torch.uint8)
    board = ((yy + xx) % 2 == 0).to(torch.uint8).expand(B, H, W).contiguous()
    return {"realistic": (P, T, 8), "percolation": (perc, T, 8), "checkerboard": (board, T, 4)}


if args.curves:
    from stfunet import threshold_curves
    from stfunet._lib import call, stream
    g = torch.Generator(device="cuda").manual_seed(4)
    uniform = torch.rand(B, 1, H, W, device="cuda", generator=g)
    ends = torch.rand(B, 1, H, W, device="cuda", generator=g)
    trained = torch.where(ends < 0.873, torch.zeros_like(uniform), torch.where(ends > 0.903, torch.ones_like(uniform),
                                                                                 uniform))
    planes = {"uniform": uniform, "trained": trained, "zeros": torch.zeros_like(uniform)}
    mask = torch.empty(B, H, W, dtype=torch.uint8, device="cuda")
    counts = torch.empty(B, 3, dtype=torch.int64, device="cuda")
    hist = torch.empty(B, 2, 4097, dtype=torch.int64, device="cuda")

    def threshold(x):
        call("stf_predict_threshold", x.data_ptr(), target.data_ptr(), B, 1, H * W, 0, 0.5, -1, mask.data_ptr(),
             counts.data_ptr(), stream())

    def histogram(x, bins, source=2, k=1):
        call("stf_score_hist", x.data_ptr(), B, k, H, W, source, 0, target.data_ptr(), -1, -1, bins, hist.data_ptr(),
             stream())

    legs = []
    for name in ("uniform", "trained"):
        x = planes[name]
        legs += [(f"threshold_{name}", lambda x=x: threshold(x)), (f"hist_{name}_b256", lambda x=x: histogram(x, 256)),
                 (f"hist_{name}_b16", lambda x=x: histogram(x, 16)), (f"hist_{name}_b4096", lambda x=x: histogram(x, 4096))]
    legs += [("hist_zeros_b256", lambda: histogram(planes["zeros"], 256)),
             ("hist_softmax_K2_b256", lambda: histogram(logits, 256, 0, 2)),
             ("hist_sigmoid_b256", lambda: histogram(logits, 256, 1, 2))]
    histogram(uniform, 256)
    tables = hist.view(-1)[:B * 2 * 257].view(B, 2, 257).clone()
    legs.append(("threshold_curves_64_tables", lambda: threshold_curves(tables)))
    for _, fn in legs:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    us = {name: [] for name, _ in legs}
    for _ in range(args.rounds):
        for name, fn in legs:
            us[name].append(timed(fn, args.iters))
    med = {k: statistics.median(v) for k, v in us.items()}
    read = B * H * W * 12
    print(json.dumps({
        "tool": "bench_predict", "leg": "curves", "batch": B, "size": [H, W], "rounds": args.rounds, "iters": args.iters,
        "us_per_call": {k: round(v, 1) for k, v in med.items()},
        "us_min_max": {k: [round(min(v), 1), round(max(v), 1)] for k, v in us.items()},
        "read_bytes": read,
        "read_GBps": {k: round(read / v / 1e3, 1) for k, v in med.items() if k.endswith("_b256") and "softmax" not in k},
        "hist_over_threshold": {name: round(med[f"hist_{name}_b256"] / med[f"threshold_{name}"], 3)
                                for name in ("uniform", "trained")},
        "interior_fraction_trained": round(float(((trained > 0) & (trained < 1)).float().mean()), 4),
    }))
    sys.exit(0)

if args.tta:
    import time
    from stfunet import flip_planes, predict_tta
    from stfunet._lib import call, stream
    from stfunet.unet import UNet
    HW = H * W
    legs = []                                             # (name, fn, bytes per call)
    for v in ("none", "w", "h", "hw"):
        legs.append((f"flip_{v}", lambda v=v: flip_planes(inputs, v), 2 * inputs.numel() * 4))
    for k in (2, 16):
        z = torch.randn(B, k, H, W, device="cuda") * 2
        acc = torch.zeros(B, k, H, W, device="cuda")
        acc1 = torch.zeros(B, 1, H, W, device="cuda")

        def accumulate(code, rule=0, z=z, acc=acc, k=k):
            call("stf_tta_accumulate", z.data_ptr(), B, k, H, W, rule, 0, code, 0, 0, acc.data_ptr(), stream())

        for code, v in ((0, "none"), (1, "w"), (3, "hw")):
            legs.append((f"accumulate_K{k}_{v}", lambda code=code, f=accumulate: f(code), 3 * k * B * HW * 4))
        legs.append((f"accumulate_sigmoid_K{k}_hw", lambda f=accumulate, a=acc1: f(3, 1, acc=a), 3 * B * HW * 4))
        legs.append((f"predict_masks_K{k}", lambda z=z: predict_masks(z, "argmax"), B * HW * (4 * k + 1)))
    for _, fn, _ in legs:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    us = {name: [] for name, _, _ in legs}
    for _ in range(args.rounds):
        for name, fn, _ in legs:
            us[name].append(timed(fn, args.iters))
    med = {k: statistics.median(v) for k, v in us.items()}
    nbytes = {name: n for name, _, n in legs}
    model = UNet(in_channels=8, num_classes=2).cuda().eval()
    raw = inputs.view(B, 1, 8, H, W)

    def four_forwards():
        with torch.no_grad():
            for _ in range(4):
                model(inputs)

    def loop_ms(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    loops = {"four_forwards": four_forwards, "predict_tta": lambda: predict_tta(model, [raw], torch.device("cuda")),
             "predict_plain": lambda: predict_tta(model, [raw], torch.device("cuda"), tta=None)}
    for fn in list(loops.values()) * 2:
        loop_ms(fn)
    loop = {k: [] for k in loops}
    for _ in range(args.rounds):
        for k, fn in loops.items():
            loop[k].append(loop_ms(fn))
    lmed = {k: statistics.median(v) for k, v in loop.items()}
    print(json.dumps({
        "tool": "bench_predict", "leg": "tta", "batch": B, "size": [H, W], "rounds": args.rounds, "iters": args.iters,
        "us_per_call": {k: round(v, 1) for k, v in med.items()},
        "us_min_max": {k: [round(min(v), 1), round(max(v), 1)] for k, v in us.items()},
        "bytes": nbytes,
        "GBps": {k: round(nbytes[k] / v / 1e3, 1) for k, v in med.items()},
        "loop_ms": {k: round(v, 3) for k, v in lmed.items()},
        "loop_ms_min_max": {k: [round(min(v), 3), round(max(v), 3)] for k, v in loop.items()},
        "tta_over_four_forwards_ms": round(lmed["predict_tta"] - lmed["four_forwards"], 3),
    }))
    sys.exit(0)

if args.components:
    import time
    from stfunet import boundary_metrics, connected_components, filter_components
    from stfunet.predict import predict
    from stfunet.unet import UNet
    data = {k: (m.cuda(), t.cuda(), c) for k, (m, t, c) in component_masks().items()}
    legs = [("predict_masks_with_counts", lambda: predict_masks(logits, args.rule, 0, 0.5, target=target))]
    for k, (m, t, c) in data.items():
        legs += [(f"label_{k}", lambda m=m, c=c: connected_components(m, c)),
                 (f"filter_{k}", lambda m=m, t=t, c=c: filter_components(m, True, 0, c, target=t)),
                 (f"boundary_{k}", lambda m=m, t=t: boundary_metrics(m, t))]
    for _, fn in legs:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    us = {name: [] for name, _ in legs}
    for _ in range(args.rounds):
        for name, fn in legs:
            us[name].append(timed(fn, args.iters) / B)
    model = UNet(in_channels=8, num_classes=2).cuda()
    loader = [(inputs.view(B, 1, 8, H, W), data["realistic"][1])] * 2

    def loop_ms(flag):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        predict(model, loader, torch.device("cuda"), keep_largest=flag)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for flag in (False, True, False, True):
        loop_ms(flag)
    loop = {False: [], True: []}
    for _ in range(args.rounds):
        for flag in (False, True):
            loop[flag].append(loop_ms(flag))
    loop_med = {k: statistics.median(v) for k, v in loop.items()}
    med = {k: statistics.median(v) for k, v in us.items()}
    num = {k: connected_components(m, c)[1].double() for k, (m, _, c) in data.items()}
    print(json.dumps({
        "tool": "bench_predict", "leg": "components", "shape": [B, H, W], "rounds": args.rounds, "iters": args.iters,
        "us_per_image": {k: round(v, 3) for k, v in med.items()},
        "us_per_image_min_max": {k: [round(min(v), 3), round(max(v), 3)] for k, v in us.items()},
        "mean_components": {k: float(v.mean()) for k, v in num.items()},
        "foreground_fraction": {k: float(m.bool().double().mean()) for k, (m, _, _) in data.items()},
        "predict_loop_ms": {"images": 2 * B, "plain": round(loop_med[False], 3),
                            "keep_largest": round(loop_med[True], 3),
                            "plain_min_max": [round(min(loop[False]), 3), round(max(loop[False]), 3)],
                            "keep_largest_min_max": [round(min(loop[True]), 3), round(max(loop[True]), 3)],
                            "added_us_per_image": round((loop_med[True] - loop_med[False]) * 1e3 / (2 * B), 2)},
    }))
    sys.exit(0)

if args.components3d:
    from stfunet import connected_components, connected_components_3d, filter_components, filter_components_3d
    data = {k: (m.cuda(), t.cuda(), c) for k, (m, t, c) in component_masks().items()}
    volumes = [v for v in (1, 8) if B % v == 0]
    legs = []
    for k, (m, t, c) in data.items():
        c3 = 26 if c == 8 else 6
        legs += [(f"label2d_{k}", lambda m=m, c=c: connected_components(m, c)),
                 (f"filter2d_{k}", lambda m=m, t=t, c=c: filter_components(m, True, 0, c, target=t))]
        for v in volumes:
            d = [B // v] * v
            legs += [(f"label3d_V{v}_{k}", lambda m=m, d=d, c3=c3: connected_components_3d(m, d, c3)),
                     (f"filter3d_V{v}_{k}",
                      lambda m=m, t=t, d=d, c3=c3: filter_components_3d(m, d, True, 0, c3, target=t))]
    for _, fn in legs:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    us = {name: [] for name, _ in legs}
    for _ in range(args.rounds):
        for name, fn in legs:
            us[name].append(timed(fn, args.iters))
    med = {k: statistics.median(v) for k, v in us.items()}
    num = {f"V{v}_{k}": connected_components_3d(m, [B // v] * v, 26 if c == 8 else 6)[1].double().mean().item()
           for k, (m, _, c) in data.items() for v in volumes}
    print(json.dumps({
        "tool": "bench_predict", "leg": "components3d", "shape": [B, H, W], "volumes": volumes,
        "rounds": args.rounds, "iters": args.iters,
        "us_per_call": {k: round(v, 1) for k, v in med.items()},
        "us_per_call_min_max": {k: [round(min(v), 1), round(max(v), 1)] for k, v in us.items()},
        "ratio_3d_over_2d": {f"{op}_V{v}_{k}": round(med[f"{op}3d_V{v}_{k}"] / med[f"{op}2d_{k}"], 2)
                             for op in ("label", "filter") for v in volumes for k in data},
        "mean_components_per_volume": num,
    }))
    sys.exit(0)

if args.lesions:
    from stfunet import _lib, connected_components_3d, lesion_metrics_3d
    volumes = [v for v in (1, 8) if B % v == 0]
    data = {}
    for k, (m, _, c) in component_masks().items():
        t = torch.roll(m, (3, 3), (1, 2)).long()                 # the same kind of mask, three voxels off
        data[k] = (m.cuda(), t.cuda(), (t > 0).to(torch.uint8).cuda(), 26 if c == 8 else 6)
    legs = []
    for k, (m, t, tb, c3) in data.items():
        legs.append((f"form_{k}", lambda m=m, t=t: ((m != 0) & (t > 0)).to(torch.uint8)))
        for v in volumes:
            d = [B // v] * v
            legs += [(f"label_x2_V{v}_{k}", lambda m=m, tb=tb, d=d, c3=c3: (connected_components_3d(m, d, c3),
                                                                             connected_components_3d(tb, d, c3))),
                     (f"lesions_V{v}_{k}", lambda m=m, t=t, d=d, c3=c3: lesion_metrics_3d(m, t, d, c3))]
    for _, fn in legs:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    us = {name: [] for name, _ in legs}
    for _ in range(args.rounds):
        for name, fn in legs:
            us[name].append(timed(fn, args.iters))
    med = {k: statistics.median(v) for k, v in us.items()}
    res = {f"V{v}_{k}": lesion_metrics_3d(m, t, [B // v] * v, c3) for k, (m, t, _, c3) in data.items() for v in volumes}
    print(json.dumps({
        "tool": "bench_predict", "leg": "lesions", "shape": [B, H, W], "volumes": volumes,
        "rounds": args.rounds, "iters": args.iters,
        "scratch_bytes": {f"V{v}": int(_lib.load().stf_lesion_scratch_bytes(B, H, W, v)) for v in volumes},
        "us_per_call": {k: round(v, 1) for k, v in med.items()},
        "us_per_call_min_max": {k: [round(min(v), 1), round(max(v), 1)] for k, v in us.items()},
        "lesions_minus_label_x2_us": {f"V{v}_{k}": round(med[f"lesions_V{v}_{k}"] - med[f"label_x2_V{v}_{k}"], 1)
                                      for k in data for v in volumes},
        "lesions_over_label_x2": {f"V{v}_{k}": round(med[f"lesions_V{v}_{k}"] / med[f"label_x2_V{v}_{k}"], 2)
                                  for k in data for v in volumes},
        "mean_n_target": {k: float(r["n_target"].double().mean()) for k, r in res.items()},
        "mean_n_pred": {k: float(r["n_pred"].double().mean()) for k, r in res.items()},
        "pooled_sensitivity": {k: float(r["matched_target"].sum() / r["n_target"].sum()) for k, r in res.items()},
    }))
    sys.exit(0)

if args.froc:
    from stfunet import _lib, froc_curves, lesion_metrics_3d, lesion_scores_3d, score_histogram
    volumes = [v for v in (1, 8) if B % v == 0]
    g = torch.Generator().manual_seed(5)
    data = {}
    for k, (m, _, c) in component_masks().items():
        t = torch.roll(m, (3, 3), (1, 2)).long()                 # the --lesions targets
        # trained-like scores whose cut at 0.5 is the mask: 97 % of the voxels at 0 or 1, the rest spread over their half
        u, sat = torch.rand(B, H, W, generator=g), torch.rand(B, H, W, generator=g) < 0.97
        s = torch.where(m != 0, torch.where(sat, 1.0, 0.5 + 0.5 * u.clamp_min(1e-3)), torch.where(sat, 0.0, 0.5 * u))
        assert bool(((s > 0.5) == (m != 0)).all())
        data[k] = (m.cuda(), s.float().cuda(), t.cuda(), 26 if c == 8 else 6)
    legs = []
    for k, (m, s, t, c3) in data.items():
        legs.append((f"score_hist_{k}", lambda s=s, t=t: score_histogram(s, t, "probs", 0, 256)))
        for v in volumes:
            d = [B // v] * v
            legs += [(f"lesions_V{v}_{k}", lambda m=m, t=t, d=d, c3=c3: lesion_metrics_3d(m, t, d, c3)),
                     (f"froc_V{v}_{k}", lambda m=m, s=s, t=t, d=d, c3=c3: lesion_scores_3d(m, s, t, d, "probs", 0, 256, c3))]
    for _, fn in legs:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    us = {name: [] for name, _ in legs}
    for _ in range(args.rounds):
        for name, fn in legs:
            us[name].append(timed(fn, args.iters))
    med = {k: statistics.median(v) for k, v in us.items()}
    res = {f"V{v}_{k}": lesion_scores_3d(m, s, t, [B // v] * v, "probs", 0, 256, c3)
           for k, (m, s, t, c3) in data.items() for v in volumes}
    print(json.dumps({
        "tool": "bench_predict", "leg": "froc", "shape": [B, H, W], "volumes": volumes, "bins": 256,
        "rounds": args.rounds, "iters": args.iters,
        "scratch_bytes": {f"V{v}": int(_lib.load().stf_froc_scratch_bytes(B, H, W, v, 256)) for v in volumes},
        "us_per_call": {k: round(v, 1) for k, v in med.items()},
        "us_per_call_min_max": {k: [round(min(v), 1), round(max(v), 1)] for k, v in us.items()},
        "froc_over_lesions_plus_score_hist": {
            f"V{v}_{k}": round(med[f"froc_V{v}_{k}"] / (med[f"lesions_V{v}_{k}"] + med[f"score_hist_{k}"]), 3)
            for k in data for v in volumes},
        "mean_n_target": {k: float(r["n_target"].double().mean()) for k, r in res.items()},
        "mean_n_pred": {k: float(r["n_pred"].double().mean()) for k, r in res.items()},
        "cpm": {k: float(froc_curves(r["froc_hist"])["cpm"]) for k, r in res.items()},
    }))
    sys.exit(0)

if args.boundary3d:
    import time
    from stfunet import _lib, boundary_metrics_3d, filter_components_3d
    from stfunet import predict as P3
    from stfunet.predict import predict_volumes
    from stfunet.unet import UNet
    V = 8 if B % 8 == 0 else 1
    D = B // V
    depths, spacing = [D] * V, (2.5, 0.75, 0.75)
    g = torch.Generator().manual_seed(5)
    zz, yy, xx = torch.meshgrid(torch.arange(D), torch.arange(H), torch.arange(W), indexing="ij")

    def ball(cz, cy, cx, rz, r):
        return ((zz - cz) / rz) ** 2 + ((yy - cy) / r) ** 2 + ((xx - cx) / r) ** 2 <= 1.0

    data = {}
    for regime in ("overlap", "far_apart"):
        Pm, Tm = torch.zeros(B, H, W, dtype=torch.uint8), torch.zeros(B, H, W, dtype=torch.int64)
        for v in range(V):
            r, rz = int(torch.randint(H // 16, H // 8, (1,), generator=g)), max(1.5, D / 5)
            if regime == "overlap":
                cy, cx = (int(c) for c in torch.randint(H // 4, 3 * H // 4, (2,), generator=g))
                dy, dx = (int(c) for c in torch.randint(-4, 5, (2,), generator=g))
                pc, tc = (D / 2 + 0.5, cy + dy, cx + dx), (D / 2, cy, cx)
            else:
                pc, tc = (rz, r + 2, r + 2), (D - 1 - rz, H - 3 - r, W - 3 - r)
            Pm[v * D:(v + 1) * D] = ball(*pc, rz, r).to(torch.uint8)
            Tm[v * D:(v + 1) * D] = ball(*tc, rz, r).long()
        data[regime] = (Pm.cuda(), Tm.cuda())
    legs = []
    for k, (m, t) in data.items():
        legs += [(f"boundary3d_{k}", lambda m=m, t=t: boundary_metrics_3d(m, t, depths, spacing)),
                 (f"filter3d_{k}", lambda m=m, t=t: filter_components_3d(m, depths, True, 0, 26, target=t))]
    for _, fn in legs:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    us = {name: [] for name, _ in legs}
    for _ in range(args.rounds):
        for name, fn in legs:
            us[name].append(timed(fn, args.iters))
    med = {k: statistics.median(v) for k, v in us.items()}
    # every launch of one call on its own: the call recorded into a plan, its entries replayed singly
    lib = _lib.load()
    names = ("memset_counts", "memset_flags", "rows", "plane", "depth", "fold")
    kernels = {}
    for k, (m, t) in data.items():
        host_starts, starts = P3._starts(depths, m.device)
        table = torch.tensor([spacing] * V, dtype=torch.float64, device=m.device)
        out = torch.empty(V, 3, dtype=torch.float64, device=m.device)
        cnt = torch.empty(V, 2, dtype=torch.int64, device=m.device)
        scratch = _lib.scratch_words(lib.stf_boundary3d_scratch_bytes(B, H, W, V), m.device)  # held while the plan replays
        plan = lib.stf_plan_create()
        assert lib.stf_plan_record(plan) == 0
        try:
            _lib.call("stf_boundary3d_metrics", m.data_ptr(), t.data_ptr(), B, H, W, starts.data_ptr(),
                      host_starts.data_ptr(), V, table.data_ptr(), -1, out.data_ptr(), cnt.data_ptr(),
                      scratch.data_ptr(), _lib.stream())
        finally:
            assert lib.stf_plan_stop() == 0
        torch.cuda.synchronize()
        assert lib.stf_plan_size(plan) == len(names), lib.stf_plan_size(plan)
        # entry i = replay of entries 0..i minus replay of 0..i-1: every replay starts from the memsets, so
        # the counts and the cursor the later launches read are those of one call
        prefix = [0.0]
        for i in range(len(names)):
            one = [timed(lambda: lib.stf_plan_replay(plan, 0, i + 1, None), args.iters) for _ in range(args.rounds)]
            prefix.append(statistics.median(one))
        kernels[k] = {name: round(prefix[i + 1] - prefix[i], 1) for i, name in enumerate(names)}
        kernels[k]["all"] = round(prefix[-1], 1)
        lib.stf_plan_destroy(plan)

    def scipy_volume_ms(m, t):
        try:
            import numpy as np
            from scipy.ndimage import binary_erosion, distance_transform_edt, generate_binary_structure
        except ImportError:
            return None
        cross = generate_binary_structure(3, 1)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        p, q = m[:D].cpu().numpy().astype(bool), t[:D].cpu().numpy() > 0
        bp, bt = p ^ binary_erosion(p, cross), q ^ binary_erosion(q, cross)
        a, c = distance_transform_edt(~bt, sampling=spacing)[bp], distance_transform_edt(~bp, sampling=spacing)[bt]
        _ = max(a.max(), c.max()), np.percentile(np.hstack((a, c)), 95), (a.mean() + c.mean()) / 2
        return (time.perf_counter() - t0) * 1e3

    host = {k: scipy_volume_ms(*v) for k, v in data.items()}
    model = UNet(in_channels=8, num_classes=2).cuda()
    half = B // 2
    loader = [(inputs[i:i + half].view(half, 1, 8, H, W), data["overlap"][1][i:i + half]) for i in (0, half)]

    def loop_ms(flag):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        predict_volumes(model, loader, torch.device("cuda"), depths, boundary=flag, spacing=spacing)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for flag in (False, True, False, True):
        loop_ms(flag)
    loop = {False: [], True: []}
    for _ in range(args.rounds):
        for flag in (False, True):
            loop[flag].append(loop_ms(flag))
    loop_med = {k: statistics.median(v) for k, v in loop.items()}
    res = {k: boundary_metrics_3d(m, t, depths, spacing) for k, (m, t) in data.items()}
    print(json.dumps({
        "tool": "bench_predict", "leg": "boundary3d", "shape": [B, H, W], "volumes": V, "spacing": spacing,
        "rounds": args.rounds, "iters": args.iters,
        "scratch_bytes": int(lib.stf_boundary3d_scratch_bytes(B, H, W, V)),
        "us_per_call": {k: round(v, 1) for k, v in med.items()},
        "us_per_call_min_max": {k: [round(min(v), 1), round(max(v), 1)] for k, v in us.items()},
        "us_per_volume": {k: round(v / V, 1) for k, v in med.items()},
        "boundary3d_over_filter3d": {k: round(med[f"boundary3d_{k}"] / med[f"filter3d_{k}"], 2) for k in data},
        "us_per_launch": kernels,
        "mean_hd95": {k: float(torch.nanmean(v["hd95"])) for k, v in res.items()},
        "mean_border_voxels": {k: float(v["border_counts"].double().mean()) for k, v in res.items()},
        "scipy_host_ms_per_volume": {k: None if v is None else round(v, 1) for k, v in host.items()},
        "predict_volumes_loop_ms": {"slices": B, "plain": round(loop_med[False], 3),
                                    "boundary": round(loop_med[True], 3),
                                    "plain_min_max": [round(min(loop[False]), 3), round(max(loop[False]), 3)],
                                    "boundary_min_max": [round(min(loop[True]), 3), round(max(loop[True]), 3)],
                                    "added_us_per_volume": round((loop_med[True] - loop_med[False]) * 1e3 / V, 1)},
    }))
    sys.exit(0)

if args.boundary:
    from stfunet import boundary_metrics
    data = {k: tuple(t.cuda() for t in blobs(k)) for k in ("overlap", "far_apart")}
    mask0 = data["overlap"][0]
    legs = (("boundary_overlap", lambda: boundary_metrics(*data["overlap"])),
            ("boundary_far_apart", lambda: boundary_metrics(*data["far_apart"])),
            ("predict_masks_with_counts", lambda: predict_masks(logits, args.rule, 0, 0.5, target=target)),
            ("overlay", lambda: overlay(frames, mask0, COLOR, ALPHA, PAINT)))
    for _, fn in legs:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    us = {name: [] for name, _ in legs}
    for _ in range(args.rounds):
        for name, fn in legs:
            us[name].append(timed(fn, args.iters) / B)
    # the predict loop (UNet, two batches of B) without and with boundary=True, interleaved: without
    # the flag the loop issues the launches it issued before the option existed
    import time
    from stfunet.predict import predict
    from stfunet.unet import UNet
    model = UNet(in_channels=8, num_classes=2).cuda()
    loader = [(inputs.view(B, 1, 8, H, W), data[k][1]) for k in ("overlap", "far_apart")]

    def loop_ms(flag):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        predict(model, loader, torch.device("cuda"), boundary=flag)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for flag in (False, True, False, True):
        loop_ms(flag)
    loop = {False: [], True: []}
    for _ in range(args.rounds):
        for flag in (False, True):
            loop[flag].append(loop_ms(flag))
    loop_med = {k: statistics.median(v) for k, v in loop.items()}
    res = {k: boundary_metrics(*v) for k, v in data.items()}
    host = {k: scipy_host_us(*v, min(B, args.host_images)) for k, v in data.items()}
    med = {k: statistics.median(v) for k, v in us.items()}
    print(json.dumps({
        "tool": "bench_predict", "leg": "boundary", "shape": [B, H, W], "rounds": args.rounds, "iters": args.iters,
        "us_per_image": {k: round(v, 3) for k, v in med.items()},
        "us_per_image_min_max": {k: [round(min(v), 3), round(max(v), 3)] for k, v in us.items()},
        "far_apart_over_overlap": round(med["boundary_far_apart"] / med["boundary_overlap"], 2),
        "mean_hd95": {k: float(torch.nanmean(v["hd95"])) for k, v in res.items()},
        "mean_border_pixels": {k: float(v["border_counts"].double().mean()) for k, v in res.items()},
        "scipy_host_us_per_image": {k: None if v is None else round(v, 1) for k, v in host.items()},
        "predict_loop_ms": {"images": 2 * B, "plain": round(loop_med[False], 3), "boundary": round(loop_med[True], 3),
                            "plain_min_max": [round(min(loop[False]), 3), round(max(loop[False]), 3)],
                            "boundary_min_max": [round(min(loop[True]), 3), round(max(loop[True]), 3)],
                            "added_us_per_image": round((loop_med[True] - loop_med[False]) * 1e3 / (2 * B), 2)},
    }))
    sys.exit(0)

paths = (("device", device_path, args.iters), ("torch_batched", torch_batched, args.iters),
         ("torch_per_slice", torch_per_slice, max(1, args.iters // 10)))
for _, fn, _ in paths:                                  # warm-up: code objects, allocator
    for _ in range(3):
        fn()
torch.cuda.synchronize()
us = {name: [] for name, _, _ in paths}
for _ in range(args.rounds):
    for name, fn, iters in paths:
        us[name].append(timed(fn, iters))

ref, got = torch_batched(), device_path()
if args.rule == "argmax":
    same_mask = int(((got[0] > 0) != (ref[0] > 0)).sum())
else:
    same_mask = int((got[0] != ref[0]).sum())
HW = H * W
algorithmic = B * HW * ((K if args.rule == "argmax" else 1) * 4 + 8 + 4 + 1 + 3) + B * 24
moved = algorithmic + B * HW * (4 + 1)
med = {k: statistics.median(v) for k, v in us.items()}
print(json.dumps({
    "tool": "bench_predict", "rule": args.rule, "shape": [B, K, H, W], "rounds": args.rounds, "iters": args.iters,
    "us_per_batch": {k: round(v, 1) for k, v in med.items()},
    "us_min_max": {k: [round(min(v), 1), round(max(v), 1)] for k, v in us.items()},
    "speedup_vs_torch_batched": round(med["torch_batched"] / med["device"], 2),
    "speedup_vs_torch_per_slice": round(med["torch_per_slice"] / med["device"], 2),
    "algorithmic_bytes": algorithmic, "moved_bytes": moved,
    "algorithmic_TBps": round(algorithmic / med["device"] / 1e6, 3),
    "moved_TBps": round(moved / med["device"] / 1e6, 3),
    "mask_pixels_differing_from_torch": same_mask,
    "overlay_bytes_differing_from_torch": int((got[3] != ref[3]).sum()),
    "max_abs_dice_difference": float((got[1] - ref[1]).abs().max()),
}))
