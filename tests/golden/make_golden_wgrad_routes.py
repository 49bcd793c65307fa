"""Pin the weight-gradient routes: which kernel stf_wgrad launches, in how many splits, on what workspace.

    STF_LIB=<parent build>/libstfunet_hip.so python tests/golden/make_golden_wgrad_routes.py --commit <hash>

writes tests/golden/wgrad_routes.json: for every launch signature below, the kernel name
(stf_wgrad_kernel_name, as the profiler prints it) and stf_wgrad_plan's split count and workspace
bytes.  The fixture is the measure of "the routes did not change" for tests/test_wgrad_routes_cpu.py,
so it is written from the build of the commit *before* a change to the route selection, never from
the code under test.  The queries launch nothing and do not depend on the CU count: the caller passes
its workgroup budget (grid_blocks; 256, the MI355X's CU count, on the side stream).

The signatures (tests/_wgrad_variants.FIELDS), in two parts:

"routes", each row with its signature: every entry of the parity table and its 4 GiB cases, and the
weight gradients of the two models at their bench shapes (UNet N = 64 at 256 x 256, STF cfg3 and
cfg5), inline and on the side stream.  The models' layers are *inferred* from make_golden_routes.py's
igemm tables, not recorded from launches: the weight gradient of a layer has the geometry of its
forward conv (x = the source, dy = the destination; a row with a bias, statistics or an LSTM epilogue
counts as a forward), a ConvT's has the geometry of its stride-2 gather (x = the 2x larger gradient
tensor, dy = the small input), which those tables list as the ConvT's dgrad.  That rule is a superset:
a dgrad that writes statistics comes in too, as a weight gradient with the channels swapped (a shape
no model launches; harmless, it is one more pinned query).  The LSTM rows have the per-step shape
(N = B), dy rows are taken dense (dycs = Nout; the route reads neither), and the STF stem's 7x7 gather
form is added by hand.  Nothing here checks the list against nhwc._PLANS of a real step.

"sweep", answers only: the whole completeness sweep of tests/test_wgrad_variants_cpu.py at
grid_blocks 0, 5 and 256 (8820 queries).  Their signatures are sweep_signatures() below, in that
order; the file stores the count and the SHA-256 of that list in place of the list itself, so a
change to sweep() fails the test instead of shifting the answers.
"""
import argparse
import ctypes
import hashlib
import importlib.util
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
REPO = os.path.dirname(TESTS)
OUT = os.path.join(HERE, "wgrad_routes.json")
RESULTS = ("name", "splits", "ws_bytes")
CUS = 256
BUDGETS = (0, 5, CUS)
PER_LINE = 24                      # sweep answers per line of the file


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _tables():
    if TESTS not in sys.path:
        sys.path.insert(0, TESTS)
    import _wgrad_variants as W
    return (W, _load("test_wgrad_variants_cpu", os.path.join(TESTS, "test_wgrad_variants_cpu.py")),
            _load("make_golden_routes", os.path.join(HERE, "make_golden_routes.py")))


def model_signatures(W, G):
    """The weight-gradient launches behind the igemm layer tables, at grid_blocks 0 and 256."""
    layers = G.unet_signatures() + G.stf_signatures(16, 8, 256) + G.stf_signatures(4, 32, 512)
    out = set()
    for s in layers:
        d = dict(zip(G.FIELDS, s))
        forward = d["bias"] or d["stats"] or d["lstm"]
        if d["transposed"] or d["scatter"] or d["Cs"] % 8 or d["Nout"] % 8 or not (forward or d["stride"] == 2):
            continue
        for gb in (0, CUS):
            out.add((d["N"], d["Hs"], d["Ws"], d["Cs"], d["scs"], 0, d["Hd"], d["Wd"], d["R"], d["stride"], d["pad"],
                     d["Nout"], d["Nout"], 0, gb))
    # the STF stem on the gather path: 7x7 / stride 2 over the 8-channel packed frames (padded form)
    for N, HW in ((16 * 8, 256), (4 * 32, 512)):
        out |= {W.sig(N, HW, HW, 8, 64, R=7, stride=2, gb=gb) for gb in (0, CUS)}
    return out


def signatures():
    """The rows of "routes": the parity table, its 4 GiB cases and the model layers."""
    W, _, G = _tables()
    s = {c for _, c, _ in W.cases()} | set(W.WIDE_4GIB.values()) | model_signatures(W, G)
    assert all(len(c) == len(W.FIELDS) for c in s)
    return sorted(s)


def sweep_signatures():
    """The queries of "sweep", in the order of its answers: sweep() x BUDGETS."""
    _, T, _ = _tables()
    return [c[:-1] + (gb,) for c in T.sweep() for gb in BUDGETS]


def digest(sigs):
    return hashlib.sha256(json.dumps([list(s) for s in sigs], separators=(",", ":")).encode()).hexdigest()


def query(lib, s):
    """The recorded answers for one signature from a loaded library (host-only calls)."""
    from stfunet import _lib
    N, Hs, Ws, Cs, xcs, xoff, Hd, Wd, R, stride, pad, Nout, dycs, dyoff, gb = s
    fake = 1 << 32                                         # the queries read no memory
    g = _lib.ConvGeom(N, Hs, Ws, Cs, xcs, Hd, Wd, R, R, stride, pad, 0)
    a = _lib.WgradArgs(g, fake + 2 * dyoff, dycs, Nout, 3 * fake + 2 * xoff, None, 0, gb)
    sp, nb = ctypes.c_int(0), ctypes.c_size_t(0)
    assert lib.stf_wgrad_plan(ctypes.byref(a), ctypes.byref(sp), ctypes.byref(nb)) == 0
    return [lib.stf_wgrad_kernel_name(ctypes.byref(a)).decode(), sp.value, nb.value]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="hash of the commit whose build is loaded (STF_LIB)")
    args = ap.parse_args()
    for p in (REPO, os.path.join(REPO, "stf-unet_amd")):
        sys.path.insert(0, p)
    import torch
    from stfunet import _lib
    W = _tables()[0]
    sigs, sweep = signatures(), sweep_signatures()
    rows, swept = ([query(_lib.load(torch.bfloat16), s) for s in part] for part in (sigs, sweep))
    assert [rows, swept] == [[query(_lib.load(torch.float16), s) for s in part] for part in (sigs, sweep)], \
        "the two storage builds disagree"
    names = sorted({r[0] for r in rows + swept})
    pack = lambda r: json.dumps([names.index(r[0])] + r[1:], separators=(",", ":"))   # noqa: E731
    with open(OUT, "w") as f:
        # an answer is [index into "names", splits, ws_bytes]; a route is [signature, answer]
        f.write('{"commit": "%s", "cus": %d,\n "fields": %s,\n "results": %s,\n "names": %s,\n "routes": [\n' %
                (args.commit, CUS, json.dumps(W.FIELDS), json.dumps(RESULTS), json.dumps(names)))
        f.write(",\n".join("[%s,%s]" % (json.dumps(list(s), separators=(",", ":")), pack(r))
                           for s, r in zip(sigs, rows)))
        f.write('\n ],\n "sweep": {"budgets": %s, "count": %d, "sha256": "%s", "answers": [\n' %
                (json.dumps(BUDGETS), len(sweep), digest(sweep)))
        f.write(",\n".join(",".join(pack(r) for r in swept[i:i + PER_LINE]) for i in range(0, len(swept), PER_LINE)))
        f.write("\n ]}}\n")
    print(f"{len(sigs)} + {len(sweep)} signatures, {len(names)} kernel names from {_lib.LIB_PATH}")
    for n in names:
        print("  ", n)


if __name__ == "__main__":
    main()
