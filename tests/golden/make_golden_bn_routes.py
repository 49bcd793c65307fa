"""Pin the BatchNorm routes that a caller can see without a GPU: the partial rows it has to allocate.

    STF_LIB=<parent build>/libstfunet_hip.so python tests/golden/make_golden_bn_routes.py --commit <hash>

writes tests/golden/bn_routes.json: for every signature (N, H, W, C, groups) below the answers of
stf_bn_bwd_tiles(N, H, W, C, groups, 0), stf_bn_bwd_tiles(..., 1) and stf_bn_bwd_apply_tiles(N*H*W, C).
The fixture is the measure of "the routes did not change" for tests/test_bn_routes_cpu.py, so it is
written from the build of the commit *before* a change to csrc/bn.hip's route selection, never from
the code under test.  The queries launch nothing.

The signatures, in two parts:

"routes", each row with its signature: every shape of the tables of tests/_bn_ref.py, and the
BatchNorms of the two models at their bench shapes (UNet N = 64 at 256 x 256, STF cfg3 and cfg5).
The models' BatchNorms are *inferred* from make_golden_routes.py's igemm tables, not recorded from
launches: every conv that writes statistics feeds a BatchNorm over its output (N, Hd, Wd, Nout) with
the conv's groups, and the STF stem (7x7 / stride 2, 64 channels, one group per time step) is added
by hand.  That rule is a superset (a dgrad that writes statistics comes in too); harmless, it is one
more pinned query.

"sweep", answers only: C x groups x pixel counts on both sides of every cap -- a group's units against
one block (256), the group-major block of 4 x 256, the 1024-row budget of the fold shared by the
groups, and the 8192-block cap.  Their signatures are sweep_signatures() below, in that order; the
file stores the count and the SHA-256 of that list in place of the list itself, so a change to the
sweep fails the test instead of shifting the answers.
"""
import argparse
import hashlib
import importlib.util
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
REPO = os.path.dirname(TESTS)
OUT = os.path.join(HERE, "bn_routes.json")
FIELDS = ("N", "H", "W", "C", "groups")
RESULTS = ("tiles", "tiles_pooled", "apply_tiles")
SWEEP_C = (8, 16, 24, 64, 512, 1024, 2048, 4096)
SWEEP_G = (1, 2, 3, 8, 128)
NT, UPT, ROW_CAP, BLOCK_CAP = 256, 4, 1024, 8192
PER_LINE = 16                      # sweep answers per line of the file


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def table_signatures():
    if TESTS not in sys.path:
        sys.path.insert(0, TESTS)
    import _bn_ref as R
    s = {c for c, _ in R.GROUP_MAJOR + R.POOL_DPP + R.POOL_WIN + R.POOL3} | set(R.GENERIC) | set(R.POOL_ACT) | {R.BIG}
    return s | set(R.DBIAS_BOUNDED)


def model_signatures():
    G = _load("make_golden_routes", os.path.join(HERE, "make_golden_routes.py"))
    out = set()
    for s in G.unet_signatures() + G.stf_signatures(16, 8, 256) + G.stf_signatures(4, 32, 512):
        d = dict(zip(G.FIELDS, s))
        if d["stats"]:
            out.add((d["N"], d["Hd"], d["Wd"], d["Nout"], d["groups"]))
    for B, T, HW in ((16, 8, 256), (4, 32, 512)):
        out.add((B * T, HW // 2, HW // 2, 64, T))
    return out


def signatures():
    """The rows of "routes": the parity tables and the models' BatchNorms."""
    return sorted(table_signatures() | model_signatures())


def sweep_signatures():
    """The queries of "sweep", in the order of its answers.  One image per group and a one-pixel-wide
    image of even height, so a group's pixel count is H: for every (C, groups) the H at which a group's
    units reach each cap of the file, and the even H on either side of it."""
    out = []
    for C in SWEEP_C:
        cg = C // 8
        for G in SWEEP_G:
            caps = (NT, NT * UPT,                                # one block: flat / pooled, group-major
                    NT * -(-ROW_CAP // G), NT * (ROW_CAP // G or 1),       # the reduce's rows per group
                    NT * ROW_CAP // G,                           # the apply's bias rows over all groups
                    NT * UPT * (BLOCK_CAP // G), 4 * NT * (-(-ROW_CAP // G)))     # the block cap; pooled rows
            hs = set()
            for units in caps:
                h = max(2, units // cg // 2 * 2)
                hs |= {max(2, h - 2), h, h + 2}
            out += [(G, h, 1, C, G) for h in sorted(hs)]
            out += [(G, h, 2, C, G) for h in sorted(hs)[::3]]    # pooled: H/2 windows of 2 x 2
    return out


def digest(sigs):
    return hashlib.sha256(json.dumps([list(s) for s in sigs], separators=(",", ":")).encode()).hexdigest()


def query(lib, s):
    """The recorded answers for one signature from a loaded library (host-only calls)."""
    N, H, W, C, G = s
    return [lib.stf_bn_bwd_tiles(N, H, W, C, G, 0), lib.stf_bn_bwd_tiles(N, H, W, C, G, 1),
            lib.stf_bn_bwd_apply_tiles(N * H * W, C)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="hash of the commit whose build is loaded (STF_LIB)")
    args = ap.parse_args()
    for p in (REPO, os.path.join(REPO, "stf-unet_amd")):
        sys.path.insert(0, p)
    import torch
    from stfunet import _lib
    sigs, sweep = signatures(), sweep_signatures()
    rows, swept = ([query(_lib.load(torch.bfloat16), s) for s in part] for part in (sigs, sweep))
    assert [rows, swept] == [[query(_lib.load(torch.float16), s) for s in part] for part in (sigs, sweep)], \
        "the two storage builds disagree"
    pack = lambda v: json.dumps(list(v), separators=(",", ":"))   # noqa: E731
    with open(OUT, "w") as f:
        f.write('{"commit": "%s",\n "fields": %s,\n "results": %s,\n "routes": [\n' %
                (args.commit, json.dumps(FIELDS), json.dumps(RESULTS)))
        f.write(",\n".join("[%s,%s]" % (pack(s), pack(r)) for s, r in zip(sigs, rows)))
        f.write('\n ],\n "sweep": {"count": %d, "sha256": "%s", "answers": [\n' % (len(sweep), digest(sweep)))
        f.write(",\n".join(",".join(pack(r) for r in swept[i:i + PER_LINE]) for i in range(0, len(swept), PER_LINE)))
        f.write("\n ]}}\n")
    print(f"{len(sigs)} + {len(sweep)} signatures from {_lib.LIB_PATH}")


if __name__ == "__main__":
    main()
