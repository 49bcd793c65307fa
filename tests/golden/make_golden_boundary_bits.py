"""Pin the distance-transform kernels' result bits and scratch sizes.

    STF_LIB=<parent build>/libstfunet_hip.so python tests/golden/make_golden_boundary_bits.py --commit <hash>
        [--out FILE]

writes tests/golden/boundary_bits.json on an MI355X: per case of tests/_boundary_bits.py (name, shape
and seed only; the inputs come from numpy.random.default_rng) the SHA-256 of the raw bytes of every
output of stf_edt_sq, stf_boundary_metrics, stf_edt3d_sq, stf_boundary3d_metrics, stf_sdf and
stf_bloss_fwd / stf_bloss_bwd, pre-filled with 0xAA, and the scratch size of the shape.  The volume
metrics' compact list is unordered by design, its outputs are not: two runs must agree before anything
is written.  The fixture is the measure of "the kernels compute the same bits" for
tests/test_boundary_bits_gpu.py, so it is written from the build of the commit *before* a change to
csrc/boundary.hip, csrc/bloss.hip or csrc/edt_rows.h, never from the code under test.
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "boundary_bits.json")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="hash of the commit whose build is loaded (STF_LIB)")
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    for p in (REPO, os.path.join(REPO, "stf-unet_amd"), os.path.join(REPO, "tests")):
        sys.path.insert(0, p)
    import _boundary_bits as bb
    from stfunet import _lib
    rows = []
    for name in bb.cases():
        d = bb.digests(name)
        assert d == bb.digests(name), f"{name}: two runs disagree"
        rows.append({"case": name, "seed": bb.seed_of(name), **d})
        print(name, {k: (v[:12] if isinstance(v, str) else v) for k, v in d.items()}, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write('{"commit": "%s", "library": "%s", "ignore_index": %d, "grad_out": %s, "alpha": %s,\n "cases": [\n' %
                (args.commit, _lib.build_info()["lib"]["bf16"], bb.IGNORE, bb.GRAD_OUT, bb.ALPHA))
        f.write(",\n".join("  " + json.dumps(r) for r in rows))
        f.write("\n ]}\n")
    print(f"{len(rows)} cases from {_lib.LIB_PATH}")


if __name__ == "__main__":
    main()
