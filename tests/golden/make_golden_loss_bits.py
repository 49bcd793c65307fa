"""Pin the criterion kernels' result bits: loss, Dice/CE terms and dlogits of both kernel families.

    STF_LIB=<parent build>/libstfunet_hip.so python tests/golden/make_golden_loss_bits.py --commit <hash>
        [--manyclass] [--out FILE]

writes tests/golden/loss_bits.json on an MI355X: per case of tests/_loss_bits.py (seed and shape
only; the inputs come from numpy.random.default_rng) the SHA-256 of the raw bytes of the loss, of
the leading N*K*3+1 (default entry points) or N*K*3+2 (every other entry point) floats of ``terms``
and of ``dlogits`` pre-filled with NaN.  --manyclass writes tests/golden/loss_bits_manyclass.json
instead: the many-class and the focal / Tversky entry points (``mc_cases``).  A fixture is the measure
of "the criterion computes the same bits" for tests/test_loss_bits_gpu.py, so it is written from the
build of the commit *before* a change to csrc/loss.hip, never from the code under test.
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "loss_bits.json")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="hash of the commit whose build is loaded (STF_LIB)")
    ap.add_argument("--manyclass", action="store_true", help="the stf_loss_mc_* / stf_loss_ft_* cases")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    args.out = args.out or (OUT.replace(".json", "_manyclass.json") if args.manyclass else OUT)
    for p in (REPO, os.path.join(REPO, "stf-unet_amd"), os.path.join(REPO, "tests")):
        sys.path.insert(0, p)
    import _loss_bits as lb
    from stfunet import _lib
    rows = []
    for family, shape in (lb.mc_cases() if args.manyclass else lb.cases()):
        d = lb.digests(family, shape)
        assert d == lb.digests(family, shape), f"{lb.case_id(family, shape)}: two runs disagree"
        rows.append({"family": family, "shape": list(shape), "seed": lb.seed_of(shape), **d})
        print(lb.case_id(family, shape), d["loss_value"], d["dlogits"][:16], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write('{"commit": "%s", "library": "%s", "ignore_index": %d, "grad_out": %s,\n "cases": [\n' %
                (args.commit, _lib.build_info()["lib"]["bf16"], lb.IGNORE, lb.GRAD_OUT))
        f.write(",\n".join("  " + json.dumps(r) for r in rows))
        f.write("\n ]}\n")
    print(f"{len(rows)} cases from {_lib.LIB_PATH}")


if __name__ == "__main__":
    main()
