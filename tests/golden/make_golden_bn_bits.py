"""Pin the BatchNorm entry points' result bits in both storage libraries.

    STF_LIB=<parent build>/libstfunet_hip.so STF_LIB_F16=<parent build>/libstfunet_hip_f16.so \\
        python tests/golden/make_golden_bn_bits.py --commit <hash> [--out FILE]

writes tests/golden/bn_bits.json on an MI355X: per case of tests/_bn_bits.py (entry point, shape,
options; the inputs come from numpy.random.default_rng) and per storage type the SHA-256 of the raw
bytes of every output buffer, pre-filled with NaN.  The grids of these kernels depend on the shapes
alone, so the digests do not depend on the chip's CU count.  The fixture is the measure of "BatchNorm
computes the same bits" for tests/test_bn_bits_gpu.py, so it is written from the build of the
commit *before* a change to csrc/bn.hip, never from the code under test.  The cases that also have
a float64 restatement (_bn_bits.is_ref) must pass it in that build (rel-L2 <= REF_BOUND); one that
does not is reported, listed under ``left_out`` and not pinned.
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "bn_bits.json")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="hash of the commit whose build is loaded (STF_LIB, STF_LIB_F16)")
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    for p in (REPO, os.path.join(REPO, "stf-unet_amd"), os.path.join(REPO, "tests")):
        sys.path.insert(0, p)
    import _bn_bits as bb
    from stfunet import _lib
    rows, left_out = [], []
    for entry, shape, opts in bb.cases():
        cid = bb.case_id(entry, shape, opts)
        row = {"id": cid, "seed": bb.seed_of(entry, shape, opts)}
        for key, dtype in bb.DTYPES.items():
            outs, cpu = bb.run(entry, shape, opts, dtype)
            d = {k: bb._sha(v) for k, v in outs.items()}
            assert d == bb.digests(entry, shape, opts, dtype), f"{cid} {key}: two runs disagree"
            row[key] = d
            if bb.is_ref(entry, shape, opts):
                errs = bb.ref_errors(entry, shape, opts, dtype, outs, cpu)
                print(cid, key, "rel-L2 vs float64", errs, flush=True)
                if max(errs.values()) > bb.REF_BOUND and cid not in left_out:
                    left_out.append(cid)
        print(cid, {k: v[:12] for k, v in row["bf16"].items()}, flush=True)
        if cid not in left_out:
            rows.append(row)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write('{"commit": "%s", "library": %s, "left_out": %s,\n "cases": [\n' %
                (args.commit, json.dumps(_lib.build_info()["lib"]), json.dumps(left_out)))
        f.write(",\n".join("  " + json.dumps(r) for r in rows))
        f.write("\n ]}\n")
    print(f"{len(rows)} cases from {_lib.LIB_PATH} and {_lib.LIB_PATH_F16}; left out: {left_out}")


if __name__ == "__main__":
    main()
