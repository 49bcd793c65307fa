"""Pin the eager launch sequence of one training step of UNet and STFLSTMUNet (without and with PK maps).

    python tests/golden/make_golden_launch_trace.py --commit <hash>

writes tests/golden/launch_trace.json on a machine with the GPU: per case of tests/_launch_trace.py
the ordered C-ABI entry points of one forward + backward (stf_igemm / stf_wgrad with their conv
geometry and output channels).  The fixture is the measure of "the schedule did not change" for
tests/test_launch_trace_gpu.py, so it is written from the tree of the commit *before* a change to
the Python programs (stfunet/program.py, unet.py, stf_lstm_unet.py, nhwc.py), never from the
code under test; ``--commit`` names that commit in the fixture's header.
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "launch_trace.json")
for p in (os.path.join(REPO, "tests"), os.path.join(REPO, "stf-unet_amd"), REPO):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="the commit whose tree writes the fixture")
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    import _launch_trace as lt
    cases = {which: lt.capture(which) for which in lt.CASES}
    with open(args.out, "w") as f:          # one launch per line: a changed schedule reads as a diff
        f.write('{"written_by_commit": %s,\n "geom_fields": %s,\n "cases": {\n'
                % (json.dumps(args.commit), json.dumps(list(lt.GEOM) + ["Nout"])))
        for i, (which, trace) in enumerate(cases.items()):
            f.write('  %s: [\n' % json.dumps(which))
            f.write(",\n".join("   " + json.dumps(e) for e in trace))
            f.write("\n  ]%s\n" % ("," if i + 1 < len(cases) else ""))
        f.write(" }\n}\n")
    print("wrote", args.out, {k: len(v) for k, v in cases.items()})


if __name__ == "__main__":
    main()
