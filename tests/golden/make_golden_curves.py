"""Writes tests/golden/curves.npz: for every case of tests/_curves_ref.py ``cases()`` the score
histogram pooled over the case's images, and scikit-learn's AUROC and average precision of it.

Independent of the restatement: a pixel's row is the number of thresholds ``j / bins``, ``j = 0 .. bins - 1``,
its score exceeds, compared in float64 (every ``j / bins`` and every float32 score is exact there; a NaN
exceeds nothing), not the float32 ``ceil`` of the row rule; ``roc_auc_score`` and
``average_precision_score`` (scikit-learn 1.7.2 where this fixture was made) see the rows as scores, one
sample per pixel.  Cases with an empty side store NaN for both.  Inputs are not stored; ``cases()``
rebuilds them (seeded PCG64 and literals).

    python tests/golden/make_golden_curves.py
"""
import os
import sys

import numpy as np
from sklearn.metrics import average_precision_score, roc_auc_score

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from _curves_ref import cases  # noqa: E402


def rows_by_counting(scores, bins):
    p = np.asarray(scores, np.float64).ravel()
    edges = np.arange(bins, dtype=np.float64) / bins
    with np.errstate(invalid="ignore"):
        return (p[:, None] > edges[None, :]).sum(1)


def main():
    out, names, auroc, ap = {}, [], [], []
    for i, c in enumerate(cases()):
        t = c["target"].ravel()
        keep = np.ones(t.shape, bool) if c["ignore"] is None else t != c["ignore"]
        y = ((t > 0) if c["positive"] is None else (t == c["positive"]))[keep]
        r = rows_by_counting(c["scores"], c["bins"])[keep]
        hist = np.stack([np.bincount(r[~y], minlength=c["bins"] + 1), np.bincount(r[y], minlength=c["bins"] + 1)])
        names.append(c["name"])
        out[f"hist_{i}"] = hist.astype(np.int64)
        both = y.any() and (~y).any()
        auroc.append(roc_auc_score(y, r) if both else np.nan)
        ap.append(average_precision_score(y, r) if both else np.nan)
    path = os.path.join(HERE, "curves.npz")
    np.savez_compressed(path, names=np.array(names), auroc=np.array(auroc, np.float64), ap=np.array(ap, np.float64),
                        **out)
    print(path, os.path.getsize(path), "bytes,", len(names), "cases")


if __name__ == "__main__":
    main()
