#!/usr/bin/env python3
"""End-to-end check in the style of the reference's only CI test (QData/FastSK
test/run_check.py:37-64): gapped-k-mer kernel on the GPU -> LinearSVC + 5-fold calibration ->
test AUC >= 0.9 on EP300. Same user code as the reference; only the import resolves to the
MI355X engine (this repo's `fastsk/` alias package). Then the same data through the resident pipeline
(`cross_validate_svm` + `fit_svm` + `decision_function_np`), which the reference does not have.

    python examples/run_check.py --train EP300.train.fasta --test EP300.test.fasta
"""
import argparse
import os
import sys
import time

import numpy as np
from sklearn.calibration import CalibratedClassifierCV
from sklearn.metrics import roc_auc_score
from sklearn.svm import LinearSVC

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fastsk import FastSK, FastaUtility  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--train", default="/root/reference/data/EP300.train.fasta")
    ap.add_argument("--test", default="/root/reference/data/EP300.test.fasta")
    ap.add_argument("-g", type=int, default=10)
    ap.add_argument("-m", type=int, default=6)
    ap.add_argument("--exact", action="store_true", help="exact kernel instead of approx=True, t=1")
    args = ap.parse_args()

    reader = FastaUtility()
    Xtrain, Ytrain = reader.read_data(args.train)
    Xtest, Ytest = reader.read_data(args.test)

    t0 = time.time()
    k = FastSK(g=args.g, m=args.m) if args.exact else FastSK(g=args.g, m=args.m, t=1, approx=True)
    k.compute_kernel(Xtrain, Xtest)
    Ktr, Kte = k.get_train_kernel_np(), k.get_test_kernel_np()  # get_train_kernel() gives lists, as upstream
    print("kernel: %d x %d train, %d x %d test in %.3f s (%s)" % (*Ktr.shape, *Kte.shape, time.time() - t0, k.stats()["path_used"]))

    clf = CalibratedClassifierCV(LinearSVC(C=1), cv=5).fit(Ktr, Ytrain)
    acc = clf.score(Kte, np.array(Ytest))
    auc = roc_auc_score(Ytest, clf.predict_proba(Kte)[:, 1])
    print("calibrated linear SVM on the kernel rows: accuracy %.4f, test AUC %.4f" % (acc, auc))
    if auc < 0.9:  # the reference's acceptance threshold (test/run_check.py:64)
        raise SystemExit("test AUC %.4f is below 0.9" % auc)

    # beside it, the resident pipeline: a C-SVC cross-validated over 5 folds x 3 values of C in one batch, refitted at the best C
    # and applied, all on the triangle the compute call left on the GPU — no kernel matrix crosses to the host (labels -1 / +1)
    t0 = time.time()
    labels = np.where(np.array(Ytrain) > 0, 1, -1)
    cv = k.cross_validate_svm(labels, Cs=(0.1, 1.0, 10.0), folds=5, eps=1e-3, refit=True)
    info = cv["refit"]
    print("5 folds x 3 C side by side (%s, %d launches, %.1f ms): out-of-fold AUC %s, best C %g"
          % (cv["form"], cv["launches"], cv["ms"], ", ".join("%.4f" % a for a in cv["auc"]), cv["best_C"]))
    dec = k.decision_function_np("test")
    auc_svm = roc_auc_score(Ytest, dec)
    print("C-SVC on the resident triangle at C = %g: %d iterations (%s), %d support vectors, sweep + fit + decision values in %.3f s, test AUC %.4f"
          % (cv["best_C"], info["iterations"], info["form"], info["n_sv"], time.time() - t0, auc_svm))
    if auc_svm < 0.9:
        raise SystemExit("test AUC %.4f of the resident SVM is below 0.9" % auc_svm)

    # third, the reference's own model family on the device: kernel_type="linear" trains on the ROWS of the kernel (the model
    # of the LinearSVC above and of FastSK::fit's default), through the rows kernel K2 built beside the triangle. Its C lives
    # on another scale — about 100 where the gapped-k-mer kernel needs 1 — so the grid reaches 10^3.
    t0 = time.time()
    cv = k.cross_validate_svm(labels, Cs=(1, 10, 100, 1000), kernel_type="linear", refit=True)
    info = cv["refit"]
    auc_rows = roc_auc_score(Ytest, k.decision_function_np("test"))
    rows = k.rows_kernel_info()
    print("kernel_type=\"linear\": rows kernel built in %.1f + %.1f ms (%d tiles of %d), out-of-fold AUC %s, best C %g: %d iterations, "
          "sweep + fit + decision values in %.3f s, test AUC %.4f"
          % (rows["ms_scratch"], rows["ms_product"], rows["tiles"], rows["tile"], ", ".join("%.4f" % a for a in cv["auc"]), cv["best_C"],
             info["iterations"], time.time() - t0, auc_rows))
    if auc_rows < 0.9:
        raise SystemExit("test AUC %.4f of the SVM on the kernel rows is below 0.9" % auc_rows)

    # fourth, what the reference's svm_parameter carries as weight / probability = 1: a class-weighted fit ("balanced": n / (2 n_pos),
    # n / (2 n_neg)) with Platt's sigmoid fitted on the out-of-fold decision values of five fold solves run side by side, and
    # P(y = +1) of the test rows — a ranking like the reference's score(), which sorts by svm_predict_probability
    t0 = time.time()
    info = k.fit_svm(labels, C=1.0, class_weight="balanced", probability=True)
    auc_proba = roc_auc_score(Ytest, k.predict_proba_np("test"))
    print("balanced, calibrated C-SVC: weights (%.3f, %.3f), %d iterations, Platt A = %.4f, B = %.4f after %d Newton steps "
          "(%d fold launches, %.1f ms), fit + calibration + probabilities in %.3f s, test AUC of P(+1) %.4f"
          % (info["class_weight"] + (info["iterations"], info["platt"]["A"], info["platt"]["B"], info["platt"]["iterations"],
                                     info["platt"]["launches"], info["platt"]["ms"], time.time() - t0, auc_proba)))
    if auc_proba < 0.9:
        raise SystemExit("test AUC %.4f of the calibrated probabilities is below 0.9" % auc_proba)


if __name__ == "__main__":
    main()
