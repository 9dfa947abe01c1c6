#!/usr/bin/env python3
"""Generate tests/golden/webkb_slice.npz (build container only): a slice of the reference's four-class dataset
(data/webkb-train.fasta / data/webkb-test.fasta, labels 0..3) with scikit-learn's one-vs-one result on it, for
tests/test_gpu_svm_multiclass.py.

The slice: every line lower-cased, documents under 60 characters skipped; in file order the first 30 / 50 / 64 / 96 training
documents of classes 0 / 1 / 2 / 3 (kept in file order, so the classes interleave) and the first 20 test documents of each
class; each cut at 160 characters; symbols numbered by first appearance from 1 (240 + 80 rows, 27 symbols).
  tokens, offsets, n_train, labels    the 320 sequences (train rows first) and their labels;
  g, m                                8, 4;
  sk_dec_test, sk_dec_train           scikit-learn's SVC(kernel="precomputed", C=1, tol=1e-3, shrinking=False,
  sk_pred_test, sk_pred_train         decision_function_shape="ovo") on the normalised g = 8, m = 4 kernel of the CPU oracle: the
                                      six pair decisions (columns (0,1), (0,2), (0,3), (1,2), (1,3), (2,3)) and the predictions.
Only data travels."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(HERE, "golden", "webkb_slice.npz")
REF_DATA = "/root/reference/data"
G, M = 8, 4
TRAIN_TAKE, TEST_TAKE, MIN_LEN, CUT = (30, 50, 64, 96), (20, 20, 20, 20), 60, 160


def documents(path, take):
    """(texts, labels) of the first take[c] documents of class c, in file order."""
    with open(path) as f:
        lines = [ln.strip().lower() for ln in f.read().split("\n")]
    if lines and lines[-1] == "":
        lines.pop()
    left, texts, labels = list(take), [], []
    for head, text in zip(lines[0::2], lines[1::2]):
        c = int(head[1:])
        if len(text) < MIN_LEN or left[c] == 0:
            continue
        left[c] -= 1
        texts.append(text[:CUT])
        labels.append(c)
    assert left == [0] * len(take), left
    return texts, labels


def main():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    from oracle import loader
    from sklearn.svm import SVC
    tr, ytr = documents(os.path.join(REF_DATA, "webkb-train.fasta"), TRAIN_TAKE)
    te, yte = documents(os.path.join(REF_DATA, "webkb-test.fasta"), TEST_TAKE)
    ids, seqs = {}, []
    for text in tr + te:
        seqs.append([ids.setdefault(ch, len(ids) + 1) for ch in text])
    tok, off = loader.flatten(seqs)
    n, nt = len(tr), len(te)
    tri, _, _ = loader.port().compute(tok, off, n, nt, G, M, t=1)
    N = n + nt
    K = np.zeros((N, N))
    K[np.tril_indices(N)] = tri
    K = K + np.tril(K, -1).T
    clf = SVC(kernel="precomputed", C=1.0, tol=1e-3, shrinking=False, decision_function_shape="ovo").fit(K[:n, :n], ytr)
    assert clf.classes_.tolist() == [0, 1, 2, 3]
    out = {}
    for name, rows in (("test", slice(n, N)), ("train", slice(0, n))):
        out["sk_dec_" + name] = clf.decision_function(K[rows, :n])
        out["sk_pred_" + name] = clf.predict(K[rows, :n]).astype(np.int32)
    np.savez_compressed(OUT, tokens=tok.astype(np.int32), offsets=off.astype(np.int64), n_train=np.int64(n),
                        labels=np.array(ytr + yte, dtype=np.int32), g=np.int64(G), m=np.int64(M), **out)
    acc = float((out["sk_pred_test"] == np.array(yte)).mean())
    print("%s: %d + %d rows, %d symbols, %d bytes, scikit-learn's test accuracy %.4f" % (OUT, n, nt, len(ids), os.path.getsize(OUT), acc))


if __name__ == "__main__":
    main()
