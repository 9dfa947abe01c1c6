"""Inputs and yardsticks of the cross-validated SVM (fsk_svm_cv, ``Engine.svm_cv``, ``FastSK.cross_validate_svm``), shared by
tests/test_emu_svm_cv.py (CPU emulation, reduced sizes) and tests/test_gpu_svm_cv.py (MI355X). Nothing here touches an engine.

The yardstick of problem ``p = c * F + f`` is tests/svm_cases.py's ``solve`` on ``K[np.ix_(idx, idx)]``, ``idx`` the rows with
``fold != f`` in row order, at ``Cs[c]``: alpha, rho, the objective, the gap and the iteration count bit for bit. The
out-of-fold decision value of row t at ``Cs[c]`` is that of problem ``c * F + fold[t]``, within ``decision_reference``'s bound
of numpy's sum over the full-length coefficient vector. The metrics are restated from the header's formulas."""
import numpy as np

import svm_cases as cases


def blocks(*runs):
    """Fold ids by runs of rows: ``blocks((1, 2), (0, 64))`` puts rows 0-1 in fold 1 and rows 2-65 in fold 0."""
    return np.concatenate([np.full(count, f, dtype=np.int32) for f, count in runs])


def paired(n, n_folds):
    """``(t // 2) % n_folds``: svm_cases.dna alternates the labels by row, so rows leave in pairs of both classes."""
    return ((np.arange(n) // 2) % n_folds).astype(np.int32)


def n_folds_of(fold):
    return int(np.max(fold)) + 1


def expected(K, y, fold, Cs, eps, max_iter=-1):
    """The restatement's result of every problem, in the engine's order, with ``idx``, ``C``, ``fold`` and ``alpha_full``."""
    K = np.asarray(K, dtype=np.float64)
    y = np.asarray(y)
    F = n_folds_of(fold)
    subs = []
    for f in range(F):
        idx = np.flatnonzero(np.asarray(fold) != f)
        subs.append((idx, K[np.ix_(idx, idx)], y[idx]))
    out = []
    for C in Cs:
        for f, (idx, Ks, ys) in enumerate(subs):
            w = cases.solve(Ks, ys, float(C), eps, max_iter)
            full = np.zeros(len(y))
            full[idx] = w["alpha"]
            w.update(idx=idx, C=float(C), fold=f, alpha_full=full)
            out.append(w)
    return out


def oof_reference(K, y, fold, want, n_C):
    """(numpy's out-of-fold decision values [n_C, n] from the problems' own models, the summation bound of every entry)."""
    F = n_folds_of(fold)
    ref, bound = np.empty((n_C, len(y))), np.empty((n_C, len(y)))
    for p, w in enumerate(want):
        c, f = divmod(p, F)
        rows = np.flatnonzero(np.asarray(fold) == f)
        ref[c, rows], bound[c, rows] = cases.decision_reference(np.asarray(K)[rows], y, w["alpha_full"], w["rho"])
    return ref, bound


def auc_restated(dec, y):
    """((#{pos > neg} + 0.5 #{pos == neg}) / (n_pos n_neg), #{pos == neg}): integer counts, then one multiply, one add and one
    divide in double."""
    pos, neg = dec[np.asarray(y) > 0], dec[np.asarray(y) < 0]
    above = int((pos[:, None] > neg[None, :]).sum())
    level = int((pos[:, None] == neg[None, :]).sum())
    return (float(above) + 0.5 * float(level)) / float(len(pos) * len(neg)), level


def accuracy_restated(dec, y):
    return float(int(((dec > 0) == (np.asarray(y) > 0)).sum())) / float(len(y))


def stratified_folds_restated(labels, k, seed=0):
    """fastsk_amd.stratified_folds as documented: walk PCG64(seed)'s permutation, the c-th row met of a class gets c % k."""
    order = np.random.Generator(np.random.PCG64(seed)).permutation(len(labels))
    fold, met = np.zeros(len(labels), dtype=np.int32), {}
    for t in order:
        key = int(labels[t])
        fold[t] = met.get(key, 0) % k
        met[key] = met.get(key, 0) + 1
    return fold
