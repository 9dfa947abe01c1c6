"""Inputs and yardsticks of the one-vs-one multi-class C-SVC (fsk_svm_train_multiclass / fsk_svm_multiclass_decision /
fsk_svm_multiclass_cv, ``fit_svm_multiclass`` / ``predict_class_np`` / ``cross_validate_svm_multiclass``), shared by
tests/test_emu_svm_multiclass.py (CPU emulation, reduced sizes) and tests/test_gpu_svm_multiclass.py (MI355X). Nothing here
touches an engine.

``expected``       pair p over classes (a, b), a < b, lexicographic: tests/svm_cases.py's ``solve`` (``solve_w`` under class
                   weights) on ``K[np.ix_(idx, idx)]``, ``idx`` the rows of class a or b ascending, a as +1 and b as -1: alpha,
                   rho, objective, gap, iterations, n_sv and n_bsv bit for bit.
``decisions``      the wave's summation restated: 64 lane sums over the list positions mod 64 in order, zero coefficients
                   skipped, then ``v = v + v[lanes ^ d]`` for d = 32 .. 1, minus rho: the pairs' decision values bit for bit.
``vote``           LIBSVM's rule: dec > 0 votes for a, anything else for b; most votes, the lowest class among equals.
``expected_cv``    the same per problem ``(c F + f) P + p`` on the pair's rows with ``fold != f``; ``oof_labels`` the vote of
                   the problems of (c, fold[t]); the accuracy an integer count divided once."""
import numpy as np

import svm_cases as cases
import svm_weighted_cases as wc

LANES = np.arange(64)
# one planted 8-mer a class (class c takes MOTIFS[c % 8] shifted by c // 8 in the alphabet)
MOTIFS = [[1, 3, 3, 2, 4, 1, 2, 2], [4, 4, 1, 2, 3, 3, 1, 4], [2, 1, 4, 4, 3, 2, 1, 1], [3, 2, 2, 1, 1, 4, 4, 3],
          [1, 1, 2, 3, 4, 4, 3, 2], [4, 2, 3, 1, 4, 2, 3, 1], [2, 2, 4, 1, 3, 3, 4, 2], [3, 4, 1, 1, 2, 4, 2, 3]]


# ---- data -------------------------------------------------------------------------------------------------------------------
def dna(sizes, n_test, length, seed, planted=0.8, labels=None):
    """sum(sizes) + n_test sequences of ``length`` tokens 1..4 (PCG64). The classes of the training rows are a permutation of
    ``sizes[c]`` copies of c (so a pair's rows interleave: ascending row order is not class order); test rows draw a class
    at random. Class c's motif overwrites a random place of ``planted`` of its rows. ``labels[c]`` is the label value of
    class index c (default c). -> (int32 [n, length], int32 labels of all rows)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    k, n_train = len(sizes), int(sum(sizes))
    cls = rng.permutation(np.repeat(np.arange(k), sizes))
    cls = np.concatenate([cls, rng.integers(0, k, size=n_test)])
    X = rng.integers(1, 5, size=(n_train + n_test, length), dtype=np.int32)
    for r, c in enumerate(cls.tolist()):
        motif = [(v - 1 + c // 8) % 4 + 1 for v in MOTIFS[c % 8]]
        at, coin = int(rng.integers(0, length - len(motif) + 1)), float(rng.random())
        if coin < planted:
            X[r, at:at + len(motif)] = motif
    values = np.arange(k, dtype=np.int64) if labels is None else np.asarray(labels, dtype=np.int64)
    return X, values[cls].astype(np.int32)


def case(sizes, n_test=0, length=24, g=6, m=2, C=1.0, eps=1e-3, seed=None, labels=None, **engine):
    """One problem in the style of svm_cases.edge_case: short sequences and few combinations, the solver sees the shapes."""
    n_train = int(sum(sizes))
    X, y = dna(sizes, n_test, length, 9100 + 31 * n_train + len(sizes) if seed is None else seed, labels=labels)
    return {"X": X, "y": y[:n_train].copy(), "y_all": y, "n_train": n_train, "n_test": n_test, "g": g, "m": m, "C": float(C),
            "eps": float(eps), "engine": engine, "sizes": tuple(sizes)}


def foreign_test_row(c):
    """The last test row shares no g-mer (at up to m mismatches the kernel still counts: so no SYMBOL) with any training
    row: token 5 throughout. Every pair's decision value of that row is -rho."""
    assert c["n_test"] >= 1
    c["X"][-1] = 5
    return c


# ---- the model, restated ----------------------------------------------------------------------------------------------------
def pairs_of(y, keep=None):
    """(classes ascending, [(a, b, idx, y_pm)] in pair order): idx the rows of class a or b (and ``keep``), ascending."""
    y = np.asarray(y)
    classes = np.unique(y)
    keep = np.ones(len(y), dtype=bool) if keep is None else np.asarray(keep)
    out = []
    for a in range(len(classes)):
        for b in range(a + 1, len(classes)):
            idx = np.flatnonzero(((y == classes[a]) | (y == classes[b])) & keep)
            out.append((a, b, idx, np.where(y[idx] == classes[a], 1, -1).astype(np.int32)))
    return classes, out


def weights_of(classes, class_weight):
    """One weight a class in ascending class order from None or a dict keyed by label (a missing class is 1)."""
    if class_weight is None:
        return None
    return np.array([float(class_weight.get(int(c), 1.0)) for c in classes])


def balanced(y):
    classes, counts = np.unique(np.asarray(y), return_counts=True)
    return {int(c): len(y) / (float(len(classes)) * float(q)) for c, q in zip(classes, counts)}


def solve_pair(Ks, ys, C, wa, wb, eps, max_iter):
    if wa is None:
        return cases.solve(Ks, ys, float(C), eps, max_iter)
    return wc.solve_w(Ks, ys, float(C) * wa, float(C) * wb, eps, max_iter)   # (each product once)


def expected(K, y, C, eps, max_iter=-1, class_weight=None, keep=None):
    """The restatement's model: ``classes`` and per pair the result of ``solve`` with ``a``, ``b``, ``idx``, ``coef``."""
    K = np.asarray(K, dtype=np.float64)
    classes, pairs = pairs_of(y, keep)
    w = weights_of(classes, class_weight)
    out = []
    for a, b, idx, ys in pairs:
        r = solve_pair(K[np.ix_(idx, idx)], ys, C, None if w is None else w[a], None if w is None else w[b], eps, max_iter)
        r.update(a=a, b=b, idx=idx, coef=r["alpha"] * ys.astype(np.float64), class_a=int(classes[a]), class_b=int(classes[b]))
        out.append(r)
    return classes, out


def wave_sum(coef, cells):
    """The wave's sums of coef[q] * cells[r, q] over the list, a row of ``cells`` a wave: lane L adds its positions L, L + 64,
    ... in order, zero coefficients skipped; then v = v + v[lanes ^ d] for d = 32 .. 1. Every lane ends with the same value."""
    cells = np.atleast_2d(np.asarray(cells, dtype=np.float64))
    v = np.zeros((len(cells), 64))
    for start in range(0, len(coef), 64):
        c = coef[start:start + 64]
        lanes = np.flatnonzero(c != 0.0)
        v[:, lanes] = v[:, lanes] + c[None, lanes] * cells[:, start + lanes]
    for d in (32, 16, 8, 4, 2, 1):
        v = v + v[:, LANES ^ d]
    assert np.all((v == v[:, :1]) | np.isnan(v))
    return v[:, 0]


def decisions(K_rows, model):
    """[rows, P] decision values of the rows whose kernel against the training rows is ``K_rows`` [rows, n_train]."""
    K_rows = np.asarray(K_rows, dtype=np.float64)
    out = np.empty((len(K_rows), len(model)))
    for p, w in enumerate(model):
        out[:, p] = wave_sum(w["coef"], K_rows[:, w["idx"]]) - w["rho"]
    return out


def votes(dec, model, k):
    """[rows, k] vote counts: dec > 0 votes for a, anything else for b."""
    v = np.zeros((len(dec), k), dtype=np.int64)
    for p, w in enumerate(model):
        for_a = dec[:, p] > 0
        v[for_a, w["a"]] += 1
        v[~for_a, w["b"]] += 1
    return v


def vote(dec, model, classes):
    """(labels [rows], vote counts): np.argmax takes the first of equal maxima, the lowest class."""
    v = votes(dec, model, len(classes))
    return np.asarray(classes)[np.argmax(v, axis=1)].astype(np.int32), v


def tied_rows(v):
    """Rows whose two highest vote counts are equal."""
    s = np.sort(v, axis=1)
    return np.flatnonzero(s[:, -1] == s[:, -2])


# ---- cross-validation -------------------------------------------------------------------------------------------------------
def expected_cv(K, y, fold, Cs, eps, max_iter=-1, class_weight=None):
    """(classes, problems in the engine's order (c F + f) P + p, each with ``C`` and ``fold``)."""
    F = int(np.max(fold)) + 1
    out, classes = [], None
    for C in Cs:
        for f in range(F):
            classes, model = expected(K, y, float(C), eps, max_iter, class_weight, keep=np.asarray(fold) != f)
            for w in model:
                w.update(C=float(C), fold=f)
            out.extend(model)
    return classes, out


def oof_labels(K, y, fold, classes, problems, n_C):
    """[n_C, n] out-of-fold labels: row t under the P problems of (c, fold[t]); and the accuracy per C."""
    K = np.asarray(K, dtype=np.float64)
    fold = np.asarray(fold)
    F = int(np.max(fold)) + 1
    k = len(classes)
    P = k * (k - 1) // 2
    pred = np.empty((n_C, len(y)), dtype=np.int32)
    for c in range(n_C):
        for f in range(F):
            model = problems[(c * F + f) * P:(c * F + f + 1) * P]
            rows = np.flatnonzero(fold == f)
            pred[c, rows] = vote(decisions(K[rows], model), model, classes)[0]
    acc = np.array([float(int((pred[c] == np.asarray(y)).sum())) / float(len(y)) for c in range(n_C)])
    return pred, acc
