"""Yardsticks of the multi-class probabilities (fsk_exp_neg, fsk_svm_multiclass_calibrate / _set_calibration / _proba;
``fit_svm_multiclass(probability=True)``, ``predict_proba_np``), shared by tests/test_emu_svm_multiclass_proba.py (CPU
emulation) and tests/test_gpu_svm_multiclass_proba.py (MI355X). Nothing here touches an engine.

``exp_neg``          fsk_exp_neg restated on Python floats (IEEE doubles, one rounding an operation): bit for bit.
``pair_prob``        LIBSVM's sigmoid_predict with that exponential and the clamp of svm_predict_probability.
``couple``           LIBSVM's multiclass_probability in its own summation orders -> (p [k], iterations).
``proba``            rows of pair decisions -> (prob [rows, k], argmax class index, iterations): what k_svm_ovo_proba gives.
``proba_libm``       the same with ``math.exp``: LIBSVM's own arithmetic, the second yardstick (``agree`` compares the two).
``calibration``      fsk_svm_multiclass_calibrate restated: svm_multiclass_cases.expected_cv at the model's one C, the
                     out-of-fold pair decisions by ``wave_sum``, svm_weighted_cases.platt_fit on every pair."""
import math
import struct

import numpy as np

import svm_multiclass_cases as mc
import svm_weighted_cases as wc

INV_LN2 = float.fromhex("0x1.71547652b82fep+0")
LN2_HI = float.fromhex("0x1.62e42fee00000p-1")     # 32 trailing zero bits: n * LN2_HI is exact for |n| < 2^21
LN2_LO = float.fromhex("0x1.a39ef35793c76p-33")
COEF = [1.0 / float(math.factorial(i)) for i in range(14)]   # 1 / i!, each the double nearest to it
MIN_PROB = 1e-7
MAX_PROB = 1 - 1e-7


# ---- the exponential --------------------------------------------------------------------------------------------------------
def exp_neg(x):
    """fsk_exp_neg: NaN -> NaN, x < -708 -> 0.0, else Cody-Waite by ln 2, the Taylor polynomial of degree 13 by Horner, 2^n from
    its exponent bits."""
    x = float(x)
    if x != x:
        return x
    if x < -708.0:
        return 0.0
    n = math.floor(x * INV_LN2 + 0.5)
    r = (x - n * LN2_HI) - n * LN2_LO
    q = COEF[13]
    for i in range(12, -1, -1):
        q = q * r + COEF[i]
    return q * struct.unpack("<d", struct.pack("<q", (int(n) + 1023) << 52))[0]


def bits(x):
    return struct.unpack("<q", struct.pack("<d", float(x)))[0]


def ulps(a, b):
    """The distance of two positive finite doubles (or zeros) in units of the last place."""
    return abs(bits(a) - bits(b))


def exp_points(seed=20260, n=100000):
    """The arguments of the host comparison: the breakpoints, the n-boundaries (n +- 1/2) ln 2 to one ulp either side, and
    ``n`` seeded points (half of them uniform in [-708, 0], half with a uniform exponent so that small arguments occur)."""
    pts = [-708.0, math.nextafter(-708.0, -math.inf), math.nextafter(-708.0, 0.0), -0.0, 0.0, float("nan"), -math.inf, -709.0, -1e300,
           -5e-324, -2.0 ** -1022, -1e-300, -1e-17, -1.0, -0.5 * math.log(2.0)]
    for k in range(0, 1022):
        for half in (-0.5, 0.5):
            b = -(k + half) * math.log(2.0)
            if -708.0 <= b <= 0.0:
                pts += [math.nextafter(b, -math.inf), b, math.nextafter(b, 0.0)]
    rng = np.random.Generator(np.random.PCG64(seed))
    pts += (-708.0 * rng.random(n // 2)).tolist()
    pts += (-(2.0 ** rng.uniform(-60.0, math.log2(708.0), n - n // 2))).tolist()
    return pts


# ---- the sigmoid and the coupling -------------------------------------------------------------------------------------------
def pair_prob(v, A, B, exp=exp_neg):
    """sigmoid_predict(v, A, B) clamped to [1e-7, 1 - 1e-7] with LIBSVM's own comparisons (a NaN becomes 1e-7)."""
    fApB = float(v) * float(A) + float(B)
    if fApB >= 0:
        e = exp(-fApB)
        s = e / (1.0 + e)
    else:
        s = 1.0 / (1 + exp(fApB))
    x = s if s > MIN_PROB else MIN_PROB
    return x if x < MAX_PROB else MAX_PROB


def libm_exp(x):
    try:
        return math.exp(x)
    except OverflowError:                 # (never: the arguments are <= 0)
        return math.inf


def couple(r):
    """multiclass_probability(k, r, p) on Python floats, operation for operation. r [k][k] with r[j][i] = 1 - r[i][j]."""
    k = len(r)
    max_iter = max(100, k)
    eps = 0.005 / k
    p = [1.0 / k] * k
    Q = [[0.0] * k for _ in range(k)]
    Qp = [0.0] * k
    for t in range(k):
        for j in range(t):
            Q[t][t] += r[j][t] * r[j][t]
            Q[t][j] = Q[j][t]
        for j in range(t + 1, k):
            Q[t][t] += r[j][t] * r[j][t]
            Q[t][j] = -r[j][t] * r[t][j]
    it = 0
    while it < max_iter:
        pQp = 0.0
        for t in range(k):
            Qp[t] = 0.0
            for j in range(k):
                Qp[t] += Q[t][j] * p[j]
            pQp += p[t] * Qp[t]
        max_error = 0.0
        for t in range(k):
            error = abs(Qp[t] - pQp)
            if error > max_error:
                max_error = error
        if max_error < eps:
            break
        for t in range(k):
            diff = (-Qp[t] + pQp) / Q[t][t]
            p[t] += diff
            pQp = (pQp + diff * (diff * Q[t][t] + 2 * Qp[t])) / (1 + diff) / (1 + diff)
            for j in range(k):
                Qp[j] = (Qp[j] + diff * Q[t][j]) / (1 + diff)
                p[j] /= (1 + diff)
        it += 1
    return p, it


def proba(dec, A, B, k, exp=exp_neg):
    """svm_predict_probability on every row of ``dec`` [rows, P] -> (prob [rows, k] float64, argmax class INDEX [rows] — the
    first of equal maxima, as LIBSVM's loop —, iterations [rows] int32; 0 for k = 2)."""
    dec = np.atleast_2d(np.asarray(dec, dtype=np.float64))
    rows = len(dec)
    prob, best, iters = np.empty((rows, k)), np.empty(rows, dtype=np.int64), np.zeros(rows, dtype=np.int32)
    for row in range(rows):
        r = [[0.0] * k for _ in range(k)]
        q = 0
        for i in range(k):
            for j in range(i + 1, k):
                r[i][j] = pair_prob(dec[row, q], A[q], B[q], exp)
                r[j][i] = 1 - r[i][j]
                q += 1
        if k == 2:
            p, it = [r[0][1], r[1][0]], 0
        else:
            p, it = couple(r)
        top = 0
        for i in range(1, k):
            if p[i] > p[top]:
                top = i
        prob[row], best[row], iters[row] = p, top, it
    return prob, best, iters


def proba_libm(dec, A, B, k):
    return proba(dec, A, B, k, exp=libm_exp)


def agree(ours, libm, k, name=""):
    """The two yardsticks on one case: where the iteration counts agree |dp| <= 1e-9 (far above the rounding of a <= 2-ulp exp
    through a few hundred operations, four orders below the stopping tolerance 0.005 / k); rows where they differ are at most
    1 % of the case and agree within 0.005 (k steps of the tolerance)."""
    (p0, _, i0), (p1, _, i1) = ours, libm
    same = i0 == i1
    d = np.abs(p0 - p1).max(axis=1) if len(p0) else np.zeros(0)
    assert np.all(d[same] <= 1e-9), (name, float(d[same].max()))
    assert int((~same).sum()) * 100 <= len(same), (name, int((~same).sum()), len(same))
    assert np.all(d[~same] <= 0.005), (name, float(d[~same].max()))
    return int((~same).sum())


# ---- chosen sigmoids --------------------------------------------------------------------------------------------------------
def pair_list(k):
    return [(a, b) for a in range(k) for b in range(a + 1, k)]


def seeded_sigmoids(k, seed):
    """Plausible fits: A in [-6, -0.5] (a positive decision favours class a), B in [-0.7, 0.7]."""
    rng = np.random.Generator(np.random.PCG64(seed))
    P = k * (k - 1) // 2
    return -rng.uniform(0.5, 6.0, P), rng.uniform(-0.7, 0.7, P)


def constant_sigmoids(k, wins):
    """A = 0 and B = -+800: pair (a, b) gives r[a][b] clamped at 1 - 1e-7 where ``wins(a, b)`` (class a beats b), else at 1e-7,
    whatever the decision value (a NaN decision still gives NaN * 0 = NaN -> 1e-7; the tests' decisions are numbers)."""
    pairs = pair_list(k)
    return np.zeros(len(pairs)), np.array([-800.0 if wins(a, b) else 800.0 for a, b in pairs])


def cyclic(k):
    """The cyclic tournament: a beats b when (b - a) mod k <= (k - 1) div 2."""
    return lambda a, b: (b - a) % k <= (k - 1) // 2


# ---- the calibration, restated ----------------------------------------------------------------------------------------------
def calibration(K, y, fold, C, eps, max_iter=-1, class_weight=None):
    """fsk_svm_multiclass_calibrate on the train x train kernel ``K``: (oof [n, P], the P fits of svm_weighted_cases.platt_fit,
    the fold problems, the classes). Problem f P + p is pair p on its rows with fold != f; oof[t, p] is row t's decision
    under problem fold[t] P + p in the wave's summation; pair p's fit runs on the oof values of the rows of classes a and b,
    ascending, label +1 for class a."""
    K = np.asarray(K, dtype=np.float64)
    y, fold = np.asarray(y), np.asarray(fold)
    classes, problems = mc.expected_cv(K, y, fold, [float(C)], eps, max_iter, class_weight)
    k = len(classes)
    P = k * (k - 1) // 2
    F = int(fold.max()) + 1
    oof = np.empty((len(y), P))
    for f in range(F):
        rows = np.flatnonzero(fold == f)
        oof[rows] = mc.decisions(K[rows], problems[f * P:(f + 1) * P])
    fits = []
    for p, (a, b) in enumerate(pair_list(k)):
        rows = np.flatnonzero((y == classes[a]) | (y == classes[b]))
        fits.append(wc.platt_fit(oof[rows, p], np.where(y[rows] == classes[a], 1, -1)))
    return oof, fits, problems, classes
