"""Inputs and yardsticks of the class-weighted C-SVC and the Platt calibration (fsk_svm_set_class_weights, fsk_svm_platt_fit,
fsk_svm_calibrate, fsk_svm_proba), shared by tests/test_emu_svm_weighted.py (CPU emulation, small scale) and
tests/test_gpu_svm_weighted.py (MI355X). Nothing here touches an engine.

``solve_w``     tests/svm_cases.py's ``solve`` with the box of row t ``C_t = Cp`` where ``y_t > 0`` and ``Cn`` where ``y_t < 0``:
                the expectation of alpha, rho, the objective, the gap, the iteration count, ``n_sv`` and ``n_bsv``, bit for bit,
                and a counter of the branches its steps took (``BRANCHES``).
``certify_w``   a solution checked from K, y and alpha alone, with per-class boxes.
``sklearn_objective_w``  the dual objective of scikit-learn's SVC(kernel="precomputed", class_weight={1: w_pos, -1: w_neg}).
``platt_fit``   LIBSVM's sigmoid_train on Python floats with ``math.exp`` / ``math.log``: the libm of the process, one
                rounding an operation, so A, B, the iteration count and the status compare bit for bit.
``sigmoid_predict``  LIBSVM's, both branches."""
import collections
import math

import numpy as np

import svm_cases as cases

TAU = cases.TAU
# the branches of a step that the weighted code adds or decides differently (a case set must reach every one)
BRANCHES = ("mixed_clip_i", "mixed_clip_j", "mixed_clip_i_between", "mixed_clip_j_between")


# ---- data -------------------------------------------------------------------------------------------------------------------
def few_positives_case(C=1.0):
    """64 rows, 3 positives."""
    y = -np.ones(64, dtype=np.int32)
    y[[5, 37, 50]] = 1
    return cases.case(64, 40, 6, 2, C=C, labels=y, seed=6403)


def boxes(c, weights):
    """(w_pos, w_neg, Cp, Cn) of a case under ``weights`` (a pair or "balanced"): each product formed once."""
    if weights == "balanced":
        n, n_pos = len(c["y"]), int((c["y"] > 0).sum())
        weights = (n / (2.0 * n_pos), n / (2.0 * (n - n_pos)))
    w_pos, w_neg = float(weights[0]), float(weights[1])
    return w_pos, w_neg, c["C"] * w_pos, c["C"] * w_neg


# ---- the algorithm, restated with C_t ------------------------------------------------------------------------------------------
def rho_and_objective_w(alpha, G, y, Cp, Cn):
    """LIBSVM's calculate_rho and objective, in index order, one rounding an operation; upper bound of row t: C_t."""
    ub, lb, sum_free, n_free, obj = math.inf, -math.inf, 0.0, 0, 0.0
    for a, g, t in zip(alpha.tolist(), G.tolist(), y.tolist()):
        yg = g if t > 0 else -g
        if a >= (Cp if t > 0 else Cn):
            if t < 0:
                ub = min(ub, yg)
            else:
                lb = max(lb, yg)
        elif a <= 0.0:
            if t > 0:
                ub = min(ub, yg)
            else:
                lb = max(lb, yg)
        else:
            n_free += 1
            sum_free += yg
        obj += a * (g - 1.0)
    rho = sum_free / n_free if n_free else (ub + lb) / 2.0
    return rho, obj / 2.0


def step_w(yi, yj, Kij, Gi, Gj, Cp, Cn, ai, aj, taken):
    """The two-variable update of LIBSVM's Solver::Solve with Q_ii = Q_jj = 1 and C_i, C_j by class; ``taken`` counts the
    branches. -> (alpha_i, alpha_j, tau used)."""
    Ci, Cj = (Cp if yi > 0 else Cn), (Cp if yj > 0 else Cn)
    Qij = Kij if yi == yj else -Kij
    tau = False
    if yi != yj:
        quad = 2.0 + 2.0 * Qij
        if quad <= 0.0:
            quad, tau = TAU, True
        delta = (-Gi - Gj) / quad
        diff = ai - aj
        ai = ai + delta
        aj = aj + delta
        if diff > 0.0:
            if aj < 0.0:
                aj, ai = 0.0, diff
        else:
            if ai < 0.0:
                ai, aj = 0.0, -diff
        d = Ci - Cj
        between = min(0.0, d) < diff < max(0.0, d)   # (here the unweighted test, diff > 0, decides the other way)
        if diff > d:
            if ai > Ci:
                ai, aj = Ci, Ci - diff
                taken["mixed_clip_i"] += 1
                taken["mixed_clip_i_between"] += int(between)
        else:
            if aj > Cj:
                aj, ai = Cj, Cj + diff
                taken["mixed_clip_j"] += 1
                taken["mixed_clip_j_between"] += int(between)
    else:
        C = Ci
        quad = 2.0 - 2.0 * Qij
        if quad <= 0.0:
            quad, tau = TAU, True
        delta = (Gi - Gj) / quad
        s = ai + aj
        ai = ai - delta
        aj = aj + delta
        if s > C:
            if ai > C:
                ai, aj = C, s - C
                taken["same_clip_i"] += 1
        else:
            if aj < 0.0:
                aj, ai = 0.0, s
        if s > C:
            if aj > C:
                aj, ai = C, s - C
                taken["same_clip_j"] += 1
        else:
            if ai < 0.0:
                ai, aj = 0.0, s
    return ai, aj, tau


def solve_w(K, y, Cp, Cn, eps, max_iter=-1):
    """``svm_cases.solve`` with the box of row t chosen by its class. Every operation is one IEEE double operation."""
    K = np.asarray(K, dtype=np.float64)
    n = len(y)
    yf = np.asarray(y, dtype=np.float64)
    pos = yf > 0
    Ct = np.where(pos, float(Cp), float(Cn))
    alpha = np.zeros(n)
    G = -np.ones(n)
    if max_iter < 0:
        max_iter = cases.DEFAULT_MAX_ITER
    it, converged, tau_steps, tau_selected, pairs = 0, False, 0, 0, []
    taken = collections.Counter()
    while True:
        v = np.where(pos, -G, G)
        up = np.where(pos, alpha < Ct, alpha > 0.0)
        low = np.where(pos, alpha > 0.0, alpha < Ct)
        vu = np.where(up, v, -np.inf)
        i = int(np.argmax(vu))            # (the first of equal maxima)
        gmax = float(vu[i])
        gmin = float(np.min(np.where(low, v, np.inf)))
        if gmax - gmin <= eps:
            converged = True
            break
        if it >= max_iter:
            break
        Ki = K[i]
        b = gmax - v
        a = 2.0 - 2.0 * Ki
        cand = low & (b > 0.0)
        tau_selected += int(np.any(cand & (a <= 0.0)))
        a = np.where(a <= 0.0, TAU, a)
        obj = np.where(cand, -((b * b) / a), np.inf)
        cand &= ~np.isnan(obj)
        if not cand.any():
            break
        j = int(np.argmin(np.where(cand, obj, np.inf)))   # (the first of equal minima)
        yi, yj = int(y[i]), int(y[j])
        ai0, aj0 = float(alpha[i]), float(alpha[j])
        ai, aj, tau = step_w(yi, yj, float(Ki[j]), float(G[i]), float(G[j]), float(Cp), float(Cn), ai0, aj0, taken)
        tau_steps += int(tau)
        taken["tau_mixed_weights"] += int(tau and yi != yj and Cp != Cn)
        dai, daj = ai - ai0, aj - aj0
        Qi = np.where(yf == yi, Ki, -Ki)
        Qj = np.where(yf == yj, K[j], -K[j])
        G = G + ((Qi * dai) + (Qj * daj))
        alpha[i], alpha[j] = ai, aj
        pairs.append((i, j))
        it += 1
    rho, objective = rho_and_objective_w(alpha, G, y, float(Cp), float(Cn))
    return {"alpha": alpha, "G": G, "rho": rho, "objective": objective, "iterations": it, "converged": converged,
            "gap": gmax - gmin, "n_sv": int((alpha > 0).sum()), "n_bsv": int((alpha >= Ct).sum()), "tau_steps": tau_steps,
            "tau_selected": tau_selected, "pairs": pairs, "branches": taken}


# ---- a solution certified from K, y, alpha alone -------------------------------------------------------------------------------
def certify_w(K, y, alpha, Cp, Cn, eps):
    """``svm_cases.certify`` with per-class boxes: 0 <= alpha_t <= C_t; |y^T alpha| <= 2^-52 sum_t C_t; the gap of the RECOMPUTED
    gradient at most eps up to the rounding bound of that recomputation."""
    K = np.asarray(K, dtype=np.float64)
    n = len(y)
    yf = np.asarray(y, dtype=np.float64)
    pos = yf > 0
    Ct = np.where(pos, float(Cp), float(Cn))
    assert alpha.shape == (n,) and np.all(alpha >= 0.0) and np.all(alpha <= Ct)
    balance = abs(math.fsum((yf * alpha).tolist()))
    assert balance <= 2.0 ** -52 * float(Ct.sum()), balance
    Q = (yf[:, None] * yf[None, :]) * K
    G = Q @ alpha - 1.0
    bound = n * 2.0 ** -53 * (np.abs(Q) @ np.abs(alpha))
    v = np.where(pos, -G, G)
    up = np.where(pos, alpha < Ct, alpha > 0.0)
    low = np.where(pos, alpha > 0.0, alpha < Ct)
    iu = int(np.argmax(np.where(up, v, -np.inf)))
    il = int(np.argmin(np.where(low, v, np.inf)))
    gap = float(v[iu] - v[il]) if up.any() and low.any() else -math.inf
    slack = float(bound[iu] + bound[il])
    assert gap <= eps + slack, (gap, eps, slack)
    objective = 0.5 * float(alpha @ (Q @ alpha)) - float(alpha.sum())
    return {"gap": gap, "slack": slack, "balance": balance, "objective": objective}


def sklearn_objective_w(K, y, C, w_pos, w_neg, eps):
    """The dual objective 1/2 a^T Q a - sum a of scikit-learn's (LIBSVM's) weighted solution on the same matrix."""
    from sklearn.svm import SVC
    clf = SVC(kernel="precomputed", C=C, tol=eps, shrinking=False, class_weight={1: w_pos, -1: w_neg}).fit(K, y)
    a = np.zeros(len(y))
    a[clf.support_] = np.abs(clf.dual_coef_[0])
    yf = np.asarray(y, dtype=np.float64)
    Q = (yf[:, None] * yf[None, :]) * np.asarray(K, dtype=np.float64)
    return 0.5 * float(a @ (Q @ a)) - float(a.sum())


# ---- Platt's sigmoid -----------------------------------------------------------------------------------------------------------
def platt_fit(dec, y):
    """LIBSVM's sigmoid_train, operation for operation, on Python floats. -> {A, B, iterations, status, halvings}: status 0 the
    gradient fell below 1e-5, 1 the 100 iterations ran out, 2 the line search failed; halvings counts the halved steps."""
    dec = [float(v) for v in np.asarray(dec).tolist()]
    y = [int(v) for v in np.asarray(y).tolist()]
    l = len(dec)
    prior1 = prior0 = 0.0
    for t in y:
        if t > 0:
            prior1 += 1
        else:
            prior0 += 1
    max_iter, min_step, sigma, eps = 100, 1e-10, 1e-12, 1e-5
    hi, lo = (prior1 + 1.0) / (prior1 + 2.0), 1 / (prior0 + 2.0)
    tg = [hi if t > 0 else lo for t in y]

    def value(A, B):
        f = 0.0
        for i in range(l):
            fApB = dec[i] * A + B
            if fApB >= 0:
                f += tg[i] * fApB + math.log(1 + math.exp(-fApB))
            else:
                f += (tg[i] - 1) * fApB + math.log(1 + math.exp(fApB))
        return f

    A, B = 0.0, math.log((prior0 + 1.0) / (prior1 + 1.0))
    fval = value(A, B)
    it, status, halvings = 0, 1, 0
    while it < max_iter:
        h11, h22, h21, g1, g2 = sigma, sigma, 0.0, 0.0, 0.0
        for i in range(l):
            fApB = dec[i] * A + B
            if fApB >= 0:
                p = math.exp(-fApB) / (1.0 + math.exp(-fApB))
                q = 1.0 / (1.0 + math.exp(-fApB))
            else:
                p = 1.0 / (1.0 + math.exp(fApB))
                q = math.exp(fApB) / (1.0 + math.exp(fApB))
            d2 = p * q
            h11 += dec[i] * dec[i] * d2
            h22 += d2
            h21 += dec[i] * d2
            d1 = tg[i] - p
            g1 += dec[i] * d1
            g2 += d1
        if abs(g1) < eps and abs(g2) < eps:
            status = 0
            break
        det = h11 * h22 - h21 * h21
        dA = -(h22 * g1 - h21 * g2) / det
        dB = -(-h21 * g1 + h11 * g2) / det
        gd = g1 * dA + g2 * dB
        stepsize = 1.0
        while stepsize >= min_step:
            newA, newB = A + stepsize * dA, B + stepsize * dB
            newf = value(newA, newB)
            if newf < fval + 0.0001 * stepsize * gd:
                A, B, fval = newA, newB, newf
                break
            stepsize = stepsize / 2.0
            halvings += 1
        if stepsize < min_step:
            status = 2
            break
        it += 1
    return {"A": A, "B": B, "iterations": it, "status": status, "halvings": halvings}


def sigmoid_predict(dec, A, B):
    """LIBSVM's sigmoid_predict on every value: P(y = +1)."""
    out = []
    for f in np.asarray(dec, dtype=np.float64).tolist():
        fApB = f * A + B
        out.append(math.exp(-fApB) / (1.0 + math.exp(-fApB)) if fApB >= 0 else 1.0 / (1 + math.exp(fApB)))
    return np.array(out, dtype=np.float64)


def platt_inputs():
    """The inputs of the host-only comparison: name -> (decision values, labels)."""
    rng = np.random.Generator(np.random.PCG64(41))
    y = np.where(np.arange(60) % 2 == 0, 1, -1).astype(np.int32)
    few = -np.ones(64, dtype=np.int32)
    few[[5, 37, 50]] = 1
    return {
        "overlapping": (0.6 * y + rng.normal(0.0, 1.0, 60), y),
        "separated": (2.0 * y + rng.normal(0.0, 0.3, 60), y),
        "far_apart": (30.0 * y + rng.normal(0.0, 1.0, 60), y),
        "all_equal": (np.full(60, 0.25), y),
        "two": (np.array([0.7, -0.4]), np.array([1, -1], dtype=np.int32)),
        "anti_correlated": (-0.8 * y + rng.normal(0.0, 1.0, 60), y),
        "few_positives": (1.5 * few - 0.5 + rng.normal(0.0, 0.8, 64), few),
    }


# ---- the case set ----------------------------------------------------------------------------------------------------------------
def table():
    """name -> (case, weights, what the engine is made with, the kernel kind). The rows, weights and C of the issue's table."""
    n96 = lambda C: cases.case(96, 60, 8, 4, C=C)
    fp64 = dict(approx=True, t=1, max_iters=6, seed=5)
    return {"n96_w4_1": (n96(1.0), (4.0, 1.0), {}, "fastsk"), "n96_w1_4": (n96(1.0), (1.0, 4.0), {}, "fastsk"),
            "bound_w8_1": (n96(0.05), (8.0, 1.0), {}, "fastsk"), "bound_w1_8": (n96(0.05), (1.0, 8.0), {}, "fastsk"),
            "few_balanced_C1": (few_positives_case(1.0), "balanced", {}, "fastsk"),
            "few_balanced_C005": (few_positives_case(0.05), "balanced", {}, "fastsk"),
            "duplicates": (cases.duplicates_case(), (2.0, 0.5), {}, "fastsk"),
            "edge257": (cases.edge_case(257), (2.0, 0.5), {}, "fastsk"),
            "edge1025": (cases.edge_case(1025), (2.0, 0.5), {}, "fastsk"),
            "fp64_few_balanced": (few_positives_case(1.0), "balanced", fp64, "fastsk"),
            "linear_n96_w4_1": (n96(1.0), (4.0, 1.0), {}, "linear")}


# ---- cross-validation and calibration --------------------------------------------------------------------------------------------
def expected_w(K, y, fold, Cs, w_pos, w_neg, eps, max_iter=-1):
    """tests/svm_cv_cases.py's ``expected`` with class weights: problem c F + f is ``solve_w`` on the rows with ``fold != f`` at
    the boxes ``Cs[c] w_pos`` / ``Cs[c] w_neg`` (the weights of the whole call: not recomputed per fold)."""
    K = np.asarray(K, dtype=np.float64)
    y = np.asarray(y)
    F = int(np.max(fold)) + 1
    out = []
    for C in Cs:
        for f in range(F):
            idx = np.flatnonzero(np.asarray(fold) != f)
            w = solve_w(K[np.ix_(idx, idx)], y[idx], float(C) * w_pos, float(C) * w_neg, eps, max_iter)
            full = np.zeros(len(y))
            full[idx] = w["alpha"]
            w.update(idx=idx, C=float(C), fold=f, alpha_full=full)
            out.append(w)
    return out
