"""Inputs and yardsticks of the SVM stage (fsk_svm_train / fsk_svm_decision, ``fit_svm`` / ``decision_function_np``), shared by
tests/test_emu_svm.py (small scale, CPU emulation) and tests/test_gpu_svm.py (scale 1, MI355X). Nothing here touches an engine.

``solve``      the algorithm of include/fastsk_amd.h restated in numpy float64 on a matrix K (the engine's own
               ``get_train``): the expectation of alpha, rho, the iteration count and the objective, bit for bit.
``certify``    a solution checked from K, y and alpha alone: the box, the equality constraint and the recomputed gap.
``sklearn_objective``  the dual objective scikit-learn's SVC(kernel="precomputed", shrinking=False) reaches on the same K.
``decision_reference`` numpy's K_rows @ (alpha y) - rho with the summation bound of a row."""
import math

import numpy as np

TAU = 1e-12
DEFAULT_MAX_ITER = 10000000
MOTIF = [1, 3, 3, 2, 4, 1, 2, 2, 4, 3]   # the 10-mer planted in 80 % of the positives


# ---- data -------------------------------------------------------------------------------------------------------------------
def dna(n, length, seed, planted=0.8):
    """n sequences of ``length`` tokens 1..4 (PCG64), labels alternating +1, -1, ... by row; the motif overwrites a random
    place of ``planted`` of the positives. -> (int32 array [n, length], int32 labels)."""
    assert length >= len(MOTIF)
    rng = np.random.Generator(np.random.PCG64(seed))
    X = rng.integers(1, 5, size=(n, length), dtype=np.int32)
    y = np.where(np.arange(n) % 2 == 0, 1, -1).astype(np.int32)
    for r in range(n):
        at, coin = int(rng.integers(0, length - len(MOTIF) + 1)), float(rng.random())
        if y[r] > 0 and coin < planted:
            X[r, at:at + len(MOTIF)] = MOTIF
    return X, y


def case(n_train, length, g, m, C=1.0, eps=1e-3, seed=None, n_test=0, labels=None, **engine):
    """One problem: sequences (train rows first), labels of the train rows, the engine's arguments."""
    X, y = dna(n_train + n_test, length, 7000 + n_train * 31 + length if seed is None else seed)
    ytr = y[:n_train].copy() if labels is None else np.asarray(labels, dtype=np.int32)
    assert len(ytr) == n_train and set(np.unique(ytr)) == {-1, 1}
    return {"X": X, "y": ytr, "y_all": y, "n_train": n_train, "n_test": n_test, "g": g, "m": m, "C": float(C), "eps": float(eps),
            "engine": engine}


# the issue's table (the sizes the numpy restatement and LIBSVM were compared at)
def table_cases():
    return {"n96": case(96, 60, 8, 4), "n300": case(300, 80, 10, 6), "n300_C100": case(300, 80, 10, 6, C=100.0),
            "n700": case(700, 100, 10, 6), "all_at_bound": case(64, 40, 6, 2, C=0.05)}


def edge_case(n_train, C=1.0, n_test=0):
    """The smallest problem of n_train rows: short sequences and few combinations (g = 6, m = 2), so that the kernel itself
    costs little on the emulator; the solver sees the same shapes."""
    assert n_train >= 2
    c = case(n_train, 24 if n_train > 2 else 16, 6, 2, C=C, n_test=n_test)
    # the last training row is its neighbour (of the other class) with three symbols changed: it cannot be classified with a
    # margin, so it becomes a support vector and takes part in a step — the last element of the last workgroup is exercised
    last = c["X"][n_train - 2].copy()
    for at in (1, 7, 12):
        last[at] = last[at] % 4 + 1
    c["X"][n_train - 1] = last
    return c


def duplicates_case():
    """Rows 0 and 1 identical with opposite labels (K = 1: a_t = 0, the TAU branch of the selection and of the step), rows 2
    and 4 identical with equal labels."""
    c = edge_case(40)
    c["X"][1] = c["X"][0]
    c["X"][4] = c["X"][2]
    assert c["y"][0] == -c["y"][1] and c["y"][2] == c["y"][4]
    return c


def unbalanced_case():
    """1 positive in 64."""
    y = -np.ones(64, dtype=np.int32)
    y[37] = 1
    return case(64, 40, 6, 2, labels=y, seed=6401)


# ---- the algorithm, restated -------------------------------------------------------------------------------------------------
def rho_and_objective(alpha, G, y, C):
    """LIBSVM's calculate_rho and objective, in index order, one rounding an operation."""
    ub, lb, sum_free, n_free, obj = math.inf, -math.inf, 0.0, 0, 0.0
    for a, g, t in zip(alpha.tolist(), G.tolist(), y.tolist()):
        yg = g if t > 0 else -g
        if a >= C:
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


def step(yi, yj, Kij, Gi, Gj, C, ai, aj):
    """The two-variable update of LIBSVM's Solver::Solve with Q_ii = Q_jj = 1, C_i = C_j = C. -> (alpha_i, alpha_j, tau used)."""
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
        if diff > 0.0:
            if ai > C:
                ai, aj = C, C - diff
        else:
            if aj > C:
                aj, ai = C, C + diff
    else:
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
        else:
            if aj < 0.0:
                aj, ai = 0.0, s
        if s > C:
            if aj > C:
                aj, ai = C, s - C
        else:
            if ai < 0.0:
                ai, aj = 0.0, s
    return ai, aj, tau


def solve(K, y, C, eps, max_iter=-1):
    """SMO with LIBSVM's second-order working-set selection, no shrinking, ties to the lowest index, on the float64 matrix K
    (unit diagonal). Every operation is one IEEE double operation: numpy's elementwise ones and Python's floats."""
    K = np.asarray(K, dtype=np.float64)
    n = len(y)
    yf = np.asarray(y, dtype=np.float64)
    pos = yf > 0
    alpha = np.zeros(n)
    G = -np.ones(n)
    if max_iter < 0:
        max_iter = DEFAULT_MAX_ITER
    it, converged, tau_steps, tau_selected, pairs = 0, False, 0, 0, []
    while True:
        v = np.where(pos, -G, G)
        up = np.where(pos, alpha < C, alpha > 0.0)
        low = np.where(pos, alpha > 0.0, alpha < C)
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
        cand &= ~np.isnan(obj)            # (a cell that is not a number wins no comparison)
        if not cand.any():                # LIBSVM's Gmin_idx == -1: the end, not converged, no step
            break
        j = int(np.argmin(np.where(cand, obj, np.inf)))   # (the first of equal minima)
        assert cand[j]
        yi, yj = int(y[i]), int(y[j])
        ai0, aj0 = float(alpha[i]), float(alpha[j])
        ai, aj, tau = step(yi, yj, float(Ki[j]), float(G[i]), float(G[j]), C, ai0, aj0)
        tau_steps += int(tau)
        dai, daj = ai - ai0, aj - aj0
        Qi = np.where(yf == yi, Ki, -Ki)
        Qj = np.where(yf == yj, K[j], -K[j])
        G = G + ((Qi * dai) + (Qj * daj))
        alpha[i], alpha[j] = ai, aj
        pairs.append((i, j))
        it += 1
    rho, objective = rho_and_objective(alpha, G, y, C)
    return {"alpha": alpha, "G": G, "rho": rho, "objective": objective, "iterations": it, "converged": converged,
            "gap": gmax - gmin, "n_sv": int((alpha > 0).sum()), "n_bsv": int((alpha >= C).sum()), "tau_steps": tau_steps,
            "tau_selected": tau_selected, "pairs": pairs}


# ---- a solution certified from K, y, alpha alone -------------------------------------------------------------------------------
def certify(K, y, alpha, C, eps):
    """0 <= alpha <= C; |y^T alpha| <= 2^-52 n C; the gap Gmax - Gmin of the RECOMPUTED gradient G = Q alpha - 1 is at most eps,
    up to the rounding bound of that recomputation, n 2^-53 sum_i |Q_it alpha_i| a cell (two cells enter the gap). Returns
    the figures."""
    K = np.asarray(K, dtype=np.float64)
    n = len(y)
    yf = np.asarray(y, dtype=np.float64)
    assert alpha.shape == (n,) and np.all(alpha >= 0.0) and np.all(alpha <= C)
    balance = abs(math.fsum((yf * alpha).tolist()))
    assert balance <= 2.0 ** -52 * n * C, balance
    Q = (yf[:, None] * yf[None, :]) * K
    G = Q @ alpha - 1.0
    bound = n * 2.0 ** -53 * (np.abs(Q) @ np.abs(alpha))
    pos = yf > 0
    v = np.where(pos, -G, G)
    up = np.where(pos, alpha < C, alpha > 0.0)
    low = np.where(pos, alpha > 0.0, alpha < C)
    iu = int(np.argmax(np.where(up, v, -np.inf)))
    il = int(np.argmin(np.where(low, v, np.inf)))
    gap = float(v[iu] - v[il]) if up.any() and low.any() else -math.inf
    slack = float(bound[iu] + bound[il])
    assert gap <= eps + slack, (gap, eps, slack)
    objective = 0.5 * float(alpha @ (Q @ alpha)) - float(alpha.sum())
    return {"gap": gap, "slack": slack, "balance": balance, "objective": objective}


def sklearn_objective(K, y, C, eps):
    """The dual objective 1/2 a^T Q a - sum a of scikit-learn's (LIBSVM's) solution on the same matrix."""
    from sklearn.svm import SVC
    clf = SVC(kernel="precomputed", C=C, tol=eps, shrinking=False).fit(K, y)
    a = np.zeros(len(y))
    a[clf.support_] = np.abs(clf.dual_coef_[0])
    yf = np.asarray(y, dtype=np.float64)
    Q = (yf[:, None] * yf[None, :]) * np.asarray(K, dtype=np.float64)
    return 0.5 * float(a @ (Q @ a)) - float(a.sum())


def decision_reference(K_rows, y, alpha, rho):
    """(K_rows @ (alpha y) - rho, the bound n_train 2^-53 sum_i |alpha_i K_ri| of every row's sum)."""
    coef = alpha * np.asarray(y, dtype=np.float64)
    K_rows = np.asarray(K_rows, dtype=np.float64)
    return K_rows @ coef - rho, len(y) * 2.0 ** -53 * (np.abs(K_rows) @ np.abs(coef))
