"""Inputs and yardsticks of the epsilon-SVR stage (fsk_svr_train / fsk_svr_cv, ``fit_svr`` / ``cross_validate_svr``), shared by
tests/test_emu_svr.py (CPU emulation) and tests/test_gpu_svr.py (MI355X). Nothing here touches an engine.

``targets``      seeded real-valued targets tied to the sequences of ``svm_cases.dna``: 1 where the motif stands, plus N(0, 0.25).
``solve_svr``    LIBSVM's 2n-element formulation restated in numpy float64 on a matrix K (the engine's own ``get_train``), with
                 ``svm_cases.step`` and ``svm_cases.TAU``: the expectation of alpha2, coef, rho, the objective, the iteration
                 count, bit for bit.
``certify``      a solution checked from K, z and coef alone: the box, the equality constraint, the recomputed gap.
``sklearn_objective``  the dual objective of scikit-learn's SVR(kernel="precomputed", shrinking=False) on the same K.
``scores``       the sums of fsk_svr_cv's header, restated (Python floats: one rounding an operation)."""
import math

import numpy as np

import svm_cases
from svm_cases import TAU, DEFAULT_MAX_ITER, MOTIF, step

SIGMA = 0.25


# ---- data -------------------------------------------------------------------------------------------------------------------
def targets(X, seed=1):
    """z[r] = 1.0 where row r of X holds the motif (0.0 elsewhere) + a PCG64(seed) normal of sigma 0.25."""
    X = np.asarray(X)
    m = len(MOTIF)
    has = np.array([any(list(row[a:a + m]) == MOTIF for a in range(len(row) - m + 1)) for row in X.tolist()], dtype=np.float64)
    return has + SIGMA * np.random.Generator(np.random.PCG64(seed)).standard_normal(len(X))


def edge_case(n_train, n_test=0):
    """``svm_cases.edge_case`` (g = 6, m = 2, length 24) with targets of its train rows."""
    c = svm_cases.edge_case(n_train, n_test=n_test)
    c["z"] = targets(c["X"][:n_train], seed=100 + n_train)
    # the last training row is its neighbour with three symbols changed (svm_cases.edge_case): with a target 1 apart the two
    # cannot both lie in a tube of 0.1, so the last row becomes a support vector and takes part in a step
    c["z"][n_train - 1] = c["z"][n_train - 2] + 1.0
    return c


def bound_case():
    """64 rows whose targets are the class labels -1 / +1 plus a seeded normal of sigma 0.05: at C = 0.05 every residual stays
    outside the tube, so every row is a support vector at the bound (and the two signs balance)."""
    c = edge_case(64)
    c["z"] = c["y"].astype(np.float64) + 0.2 * targets(c["X"][:64], seed=164)
    return c


def duplicates_case():
    """Rows 0 and 1 identical with targets 2 apart: K = 1 between different rows, so a_t = 0 — the TAU branch of the selection
    and of the step."""
    c = edge_case(40)
    c["X"][1] = c["X"][0]
    c["z"][0], c["z"][1] = 1.5, -0.5
    return c


# ---- the algorithm, restated -------------------------------------------------------------------------------------------------
def finish(alpha, G, p, n, C):
    """LIBSVM's calculate_rho over the 2n elements and the objective 1/2 sum alpha_e (G_e + p_e), in element order."""
    ub, lb, sum_free, n_free, obj = math.inf, -math.inf, 0.0, 0, 0.0
    for e, (a, g, pe) in enumerate(zip(alpha.tolist(), G.tolist(), p.tolist())):
        up = e < n
        yg = g if up else -g
        if a >= C:
            if not up:
                ub = min(ub, yg)
            else:
                lb = max(lb, yg)
        elif a <= 0.0:
            if up:
                ub = min(ub, yg)
            else:
                lb = max(lb, yg)
        else:
            n_free += 1
            sum_free += yg
        obj += a * (g + pe)
    rho = sum_free / n_free if n_free else (ub + lb) / 2.0
    return rho, obj / 2.0


def solve_svr(K, z, C, epsilon, eps, max_iter=-1):
    """SMO over the 2n elements: e < n is alpha_e (y = +1), e + n is alpha*_e (y = -1), both kernel row e; p = (epsilon - z,
    epsilon + z); alpha = 0, G = p; second-order selection, no shrinking, ties to the lowest element."""
    K = np.asarray(K, dtype=np.float64)
    z = np.asarray(z, dtype=np.float64)
    n = len(z)
    yf = np.concatenate((np.ones(n), -np.ones(n)))
    pos = yf > 0
    p = np.concatenate((epsilon - z, epsilon + z))
    alpha = np.zeros(2 * n)
    G = p.copy()
    if max_iter < 0:
        max_iter = DEFAULT_MAX_ITER
    it, converged, tau_steps, tau_selected, pairs = 0, False, 0, 0, []
    while True:
        v = np.where(pos, -G, G)
        up = np.where(pos, alpha < C, alpha > 0.0)
        low = np.where(pos, alpha > 0.0, alpha < C)
        vu = np.where(up, v, -np.inf)
        i = int(np.argmax(vu))
        gmax = float(vu[i])
        gmin = float(np.min(np.where(low, v, np.inf)))
        if gmax - gmin <= eps:
            converged = True
            break
        if it >= max_iter:
            break
        Ki = np.concatenate((K[i % n], K[i % n]))
        b = gmax - v
        a = 2.0 - 2.0 * Ki
        cand = low & (b > 0.0)
        tau_selected += int(np.any(cand & (a <= 0.0)))
        a = np.where(a <= 0.0, TAU, a)
        obj = np.where(cand, -((b * b) / a), np.inf)
        cand &= ~np.isnan(obj)
        if not cand.any():
            break
        j = int(np.argmin(np.where(cand, obj, np.inf)))
        assert cand[j] and j % n != i % n      # (a step on the twins of one row cannot be selected: b = -2 epsilon)
        yi, yj = (1 if i < n else -1), (1 if j < n else -1)
        ai0, aj0 = float(alpha[i]), float(alpha[j])
        ai, aj, tau = step(yi, yj, float(Ki[j]), float(G[i]), float(G[j]), C, ai0, aj0)
        tau_steps += int(tau)
        dai, daj = ai - ai0, aj - aj0
        Kj = np.concatenate((K[j % n], K[j % n]))
        Qi = np.where(yf == yi, Ki, -Ki)
        Qj = np.where(yf == yj, Kj, -Kj)
        G = G + ((Qi * dai) + (Qj * daj))
        alpha[i], alpha[j] = ai, aj
        pairs.append((i, j))
        it += 1
    rho, objective = finish(alpha, G, p, n, C)
    coef = alpha[:n] - alpha[n:]
    return {"alpha2": alpha, "coef": coef, "G": G, "rho": rho, "objective": objective, "iterations": it, "converged": converged,
            "gap": gmax - gmin, "n_sv": int((coef != 0).sum()), "n_bsv": int((np.abs(coef) >= C).sum()), "tau_steps": tau_steps,
            "tau_selected": tau_selected, "pairs": pairs}


# ---- a solution certified from K, z, coef alone -------------------------------------------------------------------------------
def certify(K, z, coef, C, epsilon, eps):
    """|coef| <= C; |sum coef| <= 2^-52 2n C; with alpha = max(coef, 0), alpha* = max(-coef, 0) and the RECOMPUTED gradient
    G = (K coef - z + epsilon, -(K coef) + z + epsilon), Gmax - Gmin <= eps up to the rounding bound of the recomputation:
    n 2^-53 sum_i |K_ti coef_i| for the product and 2^-52 (|K coef| + |z| + epsilon) for the two additions, a cell (two cells
    enter the gap). Returns the figures."""
    K = np.asarray(K, dtype=np.float64)
    z = np.asarray(z, dtype=np.float64)
    n = len(z)
    assert coef.shape == (n,) and np.all(np.abs(coef) <= C)
    balance = abs(math.fsum(coef.tolist()))
    assert balance <= 2.0 ** -52 * 2 * n * C, balance
    f = K @ coef
    bound = n * 2.0 ** -53 * (np.abs(K) @ np.abs(coef)) + 2.0 ** -52 * (np.abs(f) + np.abs(z) + epsilon)
    bound = np.concatenate((bound, bound))
    alpha = np.concatenate((np.maximum(coef, 0.0), np.maximum(-coef, 0.0)))
    G = np.concatenate((f - z + epsilon, -f + z + epsilon))
    pos = np.arange(2 * n) < n
    v = np.where(pos, -G, G)
    up = np.where(pos, alpha < C, alpha > 0.0)
    low = np.where(pos, alpha > 0.0, alpha < C)
    iu = int(np.argmax(np.where(up, v, -np.inf)))
    il = int(np.argmin(np.where(low, v, np.inf)))
    gap = float(v[iu] - v[il]) if up.any() and low.any() else -math.inf
    slack = float(bound[iu] + bound[il])
    assert gap <= eps + slack, (gap, eps, slack)
    objective = 0.5 * float(coef @ f) + epsilon * float(np.abs(coef).sum()) - float(z @ coef)
    return {"gap": gap, "slack": slack, "balance": balance, "objective": objective}


def sklearn_objective(K, z, C, epsilon, eps):
    """1/2 c^T K c + epsilon sum |c| - z^T c of scikit-learn's (LIBSVM's) solution on the same matrix."""
    from sklearn.svm import SVR
    m = SVR(kernel="precomputed", C=C, epsilon=epsilon, tol=eps, shrinking=False).fit(K, z)
    c = np.zeros(len(z))
    c[m.support_] = m.dual_coef_[0]
    K = np.asarray(K, dtype=np.float64)
    return 0.5 * float(c @ (K @ c)) + epsilon * float(np.abs(c).sum()) - float(np.asarray(z) @ c)


def decision_reference(K_rows, coef, rho):
    """(K_rows @ coef - rho, the bound of every row): the summation bound of ``svm_cases.decision_reference``,
    n_train 2^-53 sum_i |coef_i K_ri|, for the two sums, and 2^-53 |value| for the one rounding of ``- rho`` on either side. A
    regression's rho is of the size of the targets while a row's sum may be far smaller (two rows: sum 0.05, rho -1.6), so the
    rounding of the subtraction is not covered by the bound of the sum as it is for the C-SVC's cases."""
    K_rows = np.asarray(K_rows, dtype=np.float64)
    ref = K_rows @ coef - rho
    return ref, len(coef) * 2.0 ** -53 * (np.abs(K_rows) @ np.abs(coef)) + 2.0 ** -52 * np.abs(ref)


def scores(oof, z):
    """mse, mae, r2, r of one grid point as include/fastsk_amd.h states them: plain sums in row order."""
    oof, z = [float(x) for x in oof], [float(x) for x in z]
    n = len(z)
    sz = so = 0.0
    for a, b in zip(z, oof):
        sz += a
        so += b
    zm, om = sz / n, so / n
    sse = sae = sst = soo = szo = 0.0
    for a, b in zip(z, oof):
        d, dz, dq = b - a, a - zm, b - om
        sse += d * d
        sae += abs(d)
        sst += dz * dz
        soo += dq * dq
        szo += dq * dz
    with np.errstate(all="ignore"):
        sse_, sst_, soo_, szo_ = np.float64(sse), np.float64(sst), np.float64(soo), np.float64(szo)
        return {"mse": sse / n, "mae": sae / n, "r2": float(1.0 - sse_ / sst_), "r": float(szo_ / np.sqrt(soo_ * sst_))}
