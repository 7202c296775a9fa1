"""Writes tests/golden/l1_path.npz: per case one component's measured path P, the box's half-width b and the optimum of the LP

    minimise  w1 |D1 p|_1 + w2 |D2 p|_1 + w3 |D3 p|_1   subject to  |p - P| <= b

(w = 10, 1, 100; D_k the k-th forward difference), solved by SciPy's HiGHS (scipy.optimize.linprog; written with SciPy 1.15.3), and HiGHS's own
minimiser.  The tests read the file and never need SciPy.  Run from the repository root: python tests/golden/make_golden_l1_path.py"""
import os

import numpy as np
import scipy.sparse as sp
from scipy.optimize import linprog

HERE = os.path.dirname(os.path.abspath(__file__))
WEIGHTS = (10.0, 1.0, 100.0)


def walk(n, seed):
    """a random walk plus a pan plus a sine: hand-held footage's three ingredients"""
    rs = np.random.RandomState(seed)
    k = np.arange(n, dtype=np.float64)
    return np.cumsum(rs.normal(0.0, 2.0, n)) + 1.5 * k + 12.0 * np.sin(2.0 * np.pi * k / 37.0)


def cases():
    out = {}
    for n, seed in ((4, 11), (5, 12), (9, 13), (200, 14)):
        out["walk%d" % n] = (walk(n, seed), 20.0)
    out["walk513"] = (walk(513, 15), 15.0)   # crosses the 256-thread boundary twice
    out["ramp"] = (2.5 * np.arange(40, dtype=np.float64), 5.0)
    jolt = np.zeros(60, np.float64)
    jolt[30:] = 60.0
    out["jolt"] = (jolt, 20.0)
    out["constant"] = (np.full(40, 7.25, np.float64), 20.0)
    rs = np.random.RandomState(16)
    shake = rs.normal(0.0, 1.0, 60)
    shake = 0.5 * shake / np.sqrt(np.mean(shake * shake))   # RMS 0.5, every sample inside the box of 5: a static path is feasible
    assert np.abs(shake).max() < 5.0
    out["shake"] = (shake, 5.0)
    out["angle"] = (np.cumsum(np.random.RandomState(17).normal(0.0, 0.004, 120)), 0.05)
    return out


def difference(n, k):
    coef = {1: (-1.0, 1.0), 2: (1.0, -2.0, 1.0), 3: (-1.0, 3.0, -3.0, 1.0)}[k]
    return sp.diags(coef, range(k + 1), shape=(n - k, n), format="csr")


def solve(P, b):
    n = len(P)
    ks = [k for k in (1, 2, 3) if n > k]
    m = [n - k for k in ks]
    cost = np.concatenate([np.zeros(n)] + [np.full(mk, WEIGHTS[k - 1]) for k, mk in zip(ks, m)])
    rows = []
    for idx, k in enumerate(ks):   # +-D_k p - e_k <= 0
        D = difference(n, k)
        for sign in (1.0, -1.0):
            blocks = [sign * D] + [(-sp.identity(m[idx]) if j == idx else sp.csr_matrix((m[idx], m[j]))) for j in range(len(ks))]
            rows.append(sp.hstack(blocks, format="csr"))
    A = sp.vstack(rows, format="csr")
    bounds = [(P[i] - b, P[i] + b) for i in range(n)] + [(0.0, None)] * sum(m)
    res = linprog(cost, A_ub=A, b_ub=np.zeros(A.shape[0]), bounds=bounds, method="highs",
                  options={"primal_feasibility_tolerance": 1e-10, "dual_feasibility_tolerance": 1e-10})
    assert res.status == 0, res.message
    return float(res.fun), np.asarray(res.x[:n], np.float64)


def main():
    store = {}
    for name, (P, b) in cases().items():
        f, p = solve(P, b)
        store[name + "_P"], store[name + "_b"], store[name + "_f"], store[name + "_p"] = P, np.float64(b), np.float64(f), p
        print("%-9s n %4d  b %6.3f  f_LP %.12g" % (name, len(P), b, f))
    np.savez_compressed(os.path.join(HERE, "l1_path.npz"), **store)


if __name__ == "__main__":
    main()
